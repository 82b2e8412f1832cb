#!/usr/bin/env python3
"""Times the CYK decode of the grammar model (tehmm_cyk_decode): one interval at each of
--lengths, then one batch of --batch intervals of --batch-len rows, with M = 5 states of which two emit pairs and
tables as supervised training leaves them (every production of the training's shape present: 45 splits and 10 pair
productions).

Per case it reports the wall-clock of the whole call, the device time of the passes (HIP events,
tehmm_cyk_last_timing) and add-add-compare triples per second of the fill: a triple is one candidate of the
recurrence, (L^3 - L) / 6 split points per interval times the split productions plus one per pair production and cell
longer than two.  There is no pass mark.

    python tools/cyk_bench.py [--lengths 512,1024,2048,4096] [--batch 200] [--batch-len 500] [--out profiles/cyk_bench.txt]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_model(M, nest, seed):
    from tehmm_amd.cfg import MultitrackCfg
    from tehmm_amd.emission import IndependentMultinomialEmissionModel, PairEmissionModel
    rs = np.random.RandomState(seed)
    em = IndependentMultinomialEmissionModel(M, [4], zeroAsMissingData=False)
    cfg = MultitrackCfg(em, PairEmissionModel(em, [0.95] * M), nestStates=nest)
    cfg._tablesFromHmm(rs.dirichlet(np.ones(M)), rs.dirichlet(np.ones(M), size=M))
    return cfg, np.log(rs.dirichlet(np.ones(4), size=M))          # emission table [M][4]


def run(lib, _lib, cfg, emis, lens, seed, repeats):
    rs = np.random.RandomState(seed)
    M = cfg.M
    total = int(np.sum(lens))
    obs = rs.randint(0, 4, size=total)
    em = np.ascontiguousarray(emis[:, obs].T)
    al = rs.randint(0, 4, size=total).astype(np.uint16)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    is_nest = np.zeros(M, dtype=np.uint8)
    is_nest[cfg.nestStates] = 1
    lp1, lp2 = _lib.as_f64(cfg.logProbs1), _lib.as_f64(cfg.logProbs2)
    pri, start = _lib.as_f64(cfg.pairEmissionModel.logPriors), _lib.as_f64(cfg.startProbs)
    n = len(lens)
    scores, top, trace = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(total)
    f64p, ptr = _lib.f64p, _lib.ptr
    walls, passes = [], []
    for it in range(repeats + 1):                                 # the first call is the warm-up
        t0 = time.time()
        _lib.check(lib.tehmm_cyk_decode(n, ptr(offsets, _lib.i64p), M, ptr(em, f64p), ptr(al, _lib.u16p), 0,
                                        ptr(is_nest, _lib.u8p), ptr(lp1, f64p), ptr(lp2, f64p), ptr(pri, f64p),
                                        ptr(start, f64p), ptr(scores, f64p), ptr(top, _lib.i64p), ptr(trace, f64p)),
                   "tehmm_cyk_decode")
        wall = time.time() - t0
        names = (ctypes.c_char_p * 16)()
        ms = np.zeros(16)
        k = lib.tehmm_cyk_last_timing(16, names, ptr(ms, f64p))
        if it > 0:
            walls.append(wall)
            passes.append({names[i].decode(): ms[i] for i in range(k)})
    p1, p2 = int(np.sum(lp1 > -np.inf)), int(np.sum(lp2 > -np.inf))
    L = np.asarray(lens, dtype=np.float64)
    triples = float(np.sum((L ** 3 - L) / 6.0) * p1 + np.sum(np.maximum(L - 2, 0) * np.maximum(L - 1, 0) / 2.0) * p2)
    med = {k: float(np.median([p[k] for p in passes])) for k in passes[0]}
    return float(np.median(walls)), med, triples, float(np.sum(scores))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lengths", default="512,1024,2048,4096")
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--batch-len", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    from tehmm_amd import _lib
    if _lib.device_count() < 1:
        sys.exit("cyk_bench: no GPU")
    lib = _lib.load()
    cfg, emis = make_model(5, [1, 3], 0)
    cases = [("1 x L = %d" % int(L), [int(L)]) for L in args.lengths.split(",") if L]
    if args.batch > 0:
        cases.append(("%d x L = %d" % (args.batch, args.batch_len), [args.batch_len] * args.batch))
    lines = ["cyk_bench: M = 5, pair states 1 and 3, %d split and %d pair productions; median of %d calls after a warm-up"
             % (int(np.sum(cfg.logProbs1 > -np.inf)), int(np.sum(cfg.logProbs2 > -np.inf)), args.repeats),
             "%-14s %11s %11s %9s %9s %11s %11s %14s" % ("case", "call ms", "kernels ms", "init", "fill", "traceback",
                                                        "triples", "triples/s fill")]
    for name, lens in cases:
        wall, med, triples, _ = run(lib, _lib, cfg, emis, lens, 1, args.repeats)
        kernels = med["init"] + med["fill"] + med["traceback"]
        lines.append("%-14s %11.2f %11.2f %9.2f %9.2f %11.2f %11.3e %14.3e" % (
            name, 1e3 * wall, kernels, med["init"], med["fill"], med["traceback"], triples, triples / (1e-3 * med["fill"])))
        sys.stdout.write(lines[-1] + "\n")
        sys.stdout.flush()
    text = "\n".join(lines) + "\n"
    sys.stdout.write("\n" + text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
