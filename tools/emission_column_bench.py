"""The masked emission column of teHmmEval --ed on the device: kernel time and end-to-end rate (results:
profiles/emission_column.txt).

  python tools/emission_column_bench.py [--mb 100] [--repeats 10] [--base-repeats 2] [--kernels-only] [--out FILE]

Shapes: 35 states x 10 tracks (config 2), --mb megabases in 97 intervals (the bench shape), and 100 / 300 states on 2 Mb.
 (a) device time of one tehmm_batch_emission_masksum over the whole batch (first-row pass + row kernel, HIP events of
     tehmm_batch_last_timing "emission_column"), warm-up + --repeats runs, median and min..max, and what that is in
     rows/s and in GB/s of the emission rows the kernel forms and never writes (8 N bytes per row);
 (b) end-to-end rows/s of the column -- batch creation (H2D of the observations), the call and the 8 B/row copy -- table
     by table as teHmmEval walks them, against what the column cost before: the per-table array-level
     emissionDistribution (observations and the [K][N][S] model uploaded per call, the [T][N] fp64 frame written to
     the host) plus np.log(np.sum(np.exp(frame) * mask, axis=1)) on the host."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return "median %.3f  min %.3f  max %.3f  (n=%d)" % (np.median(xs), xs.min(), xs.max(), len(xs))


def make_case(n_states, mb, n_iv, seed):
    from tehmm_amd import synth
    model = synth.make_model(n_states, seed=seed, stay=0.99)
    total = int(mb * 1_000_000)
    block = synth.random_obs(model, min(total, 2_000_000), seed=3)
    obs = np.ascontiguousarray(np.tile(block, ((total + len(block) - 1) // len(block), 1))[:total])
    cuts = np.linspace(0, total, n_iv + 1).astype(np.int64)
    return model, obs, cuts


def run_case(name, n_states, mb, n_iv, args, out):
    from tehmm_amd import _emission
    from tehmm_amd.engine import HipBatch, HipModel
    model, obs, offs = make_case(n_states, mb, n_iv, seed=7)
    total = int(offs[-1])
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs, symbols_per_track=model.symbols_per_track)
    out("== %s: %d states, %d tracks, %d rows in %d intervals" % (name, n_states, obs.shape[1], total, n_iv))
    mask = (np.arange(n_states) % 3 == 0).astype(np.float64)
    hb = HipBatch(obs, offs)
    t_k = []
    for it in range(args.repeats + 2):
        col = hb.emission_masksum(hm, mask)
        if it >= 2:                                   # two warm-up rounds
            t_k.append(hb.timing()["emission_column"])
    med = np.median(t_k) * 1e-3
    out("(a) emission_column device time, ms:  %s   -> %.0f x1e6 rows/s, %.0f GB/s of emission rows formed"
        % (stats(t_k), total / med / 1e6, total * n_states * 8 / 1e9 / med))
    hb.close()
    if args.kernels_only:
        hm.close()
        return
    new, base = [], []
    for it in range(args.repeats + 1):
        t0 = time.perf_counter()
        cols = []
        for a, b in zip(offs[:-1], offs[1:]):
            tb = HipBatch(obs[a:b], np.asarray([0, b - a], dtype=np.int64))
            cols.append(tb.emission_masksum(hm, mask))
            tb.close()
        dt = time.perf_counter() - t0
        if it >= 1:
            new.append(total / dt)
    worst = 0.0
    for it in range(args.base_repeats + 1):
        t0 = time.perf_counter()
        for i, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
            frame = np.zeros((b - a, n_states))
            _emission.fastAllLogProbs(obs[a:b], model.log_probs, frame, 1.0, None)
            with np.errstate(divide="ignore"):
                ref = np.log(np.sum(np.exp(frame) * mask, axis=1))
            if it == 0:
                worst = max(worst, float(np.max(np.abs(ref - cols[i]) / np.maximum(1.0, np.abs(ref)))))
        dt = time.perf_counter() - t0
        if it >= 1:
            base.append(total / dt)
    assert np.array_equal(np.concatenate(cols), col)
    out("(b) column per table on the device, rows/s:                    %s" % stats(np.asarray(new) / 1e6) + "  [x1e6]")
    out("    array-level emissionDistribution + NumPy reduction, rows/s: %s" % stats(np.asarray(base) / 1e6) + "  [x1e6]")
    out("    ratio of the medians: %.1fx; largest difference of the two columns %.2e (relative, floor 1)"
        % (np.median(new) / np.median(base), worst))
    hm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--base-repeats", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from tehmm_amd import build
    build.build()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    run_case("bench shape", 35, args.mb, 97, args, out)
    run_case("wide", 100, 2.0, 8, args, out)
    run_case("large", 300, 2.0, 256, args, out)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
