"""Positions/s of the 129..1024-state kernels (tehmm_large.hip.h) against the 16-thread CPU oracle and the old
array-level posterior route (emission frame, log-space k_forward_log / k_backward_log through the host).

Workload: 256 intervals x 40 kb (10 Mb) at N = 200, 256, 512 and 256 intervals x 8 kb (2 Mb) at N = 1024, config-2
tracks; then one single 2 Mb interval at N = 256.  Every GPU figure is the second of two calls (the first warms up).
usage: python tools/large_states_bench.py [--quick] [--out FILE]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle                                   # noqa: E402
from tehmm_amd import _hmm, synth                           # noqa: E402
from tehmm_amd.engine import HipBatch, HipModel             # noqa: E402

MODES = (("viterbi", dict(viterbi=True, posterior=False)), ("posterior", dict(viterbi=False, posterior=True)),
         ("both", dict(viterbi=True, posterior=True)))


def tiled_obs(model, total, seed):
    piece = synth.sample_obs(model, 100_000, seed=seed)
    rs = np.random.RandomState(seed + 1)
    reps = [piece[s:s + 50_000] for s in rs.randint(0, 50_000, size=total // 50_000 + 1)]
    return np.ascontiguousarray(np.concatenate(reps)[:total])


def gpu_rates(model, obs, lens, warm=True):
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs, symbols_per_track=model.symbols_per_track)
    hb = HipBatch(obs, offs)
    out = {}
    for name, kw in MODES:
        if warm:
            hm.eval(hb, use_ratios=False, **kw)
        t0 = time.perf_counter()
        hm.eval(hb, use_ratios=False, **kw)
        dt = time.perf_counter() - t0
        out[name] = {"s": round(dt, 4), "pos_per_s": float("%.4g" % (offs[-1] / dt)),
                     "kernels_ms": {k: round(v, 2) for k, v in hb.timing().items()}}
        print("  gpu %-9s %8.3f s  %.3g positions/s  %s" % (name, dt, offs[-1] / dt, out[name]["kernels_ms"]), flush=True)
    hb.close()
    hm.close()
    return out


def oracle_rates(model, obs, n_iv, L):
    sub = np.ascontiguousarray(obs[:n_iv * L])
    offs = np.arange(n_iv + 1, dtype=np.int64) * L
    out = {}
    for name, want_post in (("viterbi", False), ("both", True)):
        t0 = time.perf_counter()
        oracle.eval_batch(sub, offs, model.log_probs, model.log_startprob, model.log_transmat, want_post=want_post,
                          n_threads=16)
        dt = time.perf_counter() - t0
        out[name] = {"positions": int(n_iv * L), "s": round(dt, 3), "pos_per_s": float("%.4g" % (n_iv * L / dt))}
        print("  oracle(16 threads) %-7s %d x %d rows: %.3g positions/s" % (name, n_iv, L, n_iv * L / dt), flush=True)
    return out


def array_level_posterior_rate(model, obs, T):
    """The route posteriors above 128 states took before: emission frame, log-space forward and backward, one table at
    a time through the host (BaseHMM.score_samples without the posterior normalisation, which is host NumPy)."""
    N = model.log_transmat.shape[0]
    o = np.ascontiguousarray(obs[:T])
    from tehmm_amd import _emission
    t0 = time.perf_counter()
    frame = np.zeros((T, N))
    _emission.fastAllLogProbs(o, model.log_probs, frame, 1.0, None)
    fwd = np.zeros((T, N))
    bwd = np.zeros((T, N))
    _hmm._forward(T, N, model.log_startprob, model.log_transmat, frame, None, fwd)
    _hmm._backward(T, N, model.log_startprob, model.log_transmat, frame, None, bwd)
    dt = time.perf_counter() - t0
    print("  array-level posterior route, one %d-row interval: %.3g positions/s" % (T, T / dt), flush=True)
    return {"positions": T, "s": round(dt, 3), "pos_per_s": float("%.4g" % (T / dt))}


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    res = {}
    cases = [(200, 256, 40_000), (256, 256, 40_000), (512, 256, 40_000), (1024, 256, 8_000)]
    if quick:
        cases = [(256, 256, 40_000)]
    for N, n_iv, L in cases:
        print("N = %d: %d intervals x %d rows" % (N, n_iv, L), flush=True)
        model = synth.make_model(N, seed=0)
        obs = tiled_obs(model, n_iv * L, seed=N)
        r = {"gpu": gpu_rates(model, obs, [L] * n_iv)}
        o_iv, o_L = {200: (32, 2000), 256: (32, 2000), 512: (16, 1000), 1024: (16, 100)}[N]
        r["oracle"] = oracle_rates(model, obs, o_iv, o_L)
        if N <= 512:
            r["array_level_posterior"] = array_level_posterior_rate(model, obs, 20_000 if N <= 256 else 5_000)
        r["viterbi_vs_oracle"] = round(r["gpu"]["viterbi"]["pos_per_s"] / r["oracle"]["viterbi"]["pos_per_s"], 1)
        if "array_level_posterior" in r:
            r["posterior_vs_array_level"] = round(r["gpu"]["posterior"]["pos_per_s"] /
                                                  r["array_level_posterior"]["pos_per_s"], 1)
        res["N%d" % N] = r
    print("N = 256: one interval of 2 Mb", flush=True)
    model = synth.make_model(256, seed=0)
    obs = tiled_obs(model, 2_000_000, seed=7)
    res["N256_single_2Mb"] = {"gpu": gpu_rates(model, obs, [2_000_000], warm=False)}
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
