"""Maximum-posterior decoding on the device: kernel time and end-to-end rate (results: profiles/map_decode.txt).

  python tools/map_decode_bench.py [--mb 100] [--repeats 10] [--base-repeats 3] [--kernels-only] [--out FILE]

Shapes: 35 states x 10 tracks (config 2), --mb megabases in 97 intervals (the bench shape), and 100 / 300 states on 2 Mb.
 (a) device time of the map_decode row reduction (HIP events of tehmm_batch_last_timing), without and with a mask,
     warm-up + --repeats runs, median and min..max.  Its yardstick, k_post_masksum, reads the same rows; the library
     does not event-time that kernel, so the tool reports the wall time of tehmm_batch_posterior_masksum (kernel +
     allocation + the 8 B/row copy) and, for the kernel alone, is run under
         rocprofv3 --kernel-trace --stats -- python tools/map_decode_bench.py --kernels-only
     where both kernels appear by name.
 (b) end-to-end positions/s of eval_stream(map_decode=True) against the only route there was before: eval_stream with
     the full posterior rows plus np.argmax / np.max(...).sum() on the host (--base-repeats runs: the host reduction of
     100 Mb takes seconds)."""
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
    from tehmm_amd.engine import HipBatch, HipModel, eval_stream
    model, obs, offs = make_case(n_states, mb, n_iv, seed=7)
    total = int(offs[-1])
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs, symbols_per_track=model.symbols_per_track)
    out("== %s: %d states, %d tracks, %d positions in %d intervals" % (name, n_states, obs.shape[1], total, n_iv))
    hb = HipBatch(obs, offs)
    hm.eval(hb, viterbi=False, posterior=True)
    mask = (np.arange(n_states) % 3 == 0).astype(np.float64)
    t_plain, t_mask, t_sum, t_msum = [], [], [], []
    for it in range(args.repeats + 2):
        hb.map_decode()
        tm = hb.timing()
        t0 = time.perf_counter()
        hb.posterior_masksum(mask)
        w = (time.perf_counter() - t0) * 1e3
        hb.map_decode(mask)
        tm2 = hb.timing()
        if it >= 2:                                   # two warm-up rounds
            t_plain.append(tm["map_decode"])
            t_sum.append(tm["map_logprob_sum"])
            t_mask.append(tm2["map_decode"])
            t_msum.append(w)
    gb = total * n_states * 8 / 1e9
    out("(a) map_decode kernel, ms:            %s   -> %.0f GB/s of posterior rows" % (stats(t_plain), gb / (np.median(t_plain) * 1e-3)))
    out("    map_decode kernel with mask, ms:  %s" % stats(t_mask))
    out("    interval sums (map_logprob), ms:  %s" % stats(t_sum))
    out("    posterior_masksum call (kernel + alloc + D2H of 8 B/row), wall ms: %s" % stats(t_msum))
    hb.close()
    if args.kernels_only:
        hm.close()
        return
    new, base = [], []
    for it in range(args.repeats + 1):
        t0 = time.perf_counter()
        r = eval_stream(hm, obs, offs, viterbi=False, posterior=False, map_decode=True)
        dt = time.perf_counter() - t0
        if it >= 1:
            new.append(total / dt)
    ref_mlp, ref_paths = r[5], r[4]
    for it in range(args.base_repeats + 1):
        t0 = time.perf_counter()
        _, posts, _, _ = eval_stream(hm, obs, offs, viterbi=False, posterior=True)
        paths = [np.argmax(p, axis=1) for p in posts]
        mlp = np.asarray([np.max(p, axis=1).sum() for p in posts])
        dt = time.perf_counter() - t0
        if it >= 1:
            base.append(total / dt)
    same = np.mean([np.mean(a == b) for a, b in zip(paths, ref_paths)])
    out("(b) eval_stream(map_decode=True), positions/s:             %s" % stats(np.asarray(new) / 1e6) + "  [x1e6]")
    out("    eval_stream(posterior rows) + host argmax, positions/s: %s" % stats(np.asarray(base) / 1e6) + "  [x1e6]")
    out("    ratio of the medians: %.1fx; states equal on %.6f of rows; map_logprob max rel. diff %.2e"
        % (np.median(new) / np.median(base), same, np.max(np.abs(mlp - ref_mlp) / np.abs(mlp))))
    del posts, paths
    hm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100.0)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--base-repeats", type=int, default=3)
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
    run_case("large", 300, 2.0, 256, args, out)     # (one workgroup per interval above 128 states)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
