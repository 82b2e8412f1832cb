#!/usr/bin/env python3
"""Raw E-step results of the cases of tests/test_gpu_estep_routes.py (plus a 70-state case on the item-parallel passes),
for a bit-for-bit comparison of two builds of the library (TEHMM_HIP_LIB selects the one to load):

    python tools/estep_dump.py OUT.npz              every case on every route that takes it, two calls per batch: the raw
                                                    statistics buffer of tehmm_estep_batch_device, the returned
                                                    log-likelihood, the per-interval log-probabilities
    python tools/estep_dump.py --compare A.npz B.npz    np.array_equal of every array, NaNs by position; exit 1 on a difference
    python tools/estep_dump.py --calls A.npz            the same between the first and the second call of every batch of one
                                                    dump: what a route varies by from run to run on one build (the
                                                    sequential kernels add their statistics with floating-point atomics)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CASES = ("plain5", "ratios35", "dead5", "wide70")


def dump(path):
    import test_gpu_estep_routes as routes
    from tehmm_amd.engine import DeviceStats, HipBatch, HipModel
    out = {}
    for name in CASES:
        model, log_probs, obs, offs, r, case_routes = routes.case(name)
        for route in case_routes:
            with routes.knobs(route):
                hm = HipModel(model.log_transmat, model.log_startprob, log_probs, 1.0, model.symbols_per_track)
                hb = HipBatch(obs, offs, r)
                stats = DeviceStats(hm)
                for call in range(2):
                    stats.zero()
                    lp = hm.estep_device(hb, r is not None, stats)
                    tag = "%s.%s.call%d." % (name, route, call)
                    out[tag + "stats"] = stats.to_host()
                    out[tag + "logprob"] = np.array([lp])
                    out[tag + "interval_logprobs"] = hb.interval_logprobs()
                    out[tag + "timing_keys"] = np.array(list(hb.timing()), dtype="U64")
                stats.close()
                hb.close()
                hm.close()
    np.savez(path, **out)
    print("%d arrays -> %s" % (len(out), path))


def compare(pa, pb, calls=False):
    a, b = np.load(pa), np.load(pb)
    if calls:
        a = {k.replace(".call0.", "."): a[k] for k in a.files if ".call0." in k}
        b = {k.replace(".call1.", "."): b[k] for k in b.files if ".call1." in k}
    else:
        a, b = {k: a[k] for k in a.files}, {k: b[k] for k in b.files}
    bad = sorted(set(a) ^ set(b))
    for k in bad:
        print("ONLY IN ONE  %s" % k)
    for k in sorted(set(a) & set(b)):
        x, y = a[k], b[k]
        same = x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")
        print("%-9s %-48s %s" % ("equal" if same else "DIFFERS", k, x.shape))
        if not same:
            bad.append(k)
            if x.shape == y.shape and x.dtype.kind == "f":
                where = np.flatnonzero(~((x == y) | (np.isnan(x) & np.isnan(y))).ravel())
                xs, ys = x.ravel()[where], y.ravel()[where]
                with np.errstate(all="ignore"):
                    rel = np.nanmax(np.abs(xs - ys) / np.maximum(np.abs(xs), np.abs(ys)))
                print("          %d of %d elements, first at %d: %r vs %r; largest relative difference %.3g"
                      % (len(where), x.size, where[0], float(xs[0]), float(ys[0]), rel))
    print("%d arrays compared, %d differ" % (len(set(a) | set(b)), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 3 and sys.argv[1] == "--calls":
        sys.exit(compare(sys.argv[2], sys.argv[2], calls=True))
    if len(sys.argv) != 2 or sys.argv[1].startswith("-"):
        sys.exit(__doc__)
    dump(sys.argv[1])
