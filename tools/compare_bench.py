#!/usr/bin/env python3
"""Times the three comparison calls (tehmm_compare_base, tehmm_compare_intervals in both directions,
tehmm_merge_runs) at genome scale: a prediction of --preds one-base rows against truth intervals of geometric length
(mean --truth-len) over the same bases, a handful of state names.

For each call it reports the per-pass device times (HIP events, tehmm_compare_last_timing) and the wall-clock of the
whole call, upload included; then it times the plain-Python statement of the walks (tests/compare_ref.py) on the first
--ref-bases bases of the same lists, checks that the device agrees with it there, and scales that time to the full
length (the scaled figure is an extrapolation from the sample, and is labelled so).

    python tools/compare_bench.py [--preds 10000000] [--truth-len 1000] [--repeats 3] [--out profiles/compare.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_lists(n, truth_len, n_labels, seed):
    """(truth, pred) IntervalArrays over bases [0, n) of one chromosome"""
    from tehmm_amd.compare import IntervalArrays
    rs = np.random.RandomState(seed)
    lens = rs.geometric(1.0 / truth_len, size=int(n / truth_len * 1.2) + 16)
    while lens.sum() < n:
        lens = np.concatenate([lens, rs.geometric(1.0 / truth_len, size=len(lens))])
    ends = np.cumsum(lens)
    k = int(np.searchsorted(ends, n))
    ends = np.concatenate([ends[:k], [n]]).astype(np.int64)
    starts = np.concatenate([[0], ends[:-1]]).astype(np.int64)
    tlab = rs.randint(n_labels, size=len(starts)).astype(np.int32)
    truth = IntervalArrays(np.zeros(len(starts), np.int32), starts, ends, tlab)
    pos = np.arange(n, dtype=np.int64)
    own = np.repeat(tlab, ends - starts)
    plab = np.where(rs.rand(n) < 0.8, own, rs.randint(n_labels, size=n)).astype(np.int32)
    return truth, IntervalArrays(np.zeros(n, np.int32), pos, pos + 1, plab)


def head(arrays, n_bases):
    from tehmm_amd.compare import IntervalArrays
    k = int(np.searchsorted(arrays.start, n_bases))
    end = arrays.end[:k].copy()
    end[-1] = min(int(end[-1]), n_bases)
    return IntervalArrays(arrays.chrom[:k], arrays.start[:k], end, arrays.label[:k])


def tuples(arrays):
    return [("c", int(a), int(b), int(k)) for a, b, k in zip(arrays.start, arrays.end, arrays.label)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--preds", type=int, default=10000000)
    ap.add_argument("--truth-len", type=float, default=1000.0)
    ap.add_argument("--labels", type=int, default=4)
    ap.add_argument("--threshold", type=float, default=0.8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-bases", type=int, default=1000000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    from tehmm_amd import _lib, compare
    import compare_ref as cr
    if _lib.device_count() < 1:
        sys.exit("compare_bench: no GPU")
    n, L = args.preds, args.labels
    t0 = time.time()
    truth, pred = make_lists(n, args.truth_len, L, args.seed)
    lines = ["compare_bench: %d one-base preds against %d truth intervals (mean %.0f bases), %d labels, threshold %.2f, "
             "repeats = %d" % (len(pred), len(truth), n / float(len(truth)), L, args.threshold, args.repeats),
             "lists built on the host in %.1f s" % (time.time() - t0)]
    calls = [
        ("base", lambda a, b: compare.baseConfusion(a, b, L, first=True)),
        ("intervals, truth side (long pred ranges)", lambda a, b: compare.intervalsOneSided(
            a, b, L, args.threshold, False, True, first=True)),
        ("intervals, pred side", lambda a, b: compare.intervalsOneSided(b, a, L, args.threshold, False, True,
                                                                        first=True)),
        ("merge of the preds", lambda a, b: compare.mergeRuns(b, L)),
    ]
    small = (head(truth, min(n, 1 << 16)), head(pred, min(n, 1 << 16)))
    for name, call in calls:
        call(*small)                                       # warm-up: code objects
        call(truth, pred)                                  # and this shape's device blocks
        walls, passes = [], []
        for _ in range(args.repeats):
            t0 = time.time()
            call(truth, pred)
            walls.append(time.time() - t0)
            passes.append(compare.lastTiming())
        lines.append("%s: whole call, wall-clock (median of %d): %.1f ms   [%s]" % (
            name, args.repeats, 1e3 * float(np.median(walls)), ", ".join("%.1f" % (1e3 * w) for w in walls)))
        for i, (pname, _) in enumerate(passes[0]):
            v = [p[i][1] for p in passes if len(p) == len(passes[0])]
            lines.append("  %-12s %9.3f ms (median; min %.3f, max %.3f)" % (pname, float(np.median(v)), min(v), max(v)))
    # the plain-Python walks on a sample, and the device against them there
    nref = min(args.ref_bases, n)
    ht, hp = head(truth, nref), head(pred, nref)
    tt, tp = tuples(ht), tuples(hp)
    t0 = time.time()
    cells = cr.base_confusion(tt, tp, 3)
    dt_base = time.time() - t0
    t0 = time.time()
    stats = cr.compare_intervals_one_sided(tt, tp, 3, args.threshold, False, True)[0]
    dt_int = time.time() - t0
    conf = compare.baseConfusion(ht, hp, L)
    n_hit = compare.intervalsOneSided(ht, hp, L, args.threshold, False, True)[0]
    ok = all(conf[a, b] == v for (a, b), v in cells.items()) and int(conf.sum()) == nref and \
        all(int(n_hit[k]) == v[0] for k, v in stats.items())
    lines.append("plain-Python walks (tests/compare_ref.py, piece by piece, not the reference's loop per base) on the "
                 "first %d bases: base %.2f s, intervals %.2f s; scaled to %d bases: %.0f s and %.0f s (extrapolated "
                 "from the sample); device %s there" % (nref, dt_base, dt_int, n, dt_base * n / nref, dt_int * n / nref,
                                                        "agrees" if ok else "DISAGREES"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    if not ok:
        sys.exit("compare_bench: the device disagrees with the plain-Python walks")


if __name__ == "__main__":
    main()
