#!/usr/bin/env python3
"""Times the mask interval algebra at genome scale, at array level: --chroms chromosome-wide intervals, --masks masks
and --intervals predicted intervals that tile the spaces between the masks.

  cutOutMaskIntervals        tehmm_intervals_merge on the mask records (--delMask style length filter) and
                             tehmm_intervals_subtract of the kept masks from the chromosome-wide intervals;
  interpolateMaskedRegions   tehmm_mask_fill of every mask from the prediction, and tehmm_intervals_intersect of the
                             prediction plus the fills with the chromosome-wide scope.

For each call it prints the per-pass device times (HIP events, tehmm_masking_last_timing) next to the bytes the pass
must move at least (every list read once, every output written once) and the time those bytes take at 6.3 TB/s, the
copy rate measured on an MI355X.  There is no pass/fail threshold.

    python tools/masking_bench.py [--chroms 10] [--masks 1000000] [--intervals 10000000] [--out profiles/masking_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_MS = 6.3e9      # 6.3 TB/s
ROW = 4 + 8 + 8               # bytes of one interval: int32 chrom, int64 start, int64 end


def make_input(n_chroms, n_masks, n_intervals, seed):
    """(masks, region, prediction, labels): column triples.  Masks: 1 to 400 bases, one in a hundred 6 000 to 50 000,
    50 to 3 000 bases apart.  Prediction: every space between two masks tiled by n_intervals / n_masks intervals."""
    rs = np.random.RandomState(seed)
    per = n_masks // n_chroms
    split = max(n_intervals // max(n_masks, 1), 1)
    mc, ms, me, pc, ps, pe, rend = [], [], [], [], [], [], []
    for c in range(n_chroms):
        gap = rs.randint(50, 3001, size=per).astype(np.int64)
        size = rs.randint(1, 401, size=per).astype(np.int64)
        big = rs.randint(0, 100, size=per) == 0
        size[big] = rs.randint(6000, 50001, size=int(big.sum()))
        end = np.cumsum(gap + size)
        start = end - size
        mc.append(np.full(per, c, dtype=np.int32))
        ms.append(start)
        me.append(end)
        a = np.concatenate([[0], end[:-1]])                   # the space before every mask
        pts = a[:, None] + ((start - a)[:, None] * np.arange(split + 1, dtype=np.int64)[None, :]) // split
        pc.append(np.full(per * split, c, dtype=np.int32))
        ps.append(pts[:, :-1].reshape(-1))
        pe.append(pts[:, 1:].reshape(-1))
        rend.append(int(end[-1]) + 100)
    masks = (np.concatenate(mc), np.concatenate(ms), np.concatenate(me))
    pred = (np.concatenate(pc), np.concatenate(ps), np.concatenate(pe))
    keep = pred[2] > pred[1]
    pred = tuple(x[keep] for x in pred)
    region = (np.arange(n_chroms, dtype=np.int32), np.zeros(n_chroms, dtype=np.int64), np.asarray(rend, dtype=np.int64))
    labels = rs.randint(0, 8, size=len(pred[0])).astype(np.int32)
    return masks, region, pred, labels


def report(lines, name, call, timing, repeats, floor_bytes):
    call()                                             # warm-up: code objects and this shape's device blocks
    walls, passes = [], []
    for _ in range(repeats):
        t0 = time.time()
        call()
        walls.append(time.time() - t0)
        passes.append(timing())
    lines.append("%s: whole call, wall-clock (median of %d): %.1f ms" % (name, repeats, 1e3 * float(np.median(walls))))
    kernels = 0.0
    for i, (pname, _) in enumerate(passes[0]):
        v = [p[i][1] for p in passes if len(p) == len(passes[0])]
        med = float(np.median(v))
        if pname not in ("upload", "download"):
            kernels += med
        lines.append("  %-12s %9.3f ms (median; min %.3f, max %.3f)" % (pname, med, min(v), max(v)))
    floor = floor_bytes / HBM_BYTES_PER_MS
    lines.append("  kernel passes %.3f ms; the lists are %.1f MB, %.3f ms at 6.3 TB/s: %.1f x the memory floor" % (
        kernels, floor_bytes / 1e6, floor, kernels / max(floor, 1e-9)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chroms", type=int, default=10)
    ap.add_argument("--masks", type=int, default=1000000)
    ap.add_argument("--intervals", type=int, default=10000000)
    ap.add_argument("--delMask", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    from tehmm_amd import _lib, masking
    if _lib.device_count() < 1:
        sys.exit("masking_bench: no GPU")
    t0 = time.time()
    masks, region, pred, labels = make_input(args.chroms, args.masks, args.intervals, args.seed)
    nM, nR, nI = len(masks[0]), len(region[0]), len(pred[0])
    lines = ["masking_bench: %d chromosome-wide intervals, %d masks, %d predicted intervals, delMask = maxLen = %d, "
             "repeats = %d" % (nR, nM, nI, args.delMask, args.repeats),
             "input built on the host in %.1f s" % (time.time() - t0)]
    out = {}

    def merge():
        out["long"] = masking.mergeArrays(*masks, minLen=args.delMask + 1)
    report(lines, "cutOutMaskIntervals 1/2: tehmm_intervals_merge", merge, masking.lastTiming, args.repeats,
           ROW * nM + ROW * len(masking.mergeArrays(*masks, minLen=args.delMask + 1)[0]))
    lines.append("  %d of %d masks are longer than %d" % (len(out["long"][0]), nM, args.delMask))

    def subtract_long():
        out["cut"] = masking.subtractArrays(region, out["long"])
    report(lines, "cutOutMaskIntervals 2/2: tehmm_intervals_subtract, the long masks", subtract_long,
           masking.lastTiming, args.repeats, ROW * (nR + len(out["long"][0])) + 24 * (len(out["long"][0]) + nR))
    lines.append("  %d pieces" % len(out["cut"][0]))

    def subtract_all():
        out["cut_all"] = masking.subtractArrays(region, masks)
    report(lines, "cutOutMaskIntervals (minLength -1): tehmm_intervals_subtract, every mask", subtract_all,
           masking.lastTiming, args.repeats, ROW * (nR + nM) + 24 * (nM + nR))
    lines.append("  %d pieces from %d intervals: %d pieces per interval, one lane each" % (
        len(out["cut_all"][0]), nR, len(out["cut_all"][0]) // nR))
    one = np.zeros(8, dtype=np.uint8)
    one[3] = 1

    def fill():
        out["fill"] = masking.fillArrays(masks, pred, labels, 8, None, one, False, args.delMask)
    report(lines, "interpolateMaskedRegions 1/2: tehmm_mask_fill", fill, masking.lastTiming, args.repeats,
           ROW * nM + 4 * nM + (ROW + 4) * nI)
    got = out["fill"]
    lines.append("  %d masks filled with a state, %d with the default, %d too long" % (
        int((got >= 0).sum()), int((got == masking.DEFAULT).sum()), int((got == masking.SKIPPED).sum())))
    # the prediction plus the fills, sorted, inside the scope
    kept = got != masking.SKIPPED
    c = np.concatenate([pred[0], masks[0][kept]])
    s = np.concatenate([pred[1], masks[1][kept]])
    e = np.concatenate([pred[2], masks[2][kept]])
    order = np.lexsort((s, c))
    rows_ = (c[order], s[order], e[order])

    def intersect():
        out["scope"] = masking.intersectArrays(rows_, region)
    report(lines, "interpolateMaskedRegions 2/2: tehmm_intervals_intersect with the scope", intersect,
           masking.lastTiming, args.repeats, ROW * (len(c) + nR) + 24 * len(c))
    lines.append("  %d rows" % len(out["scope"][0]))
    # every row lies inside its chromosome's interval, and every chromosome gives one piece more than it has masks
    ok = len(out["scope"][0]) == len(c) and len(out["cut_all"][0]) == nM + nR
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    if not ok:
        sys.exit("masking_bench: unexpected row counts")


if __name__ == "__main__":
    main()
