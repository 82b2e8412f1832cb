#!/usr/bin/env python3
"""Times one segmentation call (tehmm_segment_offsets_u8) at genome scale: T rows, K tracks, one table.

Data: seeded run-structured tracks -- every track keeps its value from one row to the next with probability 0.98
(run lengths are geometric; tehmm_amd/synth samples from an HMM row by row and is test-sized).  For --comp first and
prev at thresh 1 it reports the per-pass device times (HIP events, tehmm_segment_last_timing), the wall-clock of the
whole call, stripes re-walked / stripes and the segments found; then it times the plain-Python statement of the
reference's loop (tests/segmenter_ref.py) on the first --ref-rows rows of the same data and checks that the device
agrees with it there.

    python tools/segmenter_bench.py [--rows 100000000] [--tracks 10] [--repeats 3] [--out profiles/segmenter_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_data(T, K, keep, seed):
    from tehmm_amd import _lib
    rs = np.random.RandomState(seed)
    data = _lib.pinned_empty((T, K), np.uint8)          # pinned: the upload is one DMA
    for k in range(K):
        n = int(T * (1.0 - keep) * 1.05) + 1024
        lens = rs.geometric(1.0 - keep, size=n)
        while lens.sum() < T:
            lens = np.concatenate([lens, rs.geometric(1.0 - keep, size=n)])
        vals = rs.randint(1, 5, size=len(lens)).astype(np.uint8)
        data[:, k] = np.repeat(vals, lens)[:T]
    return data


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100000000)
    ap.add_argument("--tracks", type=int, default=10)
    ap.add_argument("--keep", type=float, default=0.98)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-rows", type=int, default=1000000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    from tehmm_amd import _lib, segmenter
    import segmenter_ref as sr
    if _lib.device_count() < 1:
        sys.exit("segmenter_bench: no GPU")
    T, K = args.rows, args.tracks
    lines = ["segmenter_bench: T = %d rows, K = %d tracks, keep = %.2f, thresh = 1, stripe = %d rows, repeats = %d" % (
        T, K, args.keep, _lib.load().tehmm_segment_stripe_rows(), args.repeats)]
    t0 = time.time()
    data = make_data(T, K, args.keep, args.seed)
    lines.append("data built on the host in %.1f s (%.2f GB)" % (time.time() - t0, data.nbytes / 1e9))
    none = np.zeros(K, dtype=np.uint8)
    nref = min(args.ref_rows, T)
    for comp in ("first", "prev"):
        segmenter.segmentOffsets([data[:min(T, 1 << 20)]], none, none, thresh=1, comp=comp)      # warm-up: code objects
        segmenter.segmentOffsets([data], none, none, thresh=1, comp=comp)                        # and this shape's blocks
        walls, passes = [], []
        for _ in range(args.repeats):
            t0 = time.time()
            offs = segmenter.segmentOffsets([data], none, none, thresh=1, comp=comp, _cap=T)[0]
            walls.append(time.time() - t0)
            passes.append(segmenter.lastTiming())
        stripes, rewalked = segmenter.lastCounters()
        lines.append("--comp %s: %d segments (mean %.1f rows); stripes re-walked %d / %d = %.4f%%" % (
            comp, len(offs), T / float(len(offs)), rewalked, stripes, 100.0 * rewalked / max(stripes, 1)))
        lines.append("  whole call, wall-clock (median of %d): %.1f ms   [%s]" % (
            args.repeats, 1e3 * float(np.median(walls)), ", ".join("%.1f" % (1e3 * w) for w in walls)))
        for i, (name, _) in enumerate(passes[0]):
            v = [p[i][1] for p in passes if len(p) == len(passes[0])]
            lines.append("  %-10s %9.3f ms (median; min %.3f, max %.3f)" % (name, float(np.median(v)), min(v), max(v)))
        t0 = time.time()
        want = sr.segment_offsets(data[:nref], none, none, 1, comp)
        dt = time.time() - t0
        head = segmenter.segmentOffsets([data[:nref]], none, none, thresh=1, comp=comp)[0]
        lines.append("  plain-Python loop on the first %d rows: %.2f s (%.0f rows/s; %d segments; device %s)" % (
            nref, dt, nref / dt, len(want), "agrees" if np.array_equal(head, want) else "DISAGREES"))
        if not np.array_equal(head, want):
            print("\n".join(lines))
            sys.exit("segmenter_bench: the device disagrees with the plain-Python loop")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
