#!/usr/bin/env python3
"""Times the TSD finder (tehmm_tsd_find) and the overlap clean-up (tehmm_remove_overlaps) at genome scale: --elements
candidate elements spread evenly over one seeded sequence of --bases bases, the tool's default options.

For each call it reports the per-pass device times (HIP events, tehmm_tsd_last_timing), the share of them that is
upload, and the wall-clock of the whole call; then it runs the plain-Python statement (tests/tsd_ref.py) on the first
--ref-elements elements and checks that the device agrees with it there.

    python tools/tsd_bench.py [--bases 1000000000] [--elements 10000000] [--repeats 3] [--out profiles/tsd.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_input(n_bases, n_elements, seed):
    """(bases uint8 [n_bases], start, end int64 [n_elements]): uniform acgt with a tenth of it soft-masked, elements
    of 10 to 400 bases in slots of n_bases / n_elements"""
    rs = np.random.RandomState(seed)
    table = np.frombuffer(b"acgtACGT", dtype=np.uint8)
    bases = np.empty(n_bases, dtype=np.uint8)
    for a in range(0, n_bases, 1 << 24):                   # in pieces: the index arrays of a whole genome are large
        m = min(1 << 24, n_bases - a)
        pick = rs.randint(0, 4, size=m, dtype=np.uint8)
        pick[rs.randint(0, 10, size=m, dtype=np.uint8) == 0] += 4
        bases[a:a + m] = table[pick]
    slot = n_bases // n_elements
    start = np.arange(n_elements, dtype=np.int64) * slot + rs.randint(0, max(slot // 2, 1), size=n_elements)
    end = start + rs.randint(10, 401, size=n_elements)
    return bases, start, end


def report(lines, name, call, timing, repeats):
    call()                                             # warm-up: code objects and this shape's device blocks
    walls, passes = [], []
    for _ in range(repeats):
        t0 = time.time()
        call()
        walls.append(time.time() - t0)
        passes.append(timing())
    lines.append("%s: whole call, wall-clock (median of %d): %.1f ms   [%s]" % (
        name, repeats, 1e3 * float(np.median(walls)), ", ".join("%.1f" % (1e3 * w) for w in walls)))
    med = []
    for i, (pname, _) in enumerate(passes[0]):
        v = [p[i][1] for p in passes if len(p) == len(passes[0])]
        med.append((pname, float(np.median(v))))
        lines.append("  %-12s %9.3f ms (median; min %.3f, max %.3f)" % (pname, med[-1][1], min(v), max(v)))
    total = sum(m for _, m in med)
    up = sum(m for p, m in med if p == "upload")
    lines.append("  upload is %.0f %% of the %.1f ms between the first and the last event" % (
        100.0 * up / max(total, 1e-9), total))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=1000000000)
    ap.add_argument("--elements", type=int, default=10000000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-elements", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    from tehmm_amd import _lib, tsd
    import tsd_ref as tr
    if _lib.device_count() < 1:
        sys.exit("tsd_bench: no GPU")
    t0 = time.time()
    bases, start, end = make_input(args.bases, args.elements, args.seed)
    n = len(start)
    offsets = np.asarray([0, len(bases)], dtype=np.int64)
    index = np.zeros(n, dtype=np.int32)
    lines = ["tsd_bench: %d elements on %d bases, options of the tool (min 4, max 6, left 7, right 7, overlap 3), "
             "repeats = %d" % (n, len(bases), args.repeats), "input built on the host in %.1f s" % (time.time() - t0)]
    found = {}

    def find():
        found["counts"], found["cols"] = tsd.findMatches(bases, offsets, index, start, end)
    report(lines, "tehmm_tsd_find", find, tsd.lastTiming, args.repeats)
    counts, cols = found["counts"], found["cols"]
    lines.append("  %d of %d elements have a TSD pair" % (int(counts.sum()), n))
    # the clean-up on what the finder found: both TSDs of every pair, sorted by start (one chromosome)
    s = np.concatenate([cols[0], cols[3]])
    e = np.concatenate([cols[1], cols[4]])
    order = np.argsort(s, kind="stable")
    s, e = s[order], e[order]
    chrom = np.zeros(len(s), dtype=np.int32)
    if len(s):
        kept = {}

        def clean():
            kept["idx"], kept["start"] = tsd.removeOverlapsArrays(chrom, s, e)
        report(lines, "tehmm_remove_overlaps on the %d TSDs" % len(s), clean, tsd.lastTiming, args.repeats)
        lines.append("  %d intervals kept" % len(kept["idx"]))
    # the plain-Python statement on a sample, and the device against it there
    m = min(args.ref_elements, n)
    hi = int(end[m - 1]) + 64 if m < n else len(bases)
    seqs = [("c", bases[:hi].tobytes())]
    ivs = [("c", int(a), int(b)) for a, b in zip(start[:m], end[:m])]
    t0 = time.time()
    want = tr.find_tsds(seqs, ivs)
    dt = time.time() - t0
    k = int(counts[:m].sum())
    got = [x for r in range(k) for x in (("c", int(cols[0][r]), int(cols[1][r]), "L_TSD", int(cols[2][r])),
                                         ("c", int(cols[3][r]), int(cols[4][r]), "R_TSD", int(cols[5][r])))]
    ok = got == want
    lines.append("plain-Python statement (tests/tsd_ref.py) on the first %d elements: %.2f s, %.1f us per element; "
                 "device %s there" % (m, dt, 1e6 * dt / m, "agrees" if ok else "DISAGREES"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    if not ok:
        sys.exit("tsd_bench: the device disagrees with the plain-Python statement")


if __name__ == "__main__":
    main()
