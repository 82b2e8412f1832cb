#!/usr/bin/env python3
"""Times the device call of track scaling (tehmm_track_rows_won) at genome scale: --rows rows of --tracks numeric
tracks sharing --records seeded records (those of tools/trackio_bench.py without its sequence tracks: sorted starts,
lengths of tens of bases with one in a thousand up to a million, and in the first track one record over the whole row
space listed first).

It reports the wall-clock of the whole call and the per-pass device times (HIP events, tehmm_trackio_last_timing:
upload, tree, count, download), then, in the same run and on the same records, those of tehmm_load_tracks_u8, whose
k_trk_paint does the same walk and stores a byte per row and track: the yardstick for k_trk_rows_won, which stores far
less and should not be slower.  The float paint (tehmm_load_tracks_f32) is timed on the first track alone (a float per
row).  Then it counts the first --ref-rows rows with the plain-Python statement (tests/scaling_ref.py) and checks
that the device agrees with it there, and that rows won and uncovered rows add up to the rows of every track.

    python tools/scaling_bench.py [--rows 250000000] [--tracks 10] [--records 2500000] [--out profiles/scaling_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(call, repeats, last_timing, names):
    call()                                                    # warm-up: code objects and this shape's device blocks
    walls, passes = [], []
    for _ in range(repeats):
        t0 = time.time()
        call()
        walls.append(time.time() - t0)
        passes.append(dict(last_timing()))
    med = dict((n, float(np.median([p[n] for p in passes]))) for n in names)
    lines = ["whole call, wall-clock (median of %d): %.1f ms   [%s]" % (
        repeats, 1e3 * float(np.median(walls)), ", ".join("%.1f" % (1e3 * w) for w in walls))]
    for n in names:
        v = [p[n] for p in passes]
        lines.append("  %-9s %10.3f ms (median; min %.3f, max %.3f)" % (n, med[n], min(v), max(v)))
    return med, lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=250000000)
    ap.add_argument("--tracks", type=int, default=10)
    ap.add_argument("--records", type=int, default=2500000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-rows", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    from tehmm_amd import _lib, trackIO
    import scaling_ref as sr
    from trackio_bench import make_tracks
    if _lib.device_count() < 1:
        sys.exit("scaling_bench: no GPU")
    T, K = args.rows, args.tracks
    t0 = time.time()
    tracks = make_tracks(trackIO, T, K, args.records, args.seed, n_seq=0)
    n_rec = sum(len(t.start) for t in tracks)
    lines = ["scaling_bench: %d rows x %d numeric tracks, %d records, the first of them over all rows, repeats = %d" % (
        T, K, n_rec, args.repeats), "input built on the host in %.1f s" % (time.time() - t0)]
    out = {}

    def count():
        out["won"], out["uncovered"] = trackIO.rowsWon(T, tracks)
    won_ms, text = timed(count, args.repeats, trackIO.lastTiming, ("upload", "tree", "count", "download"))
    lines += ["tehmm_track_rows_won: " + text[0]] + text[1:]

    def paint():
        out["data"] = None                                    # one table at a time on the host
        out["data"] = trackIO.paintTracks(T, tracks)
    u8_ms, text = timed(paint, args.repeats, trackIO.lastTiming, ("upload", "tree", "paint", "download"))
    out["data"] = None
    lines += ["tehmm_load_tracks_u8 on the same records: " + text[0]] + text[1:]
    lines.append("k_trk_rows_won / k_trk_paint: %.3f ms / %.3f ms = %.2f (whole calls between their first and last "
                 "event: %.1f ms / %.1f ms)" % (won_ms["count"], u8_ms["paint"], won_ms["count"] / u8_ms["paint"],
                                                sum(won_ms.values()), sum(u8_ms.values())))

    first = trackIO.FloatTrack(-1.0, tracks[0].start, tracks[0].end, np.arange(len(tracks[0].start)) % 1000)

    def paint_f32():
        out["row"] = None
        out["row"] = trackIO.paintTracksFloat(T, [first])
    _, text = timed(paint_f32, args.repeats, trackIO.lastTiming, ("upload", "tree", "paint", "download"))
    out["row"] = None
    lines += ["tehmm_load_tracks_f32 on the first track (%d records): " % len(first.start) + text[0]] + text[1:]

    ok = all(int(w.sum()) + int(u) == T for w, u in zip(out["won"], out["uncovered"]))
    lines.append("rows won + uncovered rows = rows in every track: %s" % ("yes" if ok else "NO"))
    m = min(args.ref_rows, T)
    short = []
    for t in tracks:
        n = int(np.searchsorted(t.start, m, side="left"))
        short.append(trackIO.FloatTrack(0.0, t.start[:n], np.minimum(t.end[:n], m), np.zeros(n)))
    got_won, got_unc = trackIO.rowsWon(m, short)
    t0 = time.time()
    for k, t in enumerate(short):
        want_won, want_unc = sr.rows_won(m, t.start, t.end)
        ok = ok and np.array_equal(got_won[k], want_won) and int(got_unc[k]) == want_unc
    lines.append("plain-Python statement (tests/scaling_ref.py) on the first %d rows of every track: %.2f s; device %s "
                 "there" % (m, time.time() - t0, "agrees" if ok else "DISAGREES"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    if not ok:
        sys.exit("scaling_bench: the device disagrees with the plain-Python statement")


if __name__ == "__main__":
    main()
