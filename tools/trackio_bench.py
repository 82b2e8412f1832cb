#!/usr/bin/env python3
"""Times the track paint (tehmm_load_tracks_u8) at genome scale: --rows rows of --tracks tracks, two of them sequence
tracks, the others sharing --records seeded records (sorted starts, lengths of tens of bases with one in a thousand up
to a million, and in the first track one record over the whole row space listed first).

It reports the per-pass device times (HIP events, tehmm_trackio_last_timing: upload, tree, paint, download), the
wall-clock of the whole call, and the kernels' share of their memory floor: (rows x tracks written + record bytes +
sequence bytes read) over the HBM bandwidth.  Then it paints the first --ref-rows rows with the plain-Python statement
(tests/trackio_ref.py) and checks that the device agrees with it there.

The issue's size is 10^9 rows x 10 tracks with 10^7 records: 10 GB of table on the device and again on the host.  The
defaults are a quarter of that in rows and records; pass --rows 1000000000 --records 10000000 where memory allows.

    python tools/trackio_bench.py [--rows 250000000] [--tracks 10] [--records 2500000] [--out profiles/trackio.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_MEASURED = 6.29e12      # bytes / s, float4 copy (the microarchitecture notes' measured figure; 8.0e12 is the spec)
HBM_SPEC = 8.0e12


def make_tracks(trackIO, T, K, n_records, seed, n_seq=2, full_span=True):
    rs = np.random.RandomState(seed)
    n_seq = min(n_seq, K)
    per = n_records // max(K - n_seq, 1)
    tracks = []
    for k in range(K - n_seq):
        start = np.sort(rs.randint(0, T, size=per, dtype=np.int64))
        length = rs.randint(1, 200, size=per).astype(np.int64)
        far = rs.randint(0, 1000, size=per) == 0
        length[far] = rs.randint(1000, 1000000, size=int(far.sum()))
        end = np.minimum(T, start + length)
        if k == 0 and full_span:
            start, end = np.concatenate([[0], start]), np.concatenate([[T], end])
        tracks.append(trackIO.RecordTrack(1, start, end, rs.randint(2, 200, size=len(start), dtype=np.uint8),
                                          rs.randint(2, 200, size=len(start), dtype=np.uint8)))
    table = np.frombuffer(b"acgtACGTnN", dtype=np.uint8)
    lut = np.ones(256, dtype=np.uint8)
    for i, c in enumerate(b"ACGTN"):
        lut[c] = lut[c + 32] = 2 + i
    for q in range(n_seq):
        b = np.empty(T, dtype=np.uint8)
        for a in range(0, T, 1 << 24):
            b[a:a + (1 << 24)] = table[rs.randint(0, len(table), size=min(1 << 24, T - a), dtype=np.uint8)]
        b[T - T // 50:] = 0                                   # the sequence ends before the rows do
        tracks.append(trackIO.SequenceTrack(1, b, lut))
    return tracks


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=250000000)
    ap.add_argument("--tracks", type=int, default=10)
    ap.add_argument("--records", type=int, default=2500000)
    ap.add_argument("--sequence-tracks", type=int, default=2)
    ap.add_argument("--full-span", type=int, default=1, help="0: no record over the whole row space in the first track")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-rows", type=int, default=200000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    from tehmm_amd import _lib, trackIO
    import trackio_ref as tr
    if _lib.device_count() < 1:
        sys.exit("trackio_bench: no GPU")
    T, K = args.rows, args.tracks
    t0 = time.time()
    tracks = make_tracks(trackIO, T, K, args.records, args.seed, args.sequence_tracks, bool(args.full_span))
    n_rec = sum(len(t.start) for t in tracks if t.kind == 0)
    n_seq = sum(1 for t in tracks if t.kind == 1)
    lines = ["trackio_bench: %d rows x %d tracks (%d of them sequence tracks), %d records%s, repeats = %d" % (
        T, K, n_seq, n_rec, ", the first of them over all rows" if args.full_span and n_seq < K else "", args.repeats), "input built on the host in %.1f s" % (time.time() - t0)]
    out = {}

    def call():
        out["data"] = None                                    # one table at a time on the host
        out["data"] = trackIO.paintTracks(T, tracks)
    call()                                                    # warm-up: code objects and this shape's device blocks
    walls, passes = [], []
    for _ in range(args.repeats):
        t0 = time.time()
        call()
        walls.append(time.time() - t0)
        passes.append(dict(trackIO.lastTiming()))
    lines.append("tehmm_load_tracks_u8: whole call, wall-clock (median of %d): %.1f ms   [%s]" % (
        args.repeats, 1e3 * float(np.median(walls)), ", ".join("%.1f" % (1e3 * w) for w in walls)))
    med = {}
    for name in ("upload", "tree", "paint", "download"):
        v = [p[name] for p in passes]
        med[name] = float(np.median(v))
        lines.append("  %-9s %10.3f ms (median; min %.3f, max %.3f)" % (name, med[name], min(v), max(v)))
    total = sum(med.values())
    lines.append("  upload and download are %.0f %% of the %.1f ms between the first and the last event" % (
        100.0 * (med["upload"] + med["download"]) / total, total))
    floor_bytes = T * K + n_rec * 18 + n_seq * T
    kernels = med["tree"] + med["paint"]
    lines.append("  kernels (tree + paint) %.3f ms for a floor of %.2f GB (%d x %d written, 18 bytes per record and %d x "
                 "%d sequence bytes read): %.2f TB/s" % (kernels, floor_bytes / 1e9, T, K, n_seq, T,
                                                        floor_bytes / (kernels * 1e-3) / 1e12))
    for name, bw in (("measured float4 copy, 6.29 TB/s", HBM_MEASURED), ("spec, 8.0 TB/s", HBM_SPEC)):
        floor_ms = 1e3 * floor_bytes / bw
        lines.append("  memory floor at the HBM rate (%s): %.3f ms; the kernels reach %.0f %% of it" % (
            name, floor_ms, 100.0 * floor_ms / kernels))
    # the plain-Python statement on the first rows, and the device against it there
    m = min(args.ref_rows, T)
    data = out["data"]
    t0 = time.time()
    ok = True
    for k, t in enumerate(tracks):
        if t.kind == 0:
            n = int(np.searchsorted(t.start, m, side="left"))
            want = tr.paint(m, t.fill, t.start[:n].tolist(), np.minimum(t.end[:n], m).tolist(), t.sym0[:n].tolist(),
                            t.sym[:n].tolist())
        else:
            want = np.where(t.bytes[:m] == 0, t.fill, t.lut[t.bytes[:m]])
        ok = ok and np.array_equal(data[:m, k], want)
    tail = data[T - 1000:]                                    # and the last rows of the sequence tracks: no base
    ok = ok and all((tail[:, k] == t.fill).all() for k, t in enumerate(tracks) if t.kind == 1)
    lines.append("plain-Python statement (tests/trackio_ref.py) on the first %d rows of every track: %.2f s; device %s "
                 "there" % (m, time.time() - t0, "agrees" if ok else "DISAGREES"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    if not ok:
        sys.exit("trackio_bench: the device disagrees with the plain-Python statement")


if __name__ == "__main__":
    main()
