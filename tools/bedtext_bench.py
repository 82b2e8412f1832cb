"""The states file of teHmmEval, written two ways from one evaluated batch (results: profiles/bedtext_bench.txt).

  python tools/bedtext_bench.py [--rows 10000000 [100000000 ...]] [--repeats 3] [--dir /dev/shm] [--out FILE]

Shape: 35 states x 10 tracks (config 2), --rows rows in 10 tables, Viterbi path on the device, state names of 6 to 10
bytes.  Both routes write the same file (compared once) to a tmpfs path:
 (a) the host route: HipBatch.paths() (8 B/row over PCIe), output.bedCoords (16 B/row) and tehmm_write_bed (one thread,
     snprintf per row), table by table -- what output.statesToBed does;
 (b) output.writeBatchBed: lines formatted on the device in stripes, copied back under the fwrite of the stripe before.
One warm-up run of each, then --repeats timed runs; wall-clock median and min..max, rows/s, and the ratio of the medians.
For (b) also the device passes (tehmm_bed_text_last_timing, summed over the stripes) against their byte floor -- the
8 B/row column read plus the text written -- and the host's time in fwrite and waiting for copies."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return "median %.3f  min %.3f  max %.3f  (n=%d)" % (np.median(xs), xs.min(), xs.max(), len(xs))


class Table(object):
    def __init__(self, chrom, start, rows):
        self.chrom, self.start, self.rows = chrom, start, rows

    def __len__(self):
        return self.rows

    def getChrom(self):
        return self.chrom

    def getStart(self):
        return self.start

    def getEnd(self):
        return self.start + self.rows

    def getSegmentOffsets(self):
        return None

    def getMaskRunningOffsets(self):
        return None


def run_case(rows, args, out):
    from tehmm_amd import output, synth
    from tehmm_amd.engine import HipBatch, HipModel
    model = synth.make_model(35, seed=7, stay=0.99)
    block = synth.random_obs(model, min(rows, 2_000_000), seed=3)
    obs = np.ascontiguousarray(np.tile(block, ((rows + len(block) - 1) // len(block), 1))[:rows])
    offs = np.linspace(0, rows, 11).astype(np.int64)
    tables = [Table("chr%d" % (t + 1), 1000 * t, int(offs[t + 1] - offs[t])) for t in range(10)]
    names = ["state%d" % (i * i * 37) for i in range(35)]
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs, symbols_per_track=model.symbols_per_track)
    hb = HipBatch(obs, offs)
    hm.eval(hb, viterbi=True, posterior=False, use_ratios=False)
    out("== %d rows in %d tables, 35 states x %d tracks; evaluation %s ms" % (
        rows, len(tables), obs.shape[1], ", ".join("%s %.1f" % kv for kv in hb.timing().items())))
    pa, pb = os.path.join(args.dir, "bedtext_a.bed"), os.path.join(args.dir, "bedtext_b.bed")

    def route_a():
        open(pa, "w").close()
        for t, table in enumerate(tables):
            output.statesToBed(table, hb.paths(int(offs[t]), int(offs[t + 1])), pa, stateNames=names)

    def route_b():
        output.writeBatchBed(pb, hb, output.SRC_VITERBI, tables, names=names)

    ta, tb, passes = [], [], []
    for it in range(args.repeats + 1):
        t0 = time.perf_counter()
        route_a()
        t1 = time.perf_counter()
        route_b()
        t2 = time.perf_counter()
        if it == 0:
            with open(pa, "rb") as f, open(pb, "rb") as g:
                assert f.read() == g.read(), "the two routes wrote different files"
        else:
            ta.append(t1 - t0)
            tb.append(t2 - t1)
            passes.append(dict(output.lastBedTextTiming()))
    n_rows, n_bytes, host_rows = output.lastBedTextCounters()
    out("(a) paths + bedCoords + tehmm_write_bed, s:  %s   -> %.1f x1e6 rows/s" % (stats(ta), rows / np.median(ta) / 1e6))
    out("(b) writeBatchBed, s:                        %s   -> %.1f x1e6 rows/s" % (stats(tb), rows / np.median(tb) / 1e6))
    out("    ratio of the medians (a) / (b): %.2fx; file %.1f MB, %d rows, %d formatted by the host"
        % (np.median(ta) / np.median(tb), n_bytes / 1e6, n_rows, host_rows))
    med = {k: float(np.median([p[k] for p in passes])) for k in passes[0]}
    dev = sum(med.get(k, 0.0) for k in ("measure", "scan", "patch", "emit"))
    floor_bytes = 8 * n_rows + n_bytes
    out("    device passes, ms (medians): %s" % "  ".join("%s %.2f" % (k, med[k]) for k in med))
    out("    measure + scan + emit %.2f ms for %.1f MB read + written: %.0f GB/s (HBM floor at 4 TB/s: %.2f ms)"
        % (dev, floor_bytes / 1e6, floor_bytes / 1e9 / (dev * 1e-3), floor_bytes / 4e12 * 1e3))
    out("    host: fwrite %.0f ms (%.2f GB/s into the page cache), waiting for copies %.0f ms, whole call %.0f ms"
        % (med["fwrite"], n_bytes / 1e9 / (med["fwrite"] * 1e-3), med["copy_wait"], med["wall"]))
    hb.close()
    hm.close()
    os.remove(pa)
    os.remove(pb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[10_000_000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from tehmm_amd import build
    build.build()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    for rows in args.rows:
        run_case(rows, args, out)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
