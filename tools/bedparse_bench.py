"""Reading BED text back: the interpreter's record loop against the device parse.

  python tools/bedparse_bench.py [--rows 10000000] [--segments 1000000] [--parent DIR] [--dir /dev/shm] [--out FILE]

(a) the states file of --rows rows that tools/bedtext_bench.py writes (35 state names, 10 tables; written here by the
    same writeBatchBed call) as a data file on tmpfs: BedFile construction, readBedIntervals(sort=True), codes(3);
(b) a segment file of --segments lines over 10 tables through loadTrackData(segmentIntervals=...), as a list of tuples
    and as columns;
(c) parseBed of growing prefixes of (a)'s file by both routes: the break-even size.

The baseline of (a) and (b) is --parent: the root of a checkout of the parent commit (only its tehmm_amd/*.py are
needed; it loads this tree's library through TEHMM_HIP_LIB), run in a process of its own, so that the comparison does
not rest on the tree under test.  Without --parent the host route of THIS tree (TEHMM_BED_PARSE=0) is timed instead and
the output says so.  Every timing runs in a fresh child process; nothing here asserts a speed."""
import argparse
import json
import os
import subprocess
import sys
import time
import xml.etree.ElementTree as ET

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


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


def write_states_file(rows, path):
    """the file of tools/bedtext_bench.py: 35 states x 10 tracks, the Viterbi path of `rows` rows in 10 tables"""
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
    output.writeBatchBed(path, hb, output.SRC_VITERBI, tables, names=names)
    hb.close()
    hm.close()


def write_segment_case(n_segments, folder):
    rng = np.random.default_rng(1)
    per = n_segments // 10
    intervals, seg, track = [], [], []
    for t in range(10):
        c, start = "chr%d" % (t % 5 + 1), 10_000_000 * (t // 5)
        lens = rng.integers(1, 6, per)
        s = start + np.concatenate([[0], np.cumsum(lens)])
        seg.append("".join("%s\t%d\t%d\n" % (c, a, b) for a, b in zip(s[:-1].tolist(), s[1:].tolist())))
        track.append("".join("%s\t%d\t%d\t%s\n" % (c, a, a + 40, "xyz"[a % 3]) for a in s[:-1:16].tolist()))
        intervals.append((c, start, int(s[-1])))
    paths = [os.path.join(folder, n) for n in ("bp_seg.bed", "bp_track.bed", "bp_tracks.xml")]
    open(paths[0], "w").write("".join(seg))
    open(paths[1], "w").write("".join(track))
    root = ET.Element("teModelConfig")
    root.append(ET.Element("track", dict(name="a", path=paths[1], distribution="multinomial", valCol="3")))
    ET.ElementTree(root).write(paths[2])
    return paths, intervals


# ---- the timed work, in a child process ---------------------------------------------------------------------------------
def worker(job):
    sys.path.insert(0, job["root"])
    from tehmm_amd import trackIO
    out = dict()
    clock = time.perf_counter
    if os.environ.get("TEHMM_BED_PARSE") == "1":      # the process's first device call is not part of any timing
        warm = os.path.join(os.path.dirname(job.get("path") or job.get("seg")), "bp_warm.bed")
        open(warm, "w").write("c\t1\t2\tn\n")
        trackIO.BedFile(warm).codes(3)
        os.remove(warm)
    if job["what"] == "states":
        t0 = clock()
        bed = trackIO.BedFile(job["path"])
        t1 = clock()
        code, values = bed.codes(3)
        t2 = clock()
        ivs = trackIO.readBedIntervals(job["path"], sort=True)
        t3 = clock()
        out.update(bedfile=t1 - t0, codes=t2 - t1, intervals_sorted=t3 - t2, records=len(bed.start), values=len(values),
                   check=[int(bed.start.sum()), int(code.sum()), sum(iv[1] for iv in ivs[::1009]),
                          "".join(iv[0] for iv in ivs[::100003])])
        if hasattr(trackIO, "parseBed"):
            t0 = clock()
            cols = trackIO.parseBed(job["path"])
            t1 = clock()
            out.update(route=cols.route, parse=t1 - t0)
            if cols.route == "device":
                out.update(timing=trackIO.parseTiming(), counters=trackIO.parseCounters(), bytes=int(len(cols.raw)))
                t0 = clock()
                trackIO._read_pinned(job["path"])
                out["read_pinned"] = clock() - t0
    elif job["what"] == "segments":
        from tehmm_amd.track import TrackData
        t0 = clock()
        if job["columns"]:
            segments = trackIO.readBedColumns(job["seg"], sort=True)
        else:
            segments = trackIO.readBedIntervals(job["seg"], sort=True)
        t1 = clock()
        td = TrackData()
        td.loadTrackData(job["xml"], [tuple(iv) for iv in job["intervals"]], segmentIntervals=segments)
        t2 = clock()
        out.update(read=t1 - t0, load=t2 - t1,
                   check=[int(np.asarray(t.getSegmentOffsets()).sum()) for t in td.getTrackTableList()])
    elif job["what"] == "parse":
        best = None
        for _ in range(3):
            t0 = clock()
            cols = trackIO.parseBed(job["path"])
            cols.start, cols.end, cols.chromCode
            dt = clock() - t0
            cols.close()
            best = dt if best is None else min(best, dt)
        out.update(route=cols.route, parse=best)
    print("RESULT " + json.dumps(out))


def run(job, env):
    e = dict(os.environ)
    e.update(env)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(job)], env=e,
                       stdout=subprocess.PIPE, universal_newlines=True, check=True)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--segments", type=int, default=1_000_000)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(json.loads(args.worker))
    sys.path.insert(0, ROOT)
    from tehmm_amd import _lib, build
    build.build()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    lib = {"TEHMM_HIP_LIB": _lib.LIB_PATH}
    if args.parent and os.path.isdir(os.path.join(args.parent, "tehmm_amd")):
        base_root, base_env, base_name = os.path.abspath(args.parent), dict(lib), "parent checkout"
    else:
        base_root, base_env, base_name = ROOT, dict(lib, TEHMM_BED_PARSE="0"), "host route of THIS tree (no --parent)"
    dev_env = dict(lib, TEHMM_BED_PARSE="1")
    # ---- (a) ------------------------------------------------------------------------------------------------------------
    states = os.path.join(args.dir, "bp_states.bed")
    write_states_file(args.rows, states)
    size = os.path.getsize(states)
    out("== (a) states file: %d rows, %.1f MB, on %s" % (args.rows, size / 1e6, args.dir))
    base = run(dict(what="states", root=base_root, path=states), base_env)
    dev = run(dict(what="states", root=ROOT, path=states), dev_env)
    assert base["check"] == dev["check"] and base["records"] == dev["records"], "the routes disagree"
    out("baseline = %s; device route: %s" % (base_name, dev.get("route")))
    for key, label in (("bedfile", "columns + BedFile"), ("intervals_sorted", "readBedIntervals(sort=True)"),
                       ("codes", "codes(3)")):
        out("  %-28s baseline %8.3f s   device route %8.3f s   %6.1fx" % (label, base[key], dev[key], base[key] / dev[key]))
    if dev.get("route") == "device":
        t = dev["timing"]
        kern = sum(ms for name, ms in t if name not in ("upload",))
        R = dev["counters"]["records"]
        floor = (dev["bytes"] + 86 * R) / 4e12 * 1e3
        out("  device parse (parseBed %.3f s): read into the pinned block %.3f s; passes, ms: %s"
            % (dev["parse"], dev["read_pinned"], "  ".join("%s %.2f" % (n, ms) for n, ms in t)))
        out("  kernels %.2f ms = %.1f x the floor of %.2f ms (text once + 86 B of tables per record at 4 TB/s); the rest of"
            " parseBed is copy-back and Python assembly: %.3f s" % (kern, kern / floor, floor,
                                                                    dev["parse"] - dev["read_pinned"] - sum(ms for _, ms in t) / 1e3))
        out("  counters: %s" % dev["counters"])
    # ---- (b) ------------------------------------------------------------------------------------------------------------
    (seg, _, xml), intervals = write_segment_case(args.segments, args.dir)
    out("== (b) segment file of %d lines over 10 tables through loadTrackData" % args.segments)
    job = dict(what="segments", seg=seg, xml=xml, intervals=intervals)
    asList = run(dict(job, root=base_root, columns=False), base_env)
    asCols = run(dict(job, root=ROOT, columns=True), dev_env)
    assert asList["check"] == asCols["check"], "the routes disagree"
    out("  as a list (baseline):  read %.3f s, loadTrackData %.3f s" % (asList["read"], asList["load"]))
    out("  as columns (device):   read %.3f s, loadTrackData %.3f s   %.1fx over both"
        % (asCols["read"], asCols["load"], (asList["read"] + asList["load"]) / (asCols["read"] + asCols["load"])))
    # ---- (c) ------------------------------------------------------------------------------------------------------------
    out("== (c) parseBed + start / end / chromosome codes of prefixes of (a)'s file, best of 3, host route against device")
    text = open(states, "rb").read(64 << 20)
    even = None
    for kb in (16, 64, 256, 1024, 4096, 16384):
        cut = text.rfind(b"\n", 0, kb << 10) + 1
        p = os.path.join(args.dir, "bp_prefix.bed")
        open(p, "wb").write(text[:cut])
        h = run(dict(what="parse", root=ROOT, path=p), dict(lib, TEHMM_BED_PARSE="0"))
        d = run(dict(what="parse", root=ROOT, path=p), dev_env)
        out("  %6d KiB: host %.4f s, device %.4f s (%s)" % (kb, h["parse"], d["parse"], d["route"]))
        if even is None and d["parse"] < h["parse"]:
            even = kb
    out("  the device route wins from %s on; the default threshold is 1024 KiB (arithmetic, see DESIGN.md 5u)"
        % ("%d KiB" % even if even else "no size tried"))
    for p in (states, seg, xml, os.path.join(args.dir, "bp_track.bed"), os.path.join(args.dir, "bp_prefix.bed")):
        if os.path.exists(p):
            os.remove(p)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
