#!/usr/bin/env python3
"""Golden vectors of the segmenter, by RUNNING THE REAL REFERENCE functions (recipe: make_golden_r3.py).

  segmenter   bin/segmentTracks.py: segmentTracks and isNewSegment (:200-277) are cut out of the reference at
              generation time, 2to3-converted in a scratch directory (the text never enters the repository) and
              executed on seeded tables through a stand-in table object.  Every case stores the data and, as
              one JSON text, the options, the BED the reference wrote and its --stats dict.
Re-run:  python tests/golden/make_golden_segmenter.py
"""
import json
import os
import subprocess
import sys
import tempfile
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TEHMM_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import segmenter_ref as sr          # noqa: E402  (only its seeded table maker)


def reference_functions(root):
    """segmentTracks / isNewSegment of the reference as py3 functions."""
    lines = open(os.path.join(REF, "bin", "segmentTracks.py")).read().splitlines(True)
    start = next(i for i, l in enumerate(lines) if l.startswith("def segmentTracks("))
    end = next(i for i, l in enumerate(lines) if l.startswith("def writeStats("))
    tmp = os.path.join(root, "_segment_block.py")
    open(tmp, "w").write(textwrap.dedent("".join(lines[start:end])))
    subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n", tmp],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    ns = {"np": np}
    exec(compile(open(tmp).read(), tmp, "exec"), ns)
    return ns["segmentTracks"]


class Table(object):
    def __init__(self, chrom, start, data):
        self.chrom, self.start, self.data = chrom, start, data

    def __len__(self):
        return len(self.data)

    def __getitem__(self, i):
        return self.data[i]

    def getStart(self):
        return self.start

    def getEnd(self):
        return self.start + len(self.data)

    def getChrom(self):
        return self.chrom


class Data(object):
    def __init__(self, tables):
        self.tables = tables

    def getTrackTableList(self):
        return self.tables


class Args(object):
    pass


# name, table lengths, K, options
CASES = [
    ("first_t1", [200], 4, dict(thresh=1)),
    ("first_t0", [150], 3, dict(thresh=0)),
    ("first_t2", [300], 6, dict(thresh=2)),
    ("prev_t1", [200], 4, dict(thresh=1, comp="prev")),
    ("prev_t0", [120], 5, dict(thresh=0, comp="prev")),
    ("cut_ignore", [250], 5, dict(thresh=2, cut=[0, 1, 0, 0, 0], ignore=[0, 0, 0, 1, 0])),
    ("cut_ignore_prev", [250], 5, dict(thresh=1, comp="prev", cut=[0, 0, 1, 0, 0], ignore=[1, 0, 0, 0, 0])),
    ("maxlen3", [100], 3, dict(thresh=1, maxLen=3)),
    ("maxlen17", [300], 4, dict(thresh=2, maxLen=17)),
    ("maxlen17_prev", [300], 4, dict(thresh=2, maxLen=17, comp="prev")),
    ("fixlen5", [103], 2, dict(fixLen=5)),
    ("two_tables_co", [90, 1, 140], 4, dict(thresh=1, co=254)),
    ("single_row", [1], 3, dict(thresh=1)),
]


def main():
    root = tempfile.mkdtemp(prefix="tehmm_seg_")
    segmentTracks = reference_functions(root)
    out = {"names": np.asarray([c[0] for c in CASES])}
    for n, (name, lens, K, opt) in enumerate(CASES):
        rs = np.random.RandomState(100 + n)
        tables = []
        start = 1000
        for t, T in enumerate(lens):
            tables.append(Table("chr%d" % (t + 1), start, sr.run_structured(rs, T, K, keep=0.85, n_values=3)))
            start += T + 17
        args = Args()
        args.outBed = os.path.join(root, name + ".bed")
        args.comp = opt.get("comp", "first")
        args.co = opt.get("co", 0)
        args.thresh = opt.get("thresh", 1)
        args.maxLen = opt.get("maxLen", 0)
        args.fixLen = opt.get("fixLen", 0)
        args.cutList = np.asarray(opt.get("cut", [0] * K))
        args.ignoreList = np.asarray(opt.get("ignore", [0] * K))
        args.stats = "stats"
        stats = dict()
        segmentTracks(Data(tables), args, stats)
        bed = open(args.outBed).read()
        args.stats = None                      # the early return on a cut track must not change the BED
        segmentTracks(Data(tables), args, dict())
        assert open(args.outBed).read() == bed
        keys = sorted(stats)
        meta = dict(lens=lens, starts=[t.start for t in tables], chroms=[t.chrom for t in tables],
                    cut=[int(x) for x in args.cutList], ignore=[int(x) for x in args.ignoreList],
                    thresh=args.thresh, comp=args.comp, maxLen=args.maxLen, fixLen=args.fixLen, co=args.co, bed=bed,
                    stats_tracks=[int(k) for k in keys], stats_count=[int(stats[k][0]) for k in keys],
                    stats_share=[float(stats[k][1]).hex() for k in keys])      # hex: the exact doubles
        out[name + "__data"] = np.concatenate([t.data for t in tables], axis=0)
        out[name + "__meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "segmenter.npz")
    np.savez_compressed(path, **out)
    print("wrote segmenter.npz %.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
