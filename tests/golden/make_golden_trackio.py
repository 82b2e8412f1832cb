#!/usr/bin/env python3
"""Golden vectors of track loading, by RUNNING THE REAL REFERENCE (recipe: make_golden.py, whose scratch build of the
reference package this script uses).

  trackio   trackIO.readBedData and readFastaData, track.Track (built from an XML element, so _fromXMLElement and
            _init run), TrackList, CategoryMap, BinaryMap and TrackData.loadTrackData of the reference are executed on
            the seeded cases of tests/trackio_ref.golden_cases().  Only inputs and outputs are stored: per case its
            description as JSON, the rows, the value maps as JSON, the missing values and the symbols per track.
Two things the reference needs are not available here, bedtools and Python 2's array('c'), so:
  * the generator clips and sorts each case's records itself (rule step 2 of tests/trackio_ref.py), writes them to a
    temporary BED and calls the real readBedData(..., needIntersect=False); inside loadTrackData the reference's
    readTrackData is replaced by a function that does the same for every (track, interval);
  * fastaRead is handed the case's records.
The fixture therefore DOES NOT COVER the order among records of equal clipped start (bedtools decides it in the
reference; the cases hold no such records).  Two lines of the scratch copy are adapted to Python 3 / SciPy 1.x: the
integer division of common.binSearch is spelled //, and track.mode is called with keepdims=True.
Re-run:  python tests/golden/make_golden_trackio.py
Timing:  python tests/golden/make_golden_trackio.py --time [N]   times the reference's own paint loop (readBedData,
         needIntersect=False) on N (default 200000) bases with N / 100 records and writes nothing.
"""
import json
import os
import sys
import tempfile
import time
import xml.etree.ElementTree as ET

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import trackio_ref as tr          # noqa: E402  (its seeded cases, and rule step 2 for the temporary BED files)


def reference():
    import make_golden
    root = make_golden.build_reference()
    p = os.path.join(root, "teHmm", "common.py")
    s = open(p).read()
    assert s.count("pivot = (first + last) / 2") == 1
    open(p, "w").write(s.replace("pivot = (first + last) / 2", "pivot = (first + last) // 2"))
    import teHmm.track as rtrack
    import teHmm.trackIO as rio
    from scipy.stats import mode
    rtrack.mode = lambda a: mode(a, keepdims=True)
    return rtrack, rio


def xml_element(t, name="t", path="x.bed"):
    a = dict(name=name, path=path, distribution=t["dist"], valCol=str(t["valCol"]))
    for key in ("scale", "logScale", "shift", "default"):
        if t[key] is not None:
            a[key] = str(t[key])
    if t["delta"]:
        a["delta"] = "True"
    if t["caseSensitive"]:
        a["caseSensitive"] = "True"
    return ET.Element("track", a)


def clipped_bed(text, chrom, start, end, tmp):
    path = os.path.join(tmp, "clipped_%d.bed" % len(os.listdir(tmp)))
    with open(path, "w") as f:
        for r in tr.clip_sort(tr.bed_records(text), chrom, start, end):
            f.write("\t".join(str(x) for x in r) + "\n")
    return path


def map_pairs(vmap):
    return sorted(([k, int(v)] for k, v in vmap.catMap.items()), key=lambda kv: kv[1])


def store(out, name, result):
    meta = dict()
    for key, val in result.items():
        if isinstance(val, np.ndarray):
            out["%s__%s" % (name, key)] = val.astype(np.uint8 if "offsets" not in key else np.int64)
        else:
            meta[key] = val
    out[name + "__meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)


def run_single(rtrack, rio, case, tmp):
    result = dict()
    track = rtrack.Track(xml_element(case["track"]))
    fresh = rtrack.Track(xml_element(case["track"]))
    for key, t, update in (("row", track, True), ("row_unlearned", fresh, False)):
        kw = dict(valMap=t.getValueMap(), updateValMap=update)
        if case["type"] == "bed":
            path = clipped_bed(case["bed"], case["chrom"], case["start"], case["end"], tmp)
            row = rio.readBedData(path, case["chrom"], case["start"], case["end"], valCol=t.getValCol(),
                                  useDelta=t.getDelta(), needIntersect=False, **kw)
        else:
            path = os.path.join(tmp, "records.fa")
            open(path, "w").write(tr.fasta_text(case["records"]))
            rio.fastaRead = lambda handle: iter([(n, s) for n, s in case["records"]])
            row = rio.readFastaData(path, case["chrom"], case["start"], case["end"],
                                    caseSensitive=t.getCaseSensitive(), **kw)
        result[key] = np.asarray(row, dtype=np.int64)
    vmap = track.getValueMap()
    result["maps"], result["missing"], result["symbols"] = [map_pairs(vmap)], [int(vmap.getMissingVal())], [len(vmap)]
    return result


def run_load(rtrack, rio, case, tmp):
    root = ET.Element("teModelConfig")
    for name, text in case["files"].items():
        open(os.path.join(tmp, name), "w").write(text)
    for t in case["tracks"]:
        root.append(xml_element(t, t["name"], os.path.join(tmp, t["file"])))
    xml = os.path.join(tmp, "tracks.xml")
    ET.ElementTree(root).write(xml)

    def read_track_data(path, chrom, start, end, **kw):      # stands in for intersectBed | sortBed, nothing else
        if path.endswith(".bed"):
            text = open(path).read()
            return rio.readBedData(clipped_bed(text, chrom, start, end, tmp), chrom, start, end, needIntersect=False,
                                   **kw)
        records = tr.fasta_records(open(path).read())
        rio.fastaRead = lambda handle: iter([(n, s) for n, s in records])
        return rio.readFastaData(path, chrom, start, end, **kw)
    rtrack.readTrackData = read_track_data

    result = dict()
    learned = None
    for prefix, intervals, segments in (("a_", case["intervals"], None), ("b_", case["intervals2"], None),
                                        ("c_", case["intervals2"], case["segments"])):
        td = rtrack.TrackData()
        td.loadTrackData(xml, [tuple(iv) for iv in intervals], trackList=learned,
                         segmentIntervals=None if segments is None else [tuple(s) for s in segments])
        if learned is None:
            learned = td.getTrackList()
        tables = td.getTrackTableList()
        result[prefix + "n"] = len(tables)
        for x, tab in enumerate(tables):
            result["%stable%d" % (prefix, x)] = np.asarray(tab.getNumPyArray())
            result["%swhere%d" % (prefix, x)] = [tab.getChrom(), int(tab.getStart())]
            if tab.getSegmentOffsets() is not None:
                result["%soffsets%d" % (prefix, x)] = np.asarray(tab.getSegmentOffsets(), dtype=np.int64)
        maps = [t.getValueMap() for t in td.getTrackList()]
        result[prefix + "maps"] = [map_pairs(m) for m in maps]
        result[prefix + "missing"] = [int(m.getMissingVal()) for m in maps]
        result[prefix + "symbols"] = [int(x) for x in td.getNumSymbolsPerTrack()]
    return result


def time_reference(n):
    rtrack, rio = reference()
    rng = np.random.RandomState(0)
    tmp = tempfile.mkdtemp(prefix="tehmm_trackio_")
    starts = np.sort(rng.randint(0, n, size=max(n // 100, 1)))
    path = os.path.join(tmp, "time.bed")
    with open(path, "w") as f:
        for s in starts.tolist():
            f.write("chr\t%d\t%d\tn%d\n" % (s, min(n, s + 1 + int(rng.randint(200))), rng.randint(8)))
    vmap = rtrack.CategoryMap(reserved=2)
    buf = np.zeros(n, dtype=np.uint8)
    t0 = time.time()
    rio.readBedData(path, "chr", 0, n, valCol=3, valMap=vmap, updateValMap=True, needIntersect=False, outputBuf=buf)
    dt = time.time() - t0
    print("readBedData (needIntersect=False) on %d bases, %d records: %.2f s, %.1f ns per base" % (
        n, len(starts), dt, 1e9 * dt / n))


def main():
    if "--time" in sys.argv:
        rest = sys.argv[sys.argv.index("--time") + 1:]
        return time_reference(int(rest[0]) if rest else 200000)
    rtrack, rio = reference()
    cases = tr.golden_cases()
    out = {"cases": np.frombuffer(tr.cases_json(cases).encode(), dtype=np.uint8)}
    for case in cases:
        tmp = tempfile.mkdtemp(prefix="tehmm_trackio_")
        result = (run_load if case["type"] == "load" else run_single)(rtrack, rio, case, tmp)
        store(out, case["name"], result)
        print("%-20s %s" % (case["name"], case["type"]))
    path = os.path.join(HERE, "trackio.npz")
    np.savez_compressed(path, **out)
    print("wrote trackio.npz %.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
