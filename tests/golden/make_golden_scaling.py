#!/usr/bin/env python3
"""Golden vectors of track scaling, by RUNNING THE REAL REFERENCE (recipe: make_golden.py, whose scratch build of the
reference package this script uses; bin/setTrackScaling.py is copied beside it and converted the same way).

  scaling   setTrackScale, readTrackIntoFloatArray and computeScale of the reference's bin/setTrackScaling.py, on a real
            track.Track built from an XML element, are executed on the seeded cases of
            tests/scaling_ref.golden_cases().  Only inputs and outputs are stored: the cases as JSON, per case the float
            array readTrackIntoFloatArray returned, (scaleType, scaleParam, shift) of computeScale, the count vectors of
            its two histograms (np.histogram is wrapped by a recorder while computeScale runs; the reference's code is
            not changed for that), the scaling attributes of track.toXMLElement() after setTrackScale, and the name of
            the exception where one is raised.
bedtools is not available here, so, exactly as make_golden_trackio.py does, the readTrackData that setTrackScaling
imported is replaced by a function that clips and sorts the records of the interval itself (rule step 2 of
tests/trackio_ref.py), writes them to a temporary BED and calls the real readBedData(..., needIntersect=False) with
the caller's outputBuf / valCol / useDelta.  The merged intervals of a case are given (getMergedBedIntervals needs
bedtools).  main() of the tool is not run: it needs pybedtools and reads sys.argv.
Lines of the scratch copy adapted to Python 3 / NumPy 2, by the mechanical conversion of make_golden.py but for xrange:
  bin/setTrackScaling.py:142, 179, 202   xrange is left in the text and given to the module as a name of range (the
                                         conversion to range would meet computeScale's local variable ``range``)
  bin/setTrackScaling.py:187             sys.maxint -> sys.maxsize
  trackIO.py:102                         np.float is given back to NumPy as an alias of np.float64 (make_golden.py)
  trackIO.py:206                         xrange -> range
Every case must give the scale type it was designed for and raise no AssertionError; the generator checks both.
Re-run:  python tests/golden/make_golden_scaling.py
Timing:  python tests/golden/make_golden_scaling.py --time [N]   times the reference's two per-base loops (the paint of
         readBedData into the float buffer and the strip loop of readTrackIntoFloatArray) on N (default 200000) bases
         with N / 100 records and writes nothing.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import xml.etree.ElementTree as ET

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import scaling_ref as sr          # noqa: E402  (the seeded cases)
import trackio_ref as tr          # noqa: E402  (rule step 2 for the temporary BED files)


def reference():
    import make_golden
    root = make_golden.build_reference()
    tool = os.path.join(root, "setTrackScaling.py")
    shutil.copy(os.path.join(make_golden.REF, "bin", "setTrackScaling.py"), tool)
    subprocess.check_call([sys.executable, "-m", "lib2to3", "-x", "xrange", "-w", "-n", tool], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    import setTrackScaling as sts
    sts.xrange = range
    import teHmm.track as rtrack
    import teHmm.trackIO as rio
    tmp = tempfile.mkdtemp(prefix="tehmm_scaling_")

    def read_track_data(path, chrom, start, end, **kw):      # stands in for intersectBed | sortBed, nothing else
        clipped = os.path.join(tmp, "clipped_%d.bed" % len(os.listdir(tmp)))
        with open(clipped, "w") as f:
            for r in tr.clip_sort(tr.bed_records(open(path).read()), chrom, start, end):
                f.write("\t".join(str(x) for x in r) + "\n")
        return rio.readBedData(clipped, chrom, start, end, needIntersect=False, **kw)
    sts.readTrackData = read_track_data
    return sts, rtrack, tmp


def xml_element(t, path):
    a = dict(name="t", path=path, distribution=t["dist"], valCol=str(t["valCol"]))
    for key in ("scale", "logScale", "shift", "default"):
        if t[key] is not None:
            a[key] = str(t[key])
    if t["delta"]:
        a["delta"] = "True"
    return ET.Element("track", a)


def run_case(sts, rtrack, case, tmp):
    path = os.path.join(tmp, case["name"] + ".bed")
    open(path, "w").write(case["bed"])
    intervals = [tuple(iv) for iv in case["intervals"]]
    make = lambda: rtrack.Track(xml_element(case["track"], path))
    out = dict(error=None, data=np.zeros(0, dtype=np.float32), result=None,
               linear_counts=np.zeros(0, dtype=np.int64), log_counts=np.zeros(0, dtype=np.int64))
    try:
        out["data"] = np.array(sts.readTrackIntoFloatArray(make(), intervals), dtype=np.float32)
    except ValueError:
        out["error"] = "ValueError"
    if out["error"] is None and len(out["data"]) > case["numBins"]:
        recorded, real = [], np.histogram

        def recorder(a, bins):
            recorded.append(real(a, bins))
            return recorded[-1]
        np.histogram = recorder
        try:
            r = sts.computeScale(out["data"].copy(), case["numBins"], case["noLog"])      # (it shifts its argument)
        finally:
            np.histogram = real
        assert len(recorded) == 3 or (len(recorded) == 2 and recorded[1][1][0] <= 0)
        out["result"] = [r[0], float(r[1]), float(r[2])]
        out["linear_counts"] = recorded[0][0].astype(np.int64)
        out["log_counts"] = recorded[1][0].astype(np.int64)
    track = make()
    try:
        sts.setTrackScale(track, case["numBins"], intervals, case["noLog"])
    except ValueError:
        assert out["error"] == "ValueError"
    a = track.toXMLElement().attrib
    out["attrib"] = dict((key, a[key]) for key in ("scale", "logScale", "shift", "default") if key in a)
    assert (out["result"][0] if out["result"] else None) == case["expect"], (case["name"], out["result"])
    return out


def store(out, name, result):
    meta = dict()
    for key, val in result.items():
        if isinstance(val, np.ndarray):
            out["%s__%s" % (name, key)] = val
        else:
            meta[key] = val
    out[name + "__meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)


def time_reference(n):
    sts, rtrack, tmp = reference()
    rng = np.random.RandomState(0)
    starts = np.sort(rng.randint(0, n, size=max(n // 100, 1)))
    path = os.path.join(tmp, "time.bed")
    with open(path, "w") as f:
        for s in starts.tolist():
            f.write("chr\t%d\t%d\t%.3f\n" % (s, min(n, s + 1 + int(rng.randint(200))), rng.uniform(0, 100)))
    track = rtrack.Track(ET.Element("track", dict(name="t", path=path, valCol="3")))
    t0 = time.time()
    data = sts.readTrackIntoFloatArray(track, [("chr", 0, n)])
    dt = time.time() - t0
    print("readTrackIntoFloatArray (paint and strip loops) on %d bases, %d records, %d bases kept: %.2f s, "
          "%.1f ns per base" % (n, len(starts), len(data), dt, 1e9 * dt / n))


def main():
    if "--time" in sys.argv:
        rest = sys.argv[sys.argv.index("--time") + 1:]
        return time_reference(int(rest[0]) if rest else 200000)
    sts, rtrack, tmp = reference()
    cases = sr.golden_cases()
    out = {"cases": np.frombuffer(sr.cases_json(cases).encode(), dtype=np.uint8)}
    for case in cases:
        result = run_case(sts, rtrack, case, tmp)
        store(out, case["name"], result)
        print("%-22s %s %s" % (case["name"], result["error"], result["result"]))
    path = os.path.join(HERE, "scaling.npz")
    np.savez_compressed(path, **out)
    print("wrote scaling.npz %.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
