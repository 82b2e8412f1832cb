#!/usr/bin/env python3
"""Golden vectors of the mask interpolation, by RUNNING THE REAL REFERENCE (recipe: make_golden.py, whose scratch build
of the reference package this script uses).

  masking   main() of bin/interpolateMaskedRegions.py is executed on the cases of tests/masking_ref.golden_cases().  The
            tool and bin/compareBedStates.py, which it imports, are added to the scratch copy at run time (2to3-converted
            there; the text never enters the repository), and sys.maxint is given its Python 3 spelling, sys.maxsize.
bedtools is not available here, so four names of the tool's module are replaced by stand-ins built on
tests/masking_ref.py: readBedIntervals (parse and sort as tuples), getMergedBedIntervals (the merged records of the
case's mask tracks), cutOutMaskIntervals (masking_ref.cut_out into a temporary BED) and runShellCommand (nothing).  The
fixture therefore pins the reference's FLANK LOOP AND STATE CHOICE only (interpolateMaskedRegions.py:117-162): the lines
the tool writes to its temporary mask BED.  It DOES NOT COVER sorting, merging, the cut or the final intersection.
Python 3 cannot order None against a tuple, so no case has a second mask behind the last predicted interval; that rule
is stated in tests/masking_ref.fill and DESIGN.md section 5q.
Only inputs and outputs are stored, as JSON.
Re-run:  python tests/golden/make_golden_masking.py
"""
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import xml.etree.ElementTree as ET

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import masking_ref as mr          # noqa: E402


def reference():
    import make_golden
    root = make_golden.build_reference()
    bin_dir = os.path.join(root, "teHmm", "bin")
    os.makedirs(bin_dir)
    open(os.path.join(bin_dir, "__init__.py"), "w").close()
    for f in ("interpolateMaskedRegions.py", "compareBedStates.py"):
        shutil.copy(os.path.join(make_golden.REF, "bin", f), os.path.join(bin_dir, f))
    subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n", bin_dir], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    sys.maxint = sys.maxsize
    return importlib.import_module("teHmm.bin.interpolateMaskedRegions")


def write_bed(path, rows):
    with open(path, "w") as f:
        for r in rows:
            f.write("\t".join(str(x) for x in r) + "\n")


def read_bed(path):
    rows = []
    for line in open(path):
        t = line.rstrip("\n").split("\t")
        rows.append((t[0], int(t[1]), int(t[2])) + tuple(t[3:]))
    return rows


def run_case(tool, tracks, all_bed, in_bed, options):
    tmp = tempfile.mkdtemp(prefix="tehmm_masking_")
    os.chdir(tmp)
    root = ET.Element("teModelConfig")
    for k, recs in enumerate(tracks):
        path = os.path.join(tmp, "mask%d.bed" % k)
        write_bed(path, recs)
        root.append(ET.Element("track", dict(name="mask%d" % k, path=path, distribution="mask")))
    xml = os.path.join(tmp, "tracks.xml")
    ET.ElementTree(root).write(xml)
    write_bed(os.path.join(tmp, "all.bed"), all_bed)
    write_bed(os.path.join(tmp, "in.bed"), in_bed)
    records = [r for recs in tracks for r in recs]
    made = dict()

    def temp_path(prefix="", extension="", tagLen=5):
        made[prefix] = os.path.join(tmp, "%s%d%s" % (prefix, len(made), extension))
        return made[prefix]

    def cut_out(path, min_length, max_length, tracks_xml):
        out = os.path.join(tmp, "cut.bed")
        write_bed(out, mr.cut_out(read_bed(path), records, min_length, max_length))
        return out

    tool.getLocalTempPath = temp_path
    tool.runShellCommand = lambda command: None
    tool.initBedTool = lambda *a: tmp
    tool.cleanBedTool = lambda *a: None
    tool.readBedIntervals = lambda path, ncol=3, sort=False: sorted(r[:ncol] for r in read_bed(path))
    tool.getMergedBedIntervals = lambda path, sort=False: mr.merge(mr.sort_intervals(records))
    tool.cutOutMaskIntervals = cut_out
    argv = ["interpolateMaskedRegions.py", xml, "all.bed", "in.bed", "out.bed"]
    for key, val in sorted(options.items()):
        argv += ["--" + key] if val is True else ["--" + key, str(val)]
    sys.argv = argv
    tool.main()
    return [list(r) for r in read_bed(made["Temp_om"])]


def main():
    tool = reference()
    cases = mr.golden_cases()
    doc = []
    for name, tracks, all_bed, in_bed, options in cases:
        fills = run_case(tool, tracks, all_bed, in_bed, options)
        doc.append(dict(name=name, tracks=tracks, allBed=all_bed, inBed=in_bed, options=options, fills=fills))
        print("%-14s %4d masks filled" % (name, len(fills)))
    path = os.path.join(HERE, "masking.npz")
    np.savez_compressed(path, cases=np.frombuffer(json.dumps(doc, sort_keys=True).encode(), dtype=np.uint8))
    print("wrote masking.npz %.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
