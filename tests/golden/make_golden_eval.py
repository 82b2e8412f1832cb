#!/usr/bin/env python3
"""Golden vectors of teHmmEval's helpers, by RUNNING THE REAL REFERENCE functions (recipe: make_golden_compare.py).

  eval   slicedIntervals and getPosteriorsMask of bin/teHmmEval.py, and the CategoryMap class of track.py that the
         second one builds, are cut out of the reference at generation time, 2to3-converted in a scratch directory (the
         text never enters the repository) and executed.  eval.json stores only inputs and what the functions returned.
Re-run:  python tests/golden/make_golden_eval.py
"""
import copy
import json
import logging
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TEHMM_REFERENCE", "/root/reference")

WANTED = {
    "track.py": ["class CategoryMap("],
    os.path.join("bin", "teHmmEval.py"): ["def slicedIntervals(", "def getPosteriorsMask("],
}


def reference_functions(root):
    text = []
    for rel, heads in WANTED.items():
        lines = open(os.path.join(REF, rel)).read().splitlines(True)
        for head in heads:
            start = next(i for i, l in enumerate(lines) if l.startswith(head))
            end = next((i for i in range(start + 1, len(lines))
                        if lines[i][:1] not in (" ", "\t", "\n", "#", "")), len(lines))
            text.append("".join(lines[start:end]))
    tmp = os.path.join(root, "_eval_block.py")
    open(tmp, "w").write("\n".join(text))
    subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n", tmp],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    ns = {"np": np, "math": math, "copy": copy, "sys": sys, "logger": logging.getLogger("golden")}
    exec(compile(open(tmp).read(), tmp, "exec"), ns)
    return ns


class FakeEmission(object):
    def __init__(self, n):
        self.n = n

    def getNumStates(self):
        return self.n


class FakeHmm(object):
    def __init__(self, n, stateMap):
        self.em, self.stateMap = FakeEmission(n), stateMap

    def getStateNameMap(self):
        return self.stateMap

    def getEmissionModel(self):
        return self.em


def main():
    with tempfile.TemporaryDirectory() as root:
        ns = reference_functions(root)
    sliced, getMask, CategoryMap = ns["slicedIntervals"], ns["getPosteriorsMask"], ns["CategoryMap"]
    out = {"sliced": [], "mask": []}
    lists = [
        [["chr1", 0, 3000]],
        [["chr1", 0, 1000], ["chr1", 2000, 4500], ["chr2", 0, 999]],
        [["chr1", 500, 2700], ["chrX", 10, 11]],                    # (a start that is not 0: the quirk)
        [["chr1", 0, 2000, "name", 7]],
    ]
    for intervals in lists:
        for chunk in (1, 7, 999, 1000, 1001, 2200, 1 << 62):
            if chunk < 7 and max(iv[2] - iv[1] for iv in intervals) > 100:
                continue
            try:
                got = [list(x) for x in sliced([tuple(iv) for iv in intervals], chunk)]
            except AssertionError:
                got = "AssertionError"
            out["sliced"].append({"intervals": intervals, "chunk": chunk, "out": got})
    for n, names, asked in [
        (5, None, "0"), (5, None, "1,3"), (5, None, "4,9,x"), (35, None, "34,0,17"),
        (3, ["LTR", "inside", "outside"], "inside"), (3, ["LTR", "inside", "outside"], "outside,LTR"),
        (4, ["a", "b", "c", "d"], "e,b"), (2, ["0", "1"], "1"),
    ]:
        stateMap = None
        if names is not None:
            stateMap = CategoryMap(reserved=0)
            for name in names:
                stateMap.update(name)
        mask = getMask(asked, FakeHmm(n, stateMap))
        out["mask"].append({"n": n, "names": names, "pdStates": asked, "mask": [int(x) for x in mask],
                            "dtype": str(mask.dtype)})
    with open(os.path.join(HERE, "eval.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote eval.json: %d sliced cases, %d mask cases" % (len(out["sliced"]), len(out["mask"])))


if __name__ == "__main__":
    main()
