#!/usr/bin/env python3
"""Golden vectors of the TSD finder, by RUNNING THE REAL REFERENCE functions (recipe: make_golden_compare.py).

  tsd       KmerTable and hashDNA of kmer.py and buildSeqTable, findTsds, getScore, intervalTsds, matchesToBedInts of
            bin/tsdFinder.py are cut out of the reference at generation time, 2to3-converted in a scratch directory
            (the text never enters the repository; the one integer division of intervalTsds is spelled // there) and
            executed on the seeded cases of tests/tsd_ref.golden_cases().  findTsds reads its FASTA through fastaRead:
            it is handed the case's records instead of a file.  Every case stores its records, its intervals, its
            options and the tuples findTsds returned (as integer columns plus name tables); a case on which the
            reference asserts stores asserts = 1 and no tuples.
Re-run:  python tests/golden/make_golden_tsd.py
Timing:  python tests/golden/make_golden_tsd.py --time [N]   times the same cut-out findTsds on N (default 20000)
         elements of the generator of tools/tsd_bench.py and writes nothing.
"""
import json
import logging
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TEHMM_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import tsd_ref as tr          # noqa: E402  (only its options and its seeded cases)

WANTED = {
    "kmer.py": ["hashDNA", "KmerTable"],
    os.path.join("bin", "tsdFinder.py"): ["buildSeqTable", "findTsds", "getScore", "intervalTsds", "matchesToBedInts"],
}
DIVISION = "(bedInterval[2] - bedInterval[1]) / 2 - 2"


def reference_functions(root):
    """The wanted top-level functions and classes of the reference as py3 objects, in one namespace."""
    text = []
    for rel, names in WANTED.items():
        lines = open(os.path.join(REF, rel)).read().splitlines(True)
        for name in names:
            start = next(i for i, l in enumerate(lines) if l.startswith(("def %s(" % name, "class %s:" % name)))
            end = next((i for i in range(start + 1, len(lines))
                        if lines[i][:1] not in (" ", "\t", "\n", "#", "")), len(lines))
            text.append("".join(lines[start:end]))
    text = "\n".join(text)
    assert text.count(DIVISION) == 1
    text = text.replace(DIVISION, DIVISION.replace(" / ", " // "))
    tmp = os.path.join(root, "_tsd_block.py")
    open(tmp, "w").write(text)
    subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n", tmp],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    ns = {"np": np, "logger": logging.getLogger("golden")}
    exec(compile(open(tmp).read(), tmp, "exec"), ns)
    return ns


class Args(object):
    def __init__(self, o):
        self.min, self.max, self.all, self.maxScore = o["min"], o["max"], o["all"], o["maxScore"]
        self.left, self.right, self.overlap = o["left"], o["right"], o["overlap"]
        self.leftName, self.rightName, self.id, self.names = o["leftName"], o["rightName"], o["id"], o["names"]
        self.sequences = None if o["sequenceNames"] is None else set(o["sequenceNames"].split(","))
        self.fastaSequence = "records"
        self.nextId = 0


def run_reference(ref, sequences, intervals, o):
    """what findTsds returns, or None when the reference asserts"""
    ref["open"] = lambda path, mode: None
    ref["fastaRead"] = lambda handle: ((name, bytes(seq).decode("latin-1")) for name, seq in sequences)
    try:
        return [(c, int(a), int(b), name, int(score)) for c, a, b, name, score in
                ref["findTsds"](Args(o), intervals)]
    except AssertionError:
        return None


def time_reference(n):
    import time
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tools"))
    import tsd_bench as tb
    ref = reference_functions(tempfile.mkdtemp(prefix="tehmm_tsd_"))
    bases, start, end = tb.make_input(100 * n, n, 0)
    ivs = [("chr", int(a), int(b)) for a, b in zip(start, end)]
    t0 = time.time()
    out = run_reference(ref, [("chr", bases.tobytes())], ivs, tr.options())
    dt = time.time() - t0
    print("findTsds (defaults) on %d elements: %.2f s, %.1f us per element, %d TSD pairs" % (
        n, dt, 1e6 * dt / n, len(out) // 2))


def main():
    if "--time" in sys.argv:
        rest = sys.argv[sys.argv.index("--time") + 1:]
        return time_reference(int(rest[0]) if rest else 20000)
    ref = reference_functions(tempfile.mkdtemp(prefix="tehmm_tsd_"))
    cases = tr.golden_cases()
    out = {"names": np.asarray([c[0] for c in cases])}
    for name, sequences, intervals, opt in cases:
        o = tr.options(**opt)
        tuples = run_reference(ref, sequences, intervals, o)
        chroms, labels, tnames = dict(), dict(), dict()
        number = lambda table, key: table.setdefault(key, len(table))
        out[name + "__bases"] = np.frombuffer(b"".join(bytes(s) for _, s in sequences), dtype=np.uint8)
        out[name + "__iv"] = np.asarray([[number(chroms, iv[0]), iv[1], iv[2], number(labels, iv[3] if len(iv) > 3
                                                                                       else None)]
                                         for iv in intervals], dtype=np.int64).reshape(-1, 4)
        meta = dict(options=o, records=[[rec, len(s)] for rec, s in sequences], chroms=list(chroms),
                    labels=list(labels), asserts=1 if tuples is None else 0)
        if tuples is not None:
            out[name + "__tsd"] = np.asarray([[number(chroms, c), a, b, number(tnames, nm), sc]
                                              for c, a, b, nm, sc in tuples], dtype=np.int64).reshape(-1, 5)
            meta["chroms"], meta["tsd_names"] = list(chroms), list(tnames)
        out[name + "__meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
        print("%-28s %5d elements %6s pairs" % (name, len(intervals), "assert" if tuples is None else len(tuples) // 2))
    path = os.path.join(HERE, "tsd.npz")
    np.savez_compressed(path, **out)
    print("wrote tsd.npz %.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
