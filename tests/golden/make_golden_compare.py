#!/usr/bin/env python3
"""Golden vectors of the state comparison, by RUNNING THE REAL REFERENCE functions (recipe: make_golden_segmenter.py).

  compare   bin/compareBedStates.py (compareBaseLevel, compareIntervalsOneSided, the three summaries, both state maps),
            bin/fitStateNames.py (filterStateMap, writeFittedBed) and intersectSize of common.py are cut out of the
            reference at generation time, 2to3-converted in a scratch directory (the text never enters the repository)
            and executed on seeded interval lists.  Every case stores the two lists as integer arrays and, as one JSON
            text, the name tables, the options and everything the functions returned (floats as hex, tuples as lists; the
            key order of the dicts beside them, since later tie-breaks go by it).
Re-run:  python tests/golden/make_golden_compare.py
Timing:  python tests/golden/make_golden_compare.py --time [BASES]   times the same cut-out functions on the first BASES
         (default 10^6) bases of the lists of tools/compare_bench.py and writes nothing.
"""
import itertools
import json
import logging
import os
import subprocess
import sys
import tempfile
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TEHMM_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
import compare_ref as cr          # noqa: E402  (only its seeded list maker)

WANTED = {
    os.path.join("bin", "compareBedStates.py"): [
        "compareBaseLevel", "compareIntervalsOneSided", "summarizeBaseComparision", "summarizeIntervalComparison",
        "summaryRow", "updateConfMatrix", "getStateMapFromConfMatrix_simple", "getStateMapFromConfMatrix"],
    os.path.join("bin", "fitStateNames.py"): ["filterStateMap", "writeFittedBed"],
    "common.py": ["intersectSize"],
}


def reference_functions(root):
    """The wanted top-level functions of the reference as py3 functions, in one namespace."""
    text = []
    for rel, names in WANTED.items():
        lines = open(os.path.join(REF, rel)).read().splitlines(True)
        for name in names:
            start = next(i for i, l in enumerate(lines) if l.startswith("def %s(" % name))
            end = next((i for i in range(start + 1, len(lines))
                        if lines[i][:1] not in (" ", "\t", "\n", "#", "")), len(lines))
            text.append("".join(lines[start:end]))
    tmp = os.path.join(root, "_compare_block.py")
    open(tmp, "w").write("\n".join(text))
    subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n", tmp],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    ns = {"np": np, "itertools": itertools, "defaultdict": defaultdict, "logger": logging.getLogger("golden")}
    exec(compile(open(tmp).read(), tmp, "exec"), ns)
    return ns


def plain(x):
    """JSON form: floats as "f:<hex>", tuples as lists, every dict key a string"""
    if isinstance(x, dict):
        assert all(isinstance(k, str) for k in x)
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, (float, np.floating)):
        return "f:" + float(x).hex()
    if isinstance(x, (int, np.integer)):
        return int(x)
    assert x is None or isinstance(x, str), type(x)
    return x


def order(d):
    """the keys of a dict (and of the dicts in it) in iteration order, which JSON with sorted keys does not keep"""
    return [[k, list(v)] if isinstance(v, dict) else k for k, v in d.items()]


def fit_pair(rs, n_regions, truth_names, n_states, chroms=2, mean_len=60, noise=0.25):
    """A target list and a prediction over the same cover whose states follow the target's names, with noise."""
    tgt, pred = cr.random_pair(rs, n_regions, len(truth_names), mean_len=mean_len, chroms=chroms, breaks=0.04)
    tgt = [(c, a, b, truth_names[int(n[1:])]) for c, a, b, n in tgt]
    follow = {name: [str(k) for k in range(n_states) if k % len(truth_names) == i]
              for i, name in enumerate(truth_names)}
    out = []
    j = 0
    for c, a, b, _ in pred:
        while not (tgt[j][0] == c and tgt[j][1] <= a < tgt[j][2]):
            j += 1
        own = follow[tgt[j][3]]
        out.append((c, a, b, own[rs.randint(len(own))] if rs.rand() > noise else str(rs.randint(n_states))))
    return tgt, out


def threshold_pair():
    """eight fractions of 0.1 (sum 0.7999999999999999) and one fraction 4/5 against a threshold of 0.8"""
    tgt = [("chr1", 0, 10, "A"), ("chr1", 10, 15, "A"), ("chr1", 15, 20, "B")]
    pred = [("chr1", k, k + 1, "A") for k in range(8)] + [("chr1", 8, 10, "B"), ("chr1", 10, 14, "A"),
                                                         ("chr1", 14, 15, "B"), ("chr1", 15, 20, "B")]
    return tgt, pred


def one_base_pair(rs):
    """one-base rows against long truth intervals, on two chromosomes with a gap"""
    tgt, pred = [], []
    for c, spans in (("chrA", [(1000, 1300, "TE"), (1300, 1700, "bg"), (2000, 2350, "TE")]), ("chrB", [(5, 205, "bg")])):
        for a, b, name in spans:
            tgt.append((c, a, b, name))
            for x in range(a, b):
                pred.append((c, x, x + 1, name if rs.rand() < 0.85 else ("bg" if name == "TE" else "TE")))
    return tgt, pred


class Args(object):
    unique = False


def encode(intervals, chroms, names):
    return np.asarray([[chroms.setdefault(c, len(chroms)), a, b, names.setdefault(n, len(names))]
                       for c, a, b, n in intervals], dtype=np.int64)


def time_reference(n):
    """seconds the reference's own functions take on n bases of compare_bench's lists (one CPU core)"""
    import time
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tools"))
    import compare_bench as cb
    ref = reference_functions(tempfile.mkdtemp(prefix="tehmm_cmp_"))
    truth, pred = cb.make_lists(n, 1000.0, 4, 0)
    tt, tp = cb.tuples(truth), cb.tuples(pred)
    for name, call in (("compareBaseLevel", lambda: ref["compareBaseLevel"](tt, tp, 3)),
                       ("compareIntervalsOneSided, truth side", lambda: ref["compareIntervalsOneSided"](
                           tt, tp, 3, 0.8, False, True)),
                       ("compareIntervalsOneSided, pred side", lambda: ref["compareIntervalsOneSided"](
                           tp, tt, 3, 0.8, False, True))):
        t0 = time.time()
        call()
        print("%s on %d bases: %.2f s" % (name, n, time.time() - t0))


def main():
    if "--time" in sys.argv:
        rest = sys.argv[sys.argv.index("--time") + 1:]
        return time_reference(int(rest[0]) if rest else 1000000)
    root = tempfile.mkdtemp(prefix="tehmm_cmp_")
    ref = reference_functions(root)
    rs = np.random.RandomState(20141)
    compare_cases = [
        ("cmp_threshold", threshold_pair(), 0.8),
        ("cmp_one_base", one_base_pair(rs), 0.8),
        ("cmp_chroms_gaps", cr.random_pair(rs, 12, 4, mean_len=30, chroms=3), 0.5),
        ("cmp_two_labels", cr.random_pair(rs, 30, 2, mean_len=15, chroms=1, breaks=0.2), 0.7),
        ("cmp_fit_like", fit_pair(rs, 10, ["LTR", "LINE", "bg"], 5), 0.6),
    ]
    truth = ["LTR", "LINE", "bg", "SINE"]
    fit_cases = [
        ("fit_base", dict()),
        ("fit_interval", dict(intThresh=0.3)),
        ("fit_interval_nofrag", dict(intThresh=0.3, noFrag=True)),
        ("fit_old", dict(old=True)),
        ("fit_old_interval", dict(old=True, intThresh=0.5)),
        ("fit_fdr", dict(fdr=0.45)),
        ("fit_old_qual", dict(old=True, qualThresh=0.5)),
        ("fit_old_ignore", dict(old=True, ignore=["0", "3"], ignoreTgt=["SINE"])),
        ("fit_ignore", dict(ignore=["0", "3"], ignoreTgt=["SINE"])),
        ("fit_tgt", dict(tgt=["LTR", "bg"])),
        ("fit_qual", dict(qualThresh=0.55)),
        ("fit_nomerge", dict(noMerge=True, qualThresh=0.3)),
    ]
    out = {"names": np.asarray([c[0] for c in compare_cases] + [c[0] for c in fit_cases])}

    def store(name, iv1, iv2, meta):
        chroms, names = dict(), dict()
        out[name + "__iv1"] = encode(iv1, chroms, names)
        out[name + "__iv2"] = encode(iv2, chroms, names)
        meta["chroms"], meta["labels"] = list(chroms), list(names)
        out[name + "__meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)

    for name, (iv1, iv2), thresh in compare_cases:
        stats, conf = ref["compareBaseLevel"](iv1, iv2, 3)
        right, wrong, accMap = ref["summarizeBaseComparision"](stats, set())
        accuracy = float(right) / float(right + wrong)
        header, row = ref["summaryRow"](accuracy, stats, accMap)
        one_sided = []
        for swap, upl, am in itertools.product((False, True), (False, True), (False, True)):
            t, p = (iv2, iv1) if swap else (iv1, iv2)
            st, cm = ref["compareIntervalsOneSided"](t, p, 3, thresh, upl, am)
            one_sided.append(dict(swap=swap, usePredLen=upl, allowMultiple=am, stats=plain(st), confMat=plain(cm),
                                  stats_order=order(st), confMat_order=order(cm)))
        # what main prints: recall side without usePredLen, precision side likewise, fragmented matches allowed
        trueStats = ref["compareIntervalsOneSided"](iv1, iv2, 3, thresh, False, True)[0]
        predStats = ref["compareIntervalsOneSided"](iv2, iv1, 3, thresh, False, True)[0]
        first = sorted(stats)[0]
        meta = dict(kind="compare", thresh=thresh, base_stats=plain(stats), base_confMat=plain(conf),
                    base_stats_order=order(stats), base_confMat_order=order(conf),
                    base_summary=plain([right, wrong, accMap]),
                    base_summary_ignore=plain(ref["summarizeBaseComparision"](stats, {first})), ignore=[first],
                    accuracy=plain(accuracy), summary_row=plain([header, row]), one_sided=one_sided,
                    interval_summary=plain(ref["summarizeIntervalComparison"](trueStats, predStats, False, set())),
                    interval_summary_weighted=plain(
                        ref["summarizeIntervalComparison"](trueStats, predStats, True, {first})))
        store(name, iv1, iv2, meta)

    tgt, pred = fit_pair(np.random.RandomState(7), 40, truth, 7, chroms=2)
    sizes = defaultdict(int)
    for iv in tgt:
        sizes[iv[3]] += iv[2] - iv[1]
    assert len(set(sizes.values())) == len(sizes), "equal truth sizes: the fit would hang on dict order"
    for name, opt in fit_cases:
        args = Args()
        args.ignore, args.qualThresh = set(opt.get("ignore", [])), opt.get("qualThresh", 0.1)
        ignoreTgt, tgtSet = set(opt.get("ignoreTgt", [])), set(opt.get("tgt", []))
        old, intThresh = opt.get("old", False), opt.get("intThresh")
        # the wiring of fitStateNames.py's main (:143-185)
        iv1, iv2 = (pred, tgt) if old else (tgt, pred)
        if intThresh is not None:
            confMat = ref["compareIntervalsOneSided"](iv2, iv1, 3, intThresh, False, not opt.get("noFrag", False))[1]
        else:
            confMat = ref["compareBaseLevel"](iv2, iv1, 3)[1]
        if old:
            stateMap = ref["getStateMapFromConfMatrix_simple"](confMat)
        else:
            stateMap = ref["getStateMapFromConfMatrix"](confMat, tgtSet, ignoreTgt, args.ignore, args.qualThresh,
                                                        opt.get("fdr"))
        raw = plain(stateMap)
        ref["filterStateMap"](stateMap, args)
        bed = os.path.join(root, name + ".bed")
        ref["writeFittedBed"](pred, stateMap, bed, 3, opt.get("noMerge", False), ignoreTgt)
        store(name, tgt, pred, dict(kind="fit", options=opt, confMat=plain(confMat), confMat_order=order(confMat),
                                    stateMap_raw=raw,
                                    stateMap=plain(stateMap), bed=open(bed).read()))
    path = os.path.join(HERE, "compare.npz")
    np.savez_compressed(path, **out)
    print("wrote compare.npz %.1f KB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
