"""CPU-only tests of the state comparison: the plain-Python statement (tests/compare_ref.py) and the host half of
tehmm_amd/compare.py against what the real reference returned (tests/golden/compare.npz), and the argument checks
of the new entry points, which answer before any device call."""
import ctypes
import itertools
import json

import numpy as np
import pytest

import compare_ref as cr
from conftest import load_golden

ERR_ARG, ERR_HIP, ERR_UNSUPPORTED = -1, -2, -3


def decode(x):
    """the golden's JSON form back to Python values ("f:<hex>" -> float)"""
    if isinstance(x, dict):
        return {k: decode(v) for k, v in x.items()}
    if isinstance(x, list):
        return [decode(v) for v in x]
    if isinstance(x, str) and x.startswith("f:"):
        return float.fromhex(x[2:])
    return x


def norm(x):
    """tuples as lists, numpy scalars as Python numbers: what == should not see"""
    if isinstance(x, dict):
        return {k: norm(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [norm(v) for v in x]
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    return x


def order(d):
    """the keys of a dict (and of the dicts in it) in iteration order"""
    return [[k, list(v)] if isinstance(v, dict) else k for k, v in d.items()]


def same(got, want):
    """equal, and with the keys in the same order"""
    return got == want and order(got) == order(want)


def golden_cases():
    g = load_golden("compare")
    cases = []
    for name in g["names"]:
        meta = decode(json.loads(bytes(g[str(name) + "__meta"]).decode()))
        meta["name"] = str(name)
        for key in ("iv1", "iv2"):
            meta[key] = [(meta["chroms"][c], int(a), int(b), meta["labels"][n]) for c, a, b, n in g[str(name) + "__" + key]]
        cases.append(meta)
    return cases


CASES = golden_cases()
COMPARE = [c for c in CASES if c["kind"] == "compare"]
FIT = [c for c in CASES if c["kind"] == "fit"]
ids = lambda cases: [c["name"] for c in cases]


def one_sided(case, swap, upl, am):
    return next(e for e in case["one_sided"] if (e["swap"], e["usePredLen"], e["allowMultiple"]) == (swap, upl, am))


def fit_lists(case):
    """(first, second) as fitStateNames.py's main names them: iv1 is the target, iv2 the prediction"""
    return (case["iv2"], case["iv1"]) if case["options"].get("old") else (case["iv1"], case["iv2"])


def test_fixture_covers_what_it_should():
    assert len(COMPARE) >= 5 and len(FIT) >= 12
    assert all(len(c["one_sided"]) == 8 for c in COMPARE)
    thr = next(c for c in COMPARE if c["name"] == "cmp_threshold")
    # eight fractions of 0.1 miss 0.8 in the reference's order, one fraction 4/5 meets it
    assert sum([0.1] * 8) < 0.8 and thr["thresh"] == 0.8
    assert one_sided(thr, False, False, True)["stats"]["A"] == [1, 5.0, 1, 10.0]
    assert any(len({iv[0] for iv in c["iv1"]}) >= 3 for c in COMPARE)
    assert any(all(iv[2] - iv[1] == 1 for iv in c["iv2"]) and max(iv[2] - iv[1] for iv in c["iv1"]) >= 300
               for c in COMPARE)
    opts = [c["options"] for c in FIT]
    for key in ("intThresh", "old", "fdr", "ignore", "ignoreTgt", "tgt", "qualThresh", "noMerge", "noFrag"):
        assert any(key in o for o in opts), key
    assert all(len(c["iv1"]) + len(c["iv2"]) < 4000 for c in CASES)


@pytest.mark.parametrize("case", COMPARE, ids=ids(COMPARE))
def test_restatement_equals_the_reference(case):
    assert cr.check_lists(case["iv1"], case["iv2"]) == (0, -1)
    stats, conf = cr.compare_base_level(case["iv1"], case["iv2"], 3)
    assert stats == case["base_stats"] and conf == case["base_confMat"]
    assert order(stats) == case["base_stats_order"] and order(conf) == case["base_confMat_order"]
    for swap, upl, am in itertools.product((False, True), repeat=3):
        t, p = (case["iv2"], case["iv1"]) if swap else (case["iv1"], case["iv2"])
        want = one_sided(case, swap, upl, am)
        stats, conf = cr.compare_intervals_one_sided(t, p, 3, case["thresh"], upl, am)
        assert stats == want["stats"] and conf == want["confMat"], (swap, upl, am)
        assert order(stats) == want["stats_order"] and order(conf) == want["confMat_order"], (swap, upl, am)


@pytest.mark.parametrize("case", FIT, ids=ids(FIT))
def test_restatement_equals_the_reference_fit(case):
    opt = case["options"]
    first, second = fit_lists(case)
    if opt.get("intThresh") is not None:
        conf = cr.compare_intervals_one_sided(second, first, 3, opt["intThresh"], False, not opt.get("noFrag", False))[1]
    else:
        conf = cr.compare_base_level(second, first, 3)[1]
    assert conf == case["confMat"] and order(conf) == case["confMat_order"]
    fitted, text = cr.fitted_bed(case["iv2"], case["stateMap"], 3, opt.get("noMerge", False),
                                 set(opt.get("ignoreTgt", [])))
    assert text == case["bed"]


@pytest.mark.parametrize("case", COMPARE, ids=ids(COMPARE))
def test_host_summaries_from_the_golden_matrices(case):
    from tehmm_amd import compare
    stats = case["base_stats"]
    assert norm(compare.summarizeBaseComparision(stats, set())) == case["base_summary"]
    assert norm(compare.summarizeBaseComparision(stats, set(case["ignore"]))) == case["base_summary_ignore"]
    right, wrong, accMap = compare.summarizeBaseComparision(stats, set())
    assert float(right) / float(right + wrong) == case["accuracy"]
    assert norm(compare.summaryRow(case["accuracy"], stats, accMap)) == case["summary_row"]
    trueStats = one_sided(case, False, False, True)["stats"]
    predStats = one_sided(case, True, False, True)["stats"]
    assert norm(compare.summarizeIntervalComparison(trueStats, predStats, False, set())) == case["interval_summary"]
    assert norm(compare.summarizeIntervalComparison(trueStats, predStats, True, set(case["ignore"]))) == \
        case["interval_summary_weighted"]


@pytest.mark.parametrize("case", FIT, ids=ids(FIT))
def test_host_state_maps_from_the_golden_matrices(case):
    from tehmm_amd import compare
    opt = case["options"]
    if opt.get("old"):
        stateMap = compare.getStateMapFromConfMatrix_simple(case["confMat"])
    else:
        stateMap = compare.getStateMapFromConfMatrix(case["confMat"], set(opt.get("tgt", [])),
                                                     set(opt.get("ignoreTgt", [])), set(opt.get("ignore", [])),
                                                     opt.get("qualThresh", 0.1), opt.get("fdr"))
    assert norm(stateMap) == case["stateMap_raw"]
    compare.filterStateMap(stateMap, ignore=set(opt.get("ignore", [])), qualThresh=opt.get("qualThresh", 0.1))
    assert norm(stateMap) == case["stateMap"]

    class Args(object):
        ignore, qualThresh, unique = set(opt.get("ignore", [])), opt.get("qualThresh", 0.1), False
    again = decode(json.loads(json.dumps(case["stateMap_raw"])))
    compare.filterStateMap(again, Args())                # the reference's calling form
    assert norm(again) == case["stateMap"]


def test_state_maps_are_not_trivial():
    """the fixture's fits rename something, ignore something and differ between the options"""
    maps = {c["name"]: c["stateMap"] for c in FIT}
    assert any(k != v[0] for k, v in maps["fit_base"].items())
    assert "0" not in maps["fit_ignore"] and maps["fit_old_ignore"]["0"] == ["0", 1, 1]
    assert maps["fit_base"] != maps["fit_fdr"] and maps["fit_base"] != maps["fit_qual"]
    raw = {c["name"]: c["stateMap_raw"] for c in FIT}
    assert raw["fit_old_qual"] != maps["fit_old_qual"] and raw["fit_base"] == maps["fit_base"]
    assert {v[0] for v in maps["fit_tgt"].values()} <= {"LTR", "bg"} | set(maps["fit_tgt"])
    beds = {c["name"]: c["bed"] for c in FIT}
    assert beds["fit_nomerge"].count("\n") == len(FIT[0]["iv2"]) > beds["fit_base"].count("\n")


TIE_TGT = [("c", 0, 5, "A"), ("c", 5, 10, "B"), ("c", 10, 15, "A")]
TIE_PRED = [("c", 0, 5, "Y"), ("c", 5, 10, "X"), ("c", 10, 15, "X")]


def test_a_tie_goes_to_the_pair_the_walk_meets_first():
    """X overlaps B and A by five bases each and meets B first, although A is the first state of the target list."""
    from tehmm_amd import compare
    conf = cr.compare_base_level(TIE_TGT, TIE_PRED, 3)[1]
    assert order(conf) == [["Y", ["A"]], ["X", ["B", "A"]]]
    assert compare.getStateMapFromConfMatrix_simple(conf) == {"Y": ("A", 5, 5), "X": ("B", 5, 10)}


def test_restatement_names_the_offender():
    a = [("c", 0, 10, "x"), ("c", 10, 20, "y"), ("d", 5, 9, "x")]
    assert cr.check_lists(a, a) == (0, -1)
    assert cr.check_lists(a, [a[1], a[0], a[2]]) == (2, 1)                                   # unsorted
    assert cr.check_lists(a, [a[0], ("c", 9, 20, "y"), a[2]]) == (2, 1)                      # self-overlap in list 2
    assert cr.check_lists(a, [("c", 1, 10, "x")] + a[1:]) == (1, 0)                          # one base at a region start
    assert cr.check_lists(a, a[:2] + [("d", 5, 10, "x")]) == (1, 2)                          # one base at a region end
    assert cr.check_lists(a, [a[0], ("c", 11, 20, "y"), a[2]]) == (2, 0)                     # interior gap


# ---- the entry points answer bad arguments without a device ------------------------------------------------------------
def _lists(n):
    from tehmm_amd.compare import IntervalArrays
    s = np.arange(n, dtype=np.int64) * 3
    return IntervalArrays(np.zeros(n, np.int32), s, s + 3, np.arange(n, dtype=np.int32) % 2)


def _calls(lib, a, b, L, n1=None, null=False, only=4):
    """return codes of the first `only` of the four entry points on lists a, b (outputs sized for L <= 8)"""
    from tehmm_amd._lib import i32p, i64p, ptr
    aa = a.args() if n1 is None else (n1,) + a.args()[1:]
    if null:
        aa = aa[:2] + (None,) + aa[3:]
    which, where, n_out = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
    conf = np.zeros((min(L, 8), min(L, 8)), dtype=np.int64)
    v = [np.zeros(max(L, 1), dtype=np.int64) for _ in range(4)]
    oc, ol = np.zeros(len(a), np.int32), np.zeros(len(a), np.int32)
    os_, oe = np.zeros(len(a), np.int64), np.zeros(len(a), np.int64)
    calls = [
        lambda: lib.tehmm_intervals_check(*(aa + b.args() + (L, ctypes.byref(which), ctypes.byref(where)))),
        lambda: lib.tehmm_compare_base(*(aa + b.args() + (L, ptr(conf, i64p), None))),
        lambda: lib.tehmm_compare_intervals(*(aa + b.args() + (L, 0.8, 0, 1) + tuple(ptr(x, i64p) for x in v) +
                                              (ptr(conf, i64p), None))),
        lambda: lib.tehmm_merge_runs(*(aa + (L, None, len(a), ptr(oc, i32p), ptr(os_, i64p), ptr(oe, i64p),
                                             ptr(ol, i32p), ctypes.byref(n_out)))),
    ]
    return [f() for f in calls[:only]]


def test_entry_points_reject_before_any_device_call():
    from tehmm_amd import _lib, build
    build.build()
    lib = _lib.load()
    a, b = _lists(5), _lists(5)
    assert _calls(lib, a, b, 2049) == [ERR_UNSUPPORTED] * 4
    assert b"2048" in lib.tehmm_last_error()
    assert _calls(lib, a, b, 0) == [ERR_ARG] * 4
    assert _calls(lib, a, b, 2, null=True) == [ERR_ARG] * 4
    assert _calls(lib, a, b, 2, n1=0) == [ERR_ARG] * 4
    assert _calls(lib, a, b, 2, n1=2 ** 31) == [ERR_UNSUPPORTED] * 4
    assert lib.tehmm_abi_version() == 4
    assert 1 <= lib.tehmm_compare_lds_labels() < 2048 and lib.tehmm_compare_block_items() >= 64
    names, ms = (ctypes.c_char_p * 4)(), (ctypes.c_double * 4)()
    assert lib.tehmm_compare_last_timing(4, None, ms) == ERR_ARG
    assert lib.tehmm_compare_last_timing(4, names, ms) == 0          # the failed calls above left no timing


def test_a_valid_call_needs_the_device_and_nothing_else():
    """Without a device a valid call fails with the HIP error, never with UNSUPPORTED; with one it simply works."""
    from tehmm_amd import _lib, build
    build.build()
    lib = _lib.load()
    for L in (2, 2048):
        rcs = _calls(lib, _lists(5), _lists(5), L, only=4 if L == 2 else 1)      # (the check writes no matrix)
        assert rcs == [0 if _lib.device_count() > 0 else ERR_HIP] * len(rcs)


def test_encode_intervals_numbers_by_first_appearance():
    from tehmm_amd import compare
    a, b, chroms, names = compare.encodeIntervals([("c2", 5, 9, "x", 7), ("c1", 0, 3, "y", 8)],
                                                  [("c2", 5, 6, "z", 1), ("c2", 6, 9, "x", 2), ("c1", 0, 3, "x", 3)], 3)
    assert chroms == ["c2", "c1"] and names == ["x", "y", "z"]
    assert a.chrom.tolist() == [0, 1] and a.label.tolist() == [0, 1] and a.start.dtype == np.int64
    assert b.chrom.tolist() == [0, 0, 1] and b.label.tolist() == [2, 0, 0] and b.end.tolist() == [6, 9, 3]
    a, none, chroms, names = compare.encodeIntervals([("c", 2 ** 40, 2 ** 40 + 1, "x", 7)], None, 4)
    assert none is None and names == [7] and a.start.tolist() == [2 ** 40]
