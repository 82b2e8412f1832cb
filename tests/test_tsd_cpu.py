"""CPU-only tests of the TSD finder: the plain-Python statement (tests/tsd_ref.py) and the host half of
tehmm_amd/tsd.py against what the real reference returned (tests/golden/tsd.npz), the two forms of the clean-up, and
the argument checks of the new entry points, which answer before any device call."""
import collections
import ctypes
import json

import numpy as np
import pytest

import tsd_ref as tr
from conftest import load_golden

ERR_ARG, ERR_HIP, ERR_UNSUPPORTED = -1, -2, -3


def golden_cases():
    g = load_golden("tsd")
    cases = []
    for name in g["names"]:
        name = str(name)
        meta = json.loads(bytes(g[name + "__meta"]).decode())
        meta["name"] = name
        bases, at = bytes(g[name + "__bases"]), 0
        meta["sequences"] = []
        for rec, size in meta["records"]:
            meta["sequences"].append((rec, bases[at:at + size]))
            at += size
        meta["intervals"] = [(meta["chroms"][c], int(a), int(b)) + (() if meta["labels"][n] is None
                                                                    else (meta["labels"][n],))
                             for c, a, b, n in g[name + "__iv"]]
        meta["tsds"] = None if meta["asserts"] else [
            (meta["chroms"][c], int(a), int(b), meta["tsd_names"][n], int(s)) for c, a, b, n, s in g[name + "__tsd"]]
        cases.append(meta)
    return cases


CASES = golden_cases()
FOUND = [c for c in CASES if not c["asserts"]]
ids = lambda cases: [c["name"] for c in cases]


def overrides(case):
    return {k: v for k, v in case["options"].items() if tr.DEFAULTS[k] != v}


def test_golden_is_what_the_case_maker_makes():
    made = tr.golden_cases()
    assert [c[0] for c in made] == [c["name"] for c in CASES]
    for (name, seqs, ivs, opt), case in zip(made, CASES):
        assert [(r, bytes(s)) for r, s in seqs] == case["sequences"], name
        assert [tuple(iv) for iv in ivs] == case["intervals"] and tr.options(**opt) == case["options"], name


def test_fixture_covers_what_it_should():
    opts = [c["options"] for c in CASES]
    assert {1, 4, 21} <= {o["min"] for o in opts}
    assert any(o["max"] < 2 * o["min"] and o["all"] for o in opts)
    assert any(o["max"] >= 2 * o["min"] + 1 and o["all"] for o in opts)
    assert any(o["maxScore"] == 0 for o in opts) and any(o["id"] for o in opts) and any(o["names"] for o in opts)
    assert any(o["left"] + o["overlap"] - 1 == 64 and o["right"] + o["overlap"] - 1 == 64 for o in opts)
    assert sum(c["asserts"] for c in CASES) == 1
    assert all(len(c["tsds"]) > 0 for c in FOUND) and all(len(c["intervals"]) <= 300 for c in CASES)
    by = {c["name"]: c for c in CASES}
    assert len(by["k1_dense_64"]["tsds"]) == 2 * 2 * 4096
    # extension saturates at max - k, and a run several times longer than a piece gives overlapping pieces
    ext = by["extension_one_letter"]
    lens = collections.Counter(b - a for _, a, b, _, _ in ext["tsds"])
    assert max(lens) == ext["options"]["max"] - ext["options"]["min"] and min(lens) == ext["options"]["min"]
    # no extension: nothing longer than k
    assert {b - a for _, a, b, _, _ in by["no_extension"]["tsds"]} == {4}
    assert max(b - a for _, a, b, _, _ in by["k21"]["tsds"]) == 50 - 21 and \
        {b - a for _, a, b, _, _ in by["k21_best"]["tsds"]} == {21}
    assert len({len(c["intervals"]) for c in CASES} & {1, 63, 64, 65}) == 4
    # elements 0 to 9 bases long, at base 0, at and past the sequence end
    first = by["defaults_two_letters"]
    size = len(first["sequences"][0][1])
    assert {e - s for _, s, e in first["intervals"]} >= set(range(10))
    assert any(s == 0 for _, s, e in first["intervals"]) and any(e > size for _, s, e in first["intervals"])
    assert any(e == size for _, s, e in first["intervals"])
    assert any(b"n" in s.lower() and s != s.lower() for c in CASES for _, s in c["sequences"])
    rec = by["records"]
    assert [r.split()[0] for r, _ in rec["sequences"]] != sorted(r.split()[0] for r, _ in rec["sequences"])
    assert len({t[0] for t in rec["tsds"]}) >= 4


def test_ties_of_the_selection_are_in_the_fixture():
    """an element whose best distance is shared by matches of different length, and one where distance and length are
    shared: the first goes to the longer match, the second to the first in list order"""
    on_d = on_d_and_len = 0
    for case in FOUND:
        o = dict(case["options"])
        if o["all"]:
            continue
        o["all"] = True
        for r, rec, chrom, i in tr.plan(case["sequences"], case["intervals"], o):
            iv = case["intervals"][i]
            rows = tr.element_matches(case["sequences"][r][1].decode().lower(), iv[1], iv[2], o)
            if len(rows) < 2:
                continue
            d = min(max(x[2], x[5]) for x in rows)
            best = [x[1] - x[0] for x in rows if max(x[2], x[5]) == d]
            on_d += len(set(best)) > 1
            on_d_and_len += best.count(max(best)) > 1
    assert on_d >= 3 and on_d_and_len >= 3


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_restatement_equals_the_reference(case):
    if case["asserts"]:
        with pytest.raises(tr.InvalidBase) as e:
            tr.find_tsds(case["sequences"], case["intervals"], **overrides(case))
        assert e.value.element == 4 == tr.lowest_invalid(case["sequences"], case["intervals"], **overrides(case))
    else:
        assert tr.find_tsds(case["sequences"], case["intervals"], **overrides(case)) == case["tsds"]


def columns_of(case):
    """(counts, cols) as tehmm_tsd_find would return them for the case's plan, from the restatement"""
    o = case["options"]
    counts, rows = [], []
    lower = [s.decode().lower() for _, s in case["sequences"]]
    for r, rec, chrom, i in tr.plan(case["sequences"], case["intervals"], o):
        got = tr.element_matches(lower[r], case["intervals"][i][1], case["intervals"][i][2], o)
        counts.append(len(got))
        rows += got
    return np.asarray(counts, dtype=np.int32), np.asarray(rows, dtype=np.int64).reshape(-1, 6).T


@pytest.mark.parametrize("case", FOUND, ids=ids(FOUND))
def test_host_half_of_findTsds(case):
    """planTsds and matchTuples around the restatement's columns give the reference's tuples: record matching, the
    name filters, output order and the ids are the host's"""
    from tehmm_amd import tsd
    o = case["options"]
    plan = tsd.planTsds(collections.OrderedDict(case["sequences"]), case["intervals"], o["names"], o["sequenceNames"])
    want = tr.plan(case["sequences"], case["intervals"], o)
    assert len(plan) == len(want)
    assert plan.start.tolist() == [case["intervals"][i][1] for _, _, _, i in want]
    assert [plan.chroms[s] for s in plan.seqIndex] == [chrom for _, _, chrom, _ in want]
    used = []
    for r, _, _, _ in want:
        if r not in used:
            used.append(r)
    assert bytes(plan.bases) == b"".join(case["sequences"][r][1] for r in used)        # records without elements: skipped
    assert plan.seqOffsets.tolist() == np.concatenate([[0], np.cumsum([len(case["sequences"][r][1])
                                                                         for r in used])]).tolist()
    counts, cols = columns_of(case)
    assert tsd.matchTuples(plan, counts, cols, o["leftName"], o["rightName"], o["id"]) == case["tsds"]


def test_a_reappearing_chromosome_raises():
    from tehmm_amd import tsd
    seqs = collections.OrderedDict([("a", b"acgtacgtacgt"), ("b", b"acgtacgtacgt")])
    ivs = [("a", 3, 5), ("b", 3, 5), ("a", 6, 8)]
    with pytest.raises(ValueError):
        tsd.planTsds(seqs, ivs)
    with pytest.raises(ValueError):
        tr.plan(list(seqs.items()), ivs, tr.options())
    assert len(tsd.planTsds(seqs, ivs[:2])) == 2
    assert len(tsd.planTsds(seqs, [("zz", 1, 2)])) == 0 and tsd.findTsds(seqs, [("zz", 1, 2)]) == []


def test_read_fasta(tmp_path):
    from tehmm_amd import tsd
    p = tmp_path / "x.fa"
    p.write_text(">chr1 first\nACgt\n#skipped\nnn a\tc\n>chr2\n\n>chr3\nA-C\n")
    assert list(tsd.readFasta(str(p)).items()) == [("chr1 first", b"ACgtnnac"), ("chr2", b""), ("chr3", b"A-C")]
    p.write_text(">chr1\nAC1\n")
    with pytest.raises(RuntimeError):
        tsd.readFasta(str(p))


def test_write_bed_intervals(tmp_path):
    from tehmm_amd import build, tsd
    build.build()
    p = str(tmp_path / "t.bed")
    ivs = [("c1", 3, 7, "L_TSD_0", 2), ("c1", 30, 34, "R_TSD_0", 0), ("c2 x", 5, 9, "L_TSD", 11)]
    tsd.writeBedIntervals(ivs, p)
    assert open(p).read() == "".join("%s\t%d\t%d\t%s\t%d\n" % iv for iv in ivs)
    tsd.writeBedIntervals([], p)
    assert open(p).read() == ""


# ---- the clean-up ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ivs", tr.overlap_lists(), ids=[n for n, _ in tr.overlap_lists()])
def test_running_maximum_equals_the_chain(name, ivs):
    s = tr.sort_intervals(ivs)
    chain = tr.remove_overlaps_chain(s)
    assert chain == tr.remove_overlaps_running_max(s)
    assert all(b[0] != a[0] or b[1] >= a[2] for a, b in zip(chain, chain[1:])) and all(iv[2] > iv[1] for iv in chain)
    if name == "contained":
        assert chain == [("c", 0, 100, "a", 1), ("c", 100, 120, "d", 4), ("c", 120, 121, "f", 6), ("d", 5, 9, "g", 7)]


def test_running_maximum_on_random_lists():
    rs = np.random.RandomState(5)
    for _ in range(300):
        n = rs.randint(1, 40)
        ivs = [("c%d" % rs.randint(3), int(s), int(s + rs.randint(0, 15))) for s in rs.randint(0, 60, size=n)]
        s = tr.sort_intervals(ivs)
        assert tr.remove_overlaps_chain(s) == tr.remove_overlaps_running_max(s)


# ---- the entry points answer bad arguments without a device ------------------------------------------------------------
def _find(lib, n_seq=1, bases=b"acgtacgtacgtacgtacgtacgtacgtacgt", offsets=(0, 32), n=None, index=(0, 0), start=(8, 12),
          end=(14, 20), k=4, mx=6, left=7, right=7, overlap=3, score=-1, all_=0, cap=None, null=None, n_out=True):
    from tehmm_amd._lib import i32p, i64p, ptr, u8p
    b = np.frombuffer(bases, dtype=np.uint8)
    off = np.asarray(offsets, dtype=np.int64)
    si, s, e = np.asarray(index, np.int32), np.asarray(start, np.int64), np.asarray(end, np.int64)
    n = len(si) if n is None else n
    cap = len(si) if cap is None else cap
    counts = np.zeros(max(len(si), 1), np.int32)
    cols = np.zeros((6, max(cap, 1)), np.int64)
    out = ctypes.c_int64(-7)
    args = [n_seq, ptr(b, u8p), ptr(off, i64p), n, ptr(si, i32p), ptr(s, i64p), ptr(e, i64p), k, mx, left, right,
            overlap, score, all_, ptr(counts, i32p), cap] + [ptr(cols[q], i64p) for q in range(6)] + \
           [ctypes.byref(out) if n_out else None]
    if null is not None:
        args[null] = None
    return lib.tehmm_tsd_find(*args), out.value


def _clean(lib, chrom=(0, 0, 1), start=(0, 5, 2), end=(9, 12, 4), n=None, cap=None, null=None):
    from tehmm_amd._lib import i32p, i64p, ptr
    c, s, e = np.asarray(chrom, np.int32), np.asarray(start, np.int64), np.asarray(end, np.int64)
    cap = len(c) if cap is None else cap
    oi, os_ = np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int64)
    out = ctypes.c_int64(-7)
    args = [len(c) if n is None else n, ptr(c, i32p), ptr(s, i64p), ptr(e, i64p), cap, ptr(oi, i64p), ptr(os_, i64p),
            ctypes.byref(out)]
    if null is not None:
        args[null] = None
    return lib.tehmm_remove_overlaps(*args), out.value


def test_symbols_and_argtypes_are_declared():
    from tehmm_amd import _lib, build
    build.build()
    lib = _lib.load()
    S = _lib.SIGNATURES
    for name in ("tehmm_tsd_find", "tehmm_remove_overlaps", "tehmm_tsd_last_timing", "tehmm_tsd_window"):
        assert name in S and hasattr(lib, name)
    assert len(S["tehmm_tsd_find"][1]) == 23 and S["tehmm_tsd_find"][1][1] is _lib.u8p
    assert S["tehmm_tsd_find"][1][14] is _lib.i32p and S["tehmm_tsd_find"][1][16:] == [_lib.i64p] * 7
    assert S["tehmm_remove_overlaps"][1] == [_lib.c_i64, _lib.i32p, _lib.i64p, _lib.i64p, _lib.c_i64, _lib.i64p,
                                             _lib.i64p, _lib.i64p]
    assert lib.tehmm_abi_version() == 4 and lib.tehmm_tsd_window() == 64


def test_find_rejects_before_any_device_call():
    from tehmm_amd import _lib, build
    build.build()
    lib = _lib.load()
    bad = lambda **kw: _find(lib, **kw)
    for null in (1, 2, 4, 5, 6, 14, 16, 19, 21):
        assert bad(null=null) == (ERR_ARG, 0), null
    assert bad(n_out=False)[0] == ERR_ARG
    assert bad(n=0) == (ERR_ARG, 0) and bad(n=-3) == (ERR_ARG, 0) and bad(n_seq=0) == (ERR_ARG, 0)
    assert bad(cap=-1) == (ERR_ARG, 0)
    assert bad(start=(8, 21)) == (ERR_ARG, 0) and b"element 1 has start > end" in lib.tehmm_last_error()
    assert bad(start=(-1, 12)) == (ERR_ARG, 0) and b"element 0 has start < 0" in lib.tehmm_last_error()
    assert bad(index=(0, 1)) == (ERR_ARG, 0) and b"element 1 has a seq_index" in lib.tehmm_last_error()
    assert bad(index=(-1, 0)) == (ERR_ARG, 0)
    assert bad(k=0) == (ERR_ARG, 0) and bad(k=7, mx=6) == (ERR_ARG, 0)
    assert bad(k=22, mx=30) == (ERR_ARG, 0) and b"21" in lib.tehmm_last_error()
    assert bad(offsets=(5, 2)) == (ERR_ARG, 0)
    assert bad(left=63, overlap=3) == (ERR_UNSUPPORTED, 0) and b"64" in lib.tehmm_last_error()
    assert bad(right=63, overlap=3) == (ERR_UNSUPPORTED, 0)
    assert bad(left=66, overlap=0) == (ERR_UNSUPPORTED, 0) and bad(left=66, overlap=-5) == (ERR_UNSUPPORTED, 0)
    assert bad(n=2 ** 31) == (ERR_UNSUPPORTED, 0)
    names, ms = (ctypes.c_char_p * 4)(), (ctypes.c_double * 4)()
    assert lib.tehmm_tsd_last_timing(4, None, ms) == ERR_ARG
    assert lib.tehmm_tsd_last_timing(4, names, ms) == 0          # the failed calls above left no timing


def test_remove_overlaps_rejects_before_any_device_call():
    from tehmm_amd import _lib, build
    build.build()
    lib = _lib.load()
    for null in (1, 2, 3, 5, 6):
        assert _clean(lib, null=null) == (ERR_ARG, 0), null
    assert _clean(lib, null=7)[0] == ERR_ARG
    assert _clean(lib, n=0) == (ERR_ARG, 0) and _clean(lib, cap=-1) == (ERR_ARG, 0)
    assert _clean(lib, n=2 ** 31) == (ERR_UNSUPPORTED, 0)


def test_a_valid_call_needs_the_device_and_nothing_else():
    """Without a device a valid call fails with the HIP error, never with UNSUPPORTED; with one it simply works: the
    widest window served, the longest k-mer, cap 0."""
    from tehmm_amd import _lib, build
    build.build()
    lib = _lib.load()
    want = 0 if _lib.device_count() > 0 else ERR_HIP
    for kw in (dict(), dict(left=62, right=62, overlap=3), dict(left=65, right=65, overlap=0), dict(k=21, mx=21),
               dict(k=1, mx=1, all_=1, cap=0), dict(score=0), dict(overlap=-4)):
        assert _find(lib, **kw)[0] == want, kw
    assert _clean(lib)[0] == want and _clean(lib, cap=0)[0] == want
    if want:
        assert b"UNSUPPORTED" not in lib.tehmm_last_error() and _find(lib)[1] == 0
