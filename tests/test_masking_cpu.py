"""CPU-only tests of the mask interval algebra: the plain-Python statement (tests/masking_ref.py) on cases written out
by hand, the branches its case makers must contain, what the real reference's loop wrote (tests/golden/masking.npz),
the argument checks of the new entry points, which answer before any device call, and the paths of
tehmm_amd/masking.py that need no device."""
import ctypes
import json
import logging

import numpy as np
import pytest

import masking_ref as mr
from conftest import load_golden

ERR_ARG, ERR_HIP, ERR_UNSUPPORTED = -1, -2, -3


def golden_cases():
    doc = json.loads(bytes(load_golden("masking")["cases"]).decode())
    tup = lambda rows: [tuple(r) for r in rows]
    for c in doc:
        c["tracks"] = [tup(t) for t in c["tracks"]]
        c["allBed"], c["inBed"], c["fills"] = tup(c["allBed"]), tup(c["inBed"]), tup(c["fills"])
    return doc


GOLDEN = golden_cases()


def split(x):
    return set() if x is None else set(x.split(","))


def restated_fills(case):
    """the fill rows of a fixture case by the restatement: (chrom, start, end, state)"""
    o = case["options"]
    records = [r for t in case["tracks"] for r in t]
    pred = case["inBed"]
    if o.get("cut"):
        pred = mr.cut_out(pred, records, -1, o["maxLen"] + 1)
    flank = sorted(iv[:4] for iv in pred)
    masks = mr.merge(mr.sort_intervals(records))
    states = mr.fill(masks, flank, split(o.get("tgts")), split(o.get("oneSidedTgts")), o.get("onlyDefault", False),
                     o.get("maxLen"))
    return [m + (o.get("default", "0") if s == mr.DEFAULT else s,) for m, s in zip(masks, states) if s != mr.SKIPPED]


# ---- by hand ---------------------------------------------------------------------------------------------------------
def test_merge_by_hand():
    recs, lo, hi = mr.merge_case()
    assert mr.merge_branches(recs) == {"nested", "overlapping", "abutting", "separate"}
    s = mr.sort_intervals(recs)
    assert [iv[0] for iv in s[:6]] == ["chr1"] * 6 and s[6][0] == "chr10" and s[-1][0] == "chr2"
    assert mr.merge(s) == [("chr1", 5, 50), ("chr1", 60, 95), ("chr1", 200, 210), ("chr10", 0, 3), ("chr10", 10, 500),
                           ("chr10", 600, 640), ("chr2", 0, 100)]
    # both limits are inclusive, and each drops something
    assert mr.merge(s, lo, hi) == [("chr1", 5, 50), ("chr1", 60, 95), ("chr1", 200, 210), ("chr10", 600, 640),
                                   ("chr2", 0, 100)]
    assert mr.merge(s, lo + 1, hi - 1) == [("chr1", 5, 50), ("chr1", 60, 95), ("chr10", 600, 640)]


def test_subtract_and_intersect_by_hand():
    A, B = mr.pieces_case()
    assert mr.pieces_branches(A, B) == mr.PIECES_BRANCHES
    assert mr.subtract(A, B) == [
        (0, 0, 50),
        (2, 200, 250),
        (3, 50, 100),
        (4, 0, 100), (4, 200, 300), (4, 450, 600), (4, 700, 1000),
        (5, 200, 300), (5, 450, 600),
        (6, 0, 500),
        (8, 40, 50), (8, 60, 70)]
    assert mr.intersect(A, B) == [
        (1, 120, 180),
        (2, 100, 200),
        (3, 100, 200),
        (4, 100, 200), (4, 300, 400), (4, 400, 450), (4, 600, 700),
        (5, 150, 200), (5, 300, 400), (5, 400, 450), (5, 600, 650),
        (7, 55, 58),
        (8, 50, 60)]
    assert mr.carry(A, mr.subtract(A, B))[1] == ("chr1", 200, 250, "cut_at_start")


def test_fill_by_hand():
    masks, ivs, tgt, one, max_len = mr.fill_case()
    assert ivs == sorted(ivs) and masks == mr.merge(mr.sort_intervals(masks))
    assert mr.fill_branches(masks, ivs, tgt, one, max_len) == mr.FILL_BRANCHES
    D, S = mr.DEFAULT, mr.SKIPPED
    assert mr.fill(masks, ivs, tgt, one, False, max_len) == [D, "A", D, D, "L", "L", S, D, "A", D, D, D]
    # without a target list every pair of equal flanks counts, without a length limit the long mask is looked at:
    # its flanks are C and A
    assert mr.fill(masks, ivs, (), one, False, None) == [D, "A", D, "B", "L", "L", D, D, "A", D, D, D]
    assert mr.fill(masks, ivs, tgt, one, True, max_len) == [D, D, D, D, D, D, S, D, D, D, D, D]


def test_fill_behind_the_last_interval_takes_the_interval_before_it():
    """the pointer stops ON the last index: the left candidate is the interval before the last one, so even a mask that
    abuts the last interval gets the default -- and one that abuts the interval before the last takes its state"""
    ivs = [("c", 0, 10, "A"), ("c", 10, 20, "L")]
    assert mr.fill([("c", 20, 30)], ivs, (), ("L", "A")) == [mr.DEFAULT]
    ivs = [("c", 0, 10, "A"), ("c", 5, 8, "L")]
    assert mr.fill([("c", 10, 12), ("c", 14, 15)], ivs, (), ("A",)) == ["A", mr.DEFAULT]
    # one interval: no candidate at all behind it, the right candidate before it
    one = [("c", 10, 20, "A")]
    assert mr.fill([("c", 5, 10), ("c", 20, 30), ("c", 40, 50)], one, (), ("A",)) == ["A", mr.DEFAULT, mr.DEFAULT]


def test_fill_overlap_raises_at_the_first_such_mask():
    masks, ivs = mr.overlap_case()
    with pytest.raises(mr.Overlap) as e:
        mr.fill(masks, ivs)
    assert e.value.mask == 1
    # a mask that is too long is never looked at
    assert mr.fill(masks, ivs, max_len=15) == [mr.SKIPPED, mr.SKIPPED, mr.SKIPPED, mr.DEFAULT]
    # only the two candidates are looked at: behind the last interval that is the interval BEFORE the last one, so a
    # mask inside the last interval passes
    assert mr.fill([("chr1", 520, 530)], ivs[1:]) == [mr.DEFAULT]


def test_interpolate_by_hand():
    records = [("c", 10, 20), ("c", 15, 25), ("c", 40, 50), ("d", 0, 5)]
    pred = [("c", 25, 40, "A", "x"), ("c", 0, 10, "A", "y"), ("c", 50, 60, "B", "z"), ("c", 60, 70, "B", "w")]
    scope = [("c", 5, 55), ("c", 50, 65)]
    got = mr.interpolate(records, scope, pred)
    assert got == [("c", 5, 10, "A", "y"), ("c", 10, 25, "A"), ("c", 25, 40, "A", "x"), ("c", 40, 50, "0"),
                   ("c", 50, 60, "B", "z"), ("c", 60, 65, "B", "w")]
    # with cut the prediction may cover the masks; the original rows stay, so the output overlaps itself
    whole = [("c", 0, 30, "A"), ("c", 30, 70, "A")]
    got = mr.interpolate(records, [("c", 0, 100)], whole, max_len=100, cut=True)
    assert got == [("c", 0, 30, "A"), ("c", 10, 25, "A"), ("c", 30, 70, "A"), ("c", 40, 50, "A")]
    with pytest.raises(mr.Overlap):
        mr.interpolate(records, [("c", 0, 100)], whole)


# ---- the fixture -------------------------------------------------------------------------------------------------------
def test_golden_is_what_the_case_maker_makes():
    made = mr.golden_cases()
    assert [c[0] for c in made] == [c["name"] for c in GOLDEN]
    for (name, tracks, all_bed, in_bed, options), c in zip(made, GOLDEN):
        assert [[tuple(r) for r in t] for t in tracks] == c["tracks"], name
        assert all_bed == c["allBed"] and in_bed == c["inBed"] and options == c["options"], name


def test_fixture_covers_what_it_should():
    seen = set()
    for c in GOLDEN:
        o = c["options"]
        masks = mr.merge(mr.sort_intervals([r for t in c["tracks"] for r in t]))
        if not o.get("cut") and not o.get("onlyDefault"):
            seen |= mr.fill_branches(masks, sorted(iv[:4] for iv in c["inBed"]), split(o.get("tgts")),
                                     split(o.get("oneSidedTgts")), o.get("maxLen"))
        assert len(c["fills"]) > 5
    assert seen == mr.FILL_BRANCHES - {"two_behind_last"}
    by = {c["name"]: c for c in GOLDEN}
    assert {f[3] for f in by["only_default"]["fills"]} == {"d"}
    assert len({f[3] for f in by["random_tgts"]["fills"]}) >= 4 and len(by["no_max_len"]["fills"]) > len(
        by["random"]["fills"])
    assert any(f[3] != "0" for f in by["cut"]["fills"]) and by["cut"]["options"]["cut"] is True


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_restatement_equals_the_reference(case):
    assert restated_fills(case) == case["fills"]


# ---- the generators hold their branches ----------------------------------------------------------------------------------
def test_generated_cases_are_not_vacuous():
    rs = np.random.RandomState(3)
    raw = mr.random_masks(rs, 300, merged=False)
    assert mr.merge_branches(raw) == {"nested", "overlapping", "abutting", "separate"}
    merged = mr.merge(mr.sort_intervals(raw))
    lens = [m[2] - m[1] for m in merged]
    assert min(lens) < 10 and max(lens) > 60          # a filter [10, 60] drops at both limits
    B = mr.random_disjoint(rs, 257)
    assert any(p[0] == q[0] and p[2] == q[1] for p, q in zip(B, B[1:]))
    assert all(p[0] != q[0] or p[2] <= q[1] for p, q in zip(B, B[1:]))
    A = mr.random_any(rs, 255, B)
    assert mr.pieces_branches(A, B) == mr.PIECES_BRANCHES
    def lists(r):
        masks = mr.merged_masks(r, 257)
        return masks, mr.random_prediction(r, masks, open_ends=True)
    every = lambda c: mr.fill_branches(c[0], c[1], ("A", "B"), ("L",), 40) == mr.FILL_BRANCHES
    masks, pred = mr.first_seed(lists, every, 0)
    assert len(masks) == 257 and masks == mr.merge(mr.sort_intervals(masks))
    assert pred == sorted(pred) and len(pred) > 257
    with pytest.raises(AssertionError):
        mr.first_seed(lists, lambda c: False, 0, tries=3)


# ---- the entry points answer bad arguments without a device ------------------------------------------------------------
def _lists(**kw):
    d = dict(chromA=(0, 0, 1), startA=(0, 5, 2), endA=(9, 12, 4), chromB=(0, 1), startB=(3, 0), endB=(6, 3))
    d.update(kw)
    cols = {}
    for k, v in d.items():
        cols[k] = np.asarray(v, np.int32 if k.startswith("chrom") else np.int64)
    return cols


def _merge(lib, n=None, cap=None, null=None, lo=0, hi=2 ** 63 - 1, **kw):
    from tehmm_amd._lib import i32p, i64p, ptr
    c = _lists(**kw)
    cap = 3 if cap is None else cap
    oc, os_, oe = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int64)
    out = ctypes.c_int64(-7)
    args = [len(c["chromA"]) if n is None else n, ptr(c["chromA"], i32p), ptr(c["startA"], i64p), ptr(c["endA"], i64p),
            lo, hi, cap, ptr(oc, i32p), ptr(os_, i64p), ptr(oe, i64p), ctypes.byref(out)]
    if null is not None:
        args[null] = None
    return lib.tehmm_intervals_merge(*args), out.value, (oc, os_, oe)


def _pieces(lib, which="subtract", nA=None, nB=None, cap=None, null=None, **kw):
    from tehmm_amd._lib import i32p, i64p, ptr
    c = _lists(**kw)
    cap = 8 if cap is None else cap
    cols = [np.zeros(max(cap, 1), np.int64) for _ in range(3)]
    out = ctypes.c_int64(-7)
    args = [len(c["chromA"]) if nA is None else nA, ptr(c["chromA"], i32p), ptr(c["startA"], i64p),
            ptr(c["endA"], i64p), len(c["chromB"]) if nB is None else nB, ptr(c["chromB"], i32p),
            ptr(c["startB"], i64p), ptr(c["endB"], i64p), cap] + [ptr(x, i64p) for x in cols] + [ctypes.byref(out)]
    if null is not None:
        args[null] = None
    return getattr(lib, "tehmm_intervals_" + which)(*args), out.value, cols


def _fill(lib, nM=None, nI=None, L=2, null=None, label=(0, 1), two=None, one=None, only=0, max_len=2 ** 63 - 1, **kw):
    from tehmm_amd._lib import i32p, i64p, ptr, u8p
    kw.setdefault("chromA", (0, 1))
    kw.setdefault("startA", (4, 7))
    kw.setdefault("endA", (6, 9))
    kw.setdefault("chromB", (0, 0))
    kw.setdefault("startB", (0, 6))
    kw.setdefault("endB", (4, 8))
    c = _lists(**kw)
    lab = np.asarray(label, np.int32)
    two = None if two is None else np.asarray(two, np.uint8)
    one = None if one is None else np.asarray(one, np.uint8)
    out = np.full(len(c["chromA"]), -9, np.int32)
    args = [len(c["chromA"]) if nM is None else nM, ptr(c["chromA"], i32p), ptr(c["startA"], i64p),
            ptr(c["endA"], i64p), len(c["chromB"]) if nI is None else nI, ptr(c["chromB"], i32p),
            ptr(c["startB"], i64p), ptr(c["endB"], i64p), ptr(lab, i32p), L, ptr(two, u8p), ptr(one, u8p), only,
            max_len, ptr(out, i32p)]
    if null is not None:
        args[null] = None
    return lib.tehmm_mask_fill(*args), out


@pytest.fixture(scope="module")
def lib():
    from tehmm_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_and_argtypes_are_declared(lib):
    from tehmm_amd import _lib
    S = _lib.SIGNATURES
    for name in ("tehmm_intervals_merge", "tehmm_intervals_subtract", "tehmm_intervals_intersect", "tehmm_mask_fill",
                 "tehmm_masking_last_timing"):
        assert name in S and hasattr(lib, name)
    assert S["tehmm_intervals_merge"][1] == [_lib.c_i64, _lib.i32p, _lib.i64p, _lib.i64p, _lib.c_i64, _lib.c_i64,
                                             _lib.c_i64, _lib.i32p, _lib.i64p, _lib.i64p, _lib.i64p]
    assert S["tehmm_intervals_subtract"][1] == S["tehmm_intervals_intersect"][1] and len(
        S["tehmm_intervals_subtract"][1]) == 13
    assert len(S["tehmm_mask_fill"][1]) == 15 and S["tehmm_mask_fill"][1][10] is _lib.u8p
    assert lib.tehmm_abi_version() == 4


def test_merge_rejects_before_any_device_call(lib):
    for null in (1, 2, 3, 7, 8, 9):
        assert _merge(lib, null=null)[:2] == (ERR_ARG, 0), null
    assert _merge(lib, null=10)[0] == ERR_ARG
    assert _merge(lib, n=0)[:2] == (ERR_ARG, 0) and _merge(lib, n=-1)[:2] == (ERR_ARG, 0)
    assert _merge(lib, cap=-1)[:2] == (ERR_ARG, 0)
    assert _merge(lib, n=2 ** 31)[:2] == (ERR_UNSUPPORTED, 0)
    names, ms = (ctypes.c_char_p * 4)(), (ctypes.c_double * 4)()
    assert lib.tehmm_masking_last_timing(4, None, ms) == ERR_ARG
    assert lib.tehmm_masking_last_timing(4, names, ms) == 0          # the failed calls above left no timing


@pytest.mark.parametrize("which", ["subtract", "intersect"])
def test_pieces_reject_before_any_device_call(lib, which):
    bad = lambda **kw: _pieces(lib, which, **kw)[:2]
    for null in (1, 2, 3, 5, 6, 7, 9, 10, 11):
        assert bad(null=null) == (ERR_ARG, 0), null
    assert bad(null=12)[0] == ERR_ARG
    assert bad(nA=0) == (ERR_ARG, 0) and bad(nB=0) == (ERR_ARG, 0) and bad(cap=-2) == (ERR_ARG, 0)
    assert bad(nA=2 ** 31) == (ERR_UNSUPPORTED, 0) and bad(nB=2 ** 31) == (ERR_UNSUPPORTED, 0)


def test_fill_rejects_before_any_device_call(lib):
    bad = lambda **kw: _fill(lib, **kw)[0]
    for null in (1, 2, 3, 5, 6, 7, 8, 14):
        assert bad(null=null) == ERR_ARG, null
    assert bad(nM=0) == ERR_ARG and bad(nI=0) == ERR_ARG and bad(L=0) == ERR_ARG and bad(L=-4) == ERR_ARG
    assert bad(L=2049) == ERR_UNSUPPORTED and b"2048" in lib.tehmm_last_error()
    assert bad(nM=2 ** 31) == ERR_UNSUPPORTED and bad(nI=2 ** 31) == ERR_UNSUPPORTED


def test_a_valid_call_needs_the_device_and_nothing_else(lib):
    """Without a device a valid call fails with the HIP error, never with UNSUPPORTED; with one it simply works."""
    from tehmm_amd import _lib
    want = 0 if _lib.device_count() > 0 else ERR_HIP
    assert _merge(lib)[0] == want and _merge(lib, cap=0, null=7)[0] == want
    assert _pieces(lib, "subtract")[0] == want and _pieces(lib, "intersect", cap=0, null=9)[0] == want
    assert _fill(lib)[0] == want and _fill(lib, L=2048, two=[1] * 2048, one=[0] * 2048)[0] == want
    if want:
        assert b"UNSUPPORTED" not in lib.tehmm_last_error() and _merge(lib)[1] == 0


# ---- the Python paths that need no device ------------------------------------------------------------------------------
def track_list(tmp_path, tracks):
    """an XML track list with one mask track per list of records (and one ordinary track)"""
    from tehmm_amd.track import Track, TrackList
    tl = TrackList()
    plain = tmp_path / "plain.bed"
    plain.write_text("c\t0\t10\tx\n")
    tl.addTrack(Track(name="plain", path=str(plain)))
    for k, recs in enumerate(tracks):
        p = tmp_path / ("mask%d.bed" % k)
        p.write_text("".join("%s\t%d\t%d\tignored\t5\n" % tuple(r[:3]) for r in recs))
        tl.addTrack(Track(name="mask%d" % k, dist="mask", path=str(p)))
    xml = tmp_path / "tracks.xml"
    tl.saveXML(str(xml))
    return str(xml)


def test_no_mask_tracks(tmp_path, caplog):
    from tehmm_amd import masking
    xml = track_list(tmp_path, [])
    ivs = [("c", 5, 9, "A"), ("b", 0, 3, "B")]
    assert masking.cutOutMaskIntervals(ivs, -1, None, xml) is None
    one, two = masking.cutPair(ivs, ivs[:1], xml, 5)
    assert one is ivs and two == ivs[:1]
    with caplog.at_level(logging.WARNING, logger="teHmm"):
        assert masking.interpolateMaskedRegions(xml, [("c", 0, 100)], ivs, cut=True) == ivs
    assert "No mask tracks" in caplog.text
    assert masking.maskIntervals(xml) == []


def test_empty_prediction_and_intersecting_targets(tmp_path):
    from tehmm_amd import masking
    from tehmm_amd.track import readTrackList
    xml = track_list(tmp_path, [[("c", 3, 5)]])
    assert len(readTrackList(xml).getMaskTracks()) == 1
    assert masking.interpolateMaskedRegions(xml, [("c", 0, 100)], []) == []
    assert masking.interpolateMaskedRegions(readTrackList(xml), [("c", 0, 100)], []) == []
    with pytest.raises(AssertionError):
        masking.interpolateMaskedRegions(xml, [("c", 0, 100)], [("c", 0, 3, "A")], tgts="A,B", oneSidedTgts="B")
    with pytest.raises(AssertionError):
        masking.interpolateMaskedRegions(xml, [("c", 0, 100)], [("c", 0, 3, "A")], tgts=["A"], oneSidedTgts={"A"})
    assert masking.fillMasks([], [("c", 0, 3, "A")]) == [] and masking.mergeIntervals([("c", 4, 4), ("c", 9, 2)]) == []
    assert masking.intersectIntervals([("c", 0, 3, "A")], []) == [] and masking.subtractIntervals([], [("c", 0, 3)]) == []
    assert masking.subtractIntervals([("c", 0, 3, "A"), ("c", 5, 5, "B")], []) == [("c", 0, 3, "A")]


def test_tables_and_sorting():
    from tehmm_amd import masking
    table = masking.chromTable([("chr2", 0, 1), ("chr10", 0, 1)], [("chr1", 0, 1), ("chr2", 5, 6)])
    assert table == {"chr1": 0, "chr10": 1, "chr2": 2} and list(table) == ["chr1", "chr10", "chr2"]
    labels = masking.labelTable([("c", 0, 1, "B"), ("c", 1, 2, 7), ("c", 2, 3, "B")], {"Z", "B"}, {"Q"})
    assert labels == {"B": 0, "7": 1, "Z": 2, "Q": 3}
    ivs = [("chr2", 5, 9, "a"), ("chr10", 7, 8, "b"), ("chr2", 5, 6, "c"), ("chr10", "3", 4, "d")]
    assert masking.sortIntervals(ivs) == [("chr10", 3, 4, "d"), ("chr10", 7, 8, "b"), ("chr2", 5, 9, "a"),
                                         ("chr2", 5, 6, "c")] == mr.sort_intervals(
                                             [(iv[0], int(iv[1])) + iv[2:] for iv in ivs])
    c, s, e = masking.encode(ivs[:2], table)
    assert c.tolist() == [2, 1] and c.dtype == np.int32 and s.dtype == e.dtype == np.int64 and e.tolist() == [9, 8]


def test_main_argument_parsing(tmp_path):
    from tehmm_amd import masking
    a = masking.parseArgs(["t.xml", "all.bed", "in.bed", "out.bed"])
    assert (a.tracksXML, a.allBed, a.inBed, a.outBed) == ("t.xml", "all.bed", "in.bed", "out.bed")
    assert a.maxLen is None and a.default == "0" and a.tgts is None and a.oneSidedTgts is None
    assert a.onlyDefault is False and a.cut is False
    a = masking.parseArgs(["t.xml", "a", "i", "o", "--maxLen", "5000", "--default", "X", "--tgts", "A,B",
                           "--oneSidedTgts", "L", "--onlyDefault", "--cut"])
    assert (a.maxLen, a.default, a.tgts, a.oneSidedTgts, a.onlyDefault, a.cut) == (5000, "X", "A,B", "L", True, True)
    # without mask tracks main copies the prediction, every column of it
    xml = track_list(tmp_path, [])
    inp, out = tmp_path / "in.bed", tmp_path / "out.bed"
    inp.write_text("c\t5\t9\tA\t0.5\textra\n#comment\nb\t0\t3\tB\t1\tmore\n")
    (tmp_path / "all.bed").write_text("c\t0\t100\n")
    assert masking.main([xml, str(tmp_path / "all.bed"), str(inp), str(out)]) == 0
    assert out.read_text() == "c\t5\t9\tA\t0.5\textra\nb\t0\t3\tB\t1\tmore\n"
