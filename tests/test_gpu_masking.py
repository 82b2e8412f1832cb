"""GPU tests of the mask interval algebra (tehmm_intervals_merge / _subtract / _intersect, tehmm_mask_fill,
tehmm_amd/masking.py): everything is compared for exact equality with the plain-Python statement
(tests/masking_ref.py) and with what the real reference's loop wrote (tests/golden/masking.npz)."""
import numpy as np
import pytest

import masking_ref as mr
from test_masking_cpu import ERR_ARG, GOLDEN, _fill, _merge, _pieces, restated_fills, split, track_list

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 2049]                      # around a workgroup's 256 lanes and its 2048 scan items
PAIRS = [(1, 1), (255, 257), (256, 256), (257, 255), (2049, 300), (300, 2049)]
_made = {}


def once(key, make):
    """a case and the restatement's answer, computed once"""
    if key not in _made:
        _made[key] = make()
    return _made[key]


@pytest.fixture(scope="module")
def masking():
    from tehmm_amd import masking
    return masking


@pytest.fixture(scope="module")
def lib():
    from tehmm_amd import _lib
    return _lib.load()


def rows(cols):
    return list(zip(*(c.tolist() for c in cols)))


# ---- merge -------------------------------------------------------------------------------------------------------------
def merge_case(n):
    def make():
        rs = np.random.RandomState(100 + n)
        s = mr.sort_intervals(mr.random_masks(rs, n, merged=False))
        return s, mr.merge(s), mr.merge(s, 10, 60)
    return once(("merge", n), make)


@pytest.mark.parametrize("n", SIZES + [20000])
def test_merge_equals_the_restatement(masking, n):
    s, plain, filtered = merge_case(n)
    assert len(s) == n
    table = mr.chrom_ids(s)
    names = list(table)
    back = lambda cols: [(names[c], a, b) for c, a, b in rows(cols)]
    assert back(masking.mergeArrays(*mr.columns(s, table))) == plain
    assert back(masking.mergeArrays(*mr.columns(s, table), minLen=10, maxLen=60)) == filtered
    if n >= 255:
        assert 0 < len(filtered) < len(plain) < n
        assert mr.merge_branches(s) == {"nested", "overlapping", "abutting", "separate"}
    assert masking.mergeIntervals(s[::-1], 10, 60) == filtered and masking.mergeIntervals(s) == plain
    assert [k for k, _ in masking.lastTiming()][:3] == ["upload", "check", "running_max"]


def test_merge_by_hand_and_cap(masking, lib):
    recs, lo, hi = mr.merge_case()
    assert masking.mergeIntervals(recs, lo, hi) == [("chr1", 5, 50), ("chr1", 60, 95), ("chr1", 200, 210),
                                                    ("chr10", 600, 640), ("chr2", 0, 100)]
    # one interval, one run; a filter that keeps nothing
    assert masking.mergeIntervals([("c", 3, 9)]) == [("c", 3, 9)] and masking.mergeIntervals([("c", 3, 9)], 7, None) == []
    kw = dict(chromA=(0, 0, 0, 1), startA=(0, 5, 20, 2), endA=(9, 12, 30, 4))
    rc, n_out, (oc, os_, oe) = _merge(lib, cap=2, **kw)
    assert (rc, n_out) == (0, 3) and (oc[:2].tolist(), os_[:2].tolist(), oe[:2].tolist()) == ([0, 0], [0, 20], [12, 30])
    assert _merge(lib, cap=0, null=7, **kw)[:2] == (0, 3)
    assert _merge(lib, cap=5, **kw)[:2] == (0, 3)


def test_merge_names_the_lowest_offender(lib):
    assert _merge(lib, chromA=(0, 1, 0), startA=(0, 5, 9), endA=(9, 12, 14))[:2] == (ERR_ARG, 0)
    assert b"interval 2 " in lib.tehmm_last_error() and b"not sorted" in lib.tehmm_last_error()
    assert _merge(lib, chromA=(0, 0, 0, 0), startA=(0, 5, 4, 3), endA=(9, 12, 14, 15))[:2] == (ERR_ARG, 0)
    assert b"interval 2 " in lib.tehmm_last_error()
    assert _merge(lib, chromA=(0, 0, 0), startA=(0, 5, 9), endA=(9, 5, 8))[:2] == (ERR_ARG, 0)
    assert b"interval 1 " in lib.tehmm_last_error() and b"start >= end" in lib.tehmm_last_error()


# ---- subtract and intersect ------------------------------------------------------------------------------------------
def pieces_case(nA, nB):
    def lists(rs):
        B = mr.random_disjoint(rs, nB)
        return mr.random_any(rs, nA, B), B

    def make():
        every = lambda c: min(nA, nB) < 255 or mr.pieces_branches(*c) == mr.PIECES_BRANCHES
        A, B = mr.first_seed(lists, every, 1000 * nA + nB)
        return A, B, mr.subtract(A, B), mr.intersect(A, B)
    return once(("pieces", nA, nB), make)


@pytest.mark.parametrize("nA,nB", PAIRS)
def test_pieces_equal_the_restatement(masking, nA, nB):
    A, B, sub, inter = pieces_case(nA, nB)
    assert (len(A), len(B)) == (nA, nB)
    if min(nA, nB) >= 255:
        assert mr.pieces_branches(A, B) == mr.PIECES_BRANCHES and len(sub) > 0 and len(inter) > 0
    table = mr.chrom_ids(A, B)
    a, b = mr.columns(A, table), mr.columns(B, table)
    assert rows(masking.subtractArrays(a, b)) == sub
    assert rows(masking.intersectArrays(a, b)) == inter
    assert rows(masking.subtractArrays(a, b, _cap=1)) == sub          # the second call of the cap protocol
    assert masking.subtractIntervals(A, B) == mr.carry(A, sub)
    assert masking.intersectIntervals(A, B) == mr.carry(A, inter)


def long_case():
    """about 20 000 masks under three chromosome-wide intervals, which sit among 2 500 small ones so that the scan
    over A carries thousands of pieces across its workgroup boundary at item 2048"""
    def make():
        rs = np.random.RandomState(77)
        B = mr.random_disjoint(rs, 20000, chroms=mr.CHROMS)
        end = max(b[2] for b in B) + 10
        small = [("chr30", int(s), int(s) + 5, "s%d" % k) for k, s in enumerate(rs.randint(0, 1000, size=2460))]
        real = mr.random_any(rs, 40, B, chroms=mr.CHROMS)
        wide = [(c, 0, end, "wide_" + c) for c in mr.CHROMS]
        A = small[:1500] + wide[:1] + real[:20] + small[1500:2400] + wide[1:] + real[20:] + small[2400:]
        return A, B, mr.subtract(A, B), mr.intersect(A, B)
    return once("long", make)


def test_chromosome_wide_intervals_over_many_masks(masking):
    A, B, sub, inter = long_case()
    assert len(A) > 2048 and len(B) == 20000
    per = lambda pieces: {i: sum(1 for p in pieces if p[0] == i) for i in (1500, 2421, 2422)}
    assert all(A[i][3].startswith("wide_") for i in (1500, 2421, 2422))
    assert min(per(sub).values()) > 2048 and min(per(inter).values()) > 4096      # several workgroups per a
    assert any(p[2] == q[1] and p[0] == q[0] for p, q in zip(B, B[1:]))             # abutting masks: no empty piece
    table = mr.chrom_ids(A, B)
    a, b = mr.columns(A, table), mr.columns(B, table)
    got = masking.subtractArrays(a, b)
    assert rows(got) == sub and int((got[2] > got[1]).sum()) == len(sub)
    assert rows(masking.intersectArrays(a, b)) == inter
    assert [k for k, _ in masking.lastTiming()] == ["upload", "check", "count", "scan", "emit", "download"]


def test_pieces_by_hand_and_cap(masking, lib):
    A, B = mr.pieces_case()
    assert masking.subtractIntervals(A, B)[:3] == [("chr1", 0, 50, "no_b"), ("chr1", 200, 250, "cut_at_start"),
                                                   ("chr1", 50, 100, "cut_at_end")]
    assert masking.intersectIntervals(A, B)[-2:] == [("chr2", 55, 58, "covered2"), ("chr2", 50, 60, "inner")]
    assert masking.subtractIntervals([("c", 2, 8, "x")], [("c", 0, 10)]) == []       # everything covered: no row
    kw = dict(chromA=(0, 0, 1), startA=(0, 5, 2), endA=(9, 12, 4), chromB=(0, 0), startB=(3, 6), endB=(6, 7))
    for which, want in (("subtract", [(0, 0, 3), (0, 7, 9), (1, 7, 12), (2, 2, 4)]),
                        ("intersect", [(0, 3, 6), (0, 6, 7), (1, 5, 6), (1, 6, 7)])):
        rc, n_out, cols = _pieces(lib, which, cap=2, **kw)
        assert (rc, n_out) == (0, len(want)) and rows([c[:2] for c in cols]) == want[:2]
        assert _pieces(lib, which, cap=0, null=9, **kw)[:2] == (0, len(want))
        rc, n_out, cols = _pieces(lib, which, cap=8, **kw)
        assert (rc, n_out) == (0, len(want)) and rows([c[:n_out] for c in cols]) == want


@pytest.mark.parametrize("which", ["subtract", "intersect"])
def test_pieces_name_the_lowest_offender(lib, which):
    bad = lambda **kw: _pieces(lib, which, **kw)[:2]
    msg = lib.tehmm_last_error
    assert bad(endA=(9, 5, 4)) == (ERR_ARG, 0) and b"interval 1 of A has start >= end" in msg()
    assert bad(chromB=(0, 0, 0), startB=(0, 5, 9), endB=(5, 10, 9)) == (ERR_ARG, 0)
    assert b"interval 2 of B has start >= end" in msg()
    assert bad(chromB=(1, 0), startB=(3, 0), endB=(6, 3)) == (ERR_ARG, 0) and b"interval 1 of B" in msg()
    assert bad(chromB=(0, 0, 0, 0), startB=(0, 5, 9, 8), endB=(5, 10, 12, 20)) == (ERR_ARG, 0)
    assert b"interval 2 of B" in msg() and b"disjoint" in msg()                   # overlaps its predecessor
    assert bad(chromB=(0, 0, 0), startB=(0, 5, 10), endB=(5, 10, 12))[0] == 0          # abutting is disjoint
    assert bad(chromA=(1, 0, 1), startA=(7, 5, 2), endA=(9, 12, 4))[0] == 0            # A: any order


# ---- the flank loop ----------------------------------------------------------------------------------------------------
def fill_case(n):
    def lists(rs):
        masks = mr.merged_masks(rs, n)
        return masks, mr.random_prediction(rs, masks, open_ends=n >= 255)

    def make():
        every = lambda c: n < 255 or mr.fill_branches(c[0], c[1], ("A", "B"), ("L",), 40) == mr.FILL_BRANCHES
        masks, pred = mr.first_seed(lists, every, 500 + n)
        return masks, pred, mr.fill(masks, pred, ("A", "B"), ("L",), False, 40), mr.fill(masks, pred)
    return once(("fill", n), make)


def device_fill(masking, masks, pred, tgt, one, only, max_len):
    labels = masking.labelTable(pred, set(tgt), set(one))
    names = list(labels)
    flags = lambda chosen: np.asarray([nm in chosen for nm in names], dtype=np.uint8)
    table = mr.chrom_ids(masks, pred)
    got = masking.fillArrays(mr.columns(masks, table), mr.columns(pred, table), [labels[iv[3]] for iv in pred],
                             len(names), flags(tgt) if tgt else None, flags(one) if one else None, only,
                             2 ** 63 - 1 if max_len is None else max_len)
    return [k if k < 0 else names[k] for k in got.tolist()]


@pytest.mark.parametrize("n", SIZES + [20000])
def test_fill_equals_the_restatement(masking, n):
    masks, pred, want, want_plain = fill_case(n)
    assert len(masks) == n
    if n >= 255:
        assert mr.fill_branches(masks, pred, ("A", "B"), ("L",), 40) == mr.FILL_BRANCHES
    assert device_fill(masking, masks, pred, ("A", "B"), ("L",), False, 40) == want
    assert device_fill(masking, masks, pred, (), (), False, None) == want_plain
    assert set(device_fill(masking, masks, pred, ("A",), ("L",), True, 40)) <= {mr.DEFAULT, mr.SKIPPED}
    assert [k for k, _ in masking.lastTiming()] == ["upload", "check", "fill", "download"]


def test_fill_by_hand(masking):
    masks, ivs, tgt, one, max_len = mr.fill_case()
    D, S = mr.DEFAULT, mr.SKIPPED
    assert device_fill(masking, masks, ivs, tgt, one, False, max_len) == [D, "A", D, D, "L", "L", S, D, "A", D, D, D]
    assert device_fill(masking, masks, ivs, (), one, False, None) == [D, "A", D, "B", "L", "L", D, D, "A", D, D, D]
    # behind the last interval the left candidate is the interval BEFORE the last one
    assert device_fill(masking, [("c", 20, 30)], [("c", 0, 10, "A"), ("c", 10, 20, "L")], (), ("L", "A"), False,
                       None) == [D]
    assert device_fill(masking, [("c", 10, 12), ("c", 14, 15)], [("c", 0, 10, "A"), ("c", 5, 8, "L")], (), ("A",),
                       False, None) == ["A", D]
    single = [("c", 10, 20, "A")]
    assert device_fill(masking, [("c", 5, 10), ("c", 20, 30), ("c", 40, 50)], single, (), ("A",), False, None) == [
        "A", D, D]
    assert masking.fillMasks(masks, ivs, "0", "A", ["L"], False, max_len) == [
        m + (s if s != D else "0",) for m, s in zip(masks, mr.fill(masks, ivs, tgt, one, False, max_len)) if s != S]


def test_fill_errors_name_the_lowest_offender(masking, lib):
    masks, ivs = mr.overlap_case()
    with pytest.raises(AssertionError) as e:
        masking.fillMasks(masks, ivs)
    assert "('chr1', 200, 260)" in str(e.value)
    assert masking.fillMasks(masks, ivs, maxLen=15) == [("chr1", 400, 410, "0")]      # too long: never looked at
    assert masking.fillMasks([("chr1", 520, 530)], ivs[1:]) == [("chr1", 520, 530, "0")]
    # on the ABI: masks 1 and 2 overlap the prediction, 1 is named
    kw = dict(chromA=(0, 0, 0), startA=(100, 200, 280), endA=(150, 260, 320), chromB=(0, 0, 0), startB=(0, 150, 500),
              endB=(100, 300, 600), label=(0, 1, 0))
    assert _fill(lib, **kw)[0] == ERR_ARG and b"mask 1 overlaps" in lib.tehmm_last_error()
    assert _fill(lib, label=(0, 2))[0] == ERR_ARG and b"interval 1 of the prediction has a label" in lib.tehmm_last_error()
    assert _fill(lib, label=(-1, 2))[0] == ERR_ARG and b"interval 0 of the prediction" in lib.tehmm_last_error()
    assert _fill(lib, chromA=(0, 0), startA=(4, 5), endA=(6, 9))[0] == ERR_ARG          # masks overlap each other
    assert b"interval 1 of the masks" in lib.tehmm_last_error()
    assert _fill(lib, chromB=(0, 0), startB=(0, 0), endB=(4, 3))[0] == ERR_ARG          # equal starts, ends descend
    assert b"interval 1 of the prediction" in lib.tehmm_last_error()
    rc, out = _fill(lib, one=(1, 1))
    assert rc == 0 and out.tolist() == [0, -1]          # mask (0, 4, 6) between label 0 and label 1; mask on chrom 1


# ---- the Python layer, through BED files -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_device_equals_the_reference(masking, case, tmp_path):
    o = case["options"]
    records = [r for t in case["tracks"] for r in t]
    xml = track_list(tmp_path, case["tracks"])
    masks = masking.maskIntervals(xml)
    assert masks == mr.merge(mr.sort_intervals(records))
    pred = case["inBed"]
    if o.get("cut"):
        pred = masking.cutOutMaskIntervals(pred, -1, o["maxLen"] + 1, xml)
        assert pred == mr.cut_out(case["inBed"], records, -1, o["maxLen"] + 1)
    fills = masking.fillMasks(masks, sorted(iv[:4] for iv in pred), o.get("default", "0"), o.get("tgts"),
                              o.get("oneSidedTgts"), o.get("onlyDefault", False), o.get("maxLen"))
    assert fills == case["fills"] == restated_fills(case)
    # end to end, BED files in and out
    write = lambda name, ivs: masking.writeBed(ivs, str(tmp_path / name)) or str(tmp_path / name)
    argv = [xml, write("all.bed", case["allBed"]), write("in.bed", case["inBed"]), str(tmp_path / "out.bed")]
    for key, val in sorted(o.items()):
        argv += ["--" + key] if val is True else ["--" + key, str(val)]
    assert masking.main(argv) == 0
    want = mr.interpolate(records, case["allBed"], case["inBed"], o.get("maxLen"), o.get("default", "0"),
                          split(o.get("tgts")), split(o.get("oneSidedTgts")), o.get("onlyDefault", False),
                          o.get("cut", False))
    assert masking.readBed(str(tmp_path / "out.bed")) == want and len(want) >= len(case["inBed"]) + len(case["fills"])


def test_interpolate_by_hand(masking, tmp_path):
    records = [("c", 10, 20), ("c", 15, 25), ("c", 40, 50), ("d", 0, 5)]
    xml = track_list(tmp_path, [records[:2], records[2:]])
    pred = [("c", 25, 40, "A", "x"), ("c", 0, 10, "A", "y"), ("c", 50, 60, "B", "z"), ("c", 60, 70, "B", "w")]
    got = masking.interpolateMaskedRegions(xml, [("c", 5, 55), ("c", 50, 65)], pred)
    assert got == [("c", 5, 10, "A", "y"), ("c", 10, 25, "A"), ("c", 25, 40, "A", "x"), ("c", 40, 50, "0"),
                   ("c", 50, 60, "B", "z"), ("c", 60, 65, "B", "w")]
    whole = [("c", 0, 30, "A"), ("c", 30, 70, "A")]
    got = masking.interpolateMaskedRegions(xml, [("c", 0, 100)], whole, maxLen=100, cut=True)
    assert got == [("c", 0, 30, "A"), ("c", 10, 25, "A"), ("c", 30, 70, "A"), ("c", 40, 50, "A")]
    with pytest.raises(AssertionError):
        masking.interpolateMaskedRegions(xml, [("c", 0, 100)], whole)


def test_cut_out_and_cut_pair(masking, tmp_path):
    rs = np.random.RandomState(9)
    raw = mr.random_masks(rs, 400, merged=False)
    xml = track_list(tmp_path, [raw[:150], raw[150:]])
    end = max(r[2] for r in raw) + 20
    region = [(c, 0, end) for c in mr.CHROMS[::-1]]
    pred = []
    for c in mr.CHROMS:
        cuts = sorted(set([0, end] + [int(x) for x in rs.randint(1, end, size=300)]))
        pred += [(c, a, b, "ABC"[rs.randint(3)], "0.5") for a, b in zip(cuts, cuts[1:])]
    for lo, hi in ((-1, None), (30, None), (-1, 41), (10, 60)):
        want = mr.cut_out(pred, raw, lo, hi)
        assert masking.cutOutMaskIntervals(pred, lo, hi, xml) == want and len(want) != len(pred)
    bed = str(tmp_path / "pred.bed")
    masking.writeBed(pred, bed)
    assert masking.cutOutMaskIntervals(bed, 30, None, xml) == mr.cut_out(pred, raw, 30, None)
    one, two = masking.cutPair(region, pred, xml, 30)
    assert one == mr.cut_out(region, raw, 30, None) and two == mr.cut_out(pred, raw, 30, None)
    assert [iv[0] for iv in one][0] == "chr1" and len(one) > 3
    # both cover the same bases afterwards: what checkExactOverlap needs
    cover = lambda ivs: mr.merge(mr.sort_intervals(ivs))
    assert cover(one) == cover(two)
    with pytest.raises(RuntimeError, match="removed everything"):
        masking.cutOutMaskIntervals([(raw[0][0], raw[0][1], raw[0][1] + 1)], -1, None, xml)      # inside a mask
    # mask tracks without a record: the input comes back sorted
    empty = tmp_path / "e"
    empty.mkdir()
    xml2 = track_list(empty, [[]])
    assert masking.cutOutMaskIntervals(region, -1, None, xml2) == mr.sort_intervals(region)
