"""GPU tests of the state comparison (tehmm_intervals_check, tehmm_compare_base, tehmm_compare_intervals,
tehmm_merge_runs, tehmm_amd/compare.py): every count is compared for exact equality with the plain-Python statement
(tests/compare_ref.py) and with what the real reference returned (tests/golden/compare.npz)."""
import ctypes
import itertools

import numpy as np
import pytest

import compare_ref as cr
from conftest import load_golden
from test_compare_cpu import COMPARE, FIT, TIE_PRED, TIE_TGT, ids, norm, one_sided, order, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cmp():
    from tehmm_amd import compare
    return compare


@pytest.fixture(scope="module")
def lib():
    from tehmm_amd import _lib
    return _lib.load()


def check_pair(cmp, iv1, iv2, thresholds=(0.5,), merge=True):
    """All three device calls on a pair of lists against the restatement."""
    assert cr.check_lists(iv1, iv2) == (0, -1)
    cmp.checkExactOverlap(iv1, iv2)
    got, want = cmp.compareBaseLevel(iv1, iv2, 3), cr.compare_base_level(iv1, iv2, 3)
    assert same(got[0], want[0]) and same(got[1], want[1])
    for thr in thresholds:
        for (t, p), upl, am in itertools.product(((iv1, iv2), (iv2, iv1)), (False, True), (False, True)):
            got, want = cmp.compareIntervalsOneSided(t, p, 3, thr, upl, am), \
                cr.compare_intervals_one_sided(t, p, 3, thr, upl, am)
            assert same(got[0], want[0]) and same(got[1], want[1]), (thr, upl, am)
    if merge:
        names = sorted({iv[3] for iv in iv2})
        for state_map in ({}, {n: ("m%d" % (k % 2), 1, 1) for k, n in enumerate(names)}):
            assert cmp.writeFittedBed(iv2, state_map, None, 3, False, ()) == \
                cr.fitted_bed(iv2, state_map, 3, False, ())[0]


def pair_of_length(rs, n, n_labels, start=50):
    """list 1 of exactly n intervals (a few regions with gaps between them), list 2 the same cover cut elsewhere"""
    iv1, iv2 = [], []
    pos = region = start
    for i in range(n):
        end = pos + int(rs.randint(1, 6))
        iv1.append(("chr1", pos, end, "s%d" % rs.randint(n_labels)))
        pos = end
        if i == n - 1 or rs.rand() < 0.02:
            cuts = [region] + [int(x) for x in np.flatnonzero(rs.rand(pos - region - 1) < 0.3) + region + 1] + [pos]
            iv2 += [("chr1", a, b, "s%d" % rs.randint(n_labels)) for a, b in zip(cuts[:-1], cuts[1:])]
            pos = region = pos + int(rs.randint(1, 9))
    return iv1, iv2


# ---- 1. goldens through the device -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", COMPARE, ids=ids(COMPARE))
def test_compare_fixture_on_the_device(case, cmp):
    iv1, iv2 = case["iv1"], case["iv2"]
    cmp.checkExactOverlap(iv1, iv2)
    stats, conf = cmp.compareBaseLevel(iv1, iv2, 3)
    assert stats == case["base_stats"] and conf == case["base_confMat"]
    assert order(stats) == case["base_stats_order"] and order(conf) == case["base_confMat_order"]
    assert norm(cmp.summarizeBaseComparision(stats, set())) == case["base_summary"]
    for swap, upl, am in itertools.product((False, True), repeat=3):
        t, p = (iv2, iv1) if swap else (iv1, iv2)
        want = one_sided(case, swap, upl, am)
        stats, conf = cmp.compareIntervalsOneSided(t, p, 3, case["thresh"], upl, am)
        assert stats == want["stats"] and conf == want["confMat"], (swap, upl, am)
        assert order(stats) == want["stats_order"] and order(conf) == want["confMat_order"], (swap, upl, am)
    trueStats = cmp.compareIntervalsOneSided(iv1, iv2, 3, case["thresh"], False, True)[0]
    predStats = cmp.compareIntervalsOneSided(iv2, iv1, 3, case["thresh"], False, True)[0]
    assert norm(cmp.summarizeIntervalComparison(trueStats, predStats, False, set())) == case["interval_summary"]


@pytest.mark.parametrize("case", FIT, ids=ids(FIT))
def test_fit_fixture_on_the_device(case, cmp, tmp_path):
    bed = tmp_path / "fit.bed"
    stateMap, fitted = cmp.fitStateNames(case["iv1"], case["iv2"], outBed=str(bed), col=4, **case["options"])
    assert norm(stateMap) == case["stateMap"]
    assert bed.read_text() == case["bed"]
    assert "".join("\t".join(str(x) for x in iv) + "\n" for iv in fitted) == case["bed"]


def test_a_tie_goes_to_the_pair_the_walk_meets_first(cmp):
    """equal counts: the reference takes the pair its walk inserted first, and so does the device's order"""
    got, want = cmp.compareBaseLevel(TIE_TGT, TIE_PRED, 3), cr.compare_base_level(TIE_TGT, TIE_PRED, 3)
    assert same(got[0], want[0]) and same(got[1], want[1])
    stateMap, fitted = cmp.fitStateNames(TIE_TGT, TIE_PRED, old=True)
    assert stateMap == {"Y": ("A", 5, 5), "X": ("B", 5, 10)}
    assert fitted == [("c", 0, 5, "A"), ("c", 5, 15, "B")]
    got = cmp.compareIntervalsOneSided(TIE_PRED, TIE_TGT, 3, 0.4, False, True)
    assert same(got[1], cr.compare_intervals_one_sided(TIE_PRED, TIE_TGT, 3, 0.4, False, True)[1])
    assert order(got[1]) == [["A", ["Y", "X"]], ["B", ["X"]]]


# ---- 2. list lengths and work splits -------------------------------------------------------------------------------------
LENGTHS = [("1", lambda B: 1), ("2", lambda B: 2), ("63", lambda B: 63), ("64", lambda B: 64), ("65", lambda B: 65),
           ("B-1", lambda B: B - 1), ("B", lambda B: B), ("B+1", lambda B: B + 1), ("3B+5", lambda B: 3 * B + 5)]


@pytest.mark.parametrize("name,length", LENGTHS, ids=[x[0] for x in LENGTHS])
def test_list_length_edges(name, length, cmp, lib):
    n = length(int(lib.tehmm_compare_block_items()))
    iv1, iv2 = pair_of_length(np.random.RandomState(n), n, 3)
    assert len(iv1) == n
    check_pair(cmp, iv1, iv2)
    check_pair(cmp, iv2, iv1)          # the merge and the true side on the list of exactly n too


def test_identical_breakpoints(cmp):
    rs = np.random.RandomState(12)
    iv1, _ = pair_of_length(rs, 700, 4)
    iv2 = [(c, a, b, "s%d" % rs.randint(4)) for c, a, b, _ in iv1]
    check_pair(cmp, iv1, iv2)


def test_no_breakpoint_in_common(cmp):
    rs = np.random.RandomState(13)
    end = 4 * 900 + 2
    iv1 = [("c", a, min(a + 4, end), "s%d" % rs.randint(3)) for a in range(0, end, 4)]
    cuts = [0] + list(range(2, end, 4)) + [end]
    iv2 = [("c", a, b, "s%d" % rs.randint(3)) for a, b in zip(cuts[:-1], cuts[1:])]
    assert {iv[1] for iv in iv1} & {iv[1] for iv in iv2} == {0}
    check_pair(cmp, iv1, iv2)


def test_one_interval_against_many(cmp):
    rs = np.random.RandomState(14)
    iv1 = [("c", 10, 5010, "s1")]
    cuts = [10] + sorted(int(x) for x in rs.choice(np.arange(11, 5010), 999, replace=False)) + [5010]
    iv2 = [("c", a, b, "s%d" % rs.randint(3)) for a, b in zip(cuts[:-1], cuts[1:])]
    check_pair(cmp, iv1, iv2, thresholds=(0.3, 1.0))
    check_pair(cmp, iv2, iv1, thresholds=(0.3,))


# ---- 3. label counts -----------------------------------------------------------------------------------------------------
def test_label_count_edges(cmp, lib):
    lds = int(lib.tehmm_compare_lds_labels())
    rs = np.random.RandomState(15)
    for L in (1, 2, lds, lds + 1, 2048):
        iv1, iv2 = pair_of_length(rs, 2 * L + 40, 1)
        # every one of the L names occurs, and both lists know the first and the last of them
        iv1 = [(c, a, b, "s%d" % ((7 * k) % L)) for k, (c, a, b, _) in enumerate(iv1)]
        iv2 = [(c, a, b, "s%d" % (L - 1 - (5 * k) % L)) for k, (c, a, b, _) in enumerate(iv2)]
        a, b, _, names = cmp.encodeIntervals(iv1, iv2, 3)
        assert len(names) == L
        check_pair(cmp, iv1, iv2, merge=L <= 2)
    # a label the table does not hold is refused, never used as an index
    from tehmm_amd._lib import TeHmmHipError
    a.label[3] = 2048
    with pytest.raises(TeHmmHipError) as e:
        cmp.baseConfusion(a, b, 2048)
    assert e.value.code == -1 and "interval 3 of list 1" in str(e.value)
    with pytest.raises(TeHmmHipError) as e:
        cmp.mergeRuns(a, 2048, np.zeros(2048, dtype=np.int32))
    assert e.value.code == -1 and "interval 3" in str(e.value)


# ---- 4. coordinates and chromosomes ----------------------------------------------------------------------------------------
def test_starts_above_2_pow_33(cmp):
    rs = np.random.RandomState(16)
    iv1, iv2 = cr.random_pair(rs, 40, 3, mean_len=25, chroms=2, start=2 ** 33 + 12345)
    assert min(iv[1] for iv in iv1) > 2 ** 33
    check_pair(cmp, iv1, iv2)
    # a long interval out there: the lengths are 64-bit too
    far = [("c", 2 ** 33, 2 ** 35, "x")]
    assert cmp.compareBaseLevel(far, far, 3) == ({"x": [0, 0, 2 ** 35 - 2 ** 33]}, {"x": {"x": 2 ** 35 - 2 ** 33}})


def test_300_chromosomes_of_one_interval(cmp):
    rs = np.random.RandomState(17)
    iv1, iv2 = [], []
    for c in range(300):
        a = int(rs.randint(0, 1000))
        n = int(rs.randint(1, 4))
        iv1.append(("chr%d" % c, a, a + 3 * n, "s%d" % rs.randint(3)))
        iv2 += [("chr%d" % c, a + 3 * k, a + 3 * k + 3, "s%d" % rs.randint(3)) for k in range(n)]
    check_pair(cmp, iv1, iv2)
    check_pair(cmp, iv2, iv1)


# ---- 5. a long true interval -----------------------------------------------------------------------------------------------
def test_long_true_interval_sums_in_order(cmp):
    rs = np.random.RandomState(18)
    n = 200000
    labels = np.where(rs.rand(n) < 0.7, "A", "B")
    true = [("c", 0, n, "A")]
    pred = [("c", k, k + 1, str(labels[k])) for k in range(n)]
    want_total = 0.0
    for k in range(n):
        if labels[k] == "A":
            want_total += 1.0 / float(n)
    for thr, hit in ((want_total, True), (np.nextafter(want_total, 1.0), False)):
        want = cr.compare_intervals_one_sided(true, pred, 3, thr, False, True)
        assert want[0] == {"A": [1, float(n), 0, 0.0] if hit else [0, 0.0, 1, float(n)]}
        assert cmp.compareIntervalsOneSided(true, pred, 3, thr, False, True) == want
    # the other side: every pred is a one-base true interval inside one long pred
    assert cmp.compareIntervalsOneSided(pred, true, 3, 0.5, True, True) == \
        cr.compare_intervals_one_sided(pred, true, 3, 0.5, True, True)


@pytest.mark.parametrize("n_pred", [100, 1000])
def test_in_order_total_misses_where_another_order_meets(n_pred, cmp):
    """Fractions whose sum in list order lies below their sum in descending order: with the latter as threshold the
    interval is a miss, with the former a hit.  100 preds stay in one lane, 1000 go through a wave."""
    for seed in range(200):
        rs = np.random.RandomState(seed)
        lens = rs.randint(1, 8, size=n_pred)
        total = int(lens.sum())
        fracs = [float(x) / float(total) for x in lens]
        in_order = 0.0
        for f in fracs:
            in_order += f
        other = 0.0
        for f in sorted(fracs, reverse=True):
            other += f
        if in_order < other:
            break
    assert in_order < other
    cuts = np.concatenate([[0], np.cumsum(lens)])
    true = [("c", 0, total, "A")]
    pred = [("c", int(a), int(b), "A") for a, b in zip(cuts[:-1], cuts[1:])]
    for thr, hit in ((other, False), (in_order, True)):
        want = cr.compare_intervals_one_sided(true, pred, 3, thr, False, True)
        assert (want[0]["A"][0] == 1) == hit
        assert cmp.compareIntervalsOneSided(true, pred, 3, thr, False, True) == want


# ---- 6. violations ---------------------------------------------------------------------------------------------------------
BASE = [("c", 0, 10, "x"), ("c", 10, 20, "y"), ("c", 30, 40, "x"), ("d", 5, 9, "x")]
VIOLATIONS = [
    ("unsorted", BASE, [BASE[1], BASE[0]] + BASE[2:], (2, 1)),
    ("unsorted_chrom", [BASE[0], BASE[3], BASE[1], BASE[2]], BASE, (1, 2)),
    ("empty_interval", BASE, BASE[:2] + [("c", 30, 30, "x")] + BASE[3:], (2, 2)),
    ("self_overlap_in_list_2", BASE, [BASE[0], ("c", 9, 20, "y")] + BASE[2:], (2, 1)),
    ("one_base_at_a_region_start", BASE, BASE[:2] + [("c", 31, 40, "x")] + BASE[3:], (1, 2)),
    ("one_base_at_a_region_end", BASE, BASE[:3] + [("d", 5, 10, "x")], (1, 3)),
    ("interior_gap", BASE, [BASE[0], ("c", 11, 20, "y")] + BASE[2:], (2, 0)),
    ("missing_chromosome", BASE, BASE[:3], (1, 3)),
]


@pytest.mark.parametrize("name,iv1,iv2,want", VIOLATIONS, ids=[v[0] for v in VIOLATIONS])
def test_violations_name_list_and_interval(name, iv1, iv2, want, cmp):
    from tehmm_amd._lib import TeHmmHipError
    assert cr.check_lists(iv1, iv2) == want
    a, b, _, names = cmp.encodeIntervals(iv1, iv2, 3)
    which, where, msg = cmp.checkArrays(a, b, len(names))
    assert (which, where) == want and "interval %d of list %d" % (want[1], want[0]) in msg
    with pytest.raises(RuntimeError, match="Interval %d of input%d" % (want[1], want[0])):
        cmp.checkExactOverlap(iv1, iv2)
    for call in (lambda: cmp.compareBaseLevel(iv1, iv2, 3),
                 lambda: cmp.compareIntervalsOneSided(iv1, iv2, 3, 0.8, False, True)):
        with pytest.raises(TeHmmHipError) as e:
            call()
        assert e.value.code == -1 and "interval %d of list %d" % (want[1], want[0]) in str(e.value)


# ---- 7. cap protocol ---------------------------------------------------------------------------------------------------------
def test_merge_cap_protocol(cmp, lib):
    from tehmm_amd._lib import i32p, i64p, ptr
    rs = np.random.RandomState(19)
    iv, _ = pair_of_length(rs, 3000, 2)
    want = cr.merge_runs(iv, 3)
    assert 1 < len(want) < len(iv)
    a, _, chroms, names = cmp.encodeIntervals(iv, None, 3)
    for cap in (len(want) - 1, len(want)):
        oc, ol = np.full(cap, -7, np.int32), np.full(cap, -7, np.int32)
        os_, oe = np.full(cap, -7, np.int64), np.full(cap, -7, np.int64)
        n_out = ctypes.c_int64(-1)
        rc = lib.tehmm_merge_runs(*(a.args() + (len(names), None, cap, ptr(oc, i32p), ptr(os_, i64p), ptr(oe, i64p),
                                                ptr(ol, i32p), ctypes.byref(n_out))))
        assert rc == 0 and n_out.value == len(want)
        if cap < len(want):
            assert all((x == -7).all() for x in (oc, ol, os_, oe))
        else:
            assert [(chroms[c], int(s), int(e), names[k]) for c, s, e, k in zip(oc, os_, oe, ol)] == want
    assert len(cmp.mergeRuns(a, len(names), _cap=5)) == len(want)          # the wrapper asks again
    assert [n for n, _ in cmp.lastTiming()][:2] == ["upload", "heads"]


# ---- 8. a decoded path, without a BED in between ------------------------------------------------------------------------------
def test_path_round_trip(cmp):
    from tehmm_amd.track import CategoryMap, IntegerTrackTable, Track, TrackList
    g = load_golden("segment_masked")
    gmap = CategoryMap(reserved=1, defaultVal="0", scale=float(g["gauss_scale"]))
    for v in sorted(set(float(v) for v in g["mapback"][1:] if np.isfinite(v))):      # the gaussian track's raw values
        gmap.getMap(v, update=True)
    gmap.sort()
    tracks = TrackList([Track("cat", 0), Track("gauss", 1, dist="gaussian", valueMap=gmap), Track("cat2", 2)])
    data, lens, start = g["data"], g["seg_lens"], int(g["start"])
    T = data.shape[0]
    mtab = IntegerTrackTable(2, "chrS", start, start + T)
    mtab.data = g["mask"].copy()
    tab = IntegerTrackTable(3, "chrS", start, start + T)
    tab.data = data.copy()
    tab.setMaskTable(mtab)
    seg_start = start + np.concatenate([[0], np.cumsum(lens)[:-1]])
    tab.segment([("chrS", int(a), int(a + l)) for a, l in zip(seg_start, lens)], tracks, interpolate=True)
    path = cmp.pathIntervals(tab, g["states"], names=["bg", "LTR", "LINE", "SINE"])
    assert "".join("%s\t%d\t%d\t%s\n" % (c, a, b, {"bg": 0, "LTR": 1, "LINE": 2, "SINE": 3}[n])
                   for c, a, b, n in path) == bytes(g["bed_text"]).decode()
    stats, conf = cmp.compareBaseLevel(path, path, 3)
    assert all(list(row) == [name] for name, row in conf.items())                      # diagonal
    assert sum(row[name] for name, row in conf.items()) == int(g["keep"].sum()) == sum(b - a for _, a, b, _ in path)
    assert all(v[:2] == [0, 0] for v in stats.values())
