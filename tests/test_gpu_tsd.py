"""GPU tests of the TSD finder and the overlap clean-up (tehmm_tsd_find, tehmm_remove_overlaps, tehmm_amd/tsd.py):
everything is compared for exact equality with the plain-Python statement (tests/tsd_ref.py) and with what the real
reference returned (tests/golden/tsd.npz)."""
import collections

import numpy as np
import pytest

import tsd_ref as tr
from test_tsd_cpu import CASES, ERR_ARG, ERR_UNSUPPORTED, FOUND, _clean, _find, ids, overrides

pytestmark = pytest.mark.gpu

BIG = tr.big_cases()
LISTS = tr.overlap_lists()
GOLDEN = {c[0]: c for c in tr.golden_cases()}
_want = {}


def want_of(name, seqs, ivs, opt):
    """the restatement's answer, computed once per case"""
    if name not in _want:
        _want[name] = tr.find_tsds(seqs, ivs, **opt)
    return _want[name]


@pytest.fixture(scope="module")
def tsd():
    from tehmm_amd import tsd
    return tsd


@pytest.fixture(scope="module")
def lib():
    from tehmm_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", FOUND, ids=ids(FOUND))
def test_device_equals_the_reference(tsd, case):
    opt = overrides(case)
    got = tsd.findTsds(collections.OrderedDict(case["sequences"]), case["intervals"], **opt)
    assert got == case["tsds"]
    assert got == want_of(case["name"], case["sequences"], case["intervals"], opt)


@pytest.mark.parametrize("case", BIG, ids=[c[0] for c in BIG])
def test_device_equals_the_restatement_beyond_one_workgroup(tsd, case):
    name, seqs, ivs, opt = case
    want = want_of(name, seqs, ivs, opt)
    assert len(ivs) > 2048 and len(want) > 0
    assert tsd.findTsds(collections.OrderedDict(seqs), ivs, **opt) == want
    if name == "dense_across_blocks":
        # 4096 matches per element on both sides of item 2048: the scan's carry crosses the workgroup boundary
        plan = tsd.planTsds(collections.OrderedDict(seqs), ivs)
        counts, cols = tsd.findMatches(plan.bases, plan.seqOffsets, plan.seqIndex, plan.start, plan.end,
                                       **{k: v for k, v in opt.items()})
        assert counts[2040:2056].tolist() == [4096] * 16 and counts.sum() == cols.shape[1] == len(want) // 2


def test_an_invalid_base_in_a_searched_window_names_the_lowest_element(tsd):
    from tehmm_amd._lib import TeHmmHipError
    case = next(c for c in CASES if c["asserts"])
    assert tr.lowest_invalid(case["sequences"], case["intervals"]) == 4
    with pytest.raises(TeHmmHipError) as e:
        tsd.findTsds(collections.OrderedDict(case["sequences"]), case["intervals"])
    assert e.value.code == ERR_ARG and "element 4 " in str(e.value)
    # without the two elements that search it, the same sequence is served
    ivs = [iv for x, iv in enumerate(case["intervals"]) if x not in (4, 5)]
    assert tsd.findTsds(collections.OrderedDict(case["sequences"]), ivs) == tr.find_tsds(case["sequences"], ivs)


def test_windows_of_64_are_served_and_65_refused(tsd):
    from tehmm_amd._lib import TeHmmHipError
    rs = np.random.RandomState(3)
    seqs = [("c", tr.random_bases(rs, 4000, "ac"))]
    ivs = tr.random_elements(rs, "c", 4000, 70, short=0.2)
    for opt in (dict(left=62, right=62, overlap=3), dict(left=65, right=40, overlap=0), dict(left=5, right=61, overlap=4)):
        opt.update(min=5, max=13)
        assert tsd.findTsds(collections.OrderedDict(seqs), ivs, **opt) == tr.find_tsds(seqs, ivs, **opt) != []
        opt["all"] = True
        assert tsd.findTsds(collections.OrderedDict(seqs), ivs, **opt) == tr.find_tsds(seqs, ivs, **opt)
    for opt in (dict(left=63, right=62, overlap=3), dict(left=7, right=66, overlap=0)):
        with pytest.raises(TeHmmHipError) as e:
            tsd.findTsds(collections.OrderedDict(seqs), ivs, **opt)
        assert e.value.code == ERR_UNSUPPORTED


def test_cap_and_n_out(tsd, lib):
    """*n_out is the number of matches whatever cap is, and the first min(*n_out, cap) rows are written"""
    name, seqs, ivs, opt = GOLDEN["defaults_all"]
    plan = tsd.planTsds(collections.OrderedDict(seqs), ivs)
    args = (plan.bases, plan.seqOffsets, plan.seqIndex, plan.start, plan.end)
    counts, cols = tsd.findMatches(*args, all=True)
    m = cols.shape[1]
    assert m == counts.sum() > 20
    for cap in (0, 1, 7, m - 1):
        c2, part = tsd.findMatches(*args, all=True, _cap=cap)              # grows to *n_out and calls again
        assert np.array_equal(c2, counts) and np.array_equal(part, cols)
    rc, n_out = _find(lib, bases=bytes(plan.bases), offsets=plan.seqOffsets, index=plan.seqIndex, start=plan.start,
                      end=plan.end, all_=1, cap=5)
    assert (rc, n_out) == (0, m)
    timing = tsd.lastTiming()
    assert [p for p, _ in timing] == ["upload", "find", "scan", "scatter", "download"] and all(ms >= 0 for _, ms in timing)
    rc, n_out = _find(lib, bases=bytes(plan.bases), offsets=plan.seqOffsets, index=plan.seqIndex, start=plan.start,
                      end=plan.end, all_=1, cap=0)
    assert (rc, n_out) == (0, m) and "scatter" not in [p for p, _ in tsd.lastTiming()]


def test_out_bed_and_track(tsd, tmp_path):
    name, seqs, ivs, opt = GOLDEN["records"]
    seqs_d = collections.OrderedDict(seqs)
    path = str(tmp_path / "tsd.bed")
    got = tsd.findTsds(seqs_d, ivs, outBed=path, **opt)
    assert open(path).read() == "".join("%s\t%d\t%d\t%s\t%d\n" % t for t in got) != ""
    existing = [("chr1", 10, 400, "old", 0), ("chr9", 5, 6, "old", 1)]
    want = tr.remove_overlaps_chain(tr.sort_intervals(tr.find_tsds(seqs, ivs, **opt) + existing))
    assert tsd.tsdTrack(seqs_d, ivs, existing=existing, append=True, **opt) == want
    assert tsd.tsdTrack(seqs_d, ivs, existing=existing, **opt) == \
        tr.remove_overlaps_chain(tr.sort_intervals(tr.find_tsds(seqs, ivs, **opt)))


# ---- the clean-up ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ivs", LISTS, ids=[n for n, _ in LISTS])
def test_remove_overlaps_equals_the_chain(tsd, name, ivs):
    want = tr.remove_overlaps_chain(tr.sort_intervals(ivs))
    assert tsd.removeBedOverlaps(ivs) == want
    assert len(want) < len(ivs) or len(ivs) == 1


def test_remove_overlaps_one_long_chromosome_and_one_per_interval(tsd):
    """the running maximum carried through every workgroup of the list, and dropped at every item"""
    rs = np.random.RandomState(11)
    n = 5000
    start = np.sort(rs.randint(0, 20000, size=n)).astype(np.int64)
    end = start + rs.randint(0, 40, size=n)
    end[7] = 15000                                           # one interval that swallows three quarters of the list
    for chrom in (np.zeros(n, np.int32), np.arange(n, dtype=np.int32), (np.arange(n) // 2048).astype(np.int32)):
        ivs = [(int(c), int(a), int(b)) for c, a, b in zip(chrom, start, end)]
        want = tr.remove_overlaps_running_max(ivs)
        idx, ns = tsd.removeOverlapsArrays(chrom, start, end)
        assert [(ivs[i][0], s, ivs[i][2]) for i, s in zip(idx.tolist(), ns.tolist())] == want
        part = tsd.removeOverlapsArrays(chrom, start, end, _cap=3)
        assert np.array_equal(part[0], idx) and np.array_equal(part[1], ns)


def test_remove_overlaps_names_the_first_offender(tsd, lib):
    n = 4100
    chrom, start = np.zeros(n, np.int32), np.arange(n, dtype=np.int64) * 2
    chrom[3000:] = 1
    start[3000:] -= 6000
    end = start + 3
    assert _clean(lib, chrom, start, end)[0] == 0
    edits = [({2500: (0, 4000)}, 2500),                       # a start below its predecessor's
             ({3500: (0, 1000)}, 3500),                       # a chrom id below its predecessor's
             ({4099: (1, 0)}, 4099),                          # the last interval
             ({3500: (0, 1000), 100: (0, 0)}, 100)]           # two offenders: the first is named
    for edit, where in edits:
        c2, s2 = chrom.copy(), start.copy()
        for i, (c, s) in edit.items():
            c2[i], s2[i] = c, s
        assert _clean(lib, c2, s2, end) == (ERR_ARG, 0)
        assert b"interval %d " % where in lib.tehmm_last_error()
    rc, n_out = _clean(lib, chrom, start, end, cap=0)
    assert (rc, n_out) == (0, len(tr.remove_overlaps_running_max(list(zip(chrom.tolist(), start.tolist(),
                                                                          end.tolist())))))
