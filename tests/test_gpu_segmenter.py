"""GPU tests of the segmenter (tehmm_segment_offsets_u8, tehmm_amd/segmenter.py): offsets are compared for exact
equality with the plain-Python statement of the reference's chain (tests/segmenter_ref.py) and with what the real
reference wrote (tests/golden/segmenter.npz)."""
import ctypes

import numpy as np
import pytest

import segmenter_ref as sr
from test_segmenter_cpu import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seg():
    from tehmm_amd import segmenter
    return segmenter


@pytest.fixture(scope="module")
def S():
    from tehmm_amd import _lib
    return int(_lib.load().tehmm_segment_stripe_rows())


def check_tables(seg, tables, cut, ign, **opt):
    """Device offsets of all tables in one call against the per-table restatement."""
    got = seg.segmentOffsets(tables, cut, ign, **opt)
    assert len(got) == len(tables)
    for t, (d, g) in enumerate(zip(tables, got)):
        want = sr.segment_offsets(d, ign, cut, opt.get("thresh", 1), opt.get("comp", "first"), opt.get("maxLen", 0),
                                  opt.get("fixLen", 0))
        assert g.dtype == np.int64 and np.array_equal(g, want), \
            "table %d of %d rows: first mismatch at entry %d" % (
                t, len(d), int(np.argmax(g[:min(len(g), len(want))] != want[:min(len(g), len(want))])))
    return got


# ---- 1. fixture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_on_the_device(case, seg, tmp_path):
    from tehmm_amd.track import IntegerTrackTable, Track, TrackData, TrackList
    K = case["data"].shape[1]
    opt = dict(thresh=case["thresh"], comp=case["comp"], maxLen=case["maxLen"], fixLen=case["fixLen"])
    offsets, (count, share) = seg.segmentOffsets(case["tables"], case["cut"], case["ignore"], stats=True, **opt)
    spans = [(c, s, s + n) for c, s, n in zip(case["chroms"], case["starts"], case["lens"])]
    rows = sr.bed_rows(spans, offsets, co=case["co"])
    assert "".join("%s\t%d\t%d\t%s\n" % r for r in rows) == case["bed"]          # offsets and labels
    want_count = np.zeros(K, dtype=np.int64)
    want_share = np.zeros(K)
    want_count[case["stats_tracks"]] = case["stats_count"]
    want_share[case["stats_tracks"]] = case["stats_share"]
    assert np.array_equal(count, want_count)
    # the same positive terms in another order: each sum is within n 2^-53 of the exact one, n <= 2^20
    np.testing.assert_allclose(share, want_share, rtol=1e-9, atol=0)
    # the whole pipeline: names of cut / ignored tracks in, BED and stats text out
    tl = TrackList([Track("t%d" % k, k) for k in range(K)])
    tabs = [IntegerTrackTable(K, c, int(s), int(s + n)).setData(d)
            for c, s, n, d in zip(case["chroms"], case["starts"], case["lens"], case["tables"])]
    names = lambda v: ",".join("t%d" % k for k in range(K) if v[k]) or None
    bed, stats = tmp_path / "out.bed", tmp_path / "out.stats"
    ivs = seg.segmentTracks(TrackData(tabs, tl), str(bed), cutTracks=names(case["cut"]), ignore=names(case["ignore"]),
                            co=case["co"], statsPath=str(stats), **opt)
    assert bed.read_text() == case["bed"]
    assert [tuple(iv) for iv in ivs] == [r[:3] for r in rows]
    assert stats.read_text() == "".join("t%d\t%d\t%f\n" % (k, c, s / c) for k, c, s in
                                        zip(case["stats_tracks"], case["stats_count"], case["stats_share"]))


# ---- 2. stripe edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 4, 5, 16, 17])
def test_stripe_edges(K, seg, S):
    rs = np.random.RandomState(K)
    lens = [1, 2, 63, 64, 65, S - 1, S, S + 1, 3 * S + 5]
    tables = [sr.run_structured(rs, T, K, keep=0.9) for T in lens]
    cut = np.zeros(K, dtype=np.uint8)
    ign = np.zeros(K, dtype=np.uint8)
    if K >= 3:
        cut[K - 1] = 1                                  # the last track: in the padded dword when K % 4 != 0
        ign[1] = 1
    for comp in ("first", "prev"):
        for thresh in (0, 1):
            check_tables(seg, tables, cut, ign, comp=comp, thresh=thresh)


def _table_with_cuts(T, K, cuts):
    """Constant between the given rows; every listed row changes all tracks (a cut under any thresh < K)."""
    d = np.zeros((T, K), dtype=np.uint8)
    for n, c in enumerate(sorted(cuts)):
        d[c:] = (n % 250) + 1
    return d


@pytest.mark.parametrize("comp", ["first", "prev"])
def test_true_cuts_at_stripe_borders(comp, seg, S):
    K = 3
    none = np.zeros(K, dtype=np.uint8)
    tables = [
        _table_with_cuts(3 * S + 5, K, [S - 1, 2 * S - 1, 3 * S - 1]),           # last row of a stripe
        _table_with_cuts(3 * S + 5, K, [S, 2 * S, 3 * S]),                       # first row of a stripe
        _table_with_cuts(4 * S + 9, K, [S // 2, 3 * S + S // 2]),                # a segment longer than 2 S
        _table_with_cuts(4 * S + 9, K, []),                                      # one segment
        _table_with_cuts(2 * S, K, [S - 1, S, S + 1]),
    ]
    got = check_tables(seg, tables, none, none, comp=comp, thresh=1)
    assert got[0].tolist() == [0, S - 1, 2 * S - 1, 3 * S - 1] and got[1].tolist() == [0, S, 2 * S, 3 * S]
    assert got[2].tolist() == [0, S // 2, 3 * S + S // 2] and got[3].tolist() == [0]
    # first mode, a change that only counts against the segment's first row: tracks drift one at a time
    d = np.zeros((3 * S + 5, K), dtype=np.uint8)
    d[S - 2:, 0] = 1                                                             # one track differs: no cut at thresh 1
    d[S:, 1] = 1                                                                 # two differ from row 0: cut at S (first)
    check_tables(seg, [d], none, none, comp=comp, thresh=1)


# ---- 3. many tables --------------------------------------------------------------------------------------------------
def test_many_tables_in_one_call(seg, S, tmp_path):
    from tehmm_amd import _lib
    from tehmm_amd._lib import i64p, ptr, u8p
    rs = np.random.RandomState(7)
    K = 4
    lens = np.concatenate([[1, 2, S + 7, S, S + 1, 1], rs.randint(1, S + 8, size=294)])
    assert len(lens) == 300
    # rows of neighbouring tables differ in every track: a leak across a boundary would show as a cut
    tables = [sr.run_structured(rs, int(T), K, keep=0.9) for T in lens]
    cut = np.asarray([0, 0, 1, 0], dtype=np.uint8)
    ign = np.asarray([1, 0, 0, 0], dtype=np.uint8)
    for comp, maxLen in (("first", 0), ("prev", 0), ("first", 40), ("prev", 40)):
        want = [sr.segment_offsets(d, ign, cut, 1, comp, maxLen) for d in tables]
        # the raw call: n_cuts per table and the concatenated table-relative offsets
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        data = np.ascontiguousarray(np.concatenate(tables, axis=0))
        cap = int(offs[-1])
        cuts = np.full(cap, -1, dtype=np.int64)
        n_cuts = np.zeros(300, dtype=np.int64)
        n_total = ctypes.c_int64(0)
        rc = _lib.load().tehmm_segment_offsets_u8(300, ptr(offs, i64p), K, ptr(data, u8p), ptr(ign, u8p),
                                                  ptr(cut, u8p), 1, int(comp == "prev"), maxLen, 0, cap,
                                                  ptr(cuts, i64p), ptr(n_cuts, i64p), ctypes.byref(n_total), None)
        assert rc == 0
        assert n_cuts.tolist() == [len(w) for w in want] and n_total.value == sum(len(w) for w in want)
        assert np.array_equal(cuts[:n_total.value], np.concatenate(want)) and np.all(cuts[n_total.value:] == -1)
    # the label counter runs across the tables
    from tehmm_amd.track import IntegerTrackTable, Track, TrackData, TrackList
    tl = TrackList([Track("t%d" % k, k) for k in range(K)])
    tabs = [IntegerTrackTable(K, "chr%d" % (n % 5), 100 * n, 100 * n + len(d)).setData(d)
            for n, d in enumerate(tables[:40])]
    bed = tmp_path / "many.bed"
    seg.segmentTracks(TrackData(tabs, tl), str(bed), cutTracks="t2", ignore="t0", comp="prev", maxLen=40, co=7)
    rows = sr.bed_rows([(t.getChrom(), t.getStart(), t.getEnd()) for t in tabs], want[:40], co=7)
    assert bed.read_text() == "".join("%s\t%d\t%d\t%s\n" % r for r in rows)


# ---- 4. chains that never meet their speculation ---------------------------------------------------------------------
def _next_prime_not_dividing(S, p):
    def is_prime(n):
        return n > 1 and all(n % q for q in range(2, int(n ** 0.5) + 1))
    while S % p == 0 or not is_prime(p):
        p += 1
    return p


def test_drift_never_meets_its_speculation(seg, S):
    """Row t copies row t - 1 and sets track t % P to a new value; with thresh = P - 1 against the segment's first row
    the true chain cuts at every multiple of P, while a stripe that does not start on a multiple speculates on
    another residue and never coincides."""
    P = 3 if S % 3 else 5
    K, T = P, 7 * S + 5
    d = np.ones((T, K), dtype=np.uint8)
    for t in range(1, T):
        d[t] = d[t - 1]
        d[t, t % P] = (t // P) % 250 + 2
    none = np.zeros(K, dtype=np.uint8)
    tables = [d] if S % 3 else [np.ones((1, K), dtype=np.uint8), d]
    got = check_tables(seg, tables, none, none, comp="first", thresh=P - 1)
    assert got[-1].tolist() == list(range(0, T, P))
    stripes, rewalked = seg.lastCounters()
    assert stripes >= 8 and rewalked > 0, "the exact walk was not exercised"


@pytest.mark.parametrize("comp,which", [("first", 7), ("first", "S+3"), ("prev", 19)])
def test_maxlen_never_meets_its_speculation(comp, which, seg, S):
    maxLen = S + 3 if which == "S+3" else _next_prime_not_dividing(S, which)
    T = 7 * S + 5
    d = np.full((T, 2), 3, dtype=np.uint8)
    none = np.zeros(2, dtype=np.uint8)
    got = check_tables(seg, [d], none, none, comp=comp, thresh=1, maxLen=maxLen)
    assert got[0].tolist() == list(range(0, T, maxLen))
    stripes, rewalked = seg.lastCounters()
    assert stripes == 8 and rewalked > 0, "the exact walk was not exercised"


# ---- 5. no chain where none is needed --------------------------------------------------------------------------------
def test_no_chain_where_none_is_needed(seg, S):
    rs = np.random.RandomState(11)
    K = 5
    tables = [sr.run_structured(rs, T, K, keep=0.9) for T in (3 * S + 5, 1, 77)]
    none = np.zeros(K, dtype=np.uint8)
    check_tables(seg, tables, none, none, comp="prev", thresh=1)
    assert seg.lastCounters() == (0, 0)
    for comp in ("first", "prev"):
        for fixLen in (1, 5, S, 10 * S):
            got = check_tables(seg, tables, none, none, comp=comp, thresh=1, maxLen=3, fixLen=fixLen)
            assert seg.lastCounters() == (0, 0)
            for d, g in zip(tables, got):
                assert g.tolist() == list(range(0, len(d), fixLen))
    check_tables(seg, tables, none, none, comp="first", thresh=1)              # and a chain is reported as one
    assert seg.lastCounters()[0] == 6


# ---- 6. statistics under maxLen --------------------------------------------------------------------------------------
@pytest.mark.parametrize("comp", ["first", "prev"])
def test_statistics_under_maxlen(comp, seg, S):
    rs = np.random.RandomState(13)
    K = 6
    tables = [sr.run_structured(rs, T, K, keep=0.93) for T in (S + 300, 500)]
    cut = np.asarray([0, 0, 0, 0, 1, 0], dtype=np.uint8)
    ign = np.asarray([0, 1, 0, 0, 0, 0], dtype=np.uint8)
    for maxLen in (0, 6):
        stats = {}
        want = [sr.segment_offsets(d, ign, cut, 1, comp, maxLen, stats=stats) for d in tables]
        got, (count, share) = seg.segmentOffsets(tables, cut, ign, thresh=1, comp=comp, maxLen=maxLen, stats=True)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        want_count = np.asarray([stats.get(k, [0, 0.0])[0] for k in range(K)])
        assert np.array_equal(count, want_count) and count[1] == 0
        np.testing.assert_allclose(share, [stats.get(k, [0, 0.0])[1] for k in range(K)], rtol=1e-9, atol=0)
        if maxLen:
            # some cuts come from maxLen, others from the data; only the latter are counted
            lens = np.concatenate([np.diff(w) for w in want])
            n_data_cuts = int(np.sum(lens < maxLen))
            assert 0 < n_data_cuts < len(lens) and count.max() <= n_data_cuts
    # a table cut by maxLen alone has no statistics at all
    flat = np.full((100, K), 2, dtype=np.uint8)
    _, (count, share) = seg.segmentOffsets([flat], cut, ign, comp=comp, maxLen=6, stats=True)
    assert not count.any() and not share.any()


# ---- 7. capacity -----------------------------------------------------------------------------------------------------
def test_capacity(seg, S):
    from tehmm_amd import _lib
    from tehmm_amd._lib import i64p, ptr, u8p
    rs = np.random.RandomState(17)
    K = 3
    tables = [sr.run_structured(rs, T, K, keep=0.8) for T in (S + 40, 300)]
    none = np.zeros(K, dtype=np.uint8)
    want = [sr.segment_offsets(d, none, none, 0) for d in tables]
    total = sum(len(w) for w in want)
    offs = np.asarray([0, S + 40, S + 340], dtype=np.int64)
    data = np.ascontiguousarray(np.concatenate(tables, axis=0))
    for cap in (0, 5, total - 1):
        cuts = np.full(max(cap, 1), -77, dtype=np.int64)
        n_cuts = np.zeros(2, dtype=np.int64)
        n_total = ctypes.c_int64(0)
        rc = _lib.load().tehmm_segment_offsets_u8(2, ptr(offs, i64p), K, ptr(data, u8p), ptr(none, u8p),
                                                  ptr(none, u8p), 0, 0, 0, 0, cap, ptr(cuts, i64p), ptr(n_cuts, i64p),
                                                  ctypes.byref(n_total), None)
        assert rc == 0 and n_total.value == total and n_cuts.tolist() == [len(w) for w in want]
        assert np.all(cuts == -77)
    got = seg.segmentOffsets(tables, none, none, thresh=0, _cap=5)              # the wrapper's second call
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


# ---- 8. arguments ----------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_any_device_work():
    from tehmm_amd import _lib
    from tehmm_amd._lib import i64p, ptr, u8p
    lib = _lib.load()
    d = np.zeros((10, 129), dtype=np.uint8)
    flags = np.zeros(129, dtype=np.uint8)
    cuts = np.zeros(16, dtype=np.int64)
    n_cuts = np.zeros(4, dtype=np.int64)
    n_total = ctypes.c_int64(0)

    def call(offs, K, data, thresh=1):
        offs = np.asarray(offs, dtype=np.int64)
        return lib.tehmm_segment_offsets_u8(len(offs) - 1, ptr(offs, i64p), K, data, ptr(flags, u8p), ptr(flags, u8p),
                                            thresh, 0, 0, 0, 16, ptr(cuts, i64p), ptr(n_cuts, i64p),
                                            ctypes.byref(n_total), None)
    for args, kw, word in ((([0, 10], 129, ptr(d, u8p)), {}, b"128 tracks"),
                           (([0, 4, 4, 10], 3, ptr(d, u8p)), {}, b"no empty table"),
                           (([0, 6, 4, 10], 3, ptr(d, u8p)), {}, b"ascend"),
                           (([0, 10], 3, None), {}, b"bad argument"),
                           (([0, 10], 3, ptr(d, u8p)), {"thresh": -1}, b"thresh")):
        rc = call(*args, **kw)
        assert rc in (-1, -3)                            # TEHMM_ERR_ARG / TEHMM_ERR_UNSUPPORTED
        msg = lib.tehmm_last_error()
        assert msg.startswith(b"tehmm_segment_offsets_u8") and word in msg
    assert call([0, 10], 3, ptr(d, u8p)) == 0 and n_total.value == 1


# ---- 9. end to end ---------------------------------------------------------------------------------------------------
def test_end_to_end_segment_then_decode(seg, tmp_path):
    from tehmm_amd import synth
    from tehmm_amd.emission import IndependentMultinomialEmissionModel
    from tehmm_amd.hmm import MultitrackHmm
    from tehmm_amd.track import IntegerTrackTable, Track, TrackData, TrackList
    model = synth.make_model(5, seed=3)
    K = model.log_probs.shape[0]
    syms = [int(s) for s in model.symbols_per_track]
    lens = (1500, 400)
    tl = TrackList([Track("t%d" % k, k) for k in range(K)])

    def tables():
        r = np.random.RandomState(23)
        out = []
        for n, T in enumerate(lens):
            d = np.minimum(sr.run_structured(r, T, K, keep=0.9, n_values=2) + 1, np.asarray(syms)).astype(np.uint8)
            out.append(IntegerTrackTable(K, "chr%d" % n, 50, 50 + T).setData(d))
        return out

    def decode(tabs, intervals):
        for t in tabs:
            t.segment(intervals, tl)
        em = IndependentMultinomialEmissionModel(model.n_states, syms, effectiveSegmentLength=8)
        em.logProbs = model.log_probs.copy()
        h = MultitrackHmm(em)
        h.transmat_ = model.transmat.copy()
        h.startprob_ = np.exp(model.log_startprob)
        return h.viterbi(TrackData(tabs, tl))

    tabs = tables()
    ivs = seg.segmentTracks(TrackData(tabs, tl), str(tmp_path / "seg.bed"), thresh=1, ignore=None)
    none = np.zeros(K, dtype=np.uint8)
    ref_tabs = tables()
    ref_ivs = [r[:3] for r in sr.bed_rows([(t.getChrom(), t.getStart(), t.getEnd()) for t in ref_tabs],
                                          [sr.segment_offsets(t.getNumPyArray(), none, none, 1) for t in ref_tabs])]
    assert [tuple(iv) for iv in ivs] == ref_ivs and len(ivs) > 20
    out, ref_out = decode(tabs, ivs), decode(ref_tabs, ref_ivs)
    assert len(out) == 2
    for (lp, path), (rlp, rpath), t in zip(out, ref_out, tabs):
        assert len(path) == len(t) and np.array_equal(path, rpath) and lp == rlp
