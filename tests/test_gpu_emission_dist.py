"""GPU tests of the device-side emission distribution (tehmm_edist.hip.h): the frames of
MultitrackHmm.emissionDistribution (hmm.py:265-277) and the masked column of teHmmEval --ed (teHmmEval.py:273-275).

Expected values: oracle.emission applied per interval (the reference calls fastAllLogProbs once per table, so its
leading-rows rule, quirk Q9, is per interval), then np.log(np.sum(np.exp(frame) * mask, axis=1)).  Frames are held bit
for bit.  Columns are held to rtol 1e-12, atol 1e-10: the error of the log is the relative error of an N-term positive
sum plus a few ulp of exp and log, at most about (N + 8) * 2**-52 = 2.3e-13 at N = 1024; the inputs keep every masked
sum either exactly 0 (then the column must be -inf) or >= 1e-280, clear of the denormal range -- asserted on the
expected values.

The model tables carry -1e100 (myLog(0)) cells:
  * symbol 1 of track 0: the states j % 3 == 0 cannot emit it, so they contribute exactly 0 to such a row and a mask
    that selects only them gives -inf there;
  * symbol 2 of track 0: no state can emit it -- the "impossible" rows of the Q9 cases, planted by hand only;
  * the last symbol of the table lies beyond every track's last one: the zero padding.
Intervals: 65, 1000, 1, 2, 63, 64 rows (they straddle the 64-aligned internal bases).  The SECOND interval starts with
three impossible rows (zeroed) and holds a later one (not zeroed); the first interval starts with an emittable row."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

pytestmark = pytest.mark.gpu

LENS = [65, 1000, 1, 2, 63, 64]
SYMS = (3, 5, 4, 2, 6, 3, 7, 2, 4, 5)
N_ALL = [1, 5, 35, 64, 65, 128, 129, 300, 1024]
K_ALL = [1, 3, 4, 5, 10]
LATE = 10                     # a later impossible row of the second interval
ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib, build
    build.build()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


OFFS = _offsets(LENS)
_cache = {}


def _case(N, K, normalize=1.0):
    """(log_probs [K][N][S], symbols, obs uint8 [T][K], ratios [T], expected frames without / with ratios); computed
    once per shape and never changed."""
    key = (N, K, normalize)
    if key in _cache:
        return _cache[key]
    from oracle import oracle
    rs = np.random.RandomState(1000 * N + K)
    sym = list(SYMS[:K])
    S = max(sym) + 2                                   # symbol S - 1 is beyond every track's last one
    lp = np.zeros((K, N, S))
    for k, sk in enumerate(sym):
        p = 0.2 + 0.6 * rs.rand(N, sk)
        lp[k, :, 1:1 + sk] = np.log(p / p.sum(axis=1, keepdims=True))
    lp[0, np.arange(N) % 3 == 0, 1] = -1e100
    lp[0, :, 2] = -1e100
    T = int(OFFS[-1])
    obs = np.empty((T, K), dtype=np.uint8)
    obs[:, 0] = rs.choice([0, 1, 3], size=T)
    for k in range(1, K):
        obs[:, k] = rs.randint(0, sym[k] + 1, size=T)
    obs[rs.rand(T) < 0.05, K - 1] = S - 1              # the zero padding (on track 0 when K = 1)
    obs[0, 0] = 3                                      # the first interval starts with an emittable row
    obs[OFFS[1]:OFFS[1] + 3, 0] = 2                    # the second with three impossible ones
    obs[OFFS[1] + 3, 0] = 3
    obs[OFFS[1] + LATE, 0] = 2
    obs[OFFS[1] + 20, 0] = 1
    ratios = np.minimum(1 + rs.geometric(1.0 / 20.0, size=T), 100).astype(np.float64) / 20.0
    exp = {}
    for with_r in (False, True):
        exp[with_r] = np.concatenate([
            oracle.emission(obs[a:b], lp, normalize, ratios[a:b] if with_r else None)
            for a, b in zip(OFFS[:-1], OFFS[1:])])
        exp[with_r].setflags(write=False)
    _cache[key] = (lp, sym, obs, ratios, exp)
    return _cache[key]


def _masks(N):
    dead = (np.arange(N) % 3 == 0).astype(np.float64)
    one = np.zeros(N)
    one[N - 1] = 1.0
    return {"ones": np.ones(N), "single": one, "dead": dead}


def _column(frame, mask):
    with np.errstate(divide="ignore"):
        sums = np.sum(np.exp(frame) * mask, axis=1)
        col = np.log(sums)
    # the derivation of the tolerance needs the sums out of the denormal range
    assert np.all((sums == 0.0) | (sums >= 1e-280))
    return col


def _check_column(got, want):
    inf = np.isneginf(want)
    assert_array_equal(np.isneginf(got), inf)
    assert np.all(np.isfinite(got[~inf]))
    assert_allclose(got[~inf], want[~inf], rtol=1e-12, atol=1e-10)


def _possible(obs):
    """The observations without their impossible rows (for the cases that also run the dynamic programs)."""
    out = obs.copy()
    out[out[:, 0] == 2, 0] = 3
    return out


def _handles(N, K, normalize=1.0, dtype=np.uint8, with_ratios=True, possible=False):
    from tehmm_amd.engine import HipBatch, HipModel
    lp, sym, obs, ratios, exp = _case(N, K, normalize)
    if possible:
        obs = _possible(obs)
    rs = np.random.RandomState(N)
    lt = np.log(rs.dirichlet(np.ones(N), size=N))
    hm = HipModel(lt, np.log(np.full(N, 1.0 / N)), lp, normalize, sym)
    hb = HipBatch(obs.astype(dtype), OFFS, ratios if with_ratios else None)
    return hm, hb


@pytest.mark.parametrize("K", K_ALL)
@pytest.mark.parametrize("N", N_ALL)
def test_frames_and_columns_vs_oracle(N, K):
    lp, sym, obs, ratios, exp = _case(N, K)
    hm, hb = _handles(N, K)
    n_inf = 0
    for with_r in (False, True):
        frame = hb.emissions(hm, use_ratios=with_r)
        assert frame.shape == exp[with_r].shape
        assert_array_equal(frame, exp[with_r])
        for name, mask in _masks(N).items():
            want = _column(exp[with_r], mask)
            got = hb.emission_masksum(hm, mask, use_ratios=with_r)
            _check_column(got, want)
            if name == "dead":
                n_inf += int(np.isneginf(want).sum())
                assert np.isneginf(want[OFFS[1] + 20])
    assert n_inf > 0
    hb.close()
    hm.close()


@pytest.mark.parametrize("N,K", [(35, 10), (5, 3), (129, 4), (64, 5)])
def test_leading_rows_rule_is_per_interval(N, K):
    lp, sym, obs, ratios, exp = _case(N, K)
    hm, hb = _handles(N, K)
    a = int(OFFS[1])
    for with_r in (False, True):
        frame = hb.emissions(hm, use_ratios=with_r)
        assert np.all(frame[a:a + 3] == 0.0)                       # all-zero frames ...
        assert np.all(frame[a + 3] != 0.0)
        assert np.all(frame[a + LATE] <= -1e20)                    # ... but a later impossible row is not zeroed
        assert np.any(frame[0] > -1e20)
        for mask in _masks(N).values():
            col = hb.emission_masksum(hm, mask, use_ratios=with_r)
            assert_allclose(col[a:a + 3], np.log(mask.sum()), rtol=1e-12, atol=1e-10)
            assert np.isneginf(col[a + LATE])
            # row0 inside the interval, behind / among its leading rows: the same values
            for r0, r1 in ((a + 1, a + 5), (a + 2, a + 3), (a + 3, a + 30)):
                assert_array_equal(hb.emission_masksum(hm, mask, use_ratios=with_r, row0=r0, row1=r1), col[r0:r1])
                assert_array_equal(hb.emissions(hm, use_ratios=with_r, row0=r0, row1=r1), frame[r0:r1])
    hb.close()
    hm.close()


@pytest.mark.parametrize("N,K", [(5, 3), (35, 10), (300, 4)])
def test_row_ranges_and_repeat_calls(N, K):
    hm, hb = _handles(N, K)
    mask = _masks(N)["ones"]
    frame = hb.emissions(hm, use_ratios=True)
    col = hb.emission_masksum(hm, mask, use_ratios=True)
    assert_array_equal(hb.emissions(hm, use_ratios=True), frame)               # two calls are bit-identical
    assert_array_equal(hb.emission_masksum(hm, mask, use_ratios=True), col)
    r0, r1 = int(OFFS[2]) - 5, int(OFFS[3]) + 1                                 # crosses two interval boundaries
    assert r0 < OFFS[2] < OFFS[3] < r1
    assert_array_equal(hb.emissions(hm, use_ratios=True, row0=r0, row1=r1), frame[r0:r1])
    assert_array_equal(hb.emission_masksum(hm, mask, use_ratios=True, row0=r0, row1=r1), col[r0:r1])
    for r0, r1 in ((0, 1), (63, 66), (int(OFFS[-1]) - 1, int(OFFS[-1])), (100, 100)):
        assert_array_equal(hb.emissions(hm, use_ratios=True, row0=r0, row1=r1, pinned=False), frame[r0:r1])
        assert_array_equal(hb.emission_masksum(hm, mask, use_ratios=True, row0=r0, row1=r1), col[r0:r1])
    t = hb.timing()
    assert t["emission_column"] >= 0.0 and t["emission_frame"] >= 0.0
    hb.close()
    hm.close()


@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
@pytest.mark.parametrize("N,K", [(35, 10), (129, 3)])
def test_wider_observation_types(N, K, dtype):
    lp, sym, obs, ratios, exp = _case(N, K)
    hm, hb = _handles(N, K, dtype=dtype)
    for with_r in (False, True):
        assert_array_equal(hb.emissions(hm, use_ratios=with_r), exp[with_r])
    _check_column(hb.emission_masksum(hm, _masks(N)["dead"], use_ratios=True), _column(exp[True], _masks(N)["dead"]))
    hb.close()
    hm.close()


def test_normalize_factor_and_array_level_agreement():
    from tehmm_amd import _emission
    N, K, nf = 35, 10, 0.3
    lp, sym, obs, ratios, exp = _case(N, K, nf)
    hm, hb = _handles(N, K, nf)
    for with_r in (False, True):
        frame = hb.emissions(hm, use_ratios=with_r)
        assert_array_equal(frame, exp[with_r])
        a, b = int(OFFS[1]), int(OFFS[2])
        out = np.zeros((b - a, N))
        _emission.fastAllLogProbs(obs[a:b], lp, out, nf, ratios[a:b] if with_r else None)     # tehmm_emission_u8
        assert_array_equal(frame[a:b], out)
        for mask in _masks(N).values():
            _check_column(hb.emission_masksum(hm, mask, use_ratios=with_r), _column(exp[with_r], mask))
    hb.close()
    hm.close()


def test_evaluation_results_are_not_disturbed():
    N, K = 35, 10
    mask = _masks(N)["single"]
    hm, hb = _handles(N, K, possible=True)

    def run(between):
        res = hm.eval(hb, viterbi=True, posterior=True, use_ratios=True)
        mlp = hb.map_decode(mask)
        if between:                                    # between the evaluation and the result fetches
            hb.emission_masksum(hm, _masks(N)["dead"], use_ratios=True)
            hb.emissions(hm)
            hb.emission_masksum(hm, mask, row0=70, row1=1100)
        out = [res["viterbi_logprob"], res["forward_logprob"], mlp, hb.paths(), hb.posteriors(),
               hb.posterior_masksum(mask), hb.map_paths(), hb.map_masksum(), hb.interval_logprobs()]
        return out, set(hb.timing())
    mixed, names1 = run(True)
    plain, names0 = run(False)                         # the same evaluation without the new calls
    for a, b in zip(plain, mixed):
        assert_array_equal(a, b)
    assert names1 == names0 | {"emission_column", "emission_frame"}
    hb.close()
    hm.close()


def test_no_evaluation_needed_and_errors():
    from tehmm_amd import _lib
    from tehmm_amd._lib import f64p, ptr
    N, K = 5, 3
    hm, hb = _handles(N, K, with_ratios=False)
    lib = _lib.load()
    mask = np.ones(N)
    out = np.zeros(int(OFFS[-1]) * N)
    T = int(OFFS[-1])
    assert lib.tehmm_batch_emission_masksum(hm._h, hb._h, 0, ptr(mask, f64p), 0, T, ptr(out, f64p)) == 0
    # use_ratios on a batch without ratios
    assert lib.tehmm_batch_emission_masksum(hm._h, hb._h, 1, ptr(mask, f64p), 0, T, ptr(out, f64p)) == ERR_ARG
    assert b"ratios" in lib.tehmm_last_error()
    assert lib.tehmm_batch_get_emissions(hm._h, hb._h, 1, 0, T, ptr(out, f64p)) == ERR_ARG
    # bad row ranges
    for r0, r1 in ((-1, 4), (5, 4), (0, T + 1)):
        assert lib.tehmm_batch_emission_masksum(hm._h, hb._h, 0, ptr(mask, f64p), r0, r1, ptr(out, f64p)) == ERR_ARG
        assert lib.tehmm_batch_get_emissions(hm._h, hb._h, 0, r0, r1, ptr(out, f64p)) == ERR_ARG
    # NULL arguments
    assert lib.tehmm_batch_emission_masksum(hm._h, hb._h, 0, None, 0, T, ptr(out, f64p)) == ERR_ARG
    assert lib.tehmm_batch_emission_masksum(hm._h, hb._h, 0, ptr(mask, f64p), 0, T, None) == ERR_ARG
    assert lib.tehmm_batch_get_emissions(None, hb._h, 0, 0, T, ptr(out, f64p)) == ERR_ARG
    assert lib.tehmm_batch_get_emissions(hm._h, None, 0, 0, T, ptr(out, f64p)) == ERR_ARG
    # K mismatch
    hm4, hb4 = _handles(N, 4, with_ratios=False)
    assert lib.tehmm_batch_emission_masksum(hm._h, hb4._h, 0, ptr(mask, f64p), 0, T, ptr(out, f64p)) == ERR_ARG
    assert lib.tehmm_batch_get_emissions(hm4._h, hb._h, 0, 0, T, ptr(out, f64p)) == ERR_ARG
    for h in (hb, hb4, hm, hm4):
        h.close()


class _Tables(object):
    def __init__(self, tables):
        self.tables = tables

    def getTrackTableList(self):
        return self.tables


@pytest.mark.parametrize("N", [7, 150])
def test_multitrack_hmm_mixed_tables(N):
    """emissionDistribution over segmented (ratios) and unsegmented tables, TrackTables and plain arrays mixed: one
    batch per ratio group, bit-equal to the per-table array-level path; emissionColumn and eval_stream(ed_mask=...)
    equal the direct call."""
    from tehmm_amd.emission import IndependentMultinomialEmissionModel
    from tehmm_amd.engine import HipBatch, eval_stream
    from tehmm_amd.hmm import MultitrackHmm
    from tehmm_amd.track import IntegerTrackTable
    K = 4
    lp, sym, obs, ratios, exp = _case(N, K)
    em = IndependentMultinomialEmissionModel(N, [s + 1 for s in sym], effectiveSegmentLength=7)
    assert em.logProbs.shape == lp.shape
    em.logProbs = lp.copy()
    h = MultitrackHmm(em)
    rs = np.random.RandomState(3)
    h.transmat_ = rs.dirichlet(np.ones(N), size=N)
    h._log_transmat = np.log(h.transmat_)
    h.startprob_ = np.full(N, 1.0 / N)
    h._log_startprob = np.log(h.startprob_)
    tables = []
    for i, (a, b) in enumerate(zip(OFFS[:-1], OFFS[1:])):
        rows = obs[a:b]
        if i % 2 == 1:                                  # segmented: ratios = segment length / 7
            seglen = rs.randint(1, 30, size=len(rows))
            so = np.concatenate([[0], np.cumsum(seglen)[:-1]])
            t = IntegerTrackTable(K, "c%d" % i, 100, 100 + int(seglen.sum())).setData(rows)
            t.setSegmentOffsets(so)
            assert em.getSegmentRatios(t) is not None
        elif i == 0:
            t = rows.copy()                             # a plain array
        else:
            t = IntegerTrackTable(K, "c%d" % i, 0, len(rows)).setData(rows)
        tables.append(t)
    want = [h._compute_log_likelihood(t) for t in tables]          # per table, array level
    got = h.emissionDistribution(_Tables(tables))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert_array_equal(g, w)
    assert np.all(want[1][:3] == 0.0) and not np.all(want[1][3] == 0.0)
    mask = _masks(N)["dead"]
    cols = h.emissionColumn(_Tables(tables), mask)
    hm = h._device_model()
    for t, c, w in zip(tables, cols, want):
        arr = t if isinstance(t, np.ndarray) else t.getNumPyArray()
        r = em.getSegmentRatios(t)
        hb = HipBatch(arr, _offsets([len(arr)]), r)
        assert_array_equal(c, hb.emission_masksum(hm, mask, use_ratios=r is not None))
        hb.close()
        _check_column(c, _column(w, mask))
    # eval_stream: the column of every group, fetched next to the other results
    obs = _possible(obs)
    res = eval_stream(hm, obs, OFFS, ratios=ratios, group_rows=300, viterbi=True, posterior=False, use_ratios=False,
                      ed_mask=mask, ed_use_ratios=True)
    assert len(res) == 5
    hb = HipBatch(obs, OFFS, ratios)
    direct = hb.emission_masksum(hm, mask, use_ratios=True)
    hb.close()
    for i, (a, b) in enumerate(zip(OFFS[:-1], OFFS[1:])):
        assert_array_equal(res[4][i], direct[a:b])
    plain = eval_stream(hm, obs, OFFS, ratios=ratios, group_rows=300, viterbi=True, posterior=False, use_ratios=False)
    assert len(plain) == 4
    for p, q in zip(plain[0], res[0]):
        assert_array_equal(p, q)
