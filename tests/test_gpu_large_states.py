"""GPU tests of models with 129..1024 states (tehmm_large.hip.h) against the CPU oracle: the array-level Viterbi, the
batch evaluation (decode and score_samples) on ragged intervals, ties, 16-bit back-pointers, MultitrackHmm's fused
path, the masked posterior sums.  Viterbi paths and scores are bit-identical; forward log-likelihoods and posteriors
agree to 1e-6 relative (observed error at most 3e-7)."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

pytestmark = pytest.mark.gpu

RAGGED = [1, 2, 63, 64, 65, 1000, 20000]


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib, build
    build.build()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


def _close(got, ref):
    """rtol 1e-6, and the largest relative error seen must be at most 3e-7.  (An interval whose rows were all zeroed
    by Q9 has log-likelihood 0 up to rounding: absolute 1e-12 there.)"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert_allclose(got, ref, rtol=1e-6, atol=1e-12)
    fin = np.isfinite(ref) & (np.abs(ref) > 1e-9)
    if fin.any():
        assert np.max(np.abs(got[fin] - ref[fin]) / np.abs(ref[fin])) <= 3e-7


def _close_post(got, ref):
    # posteriors carry the float32 eps (score_samples): every entry is >= ~1e-7 / N, relative error is meaningful
    assert_allclose(got, ref, rtol=1e-6, atol=1e-15)
    assert np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-12)) <= 3e-7


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("N,Ts", [(129, (1, 2, 3, 257, 20000)), (200, (1, 513, 20000)), (256, (2, 300, 20000)),
                                  (257, (1, 2, 5000)), (300, (64, 3000)), (512, (1, 700, 3000)), (1024, (2, 600))])
def test_array_level_viterbi_vs_oracle(N, Ts):
    from oracle import oracle
    from tehmm_amd import _hmm, synth
    model = synth.make_model(N, (3, 5, 4), (), seed=N)
    for T in Ts:
        obs = synth.sample_obs(model, T, seed=T)
        frame = oracle.emission(obs, model.log_probs)
        for ratios in (None, synth.random_ratios(T, seed=T + 1)):
            path, lp = _hmm._viterbi(T, N, model.log_startprob, model.log_transmat, ratios, frame)
            rpath, rlp = oracle.viterbi(model.log_startprob, model.log_transmat, frame, ratios)
            assert_array_equal(path, rpath)
            assert lp == rlp


def _tie_model(N=300, groups=10):
    from tehmm_amd import synth
    model = synth.make_model(N, (3, 5), (), seed=3)
    lp = model.log_probs.copy()
    lp[:, :, :] = lp[:, np.arange(N) % groups, :]            # states j and j + 10 k emit identically
    lt = np.full((N, N), np.log(1.0 / N))
    pi = np.full(N, np.log(1.0 / N))
    return model, np.ascontiguousarray(lp), lt, pi


@pytest.mark.timeout(300)
def test_ties_lowest_index_wins():
    from oracle import oracle
    from tehmm_amd import _hmm, synth
    from tehmm_amd.engine import HipBatch, HipModel
    N = 300
    model, lp, lt, pi = _tie_model(N)
    T = 3000
    obs = synth.random_obs(model, T, seed=5)
    frame = oracle.emission(obs, lp)
    path, v = _hmm._viterbi(T, N, pi, lt, None, frame)
    rpath, rv = oracle.viterbi(pi, lt, frame)
    assert_array_equal(path, rpath)
    assert v == rv
    assert path.max() < 10                                    # every tie went to the lowest of its group
    hm = HipModel(lt, pi, lp, symbols_per_track=model.symbols_per_track)
    offs = _offsets([T])
    hb = HipBatch(obs, offs)
    res = hm.eval(hb, viterbi=True, posterior=False)
    ref = oracle.eval_batch(obs, offs, lp, pi, lt, want_post=False)
    assert_array_equal(hb.paths(), ref[0])
    assert_array_equal(res["viterbi_logprob"], ref[1])
    hb.close()
    hm.close()


@pytest.mark.timeout(300)
def test_sixteen_bit_back_pointers():
    from oracle import oracle
    from tehmm_amd import _hmm, synth
    N, T = 300, 20000
    model = synth.make_model(N, (3, 5, 4), (), seed=11, stay=0.9)
    obs = synth.sample_obs(model, T, seed=12)
    frame = oracle.emission(obs, model.log_probs)
    path, v = _hmm._viterbi(T, N, model.log_startprob, model.log_transmat, None, frame)
    rpath, rv = oracle.viterbi(model.log_startprob, model.log_transmat, frame)
    assert_array_equal(path, rpath)
    assert v == rv
    assert path.max() >= 256


def _eval_case(model, lp, obs, lens, ratios, dtype, n_threads=16):
    from oracle import oracle
    from tehmm_amd.engine import HipBatch, HipModel
    offs = _offsets(lens)
    hm = HipModel(model.log_transmat, model.log_startprob, lp, symbols_per_track=model.symbols_per_track)
    N = lp.shape[1]
    # decode with the segment ratios (transitions only, Q11) and score_samples (no ratios, Q12) in one call
    hb = HipBatch(obs.astype(dtype), offs, ratios)
    res = hm.eval(hb, viterbi=True, posterior=True, use_ratios=True)
    names = hb.timing()
    assert {"k_vit_large", "k_fwd_large", "k_bwd_large"} <= set(names)
    paths, post, lpi = hb.paths(), hb.posteriors(N), hb.interval_logprobs()
    rp, rv, rf, rpost = oracle.eval_batch(obs, offs, lp, model.log_startprob, model.log_transmat, ratios=ratios,
                                          n_threads=n_threads)
    assert_array_equal(paths, rp)
    assert_array_equal(res["viterbi_logprob"], rv)
    _close(res["forward_logprob"], rf)
    _close(lpi, rf)
    _close_post(post, rpost)
    # decode without ratios
    res2 = hm.eval(hb, viterbi=True, posterior=False, use_ratios=False)
    rp2, rv2, _, _ = oracle.eval_batch(obs, offs, lp, model.log_startprob, model.log_transmat, want_post=False,
                                       n_threads=n_threads)
    assert_array_equal(hb.paths(), rp2)
    assert_array_equal(res2["viterbi_logprob"], rv2)
    hb.close()
    hm.close()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", ["plain200_u8", "sticky300_u16_q9", "sparse512_i32"])
def test_batch_eval_vs_oracle(case):
    from tehmm_amd import synth
    if case == "plain200_u8":
        N, lens, dtype = 200, RAGGED, np.uint8
        model = synth.make_model(N, seed=21)
    elif case == "sticky300_u16_q9":
        N, lens, dtype = 300, RAGGED, np.uint16
        model = synth.make_model(N, (3, 5, 4), (), seed=22, stay=0.999)
    else:
        N, lens, dtype = 512, [1, 2, 63, 64, 65, 1000, 2500], np.int32
        model = synth.make_model(N, (3, 5, 4), (), seed=23, sparse=0.5)
    lp = model.log_probs.copy()
    offs = _offsets(lens)
    obs = np.concatenate([synth.sample_obs(model, T, seed=100 + i, missing=0.02) for i, T in enumerate(lens)])
    if case == "sticky300_u16_q9":
        # symbol 1 of track 0 no state can emit: leading rows carrying it are zeroed (Q9), so never use it elsewhere
        lp[0, :, 1] = -np.inf
        obs[:, 0] = np.where(obs[:, 0] == 1, 2, obs[:, 0])
        for i in (1, 4, 5, 6):
            obs[offs[i]:offs[i] + min(lens[i], 3 + i), 0] = 1
    ratios = synth.random_ratios(int(offs[-1]), seed=7)
    _eval_case(model, lp, obs, lens, ratios, dtype)


class _Tables(object):
    def __init__(self, tables):
        self.tables = tables

    def getTrackTableList(self):
        return self.tables


@pytest.mark.timeout(600)
def test_multitrack_hmm_200_states_on_the_batch_path(monkeypatch):
    from oracle import oracle
    from tehmm_amd import _lib, synth
    from tehmm_amd.emission import IndependentMultinomialEmissionModel
    from tehmm_amd.engine import HipBatch
    from tehmm_amd.hmm import MultitrackHmm
    N, sym = 200, [3, 5, 4]
    model = synth.make_model(N, tuple(sym), (), seed=31)
    em = IndependentMultinomialEmissionModel(N, sym)
    em.logProbs = model.log_probs.copy()
    h = MultitrackHmm(em)
    h.transmat_ = model.transmat.copy()
    h._log_transmat = model.log_transmat.copy()
    h.startprob_ = np.exp(model.log_startprob)
    h._log_startprob = model.log_startprob.copy()
    tables = [synth.sample_obs(model, T, seed=40 + T) for T in (3000, 1, 700)]
    seen = []
    orig = HipBatch.close

    def spy(self):
        if getattr(self, "_h", None):
            seen.append(set(self.timing()))
        orig(self)
    monkeypatch.setattr(HipBatch, "close", spy)
    for t in tables:
        offs = _offsets([len(t)])
        rp, rv, rf, rpost = oracle.eval_batch(t, offs, model.log_probs, model.log_startprob, model.log_transmat)
        v, p = h.decode(t)
        assert_array_equal(p, rp)
        assert v == rv[0]
        assert "k_vit_large" in seen[-1]
        f, q = h.score_samples(t)
        _close([f], rf)
        _close_post(q, rpost)
        assert "k_fwd_large" in seen[-1]
    out = h.viterbi(_Tables(tables))
    post = h.posteriorDistribution(_Tables(tables))
    offs = _offsets([len(t) for t in tables])
    rp, rv, rf, rpost = oracle.eval_batch(np.concatenate(tables), offs, model.log_probs, model.log_startprob,
                                          model.log_transmat)
    for i, (v, p) in enumerate(out):
        assert v == rv[i]
        assert_array_equal(np.asarray(p), rp[offs[i]:offs[i + 1]])
        _close_post(post[i], rpost[offs[i]:offs[i + 1]])
    # training at 150 states stays on the array-level loop and completes
    N2 = 150
    m2 = synth.make_model(N2, tuple(sym), (), seed=32)
    em2 = IndependentMultinomialEmissionModel(N2, sym)
    h2 = MultitrackHmm(em2, n_iter=2, thresh=0.0)
    seqs = [synth.sample_obs(m2, T, seed=50 + T) for T in (2000, 1500)]
    assert not h2._can_fit_on_device(seqs)
    h2.fit(seqs)
    assert np.all(np.isfinite(h2._log_transmat[h2.transmat_ > 0]))
    assert _lib.load().tehmm_max_states_any() == 1024


@pytest.mark.timeout(300)
def test_masksum_and_interval_logprobs_300_states():
    from tehmm_amd import _lib, synth
    from tehmm_amd.engine import DeviceStats, HipBatch, HipModel
    N = 300
    model = synth.make_model(N, (3, 5, 4), (), seed=41)
    lens = [5000, 1, 64, 777]
    offs = _offsets(lens)
    obs = synth.sample_obs(model, int(offs[-1]), seed=42)
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs, symbols_per_track=model.symbols_per_track)
    hb = HipBatch(obs, offs)
    res = hm.eval(hb, viterbi=False, posterior=True)
    post = hb.posteriors(N)
    mask = (np.arange(N) % 3 == 0).astype(np.float64) * 0.5 + (np.arange(N) >= 200)
    got = hb.posterior_masksum(mask)
    assert_allclose(got, post @ mask, rtol=1e-12, atol=1e-15)
    sub = hb.posterior_masksum(mask, 4990, 5070)
    assert_allclose(sub, post[4990:5070] @ mask, rtol=1e-12, atol=1e-15)
    assert_array_equal(hb.interval_logprobs(), res["forward_logprob"])
    # the device E-step / M-step / statistics entry points refuse a large model with TEHMM_ERR_UNSUPPORTED
    K, _, S = model.log_probs.shape
    with pytest.raises(_lib.TeHmmHipError) as ei:
        hm.estep(hb, False, np.zeros(N), np.zeros((N, N)), np.zeros((K, N, S)))
    assert ei.value.code == -3
    with pytest.raises(_lib.TeHmmHipError) as ei:
        DeviceStats(hm)
    assert ei.value.code == -3 or ei.value.code == -1
    hb.close()
    hm.close()


@pytest.mark.timeout(900)
def test_256_states_64_intervals_of_50kb():
    from oracle import oracle
    from tehmm_amd import synth
    from tehmm_amd.engine import HipBatch, HipModel
    N, n, L = 256, 64, 50_000
    model = synth.make_model(N, (3, 5, 4), (), seed=51, stay=0.99)
    piece = synth.sample_obs(model, 200_000, seed=52)
    rs = np.random.RandomState(53)
    obs = np.concatenate([piece[s:s + L] for s in rs.randint(0, 200_000 - L, size=n)])
    offs = _offsets([L] * n)
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs, symbols_per_track=model.symbols_per_track)
    hb = HipBatch(obs, offs)
    res = hm.eval(hb, viterbi=True, posterior=True)
    paths = hb.paths()
    rp, rv, _, _ = oracle.eval_batch(obs, offs, model.log_probs, model.log_startprob, model.log_transmat,
                                     want_post=False, n_threads=16)
    assert_array_equal(res["viterbi_logprob"], rv)
    assert_array_equal(paths, rp)
    pick = [0, 17, 40, 63]
    sel = np.concatenate([obs[offs[i]:offs[i + 1]] for i in pick])
    so = _offsets([L] * len(pick))
    _, _, rf, rpost = oracle.eval_batch(sel, so, model.log_probs, model.log_startprob, model.log_transmat,
                                        n_threads=len(pick))
    for k, i in enumerate(pick):
        _close([res["forward_logprob"][i]], [rf[k]])
        _close_post(hb.posteriors(N, int(offs[i]), int(offs[i + 1])), rpost[so[k]:so[k + 1]])
    hb.close()
    hm.close()
