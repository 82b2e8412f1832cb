"""Semi-supervised Baum-Welch on the device (run with -m gpu): the constraints tehmm_model_set_constraints keeps on a
model handle and tehmm_model_mstep applies, against what the real reference computes with its force files
(tests/golden/user_params.npz) and against this package's host loop.

Bars as test_gpu_r2.py: parameters within 1e-6 relative, log-likelihoods within 1e-9, logProbs with atol 1e-9; forced
cells within 1e-12 (they are log(value), computed on the device)."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

from conftest import load_golden
from user_params_model import forced_cells, make_hmm, write_force_files

pytestmark = pytest.mark.gpu
RTOL = 1e-6


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1, "no HIP device visible"
    return _lib


@pytest.fixture(scope="module")
def g():
    return load_golden("user_params")


def _check_against_fixture(h, g, tag, masks=None, logprob_rtol=1e-9):
    em = h.emissionModel
    print("%s: last log-probability %.9f, reference %.9f, relative difference %.3e" % (
        tag, h.last_forward_log_prob, float(g[tag + "_last_logprob"]),
        abs(h.last_forward_log_prob / float(g[tag + "_last_logprob"]) - 1.0)))
    assert_allclose(h.transmat_, g[tag + "_transmat_after"], rtol=RTOL)
    assert_allclose(h.startprob_, g[tag + "_startprob_after"], rtol=RTOL)
    assert_allclose(em.gaussParams, g[tag + "_gauss_after"], rtol=RTOL)
    assert_allclose(em.logProbs, g[tag + "_log_probs_after"], rtol=RTOL, atol=1e-9)
    if masks is not None:
        tm, sm, emk = masks
        assert tm.sum() == 2 and sm.sum() == 1 and emk.sum() >= 2 + 9
        assert_allclose(h._log_transmat[tm], g[tag + "_log_transmat_after"][tm], rtol=1e-12)
        assert_allclose(h._log_startprob[sm], g[tag + "_log_startprob_after"][sm], rtol=1e-12)
        assert_allclose(em.logProbs[emk], g[tag + "_log_probs_after"][emk], rtol=1e-12)
    assert_allclose(h.last_forward_log_prob, g[tag + "_last_logprob"], rtol=logprob_rtol)


def _forced_hmm(g, tmp_path, **kw):
    h = make_hmm(g, thresh=0.0, fixStart=False, **dict(write_force_files(g, tmp_path), **kw))
    h.init_params = ""
    return h


def test_device_mstep_with_force_lists_matches_reference(g, tmp_path, monkeypatch):
    """One Baum-Welch iteration with all three force lists through _fit_device: exactly one
    tehmm_model_set_constraints before the loop and one (clearing) after it."""
    from tehmm_amd.engine import DeviceModel
    calls = []
    orig = DeviceModel.set_constraints

    def spy(self, *a, **kw):
        calls.append(kw)
        return orig(self, *a, **kw)
    monkeypatch.setattr(DeviceModel, "set_constraints", spy)
    monkeypatch.setenv("TEHMM_DEVICE_EM", "1")
    h = _forced_hmm(g, tmp_path, n_iter=2)
    tables = [g["obs0"], g["obs1"]]
    assert h._can_fit_on_device(tables)
    h.fit(tables)
    assert len(calls) == 2
    assert all(calls[0][k] is not None for k in ("trans", "start", "emission")) and calls[1] == {}
    _check_against_fixture(h, g, "it1", forced_cells(h, g))
    assert h.numZeroInitEdges == int(g["it1_nzero"])
    assert tuple(h.emissionModel.gaussParams[2, 4]) == (6.0, 2.5)
    # the cached handle is reused by evaluation: it must come out of the fit unconstrained and current
    lp = h.score_samples(g["obs1"])[0]
    h._dev = None
    assert_allclose(h.score_samples(g["obs1"])[0], lp, rtol=1e-12)


def test_device_mstep_with_transmat_epsilons_matches_reference(g, monkeypatch):
    """transMatEpsilons alone (the default of unsupervised training) stays on the device-resident loop."""
    from tehmm_amd.common import myLog
    from tehmm_amd.emission import IndependentMultinomialEmissionModel
    from tehmm_amd.hmm import MultitrackHmm
    monkeypatch.setenv("TEHMM_DEVICE_EM", "1")
    h = make_hmm(g, transMatEpsilons=True, n_iter=2, thresh=0.0, fixStart=False)
    h.init_params = ""
    h._log_transmat = np.asarray(myLog(g["eps_transmat"].copy()))     # the zero is still there when fit starts
    tables = [g["obs0"], g["obs1"]]
    assert h._can_fit_on_device(tables)
    fitted = []
    orig = h._fit_device
    h._fit_device = lambda *a, **kw: fitted.append(1) or orig(*a, **kw)
    h.fit(tables)
    assert fitted == [1]
    _check_against_fixture(h, g, "eps")
    assert g["eps_transmat"][1, 3] == 0.0
    assert_allclose(h._log_transmat[1, 3], g["eps_log_transmat_after"][1, 3], rtol=1e-12)   # log(eps), not -1e100
    plain = MultitrackHmm(IndependentMultinomialEmissionModel(5, [2, 4, 8]), transMatEpsilons=True)
    assert plain._can_fit_on_device(tables)


def _three_iterations(g, tmp_path_factory, knobs):
    """Three Baum-Welch iterations with the three force lists: the device-resident loop ("1") and the host loop ("0"),
    with `knobs` in the environment while they run."""
    import os
    out = {}
    names = ["TEHMM_DEVICE_EM"] + sorted(knobs)
    keep = {k: os.environ.get(k) for k in names}
    try:
        os.environ.update(knobs)
        for dev in ("1", "0"):
            os.environ["TEHMM_DEVICE_EM"] = dev
            h = _forced_hmm(g, tmp_path_factory.mktemp("force" + dev), n_iter=4)
            h.fit([g["obs0"], g["obs1"]])
            out[dev] = h
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


@pytest.fixture(scope="module")
def three_iterations(g, tmp_path_factory):
    """On the E-step that keeps fp64 rows (k_fb_coop + k_estep_accum): the fixture's 1 024 rows are exactly the size
    from which the E-step takes the chunk-parallel passes instead, whose rows are floats; TEHMM_ESTEP_FUSED=0 is the
    library's switch for the fp64 one."""
    return _three_iterations(g, tmp_path_factory, {"TEHMM_ESTEP_FUSED": "0"})


@pytest.fixture(scope="module")
def three_iterations_float_rows(g, tmp_path_factory):
    """As the library routes these tables by itself: the chunk-parallel passes."""
    return _three_iterations(g, tmp_path_factory, {})


def _loops_agree(g, a, b):
    assert_allclose(a.last_forward_log_prob, b.last_forward_log_prob, rtol=1e-9)
    assert_allclose(a.transmat_, b.transmat_, rtol=1e-6)
    assert_allclose(a.startprob_, b.startprob_, rtol=1e-6)
    assert_allclose(a.emissionModel.logProbs, b.emissionModel.logProbs, rtol=1e-6, atol=1e-9)
    assert_allclose(a.emissionModel.gaussParams, b.emissionModel.gaussParams, rtol=1e-6)
    assert a.numZeroInitEdges == b.numZeroInitEdges == int(g["it3_nzero"])


def test_three_iterations_device_and_host_loop_agree(g, three_iterations):
    _loops_agree(g, three_iterations["1"], three_iterations["0"])


def test_three_iterations_device_and_host_loop_agree_float_rows(g, three_iterations_float_rows):
    _loops_agree(g, three_iterations_float_rows["1"], three_iterations_float_rows["0"])


@pytest.mark.parametrize("dev", ["1", "0"])
def test_three_iterations_match_reference(g, three_iterations, dev):
    """Both loops against the reference's model after three iterations, at the bars of the one-iteration tests:
    parameters 1e-6, forced cells 1e-12, last log-probability 1e-9.

    The 1e-9 on a log-probability is test_gpu_r2.py's bar for training runs, and every run it is asserted on there is
    below 1 024 rows, where the E-step keeps its rows in fp64.  This fixture's 600 + 424 rows are the first size that
    takes the chunk-parallel passes, whose alpha' / gamma / wz rows are floats (6e-8 each, statistics ~1e-7:
    tehmm_estep.hip.h) -- see test_three_iterations_match_reference_float_rows for that route.  Here the same tables
    run on the fp64 rows, so that what the bar measures is the constrained M-step carried through three iterations."""
    h = three_iterations[dev]
    _check_against_fixture(h, g, "it3", forced_cells(h, g))


@pytest.mark.parametrize("dev", ["1", "0"])
def test_three_iterations_match_reference_float_rows(g, three_iterations_float_rows, dev):
    """The same on the route the library picks for 1 024 rows.  Parameters 1e-6 and forced cells 1e-12 as everywhere.
    The last log-probability is held to 1e-6, the suite's bar for a forward log-likelihood of the chunk-parallel
    passes (test_gpu_r2.py, test_gpu_r3.py) -- NOT to 1e-9.  Why: the statistics of this route carry the float rows'
    ~1e-7; a relative error d in every parameter moves each of the T positions' K + 1 factors by d, so the
    log-probability by at most T (K + 1) d = 1 024 x 4 x 1e-7 = 4e-4 of 4 072, i.e. 1e-7 per M-step and 3e-7 after three.

    MEASURED (MI355X), both loops alike: 2.450e-9 (-4072.187504984 here, -4072.187514962 in the reference; 3.5e-10
    after one iteration), with transmat at 4.4e-8, startprob 8.8e-8, gaussParams 4.4e-8 relative and the emission
    probabilities at 8.9e-9 absolute.  The two loops agree with each other to 1.1e-16 on this route too."""
    h = three_iterations_float_rows[dev]
    _check_against_fixture(h, g, "it3", forced_cells(h, g), logprob_rtol=RTOL)


# ------------------------------------------------------------------ the handle itself
def _setup(N, symbols, lens, seed, ratios=False):
    from tehmm_amd import synth
    from tehmm_amd.engine import DeviceStats, HipBatch, HipModel
    model = synth.make_model(N, symbols, (), seed=seed)
    obs = synth.sample_obs(model, int(np.sum(lens)), seed=seed + 1, missing=0.02)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    r = synth.random_ratios(len(obs), seed=seed + 2) if ratios else None
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs, symbols_per_track=model.symbols_per_track)
    hb = HipBatch(obs, offs, r)
    stats = DeviceStats(hm)
    hm.estep_device(hb, ratios, stats)
    hb.close()
    return model, obs, offs, r, hm, stats


def _constraints(model):
    """A forced transition, a forced zero transition, a forced start and two forced emissions."""
    N, (K, _, S) = model.n_states, model.log_probs.shape
    tm, tv = np.zeros((N, N), np.uint8), np.zeros((N, N))
    tm[0, 1], tv[0, 1] = 1, 0.3
    tm[2, 0], tv[2, 0] = 1, 0.0
    sm, sv = np.zeros(N, np.uint8), np.zeros(N)
    sm[0], sv[0] = 1, 0.4
    em, ev = np.zeros((K, N, S), np.uint8), np.zeros((K, N, S))
    em[0, 0, 1], ev[0, 0, 1] = 1, 0.5
    em[1, 2, 2], ev[1, 2, 2] = 1, 0.25
    return dict(trans=(tm, tv), start=(sm, sv), emission=(em, ev))


def _eval(hm, obs, offs, r):
    from tehmm_amd.engine import HipBatch
    hb = HipBatch(obs, offs, r)
    res = hm.eval(hb, viterbi=True, posterior=True, use_ratios=r is not None)
    out = hb.paths().copy(), hb.posteriors().copy(), res["viterbi_logprob"].copy(), res["forward_logprob"].copy()
    hb.close()
    return out


@pytest.mark.parametrize("N,lens,ratios", [(5, (700, 324), False), (70, (2048,), False), (5, (1024,), True)],
                         ids=["narrow", "item-parallel", "ratios"])
def test_derived_layouts_follow_a_constrained_mstep(N, lens, ratios):
    """Every copy the M-step rewrites (ptab, ltab, the k_model_layouts outputs) is rebuilt from the CONSTRAINED tables:
    the handle evaluates exactly as a fresh handle created from its parameters."""
    from tehmm_amd.engine import HipModel
    model, obs, offs, r, hm, stats = _setup(N, (3, 5, 4), lens, seed=40 + N, ratios=ratios)
    hm.set_constraints(**_constraints(model))
    hm.mstep(stats, True, True, True, 1.0, 1.0, 0.0)
    lt, pi, lp = hm.get_params(model.log_probs)
    assert_allclose(lt[0, 1], np.log(0.3), rtol=1e-12)
    assert lt[2, 0] == -1e100
    assert_allclose([lp[0, 0, 1], lp[1, 2, 2]], np.log([0.5, 0.25]), rtol=1e-12)
    assert_allclose(pi[0], np.log(0.4), rtol=1e-12)
    assert_allclose(np.exp(lt).sum(axis=1), 1.0, rtol=1e-12)
    for k, n in enumerate(model.symbols_per_track):
        assert_allclose(np.exp(lp[k, :, 1:n + 1]).sum(axis=1), 1.0, rtol=1e-12)
    assert not np.any(lp == -1e6)
    fresh = HipModel(lt, pi, lp, symbols_per_track=model.symbols_per_track)
    a, b = _eval(hm, obs, offs, r), _eval(fresh, obs, offs, r)
    assert_array_equal(a[0], b[0])
    assert_array_equal(a[1], b[1])
    assert_array_equal(a[2], b[2])
    assert_array_equal(a[3], b[3])
    stats.close()


def test_forced_cells_apply_whatever_the_update_flags_say():
    """fixTrans with a force list: the forced application still runs; lt then moves only by the exp / log round trip
    and the rescale of the rows that hold forced cells."""
    model, obs, offs, r, hm, stats = _setup(5, (3, 5, 4), (1024,), seed=7)
    before = hm.get_params(model.log_probs)
    hm.set_constraints(**_constraints(model))
    hm.mstep(stats, False, False, False, 1.0, 1.0, 0.0)
    lt, pi, lp = hm.get_params(model.log_probs)
    A0, A1 = np.exp(before[0]), np.exp(lt)
    assert_allclose(A1[[1, 3, 4]], A0[[1, 3, 4]], rtol=1e-14, atol=1e-15)   # rows without forced cells: round trip only
    assert_allclose(lt[0, 1], np.log(0.3), rtol=1e-12)
    rest = [0, 2, 3, 4]
    assert_allclose(A1[0, rest], A0[0, rest] * (0.7 / A0[0, rest].sum()), rtol=1e-12)
    assert A1[2, 0] == 0.0
    assert_allclose(A1[2, 1:], A0[2, 1:] / A0[2, 1:].sum(), rtol=1e-12)
    p0, p1 = np.exp(before[1]), np.exp(pi)
    assert_allclose(p1[0], 0.4, rtol=1e-12)
    assert_allclose(p1[1:], p0[1:] * (0.6 / p0[1:].sum()), rtol=1e-12)
    E0, E1 = np.exp(before[2]), np.exp(lp)
    assert_allclose(E1[0, 0, 1], 0.5, rtol=1e-12)
    assert_allclose(E1[0, 0, 2:4], E0[0, 0, 2:4] * (0.5 / E0[0, 0, 2:4].sum()), rtol=1e-12)
    assert_allclose(E1[2], E0[2], rtol=1e-14, atol=1e-15)              # a track without forced cells
    stats.close()


def test_cleared_constraints_leave_a_plain_mstep():
    """After clearing, an M-step equals an unconstrained M-step bit for bit."""
    from tehmm_amd.engine import HipModel
    model, obs, offs, r, hm, stats = _setup(5, (3, 5, 4), (1024,), seed=9)
    other = HipModel(model.log_transmat, model.log_startprob, model.log_probs,
                     symbols_per_track=model.symbols_per_track)
    hm.set_constraints(trans_epsilons=True, **_constraints(model))
    hm.set_constraints()
    hm.mstep(stats, True, True, True, 1.0, 1.0, 0.0)
    other.mstep(stats, True, True, True, 1.0, 1.0, 0.0)
    for x, y in zip(hm.get_params(model.log_probs), other.get_params(model.log_probs)):
        assert_array_equal(x, y)
    stats.close()


def test_set_constraints_checks_what_the_values_decide():
    from tehmm_amd._lib import TeHmmHipError
    model, obs, offs, r, hm, stats = _setup(5, (3, 5, 4), (1024,), seed=11)
    c = _constraints(model)
    c["trans"][0][0, 2], c["trans"][1][0, 2] = 1, 0.8                  # 0.3 + 0.8 from state 0
    with pytest.raises(TeHmmHipError) as e:
        hm.set_constraints(**c)
    assert e.value.code == -1
    c = _constraints(model)
    c["emission"][0][0, 0, 1:4] = 1                                    # all three symbols forced, to 0.5 in total
    with pytest.raises(TeHmmHipError) as e:
        hm.set_constraints(**c)
    assert e.value.code == -1
    stats.close()


def test_status_word_unmasked_mass_zero():
    """What only the device can see: the one symbol a track ever showed is forced to zero, so after the emission update
    nothing learned is left to scale and the forced symbols total zero -- the reference's `assert curTotal > 0.`.  The
    M-step returns TEHMM_ERR_ARG and the handle keeps the parameters from before the call."""
    from tehmm_amd import synth
    from tehmm_amd._lib import TeHmmHipError
    from tehmm_amd.engine import DeviceStats, HipBatch, HipModel
    model = synth.make_model(5, (3, 5, 4), (), seed=13)
    obs = synth.sample_obs(model, 1024, seed=14)
    obs[:, 0] = 2                                                      # track 0 only ever shows symbol 2
    offs = np.asarray([0, 1024], dtype=np.int64)
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs, symbols_per_track=model.symbols_per_track)
    stats = DeviceStats(hm)
    hb = HipBatch(obs, offs)
    hm.estep_device(hb, False, stats)
    hb.close()
    K, N, S = model.log_probs.shape
    em, ev = np.zeros((K, N, S), np.uint8), np.zeros((K, N, S))
    em[0, 1, 2] = 1                                                    # ... and state 1 is told never to emit it
    hm.set_constraints(emission=(em, ev))
    before = hm.get_params(model.log_probs)
    with pytest.raises(TeHmmHipError) as e:
        hm.mstep(stats, True, True, True, 1.0, 1.0, 0.0)
    assert e.value.code == -1 and "curTotal" in str(e.value)
    for x, y in zip(hm.get_params(model.log_probs), before):
        assert_array_equal(x, y)
    # forced mass of exactly 1 on that symbol is fine: the others are zeroed
    ev[0, 1, 2] = 1.0
    hm.set_constraints(emission=(em, ev))
    hm.mstep(stats, True, True, True, 1.0, 1.0, 0.0)
    lp = hm.get_params(model.log_probs)[2]
    assert lp[0, 1, 2] == 0.0 and np.all(lp[0, 1, [1, 3]] == -1e100)
    # and the handle still evaluates as a fresh one built from its parameters
    lt, pi, lp = hm.get_params(model.log_probs)
    fresh = HipModel(lt, pi, lp, symbols_per_track=model.symbols_per_track)
    a, b = _eval(hm, obs, offs, None), _eval(fresh, obs, offs, None)
    assert_array_equal(a[0], b[0])
    assert_array_equal(a[1], b[1])
    stats.close()


def test_additive_branch_on_the_device():
    """The additive branch of k_constrain_emis: the one symbol a track ever showed is forced below 1, nothing learned is
    left to scale, so the FORCED mass is spread over the unforced symbols (emission.py:401-420 adds
    (1 - leftover) / numUnmasked; the row then sums to 1 + the forced mass, the reference's arithmetic)."""
    from tehmm_amd import synth
    from tehmm_amd.engine import DeviceStats, HipBatch, HipModel
    model = synth.make_model(5, (3, 5, 4), (), seed=13)
    obs = synth.sample_obs(model, 1024, seed=14)
    obs[:, 0] = 2                                                      # track 0 only ever shows symbol 2
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs, symbols_per_track=model.symbols_per_track)
    stats = DeviceStats(hm)
    hb = HipBatch(obs, np.asarray([0, 1024], dtype=np.int64))
    hm.estep_device(hb, False, stats)
    hb.close()
    K, N, S = model.log_probs.shape
    em, ev = np.zeros((K, N, S), np.uint8), np.zeros((K, N, S))
    em[0, 1, 2], ev[0, 1, 2] = 1, 0.6                                  # two unforced symbols: 0.6 / 2 each
    em[0, 3, 2], ev[0, 3, 2] = 1, 0.25
    em[0, 3, 1], ev[0, 3, 1] = 1, 0.25                                 # one unforced symbol: 0.5 / 1
    hm.set_constraints(emission=(em, ev))
    hm.mstep(stats, True, True, True, 1.0, 1.0, 0.0)
    lp = hm.get_params(model.log_probs)[2]
    assert_allclose(lp[0, 1, 1:4], np.log([0.3, 0.6, 0.3]), rtol=1e-12)
    assert_allclose(lp[0, 3, 1:4], np.log([0.25, 0.25, 0.5]), rtol=1e-12)
    assert lp[0, 0, 2] == 0.0 and np.all(lp[0, 0, [1, 3]] == -1e100)   # an unforced row: what was learned, -1e6 gone
    stats.close()


# ------------------------------------------------------------------ train.main end to end
def _write_tracks(g, tmp_path, keys=("obs0", "obs1")):
    """Two of the fixture's tables as BED tracks of chrA / chrB, the XML track list and the training BED."""
    names = {2: "a", 3: "b", 4: "c"}
    beds = {"bin": [], "cat": [], "gauss": []}
    train_bed = []
    for chrom, obs in zip(("chrA", "chrB"), (g[k] for k in keys)):
        train_bed.append("%s\t0\t%d\n" % (chrom, len(obs)))
        for i, (b, c, v) in enumerate(obs):
            if b == 2:
                beds["bin"].append("%s\t%d\t%d\n" % (chrom, i, i + 1))
            if int(c) in names:
                beds["cat"].append("%s\t%d\t%d\t%s\n" % (chrom, i, i + 1, names[int(c)]))
            beds["gauss"].append("%s\t%d\t%d\t%d\n" % (chrom, i, i + 1, 2 * (int(v) - 1)))
    for name, lines in beds.items():
        (tmp_path / (name + ".bed")).write_text("".join(lines))
    xml = tmp_path / "tracks.xml"
    xml.write_text('<teModelConfig>\n<track name="bin" path="%s" distribution="binary"/>\n'
                   '<track name="cat" path="%s"/>\n'
                   '<track name="gauss" path="%s" distribution="gaussian" default="0" scale="0.5"/>\n'
                   '</teModelConfig>\n' % tuple(str(tmp_path / (n + ".bed")) for n in ("bin", "cat", "gauss")))
    bed = tmp_path / "train.bed"
    bed.write_text("".join(train_bed))
    return str(xml), str(bed)


def _tool_files(g, tmp_path):
    """The init and force files of the fixture's tool_ case, as the reference read them."""
    from user_params_model import lines_of
    out = {}
    for name in ("init_trans", "init_emis", "init_start", "force_trans", "force_emis"):
        p = tmp_path / (name + ".txt")
        p.write_text("".join(lines_of(g, "tool_" + name)))
        out[name] = str(p)
    return out


def _load_tables(xml, bed):
    from tehmm_amd import trackIO
    from tehmm_amd.track import TrackData
    td = TrackData()
    td.loadTrackData(xml, trackIO.getMergedBedIntervals(bed, ncol=3))
    return td


def _tool_args(g, tmp_path, n_iter):
    xml, bed = _write_tracks(g, tmp_path, ("tool_obs0", "tool_obs1"))
    f = _tool_files(g, tmp_path)
    return xml, bed, f, ["--flatEm", "--initTransProbs", f["init_trans"], "--initEmProbs", f["init_emis"],
                         "--initStartProbs", f["init_start"], "--forceTransProbs", f["force_trans"],
                         "--forceEmProbs", f["force_emis"], "--iter", str(n_iter), "--emThresh", "0"]


def _check_tool_model(h, g, tag, f):
    """A saved model against what the reference's trainModel statements leave (tool0_ / tool3_): the state names in
    the transition file's order, parameters at 1e-6, the last log-probability at 1e-9, the entries the closing
    re-application wrote at 1e-12 (transitions bit for bit: they are myLog(value), computed on the host)."""
    from tehmm_amd.common import myLog
    em = h.emissionModel
    assert [h.stateNameMap.getMapBack(i) for i in range(5)] == [str(x) for x in g[tag + "_state_names"]]
    assert h.transMatEpsilons is False and h.forceUserTrans == open(f["force_trans"]).readlines()
    assert h.forceUserEmissions == open(f["force_emis"]).readlines() and h.forceUserStart is None
    assert_allclose(np.exp(h._log_transmat), np.exp(g[tag + "_log_transmat"]), rtol=RTOL)
    assert_allclose(np.exp(h._log_startprob), np.exp(g[tag + "_log_startprob"]), rtol=RTOL)
    assert_allclose(em.gaussParams, g[tag + "_gauss"], rtol=RTOL)
    assert_allclose(em.logProbs, g[tag + "_log_probs"], rtol=RTOL, atol=1e-9)
    s0, s1, s3, s4 = (h.stateNameMap.getMap(s) for s in ("s0", "s1", "s3", "s4"))
    assert (s0, s1, s3, s4) == (1, 2, 3, 4)
    assert h._log_transmat[s0, s1] == myLog(0.3) == g[tag + "_log_transmat"][s0, s1]
    assert h._log_transmat[s3, s4] == -1e100 == g[tag + "_log_transmat"][s3, s4]
    assert tuple(em.gaussParams[2, s4]) == (6.0, 2.5)
    cat = h.trackList.getTrackByName("cat")
    a = cat.getValueMap().getMap("a")
    assert cat.getNumber() == 1
    assert_allclose([em.logProbs[1, s0, a], g[tag + "_log_probs"][1, s0, a]], np.log(0.5), rtol=1e-12)
    assert_allclose(em.logProbs[2, s4], g[tag + "_log_probs"][2, s4], rtol=1e-12)      # the forced gaussian row
    if np.isnan(g[tag + "_last_logprob"]):
        assert h.getLastLogProb() is None
    else:
        print("%s: last log-probability %.9f, reference %.9f" % (tag, h.getLastLogProb(), g[tag + "_last_logprob"]))
        assert_allclose(h.getLastLogProb(), g[tag + "_last_logprob"], rtol=1e-9)


def test_tool_tables_survive_the_bed_files(g, tmp_path):
    """What the train.main tests below stand on: the tracks written from the fixture's tool_ tables load as exactly
    those tables, with the symbol counts the reference's model was built with."""
    xml, bed = _write_tracks(g, tmp_path, ("tool_obs0", "tool_obs1"))
    td = _load_tables(xml, bed)
    assert list(td.getNumSymbolsPerTrack()) == g["symbols"].tolist()
    tabs = td.getTrackTableList()
    assert len(tabs) == 2
    assert_array_equal(tabs[0].getNumPyArray(), g["tool_obs0"])
    assert_array_equal(tabs[1].getNumPyArray(), g["tool_obs1"])


@pytest.mark.parametrize("dev", ["1", "0"])
def test_train_main_semi_supervised_matches_reference(g, tmp_path, monkeypatch, dev):
    """--flatEm with init and force files, --iter 3, on the device-resident loop and on the host loop: the saved model
    is the one the reference's trainModel statements give (state names by stateNamesFromUserTrans -- the file starts
    with s2's row --, init files before, force files once more after, transMatEpsilons off by default here).  The
    tables hold 1 000 rows: the E-step keeps fp64 rows, where a log-probability is held to 1e-9."""
    from tehmm_amd import modelIO, train
    from tehmm_amd.hmm import MultitrackHmm
    xml, bed, f, opts = _tool_args(g, tmp_path, 3)
    fitted = []
    orig = MultitrackHmm._fit_device
    monkeypatch.setattr(MultitrackHmm, "_fit_device", lambda self, *a, **kw: fitted.append(1) or orig(self, *a, **kw))
    monkeypatch.setenv("TEHMM_DEVICE_EM", dev)
    out = str(tmp_path / "model.npz")
    assert train.main([xml, bed, out] + opts) == 0
    assert fitted == ([1] if dev == "1" else [])
    h = modelIO.loadModel(out)
    assert h.current_iteration == 3
    _check_tool_model(h, g, "tool3", f)
    assert np.abs(np.exp(h._log_transmat) - np.exp(g["tool0_log_transmat"])).max() > 1e-3        # it did train


def test_train_main_iter_0(g, tmp_path):
    """--iter 0: the init files, no EM iteration, the force files, the model saved -- against the reference's."""
    from tehmm_amd import modelIO, train
    xml, bed, f, opts = _tool_args(g, tmp_path, 0)
    out = str(tmp_path / "model0.npz")
    assert train.main([xml, bed, out] + opts) == 0
    _check_tool_model(modelIO.loadModel(out), g, "tool0", f)


def test_train_main_supervised(g, tmp_path):
    """--supervised through the tool: the 4-column training BED is read unmerged, its names numbered in the order they
    appear (mapStateNames), the model is the one supervisedTrain gives when called directly, and -- no replicate has a
    log-probability -- the LAST replicate is saved and --saveAllReps writes every replicate (teHmmTrain.py:294-320)."""
    import os
    from tehmm_amd import modelIO, train, trackIO
    from tehmm_amd.emission import IndependentMultinomialAndGaussianEmissionModel
    from tehmm_amd.hmm import MultitrackHmm
    xml, _ = _write_tracks(g, tmp_path, ("tool_obs0", "tool_obs1"))
    bed = tmp_path / "truth.bed"
    rows = [("chrA", 0, 150, "TE"), ("chrA", 150, 400, "bg"), ("chrA", 400, 600, "TE"), ("chrB", 0, 90, "ltr"),
            ("chrB", 90, 300, "bg"), ("chrB", 300, 400, "TE")]
    bed.write_text("".join("%s\t%d\t%d\t%s\n" % r for r in rows))
    out = str(tmp_path / "sup.npz")
    assert train.main([xml, str(bed), out, "--supervised", "--reps", "2", "--seed", "3", "--saveAllReps"]) == 0
    h = modelIO.loadModel(out)
    assert [h.stateNameMap.getMapBack(i) for i in range(3)] == ["TE", "bg", "ltr"]
    assert h.getLastLogProb() is None and h.transMatEpsilons is False
    assert os.path.exists(out + ".rep0") and os.path.exists(out + ".rep1") and not os.path.exists(out + ".rep2")
    # supervisedTrain called directly on the same tracks and intervals
    td = _load_tables(xml, str(bed))
    truth = trackIO.readBedIntervals(str(bed), ncol=4)
    names = train.mapStateNames(truth)
    assert [t[3] for t in truth] == [0, 1, 0, 2, 1, 0]
    em = IndependentMultinomialAndGaussianEmissionModel(3, td.getNumSymbolsPerTrack(), td.getTrackList())
    d = MultitrackHmm(em, state_name_map=names)
    d.supervisedTrain(td, truth)
    for m in (h, modelIO.loadModel(out + ".rep0"), modelIO.loadModel(out + ".rep1")):
        assert_array_equal(m._log_transmat, d._log_transmat)
        assert_array_equal(m._log_startprob, d._log_startprob)
        assert_array_equal(m.emissionModel.logProbs, d.emissionModel.logProbs)
        assert_array_equal(m.emissionModel.gaussParams, d.emissionModel.gaussParams)
    A = np.exp(d._log_transmat)
    assert A[0, 0] > 0.9 and A[2, 1] > A[2, 0]                      # TE mostly stays; ltr is only ever left for bg


def test_train_main_replicates(g, tmp_path):
    """--reps 2 --seed 1: the saved model is the replicate with the larger last log-probability, and the same seed
    gives the same model."""
    from tehmm_amd import modelIO, train
    xml, bed = _write_tracks(g, tmp_path)
    runs = []
    for tag in ("x", "y"):
        out = str(tmp_path / ("reps_%s.npz" % tag))
        assert train.main([xml, bed, out, "--numStates", "3", "--iter", "3", "--reps", "2", "--seed", "1",
                           "--saveAllReps"]) == 0
        runs.append((modelIO.loadModel(out), modelIO.loadModel(out + ".rep0")))
    best, other = runs[0]
    assert best.transMatEpsilons is True                           # plain unsupervised training: on by default
    assert best.getLastLogProb() is not None and best.getLastLogProb() >= other.getLastLogProb()
    assert best.getLastLogProb() != other.getLastLogProb()         # two different random starts
    assert_array_equal(best._log_transmat, runs[1][0]._log_transmat)
    assert_array_equal(best.emissionModel.logProbs, runs[1][0].emissionModel.logProbs)
    assert best.getLastLogProb() == runs[1][0].getLastLogProb()
