"""User parameter files (semi-supervised training) on the host: applyUserTrans / applyUserStarts / applyUserEmissions
against what the real reference computes (tests/golden/user_params.npz), the force lists through _do_mstep and
modelIO, and the tools built on them (train, bootstrap).  No device is needed."""
import builtins
import json

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

from conftest import load_golden
from user_params_model import lines_of, make_hmm, write_force_files

# host-side parameter arithmetic against the reference: the bar of test_gpu_r2.py
RTOL = 1e-12

TRANS_CASES = ["trans_plain", "trans_fullrow", "trans_zero", "trans_zero_eps", "trans_over", "trans_unknown"]
START_CASES = ["start_plain", "start_over", "start_unknown"]
EMIS_CASES = ["emis_plain", "emis_binary_names", "emis_fullrow", "emis_additive", "emis_gauss", "emis_unknown", "emis_over",
              "emis_noleft", "emis_badstate"]


@pytest.fixture(scope="module")
def g():
    return load_golden("user_params")


def _apply(fn, exc_name):
    """Run fn; the exception type must be the one the reference ended in ("" = none)."""
    if exc_name:
        with pytest.raises(getattr(builtins, exc_name)):
            fn()
    else:
        fn()


def _tokens(lines):
    return [l.split() for l in lines if l.strip() and not l.lstrip().startswith("#")]


@pytest.mark.parametrize("case", TRANS_CASES)
def test_apply_user_trans(g, case):
    from tehmm_amd.common import myLog
    lines = lines_of(g, case + "_lines")
    eps =bool(g[case + "_eps"])
    h = make_hmm(g, transMatEpsilons=eps)
    exc = str(g[case + "_exc"])
    _apply(lambda: h.applyUserTrans(lines), exc)
    want = g[case + "_after"]
    assert_allclose(h._log_transmat, want, rtol=RTOL)
    if exc:
        assert exc == "RuntimeError"
        assert_array_equal(h._log_transmat, want)                # nothing was assigned
        return
    assert h.numZeroInitEdges == int(g[case + "_nzero"])
    names = [str(s) for s in g["state_names"]]
    for frm, to, prob in _tokens(lines):
        i, j = names.index(frm), names.index(to)
        assert h._log_transmat[i, j] == want[i, j]               # forced cells: bit for bit
        if not eps:                                              # (with epsilons a forced zero is normalised away)
            assert h._log_transmat[i, j] == myLog(float(prob))
    assert_allclose(h.transmat_.sum(axis=1), 1.0, rtol=1e-12)


def test_apply_user_trans_cases_do_what_they_are_named_for(g):
    """The fixture's cases reach the branches they are there for (a guard on the fixture itself)."""
    assert np.all(g["trans_fullrow_after"][1, [0, 2, 3, 4]] == -1e100) and g["trans_fullrow_after"][1, 1] == 0.0
    assert g["trans_zero_after"][3, 4] == -1e100
    assert g["trans_zero_eps_after"][3, 4] > -40.0               # normalize(axis=1): the zero became an epsilon
    assert int(g["trans_zero_nzero"]) == 1 and int(g["trans_plain_nzero"]) == 0
    assert str(g["emis_additive_exc"]) == "AssertionError"        # the additive branch over-fills the row; validate() says so
    assert str(g["emis_over_exc"]) == str(g["emis_noleft_exc"]) == "RuntimeError"
    assert str(g["start_zero_exc"]) == "AttributeError"           # quirk Q23


@pytest.mark.parametrize("case", START_CASES)
def test_apply_user_starts(g, case):
    from tehmm_amd.common import myLog
    lines = lines_of(g, case + "_lines")
    h = make_hmm(g)
    exc = str(g[case + "_exc"])
    _apply(lambda: h.applyUserStarts(lines), exc)
    want = g[case + "_after"]
    assert_allclose(h._log_startprob, want, rtol=RTOL)
    if not exc:
        names = [str(s) for s in g["state_names"]]
        for state, prob in _tokens(lines):
            assert h._log_startprob[names.index(state)] == myLog(float(prob))
        assert h.numZeroInitStarts == 0


def test_apply_user_starts_counts_zeros_instead_of_crashing(g):
    """Quirk Q23: the reference writes numZeroInitStart (no s) and dies with AttributeError at the first start
    probability below EPSILON; here the zero is counted."""
    from tehmm_amd.common import myLog
    assert str(g["start_zero_exc"]) == "AttributeError"
    h = make_hmm(g)
    h.applyUserStarts(lines_of(g, "start_zero_lines"))
    assert h.numZeroInitStarts == 1
    assert h._log_startprob[1] == myLog(0.0) == -1e100
    assert h._log_startprob[0] == myLog(0.4)
    sp = g["startprob"]
    rest = [2, 3, 4]
    assert_allclose(h.startprob_[rest], sp[rest] * (0.6 / sp[rest].sum()), rtol=RTOL)


@pytest.mark.parametrize("case", EMIS_CASES)
def test_apply_user_emissions(g, case, caplog):
    from tehmm_amd.common import myLog
    lines = lines_of(g, case + "_lines")
    h = make_hmm(g)
    h.emissionModel.logProbs = g["emis_before"].copy()
    exc = str(g[case + "_exc"])
    _apply(lambda: h.applyUserEmissions(lines), exc)
    want = g[case + "_after"]
    got = h.emissionModel.logProbs
    assert_allclose(got, want, rtol=RTOL)
    assert_allclose(h.emissionModel.gaussParams, g[case + "_gauss_after"], rtol=RTOL)
    if exc:
        return
    # forced cells bit for bit; the closing myLog(exp(.)) turned every -1e6 of the table into -1e100
    rec = {}
    probe = make_hmm(g)
    probe.emissionModel.logProbs = g["emis_before"].copy()
    probe.applyUserEmissions(lines, record=rec)
    forced = rec["emis_mask"] == 1
    assert forced.any()
    assert_array_equal(got[forced], want[forced])
    assert_array_equal(got[forced], myLog(rec["emis_val"][forced]))
    was_1e6 = g["emis_before"] == -1e6
    assert was_1e6.sum() == 4 and np.all(got[was_1e6 & ~forced] == -1e100)


def test_user_emission_lines_by_kind(g, caplog):
    """What each kind of line does: a symbol line sets myLog(prob) exactly, the binary map takes "0" / "None", an unknown
    symbol goes to the missing value with a warning, a gaussian line sets (mu, sigma) and masks the row."""
    import logging
    from tehmm_amd.common import myLog
    h = make_hmm(g)
    em = h.emissionModel
    mask = np.zeros(em.logProbs.shape, dtype=np.int8)
    lp = em.logProbs.copy()
    tl = h.trackList
    em.applyUserEmissionLine(tl.getTrackByName("cat"), 0, "s0 cat b 0.25".split(), lp, mask)
    assert lp[1, 0, 3] == myLog(0.25) and mask[1, 0, 3] == 1
    em.applyUserEmissionLine(tl.getTrackByName("bin"), 2, "s2 bin None 0.2".split(), lp, mask)
    em.applyUserEmissionLine(tl.getTrackByName("bin"), 3, "s3 bin 0 0.3".split(), lp, mask)
    em.applyUserEmissionLine(tl.getTrackByName("bin"), 3, "s3 bin 1 0.7".split(), lp, mask)
    assert lp[0, 2, 1] == myLog(0.2) and lp[0, 3, 1] == myLog(0.3) and lp[0, 3, 2] == myLog(0.7)
    with caplog.at_level(logging.WARNING):
        em.applyUserEmissionLine(tl.getTrackByName("cat"), 1, "s1 cat zzz 0.2".split(), lp, mask)
    assert "zzz" in caplog.text
    assert lp[1, 1, 1] == myLog(0.2) and mask[1, 1, 1] == 1      # symbol 1: the track's unknown value
    em.applyUserEmissionLine(tl.getTrackByName("gauss"), 4, "s4 gauss 6.0 2.5".split(), lp, mask)
    assert tuple(em.gaussParams[2, 4]) == (6.0, 2.5) and np.all(mask[2, 4] == 1)
    assert_allclose(np.exp(lp[2, 4, 1:]).sum(), 1.0, rtol=1e-12)
    assert np.argmax(lp[2, 4, 1:]) == 3                          # value 6 is symbol 4


def test_recording_mode_leaves_the_model_alone_and_checks_what_the_values_decide(g):
    h = make_hmm(g)
    lt, pi = h._log_transmat.copy(), h._log_startprob.copy()
    rec = {}
    h.applyUserTrans(lines_of(g, "forceUserTrans"), record=rec)
    h.applyUserStarts(lines_of(g, "forceUserStart"), record=rec)
    assert_array_equal(h._log_transmat, lt)
    assert_array_equal(h._log_startprob, pi)
    assert rec["trans_mask"].dtype == np.uint8 and rec["trans_mask"].sum() == 2 and rec["start_mask"].sum() == 1
    assert rec["trans_val"][0, 1] == 0.3 and rec["trans_val"][3, 4] == 0.0 and rec["start_val"][0] == 0.4
    for case, fn in (("trans_over", h.applyUserTrans), ("start_over", h.applyUserStarts),
                     ("emis_over", h.applyUserEmissions), ("emis_noleft", h.applyUserEmissions)):
        with pytest.raises(RuntimeError):
            fn(lines_of(g, case + "_lines"), record={})
    cons = make_hmm(g, transMatEpsilons=True)._device_constraints()
    assert cons["trans"] is None and cons["emission"] is None and cons["trans_epsilons"] is True
    assert make_hmm(g)._device_constraints() is None


def test_force_lists_are_read_at_construction_and_reapplied_by_the_mstep(g, tmp_path):
    """_do_mstep re-applies transitions, emissions, starts -- also for parameters that are not in `params`."""
    from tehmm_amd.common import myLog
    paths = write_force_files(g, tmp_path)
    h = make_hmm(g, **paths)
    assert h.forceUserTrans == lines_of(g, "forceUserTrans")
    assert h.forceUserEmissions == lines_of(g, "forceUserEmissions")
    assert h.forceUserStart == lines_of(g, "forceUserStart")
    with pytest.raises(RuntimeError):
        h.getNumFreeParameters()
    h.current_iteration = 1
    h._do_mstep({"start": np.ones(5), "trans": np.ones((5, 5)), "obs": h.emissionModel.initStats()}, "")
    assert h.current_iteration == 2
    assert h._log_transmat[0, 1] == myLog(0.3) and h._log_transmat[3, 4] == -1e100
    assert h._log_startprob[0] == myLog(0.4)
    assert_allclose(h.emissionModel.logProbs[1, 0, 2], np.log(0.5), rtol=RTOL)
    assert_allclose(h.emissionModel.logProbs[0, 1, 2], np.log(0.9), rtol=RTOL)
    assert tuple(h.emissionModel.gaussParams[2, 4]) == (6.0, 2.5)
    assert h.numZeroInitEdges == 1
    # the same three calls by hand, in the reference's order
    ref = make_hmm(g)
    ref.applyUserTrans(h.forceUserTrans)
    ref.applyUserEmissions(h.forceUserEmissions)
    ref.applyUserStarts(h.forceUserStart)
    assert_array_equal(h._log_transmat, ref._log_transmat)
    assert_array_equal(h._log_startprob, ref._log_startprob)
    assert_array_equal(h.emissionModel.logProbs, ref.emissionModel.logProbs)


def test_model_io_keeps_the_force_lists(g, tmp_path):
    from tehmm_amd import modelIO
    paths = write_force_files(g, tmp_path)
    h = make_hmm(g, **paths)
    p = str(tmp_path / "forced.npz")
    modelIO.saveModel(p, h)
    back = modelIO.loadModel(p)
    assert back.forceUserTrans == h.forceUserTrans
    assert back.forceUserEmissions == h.forceUserEmissions
    assert back.forceUserStart == h.forceUserStart
    assert_array_equal(back._log_transmat, h._log_transmat)
    with pytest.raises(RuntimeError):
        back.getNumFreeParameters()
    # one list only; and a file without the key (what every earlier version wrote) loads as before
    h2 = make_hmm(g, forceUserStart=paths["forceUserStart"])
    modelIO.saveModel(p, h2)
    back = modelIO.loadModel(p)
    assert back.forceUserTrans is None and back.forceUserStart == h2.forceUserStart
    plain = str(tmp_path / "plain.npz")
    modelIO.saveModel(plain, make_hmm(g))
    with np.load(plain) as z:
        assert "forceUser" not in json.loads(str(z["meta"]))
    back = modelIO.loadModel(plain)
    assert back.forceUserTrans is None and back.forceUserEmissions is None and back.forceUserStart is None
    assert back.getNumFreeParameters() > 0


# ------------------------------------------------------------------ the tools
def _bootstrap(g, tmp_path, *options):
    from tehmm_amd import bootstrap, modelIO
    model = str(tmp_path / "model.npz")
    modelIO.saveModel(model, make_hmm(g))
    tpath, epath = str(tmp_path / "trans.txt"), str(tmp_path / "emis.txt")
    assert bootstrap.main([model, tpath, epath] + list(options)) == 0
    return open(tpath).readlines(), open(epath).readlines()


def _flat_hmm(g):
    from tehmm_amd.emission import IndependentMultinomialAndGaussianEmissionModel
    from tehmm_amd.hmm import MultitrackHmm
    h = make_hmm(g)
    em = IndependentMultinomialAndGaussianEmissionModel(5, g["symbols"].tolist(), h.trackList)
    flat = MultitrackHmm(em, state_name_map=h.stateNameMap)
    flat.trackList = h.trackList
    return flat


def test_bootstrap_files(g, tmp_path):
    """What is written: self transitions by default, --ignore, --numTotal / --numAdd / --stp, the reference's formats,
    and rows that never sum above 1 (the round-down helper)."""
    from tehmm_amd import bootstrap
    tlines, elines = _bootstrap(g, tmp_path, "--ignore", "s3", "--numTotal", "6", "--stp", "0.8")
    assert [l.split()[:2] for l in tlines] == [[s, s] for s in ("s0", "s1", "s2", "s4", "Unlabeled0", "Unlabeled1")]
    assert tlines[0] == "s0\ts0\t%.12e\n" % bootstrap.roundDown(g["transmat"][0, 0])          # (quirk Q25)
    assert tlines[-1] == "Unlabeled1\tUnlabeled1\t%e\n" % 0.8
    assert not any(l.startswith("s3") for l in elines)
    assert len(elines) == 4 * (1 + 3 + 1)                         # per state: bin "1", cat a b c, gauss mean stdev
    assert elines[0].split()[:3] == ["s0", "bin", "1"] and elines[4].split()[:2] == ["s0", "gauss"]
    assert elines[4] == "s0\tgauss\t%.12e\t%.12e\n" % tuple(g["gauss_params"][2, 0])
    p = np.exp(g["log_probs"])
    assert float(elines[1].split()[3]) <= p[1, 0, 2] and p[1, 0, 2] - float(elines[1].split()[3]) < 2e-12
    assert bootstrap.roundDown(0.5) == 0.5 and 0.1 - 2e-12 < bootstrap.roundDown(0.1) < 0.1
    with pytest.raises(RuntimeError):
        _bootstrap(g, tmp_path, "--numAdd", "1", "--numTotal", "7")
    tlines, _ = _bootstrap(g, tmp_path, "--allTrans", "--numAdd", "1")
    assert len(tlines) == 25 + 1


def test_bootstrap_round_trip_emissions(g, tmp_path):
    """bootstrap --allTrans, then applyUserEmissions of the written file on a flat model: the model is back.  The
    written probabilities are rounded down at steps of 12^-11 = 1.3e-12 and printed with 13 digits, the symbol that is
    not written takes what is left, so a probability above 0.0135 comes back within 1e-10 relative (all of this
    model's written ones are; the bar is asserted on every probability above 1e-6)."""
    _, elines = _bootstrap(g, tmp_path, "--allTrans")
    flat = _flat_hmm(g)
    flat.applyUserEmissions(elines)
    want, got = np.exp(g["log_probs"]), np.exp(flat.emissionModel.logProbs)
    assert (want > 1e-6).sum() > 5 * (2 + 4 + 8)
    assert_allclose(got[want > 1e-6], want[want > 1e-6], rtol=1e-10)
    assert_allclose(flat.emissionModel.gaussParams, g["gauss_params"], rtol=1e-12)


def test_bootstrap_round_trip_transitions(g, tmp_path):
    """bootstrap --allTrans, then applyUserTrans of the written file on a flat model: the matrix is back, at rtol=1e-10
    on probabilities above 1e-6.  Written as the reference writes them ("%e", seven digits) the rows of this very
    matrix sum above 1 and applyUserTrans refuses the file; they go through the round-down helper like the emissions
    (quirk Q25), which truncates at 12^-11 = 1.3e-12: within 1e-10 relative for a transition above 0.0135, as all of
    this matrix are."""
    tlines, _ = _bootstrap(g, tmp_path, "--allTrans")
    flat = _flat_hmm(g)
    flat.applyUserTrans(tlines)
    want, got = g["transmat"], flat.transmat_
    assert want.min() > 0.0135
    assert_allclose(got[want > 1e-6], want[want > 1e-6], rtol=1e-10)
    assert np.all(got <= want) and np.all(got.sum(axis=1) <= 1.0)
    # the reference's own format on the same matrix: a row above 1, refused
    ref_lines = ["s%d\ts%d\t%e\n" % (i, j, want[i, j]) for i in range(5) for j in range(5)]
    with pytest.raises(RuntimeError):
        _flat_hmm(g).applyUserTrans(ref_lines)


def _train_args(*options):
    from tehmm_amd import train
    return train.parseArgs(["tracks.xml", "train.bed", "out.mod"] + list(options))


def test_train_option_conflicts_and_defaults(tmp_path):
    """The checks of teHmmTrain.py:188-225, which run before anything is loaded."""
    for options in (("--fixTrans", "--supervised"), ("--fixEm", "--supervised"), ("--flatEm",),
                    ("--initEmProbs", "e.txt"), ("--emRandRange", "0.2"), ("--emRandRange", "a,b"), ("--cfg",),
                    ("--segLen", "1")):
        with pytest.raises(RuntimeError):
            _train_args(*options)
    # transMatEpsilons: on for plain unsupervised training only, unless asked for
    assert _train_args().transMatEpsilons is True
    assert _train_args("--supervised").transMatEpsilons is False
    assert _train_args("--initTransProbs", "t.txt").transMatEpsilons is False
    assert _train_args("--forceTransProbs", "t.txt").transMatEpsilons is False
    assert _train_args("--forceTransProbs", "t.txt", "--transMatEpsilons").transMatEpsilons is True
    a = _train_args("--flatEm", "--initTransProbs", "t.txt", "--initEmProbs", "e.txt", "--forceTransProbs", "t.txt",
                    "--iter", "0")
    assert a.iter == 0 and a.emRandRange == (0.2, 0.8) and a.segLen is None and a.numStates == 2 and a.reps == 1
    from tehmm_amd import train
    with pytest.raises(RuntimeError):                             # a training BED that does not exist
        train.main(["tracks.xml", str(tmp_path / "none.bed"), "out.mod", "--supervised"])


def test_train_state_names_and_best_replicate(g, tmp_path):
    from tehmm_amd import train
    p = tmp_path / "trans.txt"
    p.write_text("# comment\n\nTE TE 0.9\nTE other 0.1\nother LTR 1e-3\n")
    names = train.stateNamesFromUserTrans(str(p))
    assert [names.getMapBack(i) for i in range(len(names))] == ["TE", "other", "LTR"]
    p.write_text("TE other x\n")
    with pytest.raises(ValueError):
        train.stateNamesFromUserTrans(str(p))
    ivs = [("chr1", 0, 10, "b"), ("chr1", 10, 20, "a"), ("chr1", 20, 30, "b")]
    names = train.mapStateNames(ivs)
    assert ivs == [("chr1", 0, 10, 0), ("chr1", 10, 20, 1), ("chr1", 20, 30, 0)] and len(names) == 2
    with pytest.raises(RuntimeError):
        train.mapStateNames([("chr1", 0, 10)])

    class Rep(object):
        def __init__(self, lp):
            self.lp = lp

        def getLastLogProb(self):
            return self.lp
    assert train.bestReplicate([Rep(-30.0), Rep(-10.0), Rep(-20.0)]) == 1
    assert train.bestReplicate([Rep(None), Rep(None)]) == -1      # supervised models have no log-probability
    assert make_hmm(g).getLastLogProb() is None
