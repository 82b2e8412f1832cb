"""CPU-only tests of the grammar model: the NumPy restatement of the CYK semantics (cfg_ref.py) against every case
of tests/golden/cfg.npz (what the reference returned), the host-side tables of MultitrackCfg and PairEmissionModel,
model files of both kinds, the option conflicts of the two commands and the alignment track's opt-in."""
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import cfg_ref
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "cfg.npz"))


def _names():
    with np.load(os.path.join(GOLDEN, "cfg.npz")) as f:
        return [str(n) for n in f["names"]]


def test_fixture_holds_the_cases_the_kernels_need(z):
    names = set(_names())
    assert {"unit_default", "unit_traceback", "unit_nest_match", "unit_nest_nomatch", "ties", "sup"} <= names
    for M in (1, 2, 3, 5, 8):
        for L in (1, 2, 3, 4, 7, 24):
            assert "r_M%d_L%d_dp" % (M, L) in z.files
    for M, L in ((33, 65), (5, 63), (5, 64), (5, 65), (5, 130), (5, 300), (5, 700)):
        assert "r_M%d_L%d" % (M, L) in names
    assert np.any(np.isneginf(z["r1_M5_L24_priors"])) and np.any(z["sup_lp1"] == -1e100)
    assert os.path.getsize(os.path.join(GOLDEN, "cfg.npz")) < 1 << 20
    # the planted repeats do make pair productions win somewhere, and the tie case is one
    assert len(np.unique(z["ties_em"])) == 1


@pytest.mark.parametrize("name", _names())
def test_restatement_equals_the_reference(z, name):
    score, top, trace, dp = cfg_ref.cyk(**cfg_ref.golden_case(z, name))
    assert score == z[name + "_score"]
    assert_array_equal(trace, z[name + "_trace"])
    if name + "_dp" in z.files:
        assert_array_equal(dp, z[name + "_dp"])


def test_unit_cases_decode_as_the_reference_tests_say(z):
    assert_array_equal(z["unit_traceback_trace"], [0, 0, 1, 0])
    assert_array_equal(z["unit_nest_match_trace"], [1, 0, 0, 1])
    assert_array_equal(z["unit_nest_nomatch_trace"], [2, 0, 0, 2])


def _flat(M=5, nest=(1, 3), prior=0.95):
    from tehmm_amd.cfg import MultitrackCfg
    from tehmm_amd.emission import IndependentMultinomialEmissionModel, PairEmissionModel
    em = IndependentMultinomialEmissionModel(M, [3], zeroAsMissingData=False)
    return MultitrackCfg(em, PairEmissionModel(em, [prior] * M), nestStates=list(nest))


def test_init_params_and_helper_tables(z):
    cfg = _flat()
    lp1, lp2 = cfg.getLogProbTables()
    assert_array_equal(lp1, z["init_M5_lp1"])
    assert_array_equal(lp2, z["init_M5_lp2"])
    assert_array_equal(cfg.startProbs, z["init_M5_start"])
    assert lp2[1, 0] == np.log(1. / 14.)                      # the 1 / (3M - 1) share of a pair state
    for key in ("helper1", "helperDim1", "helper2", "helperDim2"):
        got = getattr(cfg, key)
        assert got.dtype == np.int32
        assert_array_equal(got, z["init_M5_" + key])
    assert_allclose(cfg.getStartProbs(), np.full(5, 0.2))
    assert cfg.getTrackList() is None
    cfg.validate()
    cfg.logProbs2[1, 0] = -1e100                              # a zero from training is still a production
    cfg.createHelperTables()
    assert cfg.helperDim2[1] == 5
    with pytest.raises(AssertionError):
        cfg.validate()
    assert "NumStates = 5:\nSingle:[0, 2, 4]\nPair:[1, 3]\n" in str(_flat())


def test_tables_from_a_trained_hmm(z):
    """The /2 and /3 splits of supervisedTrain on the golden's HMM tables (the emission counts need the device: the
    whole of supervisedTrain is a GPU test)."""
    from tehmm_amd.cfg import MultitrackCfg
    from tehmm_amd.emission import IndependentMultinomialEmissionModel, PairEmissionModel
    em = IndependentMultinomialEmissionModel(4, [4, 2])
    cfg = MultitrackCfg(em, PairEmissionModel(em, [0.95] * 4), nestStates=[1])
    cfg._tablesFromHmm(z["sup_hmm_startprob"], z["sup_hmm_transmat"])
    for got, want in ((cfg.logProbs1, z["sup_lp1"]), (cfg.logProbs2, z["sup_lp2"]), (cfg.startProbs, z["sup_start"])):
        assert_array_equal(np.isneginf(got), np.isneginf(want))
        assert_array_equal(got == -1e100, want == -1e100)
        assert_allclose(got, want, rtol=1e-12)
    h1, _ = cfg_ref.helper_lists(z["sup_lp1"], z["sup_lp2"])
    assert_array_equal(cfg.helperDim1, [len(r) for r in h1])
    cfg.validate()


def test_pair_emission_model():
    from tehmm_amd.emission import IndependentMultinomialEmissionModel, PairEmissionModel
    em = IndependentMultinomialEmissionModel(4, [3])
    pm = PairEmissionModel(em, [None, 1, 1.0, 0.95])
    assert pm.logPriors.shape == (4, 2) and pm.logPriors.dtype == np.float64
    assert_array_equal(pm.logPriors[0], [0, 0])
    assert_array_equal(pm.logPriors[1], [-np.inf, 0])
    assert_array_equal(pm.logPriors[2], [-np.inf, 0])
    assert_array_equal(pm.logPriors[3], [np.log(1. - 0.95), np.log(0.95)])
    assert pm.pairLogProb(3, -1.5, -0.25, True) == -1.5 + -0.25 + np.log(0.95)
    assert pm.pairLogProb(3, -1.5, -0.25, 0) == -1.5 + -0.25 + np.log(1. - 0.95)
    with pytest.raises(AssertionError):
        PairEmissionModel(em, [0.5] * 3)


def test_model_files_of_both_kinds(tmp_path, z):
    from tehmm_amd import modelIO
    from tehmm_amd.cfg import MultitrackCfg
    from tehmm_amd.emission import IndependentMultinomialEmissionModel
    from tehmm_amd.hmm import MultitrackHmm
    from tehmm_amd.track import BinaryMap, CategoryMap, Track, TrackList
    cfg = _flat(4, (1,), 1.0)
    cfg._tablesFromHmm(z["sup_hmm_startprob"], z["sup_hmm_transmat"])
    names = CategoryMap(reserved=0)
    for n in ("out", "LTR", "in", "x"):
        names.update(n)
    cfg.stateNameMap = names
    tl = TrackList()
    tl.addTrack(Track("cat", path="cat.bed"))
    tl.addTrack(Track("bin", dist="binary", path="bin.bed"))
    al = Track("sa", dist="alignment", path="sa.bed")
    al.getValueMap().getMap("7", update=True)
    tl.addTrack(al, allowAlignment=True)
    cfg.trackList = tl
    p = str(tmp_path / "cfg.npz")
    modelIO.saveModel(p, cfg)
    got = modelIO.loadModel(p)
    assert isinstance(got, MultitrackCfg)
    assert_array_equal(got.logProbs1, cfg.logProbs1)
    assert_array_equal(got.logProbs2, cfg.logProbs2)
    assert_array_equal(got.startProbs, cfg.startProbs)
    assert_array_equal(got.nestStates, [1])
    assert_array_equal(got.hmmStates, [0, 2, 3])
    assert_array_equal(got.pairEmissionModel.logPriors, cfg.pairEmissionModel.logPriors)
    assert_array_equal(got.helper1, cfg.helper1)
    assert_array_equal(got.getEmissionModel().getLogProbs(), cfg.getEmissionModel().getLogProbs())
    assert got.getEmissionModel().zeroAsMissingData is False
    assert [t.getName() for t in got.getTrackList()] == ["cat", "bin"]
    # a binary track's map comes back as one: covered rows are symbol 2 again when the model evaluates new data
    assert isinstance(got.getTrackList()[1].getValueMap(), BinaryMap)
    assert got.getTrackList()[1].getValueMap().getMap("x") == 2 and got.getTrackList()[1].getValueMap().getMap(None) == 1
    assert got.getTrackList().getAlignmentTrack().getName() == "sa"
    assert got.getTrackList().getAlignmentTrack().getValueMap().getMap("7") == al.getValueMap().getMap("7")
    assert got.getStateNameMap().getMapBack(1) == "LTR"
    with np.load(p, allow_pickle=False) as f:
        assert str(f["kind"]) == "cfg"
    # an HMM file of today, and one as it was written before files had a kind
    hmm = MultitrackHmm(IndependentMultinomialEmissionModel(3, [2, 4]))
    q = str(tmp_path / "hmm.npz")
    modelIO.saveModel(q, hmm)
    with np.load(q, allow_pickle=False) as f:
        assert str(f["kind"]) == "hmm"
        old = {k: f[k] for k in f.files if k != "kind"}
    r = str(tmp_path / "hmm_old.npz")
    np.savez(r, **old)
    for path in (q, r):
        back = modelIO.loadModel(path)
        assert isinstance(back, MultitrackHmm)
        assert_array_equal(back._log_transmat, hmm._log_transmat)
        assert_array_equal(back.getEmissionModel().getLogProbs(), hmm.getEmissionModel().getLogProbs())


def _train_args(*options):
    from tehmm_amd import train
    return train.parseArgs(["tracks.xml", "train.bed", "out.mod"] + list(options))


def test_train_options_of_the_grammar_model():
    a = _train_args("--cfg", "--supervised", "--pairStates", "LTR,TSD", "--saPrior", "0.9")
    assert a.cfg is True and a.pairStates == "LTR,TSD" and a.saPrior == 0.9
    assert _train_args("--cfg", "--supervised").saPrior == 0.95
    for options in (("--cfg",), ("--pairStates", "LTR"), ("--pairStates", "LTR", "--supervised"),
                    ("--cfg", "--supervised", "--saPrior", "1.5"), ("--cfg", "--supervised", "--saPrior", "-0.1"),
                    ("--cfg", "--supervised", "--initTransProbs", "t.txt"),
                    ("--cfg", "--supervised", "--initStartProbs", "s.txt"),
                    ("--cfg", "--supervised", "--fixTrans"), ("--cfg", "--supervised", "--fixEm"),
                    ("--cfg", "--supervised", "--forceTransProbs", "t.txt"),
                    ("--cfg", "--supervised", "--forceEmProbs", "e.txt")):
        with pytest.raises(RuntimeError):
            _train_args(*options)


def test_eval_refuses_what_the_grammar_model_cannot_serve(tmp_path):
    from tehmm_amd import eval as te, modelIO
    p = str(tmp_path / "cfg.npz")
    modelIO.saveModel(p, _flat())
    regions = tmp_path / "none.bed"                       # (never read: the refusals come before any data)
    for options in (["--maxPost"], ["--bed", "o.bed", "--pd", "p.bed", "--pdStates", "1"],
                    ["--bed", "o.bed", "--ed", "e.bed", "--edStates", "1"], ["--segment"]):
        with pytest.raises(RuntimeError, match="CFG"):
            te.main(["tracks.xml", p, str(regions)] + options)


def test_alignment_track_needs_the_opt_in(tmp_path):
    """The parsing side of the alignment track (its rows are painted on the device: test_gpu_cfg.py loads them)."""
    from tehmm_amd.track import Track, TrackData, TrackList, readTrackList
    (tmp_path / "sa.bed").write_text("chr1\t2\t5\tr1\nchr1\t7\t9\tr2\nchr1\t12\t15\tr1\n")
    (tmp_path / "cat.bed").write_text("chr1\t0\t20\ta\n")
    xml = tmp_path / "tracks.xml"
    xml.write_text('<teModelConfig>\n<track name="cat" path="%s"/>\n<track name="sa" path="%s" '
                   'distribution="alignment"/>\n</teModelConfig>\n' % (tmp_path / "cat.bed", tmp_path / "sa.bed"))
    with pytest.raises(NotImplementedError):
        readTrackList(str(xml))
    with pytest.raises(NotImplementedError):
        TrackData().loadTrackData(str(xml), [("chr1", 0, 20)])
    tl = readTrackList(str(xml), allowAlignment=True)
    assert [t.getName() for t in tl] == ["cat"]
    al = tl.getAlignmentTrack()
    assert al.getName() == "sa" and al.getNumber() == 0 and al.getDist() == "alignment"
    assert readTrackList(str(xml), allowAlignment=True).getTrackByName("sa") is None
    with pytest.raises(RuntimeError):
        tl.addTrack(Track("sa2", dist="alignment", path="x.bed"), allowAlignment=True)
    out = tmp_path / "saved.xml"
    tl.saveXML(str(out))
    back = readTrackList(str(out), allowAlignment=True)
    assert back.getAlignmentTrack().getName() == "sa" and [t.getName() for t in back] == ["cat"]
    assert TrackList().getAlignmentTrack() is None and TrackData().getAlignmentTrackTableList() == []
