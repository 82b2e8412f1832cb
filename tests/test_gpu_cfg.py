"""CYK decode of the grammar model on the device against tests/golden/cfg.npz -- what the
reference's MultitrackCfg.decode returned -- and against the NumPy restatement in cfg_ref.py: scores and every stored
dp cell bit-equal, top and trace equal."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import cfg_ref
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib, build
    build.build()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


@pytest.fixture(scope="module")
def z():
    with np.load(os.path.join(GOLDEN, "cfg.npz")) as f:
        return {k: f[k] for k in f.files}


class _Z(dict):
    @property
    def files(self):
        return list(self.keys())


def _case(z, name):
    return cfg_ref.golden_case(_Z(z), name)


def _model_args(c):
    from tehmm_amd._lib import as_f64, f64p, ptr, u8p
    M = c["em"].shape[1]
    keep = [np.ascontiguousarray(c["is_nest"], dtype=np.uint8), as_f64(c["lp1"]), as_f64(c["lp2"]), as_f64(c["priors"]),
            as_f64(c["log_start"])]
    return M, keep, [ptr(keep[0], u8p)] + [ptr(a, f64p) for a in keep[1:]]


def decode_batch(cases):
    """One tehmm_cyk_decode call over cases that share a model: [(score, top, trace)]."""
    from tehmm_amd import _lib
    from tehmm_amd._lib import f64p, i64p, ptr, u16p
    M, keep, margs = _model_args(cases[0])
    lens = [len(c["em"]) for c in cases]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    em = np.ascontiguousarray(np.concatenate([c["em"] for c in cases]), dtype=np.float64)
    al = None
    if cases[0]["al"] is not None:
        al = np.ascontiguousarray(np.concatenate([c["al"] for c in cases]), dtype=np.uint16)
    n = len(cases)
    scores, top, trace = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(int(offsets[-1]))
    _lib.check(_lib.load().tehmm_cyk_decode(n, ptr(offsets, i64p), M, ptr(em, f64p), ptr(al, u16p), cases[0]["def_sym"],
                                            *margs, ptr(scores, f64p), ptr(top, i64p), ptr(trace, f64p)),
               "tehmm_cyk_decode")
    return [(scores[t], int(top[t]), trace[offsets[t]:offsets[t + 1]]) for t in range(n)]


def get_dp(c):
    from tehmm_amd import _lib
    from tehmm_amd._lib import f64p, ptr, u16p
    M, keep, margs = _model_args(c)
    L = len(c["em"])
    em = np.ascontiguousarray(c["em"], dtype=np.float64)
    al = None if c["al"] is None else np.ascontiguousarray(c["al"], dtype=np.uint16)
    dp = np.zeros((L, L, M))
    _lib.check(_lib.load().tehmm_cyk_get_dp(L, M, ptr(em, f64p), ptr(al, u16p), c["def_sym"], *margs, ptr(dp, f64p)),
               "tehmm_cyk_get_dp")
    return dp


def _golden_names():
    with np.load(os.path.join(GOLDEN, "cfg.npz")) as f:
        return [str(n) for n in f["names"]]


@pytest.mark.parametrize("name", _golden_names())
def test_decode_equals_the_reference(z, name):
    """Every golden case; r_M5_L130 and below stay on the wave form, r_M5_L300 and r_M5_L700 reach the workgroup form
    (sizes above 256 of a single interval)."""
    c = _case(z, name)
    (score, top, trace), = decode_batch([c])
    assert score == z[name + "_score"]
    assert_array_equal(trace, z[name + "_trace"])
    if name + "_dp" in z:
        assert top == int(np.argmax(c["log_start"] + z[name + "_dp"][0, -1]))
        assert_array_equal(get_dp(c), z[name + "_dp"])


@pytest.fixture(scope="module")
def mixed(z):
    """One model (that of r_M5_L130), intervals of lengths 1, 2, 3, 5, 64, 65 and 130 cut from its rows, and what the
    restatement returns for each (the whole of the longest one is the golden's own case)."""
    c = _case(z, "r_M5_L130")
    cases, want = [], []
    at = 0
    for L in (1, 2, 3, 5, 64, 65):
        lo = at % (130 - L)
        at += 37
        cases.append(dict(c, em=c["em"][lo:lo + L], al=c["al"][lo:lo + L]))
    cases.append(c)
    for d in cases[:-1]:
        want.append(cfg_ref.cyk(**d))
    want.append((z["r_M5_L130_score"], None, z["r_M5_L130_trace"], None))
    return cases, want


def _check_batch(got, want):
    for (score, top, trace), (wscore, wtop, wtrace, _) in zip(got, want):
        assert score == wscore
        assert_array_equal(trace, wtrace)
        if wtop is not None:
            assert top == wtop


def test_mixed_batch_in_one_call(mixed):
    cases, want = mixed
    _check_batch(decode_batch(cases), want)


def test_mixed_batch_reversed(mixed):
    cases, want = mixed
    _check_batch(decode_batch(cases[::-1]), want[::-1])


def test_dp_of_the_restatement_at_a_size_without_golden(z):
    """dp cell by cell on a length that is no golden: 65 rows of the M = 5 model with its own alignment row, the -inf
    prior model (r1_M5_L24) stretched over them."""
    c = _case(z, "r1_M5_L24")
    big = _case(z, "r_M5_L65")
    d = dict(c, em=big["em"], al=big["al"])
    score, top, trace, dp = cfg_ref.cyk(**d)
    (gscore, gtop, gtrace), = decode_batch([d])
    assert gscore == score and gtop == top
    assert_array_equal(gtrace, trace)
    assert_array_equal(get_dp(d), dp)


def test_no_derivation_is_an_error(z):
    """Three rows and one state that emits pairs only, under a prior of -inf without a match: nothing derives the
    rows, the top cell is -inf and the call fails where the reference's traceback asserts."""
    from tehmm_amd._lib import TeHmmHipError
    c = dict(em=np.log(np.full((3, 1), 0.5)), al=np.asarray([1, 2, 3], dtype=np.uint16), def_sym=0,
             is_nest=np.ones(1, dtype=np.uint8), lp1=np.zeros((1, 1, 1)), lp2=np.full((1, 1), -np.inf),
             priors=np.asarray([[-np.inf, 0.0]]), log_start=np.zeros(1))
    with pytest.raises(TeHmmHipError, match="no derivation"):
        decode_batch([c])
    with pytest.raises(ValueError):
        cfg_ref.cyk(**c)


def test_limits_are_refused_before_any_allocation(z, monkeypatch):
    from tehmm_amd import _lib
    c = _case(z, "r_M5_L300")
    monkeypatch.setenv("TEHMM_CYK_MAX_BYTES", str(1 << 20))
    with pytest.raises(_lib.TeHmmHipError, match=r"largest single interval that fits at M = 5 is L = 1\d\d ") as e:
        decode_batch([c])
    assert e.value.code == -3
    monkeypatch.delenv("TEHMM_CYK_MAX_BYTES")
    M = 65
    big = dict(em=np.zeros((2, M)), al=None, def_sym=0, is_nest=np.zeros(M, dtype=np.uint8), lp1=np.zeros((M, M, M)),
               lp2=np.zeros((M, M)), priors=np.zeros((M, 2)), log_start=np.zeros(M))
    with pytest.raises(_lib.TeHmmHipError) as e:
        decode_batch([big])
    assert e.value.code == -3


def test_last_timing_names_the_passes(z):
    from tehmm_amd import _lib
    decode_batch([_case(z, "r_M5_L65")])
    names = (ctypes.c_char_p * 16)()
    ms = np.zeros(16)
    n = _lib.load().tehmm_cyk_last_timing(16, names, _lib.ptr(ms, _lib.f64p))
    got = [names[i].decode() for i in range(n)]
    assert got == ["upload", "init", "fill", "traceback", "copy_back", "wall"]
    assert np.all(ms[:n] >= 0.0) and ms[n - 1] > 0.0


# ---- the model class ---------------------------------------------------------------------------------------------------
def _sup_model(z):
    """The trained model of the golden's supervisedTrain case, trained here from the same data."""
    from tehmm_amd.cfg import MultitrackCfg
    from tehmm_amd.emission import IndependentMultinomialEmissionModel, PairEmissionModel
    from tehmm_amd.track import IntegerTrackTable, TrackData
    obs = z["sup_obs"]
    start = int(z["sup_table_start"])
    tab = IntegerTrackTable(2, "chrC", start, start + len(obs)).setData(obs)
    beds = [("chrC", int(a), int(b), int(s)) for a, b, s in z["sup_bed"]]
    em = IndependentMultinomialEmissionModel(4, [4, 2])
    cfg = MultitrackCfg(em, PairEmissionModel(em, [0.95] * 4), nestStates=[1])
    cfg.supervisedTrain(TrackData([tab]), beds)
    return cfg, tab


def test_supervised_train_and_decode_end_to_end(z):
    from numpy.testing import assert_allclose
    from tehmm_amd.track import IntegerTrackTable, TrackData
    cfg, tab = _sup_model(z)
    assert_allclose(cfg.emissionModel.getLogProbs(), z["sup_log_probs"], rtol=1e-12)
    for got, want in zip(cfg.getLogProbTables() + (cfg.startProbs,), (z["sup_lp1"], z["sup_lp2"], z["sup_start"])):
        assert_array_equal(np.isneginf(got), np.isneginf(want))
        assert_array_equal(got == -1e100, want == -1e100)
        assert_allclose(got, want, rtol=1e-12)
    assert np.any(z["sup_lp1"] == -1e100)
    al = z["sup_al"].reshape(-1, 1)
    score, trace = cfg.decode(tab, alignmentTrack=al, defAlignmentSymbol=0)
    assert_allclose(score, z["sup_score"], rtol=1e-12)
    assert_array_equal(trace, z["sup_trace"])
    assert trace.dtype == np.float64
    # viterbi: the same table twice and its alignment tables, one device call
    td = TrackData([tab, tab])
    alt = IntegerTrackTable(1, "chrC", tab.getStart(), tab.getEnd(), dtype=np.uint16).setData(al)
    td.alignmentTrackTableList = [alt, alt]
    out = cfg.viterbi(td)
    assert len(out) == 2
    for p, states in out:
        assert p == score
        assert_array_equal(states, trace)


def test_decode_with_the_golden_tables(z):
    """MultitrackCfg.decode with the reference's own tables put into the model: bit-equal score."""
    cfg, tab = _sup_model(z)
    cfg.logProbs1, cfg.logProbs2, cfg.startProbs = z["sup_lp1"].copy(), z["sup_lp2"].copy(), z["sup_start"].copy()
    cfg.emissionModel.logProbs = z["sup_log_probs"].copy()
    cfg.createHelperTables()
    score, trace = cfg.decode(tab, alignmentTrack=z["sup_al"].reshape(-1, 1))
    assert score == z["sup_score"]
    assert_array_equal(trace, z["sup_trace"])
    assert_array_equal(cfg.emissionModel.allLogProbs(tab), z["sup_em"])


# ---- the two commands --------------------------------------------------------------------------------------------------
def _runs(col):
    """[(start, end, value)] of the runs of equal values of a column"""
    cuts = np.flatnonzero(np.diff(col)) + 1
    return [(int(a), int(b), int(col[a])) for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(col)]]))]


@pytest.fixture(scope="module")
def files(z, tmp_path_factory):
    """The golden's supervisedTrain case as files: a multinomial and a binary track whose tables are its observations
    (symbols are handed out in order of first appearance: 2, 3, 4 as in the data), the alignment row as a third BED,
    the labelled intervals as the training BED."""
    root = tmp_path_factory.mktemp("cfgcli")
    start = int(z["sup_table_start"])
    obs, al = z["sup_obs"], z["sup_al"]
    (root / "cat.bed").write_text("".join("chrC\t%d\t%d\tv%d\n" % (start + a, start + b, v)
                                          for a, b, v in _runs(obs[:, 0]) if v >= 2))
    (root / "bin.bed").write_text("".join("chrC\t%d\t%d\n" % (start + a, start + b)
                                          for a, b, v in _runs(obs[:, 1]) if v == 2))
    (root / "sa.bed").write_text("".join("chrC\t%d\t%d\tr%d\n" % (start + a, start + b, v)
                                         for a, b, v in _runs(al) if v != 0))
    (root / "truth.bed").write_text("".join("chrC\t%d\t%d\ts%d\n" % (a, b, s) for a, b, s in z["sup_bed"]))
    (root / "regions.bed").write_text("chrC\t%d\t%d\n" % (start, start + len(obs)))
    (root / "tracks.xml").write_text(
        '<teModelConfig>\n<track name="cat" path="%s"/>\n<track name="bin" path="%s" distribution="binary"/>\n'
        '<track name="sa" path="%s" distribution="alignment"/>\n</teModelConfig>\n'
        % tuple(str(root / n) for n in ("cat.bed", "bin.bed", "sa.bed")))
    return root


def test_alignment_track_loads_through_the_opt_in(z, files):
    from tehmm_amd.track import TrackData
    start = int(z["sup_table_start"])
    td = TrackData()
    td.loadTrackData(str(files / "tracks.xml"), [("chrC", start, start + len(z["sup_obs"]))], allowAlignment=True)
    assert_array_equal(td.getTrackTableList()[0].getNumPyArray(), z["sup_obs"])
    tabs = td.getAlignmentTrackTableList()
    assert len(tabs) == 1 and tabs[0].getNumTracks() == 1
    assert tabs[0].getNumPyArray().dtype == np.uint16
    assert_array_equal(tabs[0].getNumPyArray()[:, 0], z["sup_al"])
    assert td.getNumSymbolsPerTrack() == [4, 2]
    with pytest.raises(NotImplementedError):
        TrackData().loadTrackData(str(files / "tracks.xml"), [("chrC", start, start + 10)])


def test_train_and_eval_commands(z, files):
    """python -m tehmm_amd.train --cfg --supervised, then python -m tehmm_amd.eval --bed: the rows of the BED file are
    those of the reference's trace."""
    from tehmm_amd import modelIO, output
    from tehmm_amd.cfg import MultitrackCfg
    from tehmm_amd.track import IntegerTrackTable
    model, bed, bic = str(files / "model.npz"), str(files / "out.bed"), str(files / "out.bic")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-m", "tehmm_amd.train", str(files / "tracks.xml"), str(files / "truth.bed"), model,
                    "--cfg", "--supervised", "--pairStates", "s1", "--saPrior", "0.95"], check=True, env=env, cwd=ROOT,
                   timeout=120)
    m = modelIO.loadModel(model)
    assert isinstance(m, MultitrackCfg)
    assert_array_equal(m.nestStates, [1])
    assert m.getTrackList().getAlignmentTrack().getName() == "sa"
    np.testing.assert_allclose(m.logProbs1, z["sup_lp1"], rtol=1e-12)
    np.testing.assert_allclose(m.getEmissionModel().getLogProbs(), z["sup_log_probs"], rtol=1e-12)
    run = subprocess.run([sys.executable, "-m", "tehmm_amd.eval", str(files / "tracks.xml"), model,
                          str(files / "regions.bed"), "--bed", bed, "--bic", bic], check=True, env=env, cwd=ROOT,
                         timeout=120, capture_output=True, text=True)
    assert run.stdout == "Viterbi (log) score: %f\n" % float(z["sup_score"])
    start = int(z["sup_table_start"])
    want = str(files / "want.bed")
    with open(want, "w") as f:
        f.write("#Viterbi Score: %f\n" % float(z["sup_score"]))
    table = IntegerTrackTable(2, "chrC", start, start + len(z["sup_obs"]))
    output.statesToBed(table, [int(s) for s in z["sup_trace"]], want, stateNames=["s0", "s1", "s2", "s3"])
    assert open(bed).read() == open(want).read()
    assert "s1" in open(bed).read()
    assert os.path.getsize(bic) > 0
