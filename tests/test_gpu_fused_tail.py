"""GPU tests of the tail form of the fused posterior passes (run with -m gpu).

At 20 and 36 padded states k_fused_fwd and k_fused_bwd compute the last four state rows of the transposed product with
row-broadcast FMAs on the vector pipe and a reduce-scatter over the wave's four rows, instead of a padded third (second)
MFMA row tile (tehmm_fused.hip.h: TEHMM_TAIL_FMA, fused_tail_scatter; knob TEHMM_FUSED_TAIL, counter count:fused_tail).
What that can get wrong is a coefficient taken from the wrong lane, a transposed one, or a tail sum landing in the wrong
row: O(1) errors in the last states of an asymmetric model.  Every case runs with the knob at 1 and at 0 against the CPU
oracle at the bar of bench.py: forward log-likelihood and every posterior value within 1e-6 relative; the E-step at the
floors and bar of bench.py's verify_estep."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-6
LENS = [1, 63, 300, 257, 1000, 4099, 2560]      # the batch of test_gpu_fused_store.py: 8 280 positions
OFFS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
KNOBS = ("TEHMM_SPEC_CHUNK", "TEHMM_LANE_SUB", "TEHMM_LANE_WARMUP", "TEHMM_LANE_VIT", "TEHMM_LANE_P0", "TEHMM_FUSED",
         "TEHMM_ROWINDEX_REF", "TEHMM_DEFER", "TEHMM_ESTEP_FUSED", "TEHMM_ESTEP_WIDE", "TEHMM_FUSED_TAIL")
ESTEP_INTERVALS = 5                             # the E-step cases: the first five intervals, 1 621 positions
REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r10_tail_vs_tile.txt")

_CASES = {
    # name: (states, sparse, normalize, model seed)
    # (the padded state count is strictly greater than N -- pad_states: the last lane of a tile is always a pad lane --, so
    #  36 padded states are N = 32 .. 35 and 20 are N = 16 .. 19; N = 36 and N = 20 run at 40 and 24 and have no tail form)
    "n32": (32, 0.0, 1.0, 132),                 # 36 padded states: 0 .. 3 live tail rows, pads among the broadcast sources
    "n33": (33, 0.0, 1.0, 133),
    "n34": (34, 0.0, 1.0, 134),
    "n35": (35, 0.0, 1.0, 135),
    "n36": (36, 0.0, 1.0, 136),                 # 40 padded states: no tail form
    "n16": (16, 0.0, 1.0, 116),                 # 20 padded states: one full tile plus the tail, no live tail row
    "n17": (17, 0.0, 1.0, 117),
    "n19": (19, 0.0, 1.0, 119),                 # ... three live tail rows
    "n20": (20, 0.0, 1.0, 120),                 # 24 padded states: no tail form
    "n21": (21, 0.0, 1.0, 121),
    "n35-sparse": (35, 0.5, 1.0, 235),          # half the transitions impossible: a swapped coefficient is an O(1) error
    "n35-emfac": (35, 0.0, 0.5, 335),           # normalize != 1: the log-domain form keeps its tile
}
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1, "no HIP device visible"
    return _lib


def _padded(N):
    return N // 4 * 4 + 4                       # (pad_states below 40: the next multiple of 4 strictly above N)


def _has_tail_form(N):
    return _padded(N) in (20, 36)


def _tail_states(N):
    """The states the tail form computes on the vector pipe (none where the state count has no such form)."""
    if not _has_tail_form(N):
        return np.zeros(N, dtype=bool)
    return np.arange(N) >= _padded(N) - 4


def _expect_tail(name, knob):
    N, _, normalize, _ = _CASES[name]
    return int(bool(knob) and normalize == 1.0 and _has_tail_form(N))


def _set_env(monkeypatch, knob):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TEHMM_SPEC_CHUNK", "256")
    monkeypatch.setenv("TEHMM_LANE_SUB", "64")
    monkeypatch.setenv("TEHMM_FUSED_TAIL", str(knob))


def _case(name):
    """Model and observations of a case: made once, shared, read-only."""
    from tehmm_amd import synth
    if name not in _cache:
        N, sparse, _, seed = _CASES[name]
        model = synth.make_model(N, synth.CONFIG2_SYMBOLS, synth.CONFIG2_GAUSSIAN, seed=seed, sparse=sparse)
        obs = synth.sample_obs(model, int(OFFS[-1]), seed=17 + N, missing=0.03)
        obs.setflags(write=False)
        _cache[name] = {"model": model, "obs": obs}
    return _cache[name]


def _eval_ref(name):
    from oracle import oracle
    ent = _case(name)
    if "eval_ref" not in ent:
        model = ent["model"]
        _, _, flp, post = oracle.eval_batch(ent["obs"], OFFS, model.log_probs, model.log_startprob, model.log_transmat,
                                            _CASES[name][2], None, want_post=True, n_threads=4)
        flp.setflags(write=False)
        post.setflags(write=False)
        ent["eval_ref"] = (flp, post)
    return ent["eval_ref"]


def _estep_ref(name):
    from oracle import oracle
    ent = _case(name)
    if "estep_ref" not in ent:
        model, obs = ent["model"], ent["obs"]
        seqs = [obs[int(OFFS[i]):int(OFFS[i + 1])] for i in range(ESTEP_INTERVALS)]
        ent["estep_ref"] = oracle.estep(seqs, model.log_probs, model.log_startprob, model.log_transmat, 1.0, None)
    return ent["estep_ref"]


def _hip_model(name):
    from tehmm_amd.engine import HipModel
    model = _case(name)["model"]
    return HipModel(model.log_transmat, model.log_startprob, model.log_probs, _CASES[name][2], model.symbols_per_track)


def _eval(monkeypatch, name, knob):
    """Posterior-only evaluation under the knob: (forward log-likelihoods, posteriors, timing); kept per (case, knob)."""
    from tehmm_amd.engine import HipBatch
    ent = _case(name)
    key = ("eval", knob)
    if key not in ent:
        _set_env(monkeypatch, knob)
        hm = _hip_model(name)
        hb = HipBatch(ent["obs"], OFFS)
        try:
            res = hm.eval(hb, viterbi=False, posterior=True)
            ent[key] = (np.array(res["forward_logprob"]), np.array(hb.posteriors()), hb.timing())
        finally:
            hb.close()
            hm.close()
    return ent[key]


def _estep(monkeypatch, name, knob):
    """E-step of the first intervals under the knob: (logprob, start, trans, obs statistics, timing)."""
    from tehmm_amd.engine import HipBatch
    ent = _case(name)
    key = ("estep", knob)
    if key not in ent:
        _set_env(monkeypatch, knob)
        model = ent["model"]
        K, N, S = model.log_probs.shape
        so = OFFS[:ESTEP_INTERVALS + 1].copy()
        hm = _hip_model(name)
        hb = HipBatch(np.ascontiguousarray(ent["obs"][:int(so[-1])]), so)
        try:
            start, trans, st = np.zeros(N), np.zeros((N, N)), np.zeros((K, N, S))
            lp = hm.estep(hb, False, start, trans, st)
            ent[key] = (lp, start, trans, st, hb.timing())
        finally:
            hb.close()
            hm.close()
    return ent[key]


def _report(tag, line):
    """Print a figure and keep it in profiles/r10_tail_vs_tile.txt (one line per tag, replaced on every run)."""
    print(line)
    try:
        lines = []
        if os.path.exists(REPORT):
            with open(REPORT) as f:
                lines = [l.rstrip("\n") for l in f if not l.startswith(tag + ":")]
        lines.append(tag + ": " + line)
        with open(REPORT, "w") as f:
            f.write("\n".join(sorted(lines)) + "\n")
    except OSError:
        pass                                    # (a read-only checkout: the figure was printed)


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("name", list(_CASES))
def test_posteriors_match_oracle(monkeypatch, name, knob):
    flp, post, tm = _eval(monkeypatch, name, knob)
    flp_o, post_o = _eval_ref(name)
    N = _CASES[name][0]
    assert {"forward_pass", "backward_posterior_pass"} <= set(tm)            # the fused passes ran
    assert tm["count:fused_tail"] == _expect_tail(name, knob)
    assert post.shape == post_o.shape
    rel_lp = float(np.max(np.abs(flp - flp_o) / np.abs(flp_o)))
    rel = np.abs(post - post_o) / post_o
    tail = _tail_states(N)
    worst_tail = float(np.max(rel[:, tail])) if tail.any() else 0.0
    worst_rest = float(np.max(rel[:, ~tail]))
    print("case %s knob %d: forward log-likelihood rel. err %.3g, posterior max rel. err: tail states %.3g (%d of "
          "them), other states %.3g" % (name, knob, rel_lp, worst_tail, int(tail.sum()), worst_rest))
    assert rel_lp <= RTOL
    assert worst_tail <= RTOL
    assert worst_rest <= RTOL


def test_posterior_tail_against_tile(monkeypatch):
    """Knob 1 against knob 0, posterior form: the summation order of the last rows differs, nothing else.  Reported, no
    threshold of its own (the oracle bar above decides)."""
    for name in ("n35", "n19"):
        a, b = _eval(monkeypatch, name, 1), _eval(monkeypatch, name, 0)
        assert a[2]["count:fused_tail"] == 1 and b[2]["count:fused_tail"] == 0
        d_lp = float(np.max(np.abs(a[0] - b[0]) / np.abs(b[0])))
        d_post = float(np.max(np.abs(a[1] - b[1]) / b[1]))
        _report("posterior %s" % name, "tail form against padded tile: forward log-likelihood max rel. difference %.3g, "
                "posterior max rel. difference %.3g" % (d_lp, d_post))
        assert np.isfinite(d_lp) and np.isfinite(d_post)


def _rel(a, b, floor):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("name", ["n35", "n20", "n19"])
def test_estep_matches_oracle(monkeypatch, name, knob):
    lp, start, trans, st, tm = _estep(monkeypatch, name, knob)
    ref = _estep_ref(name)
    assert "estep_backward_chain" in tm                                      # the fused E-step ran
    assert tm["count:fused_tail"] == _expect_tail(name, knob)
    worst = max(_rel(start, ref["start"], 1e-12), _rel(trans, ref["trans"], 1e-6), _rel(st, ref["obs"], 1e-6))
    rel_lp = abs(lp - ref["logprob"]) / abs(ref["logprob"])
    print("E-step %s knob %d: statistics max rel. err %.3g, log-likelihood rel. err %.3g" % (name, knob, worst, rel_lp))
    assert worst <= 1e-6
    assert rel_lp <= 1e-9


def test_estep_tail_against_tile(monkeypatch):
    """Knob 1 against knob 0, E-step form (reported, no threshold of its own)."""
    for name in ("n35", "n19"):
        a, b = _estep(monkeypatch, name, 1), _estep(monkeypatch, name, 0)
        assert a[4]["count:fused_tail"] == 1 and b[4]["count:fused_tail"] == 0
        d_lp = abs(a[0] - b[0]) / abs(b[0])
        d_st = max(_rel(a[1], b[1], 1e-12), _rel(a[2], b[2], 1e-6), _rel(a[3], b[3], 1e-6))
        _report("estep %s" % name, "tail form against padded tile: log-likelihood rel. difference %.3g, statistics max "
                "rel. difference %.3g" % (d_lp, d_st))
        assert np.isfinite(d_lp) and np.isfinite(d_st)
