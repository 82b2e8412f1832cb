"""GPU tests of the posterior store of the fused backward pass (run with -m gpu).

k_fused_bwd writes the posterior row of a step one step late, from inside the next step's matrix loop, and flushes the
row of step 0 behind the loop.  What that can get wrong shows at the edges: the first official step behind the warm-up,
the flush, rows of chunks the exact chain owns, tiles that straddle two intervals, a last tile with invalid items.
The batch holds all of them; results are checked against the CPU oracle at the bar of bench.py: forward
log-likelihood and every posterior value within 1e-6 relative."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-6
LENS = [1, 63, 300, 257, 1000, 4099, 2560]      # the batch of test_gpu_rowindex.py: 8 280 positions
KNOBS = ("TEHMM_SPEC_CHUNK", "TEHMM_LANE_SUB", "TEHMM_LANE_WARMUP", "TEHMM_LANE_VIT", "TEHMM_LANE_P0", "TEHMM_FUSED",
         "TEHMM_ROWINDEX_REF", "TEHMM_DEFER", "TEHMM_ESTEP_FUSED")
OFFS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)

_CASES = {
    # name: (states, synth configuration or symbols per track, item length, model seed)
    "n35": (35, "CONFIG2", 64, 38),
    "n35-other": (35, "CONFIG2", 64, 1038),        # same shapes, another seed: the model evaluated FIRST in the stale-row test
    "n35-128": (35, "CONFIG4", 128, 38),
    "n35-128-other": (35, "CONFIG4", 128, 1038),
    "n5": (5, (4,), 64, 8),
    "n20": (20, "CONFIG2", 64, 23),
    "n60": (60, "CONFIG2", 64, 63),                # one wave per SIMD
}
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1, "no HIP device visible"
    return _lib


def _set_env(monkeypatch, item_len, warmup):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TEHMM_SPEC_CHUNK", "256")
    monkeypatch.setenv("TEHMM_LANE_SUB", str(item_len))
    if warmup is not None:
        monkeypatch.setenv("TEHMM_LANE_WARMUP", str(warmup))


def _case(name, want_ref=True):
    """Model, observations and the oracle's results of a case: computed once, shared, read-only.  The observations
    depend on the shapes only (sampled from the case's base model), so a case and its '-other' twin share them."""
    from oracle import oracle
    from tehmm_amd import synth
    N, sym, item_len, seed = _CASES[name]
    if name not in _cache:
        if isinstance(sym, str):
            symbols, gauss = getattr(synth, sym + "_SYMBOLS"), getattr(synth, sym + "_GAUSSIAN")
        else:
            symbols, gauss = sym, ()
        model = synth.make_model(N, symbols, gauss, seed=seed)
        base = name[:-len("-other")] if name.endswith("-other") else name
        if base != name:
            obs = _case(base, want_ref=False)[1]
        else:
            obs = synth.sample_obs(model, int(OFFS[-1]), seed=17 + N, missing=0.03)
            obs.setflags(write=False)
        _cache[name] = [model, obs, None, item_len]
    ent = _cache[name]
    if want_ref and ent[2] is None:
        model, obs = ent[0], ent[1]
        _, _, flp, post = oracle.eval_batch(obs, OFFS, model.log_probs, model.log_startprob, model.log_transmat,
                                            1.0, None, want_post=True, n_threads=4)
        flp.setflags(write=False)
        post.setflags(write=False)
        ent[2] = (flp, post)
    return tuple(ent)


def _hip_model(model):
    from tehmm_amd.engine import HipModel
    return HipModel(model.log_transmat, model.log_startprob, model.log_probs, 1.0, model.symbols_per_track)


def _check(tag, flp, post, ref):
    flp_o, post_o = ref
    assert post.shape == post_o.shape
    rel_lp = float(np.max(np.abs(flp - flp_o) / np.abs(flp_o)))
    rel = np.abs(post - post_o) / post_o
    rel_post = float(np.max(rel))
    print("%s: forward log-likelihood rel. err %.3g, posterior max rel. err %.3g" % (tag, rel_lp, rel_post))
    assert rel_lp <= RTOL
    assert rel_post <= RTOL
    return rel


def _item_edges(item_len):
    """First and last position of every item: an interval is cut into items of item_len from its start."""
    first, last = [], []
    for o, T in zip(OFFS[:-1], LENS):
        t0 = np.arange(0, T, item_len)
        first.append(o + t0)
        last.append(o + np.minimum(t0 + item_len, T) - 1)
    return np.concatenate(first), np.concatenate(last)


@pytest.mark.parametrize("name,warmup", [("n35", 32), ("n35", 64), ("n35", 200), ("n35-128", None), ("n5", None),
                                         ("n20", None), ("n60", None)])
def test_posteriors_match_oracle(monkeypatch, name, warmup):
    from tehmm_amd.engine import HipBatch
    model, obs, ref, item_len = _case(name)
    _set_env(monkeypatch, item_len, warmup)
    hm = _hip_model(model)
    hb = HipBatch(obs, OFFS)
    try:
        res = hm.eval(hb, viterbi=False, posterior=True)
        post = np.array(hb.posteriors())
        flp = np.array(res["forward_logprob"])
    finally:
        hb.close()
        hm.close()
    rel = _check("case %s warm-up %s" % (name, warmup), flp, post, ref)
    if name.startswith("n35"):
        # the pipeline starts at an item's last position (first official step behind the warm-up) and flushes its first
        first, last = _item_edges(item_len)
        worst_first, worst_last = float(np.max(rel[first])), float(np.max(rel[last]))
        print("  item edges: %d items, worst rel. err at first positions %.3g, at last positions %.3g"
              % (first.size, worst_first, worst_last))
        assert worst_first <= RTOL
        assert worst_last <= RTOL


@pytest.mark.parametrize("name", ["n35", "n35-128"])
def test_no_stale_rows_from_an_earlier_model(monkeypatch, name):
    """Model A, then model B on the same batch: a row the pass fails to write still holds A's posterior and fails."""
    from tehmm_amd.engine import HipBatch
    model_b, obs, ref_b, item_len = _case(name)
    model_a, _, ref_a, _ = _case(name + "-other")
    # the check has teeth only if A's rows would not pass as B's: nearly all of them are far apart
    apart = np.abs(ref_a[1] - ref_b[1]).max(axis=1) / np.abs(ref_b[1]).max(axis=1) > 1e3 * RTOL
    print("rows in which A's posterior differs from B's by more than 1e-3 of the row's largest value: %d of %d"
          % (int(apart.sum()), apart.size))
    assert apart.mean() > 0.99
    _set_env(monkeypatch, item_len, None)
    hm_a, hm_b = _hip_model(model_a), _hip_model(model_b)
    hb = HipBatch(obs, OFFS)
    try:
        hm_a.eval(hb, viterbi=False, posterior=True)
        post_a = np.array(hb.posteriors())
        res = hm_b.eval(hb, viterbi=False, posterior=True)
        post_b = np.array(hb.posteriors())
        flp_b = np.array(res["forward_logprob"])
    finally:
        hb.close()
        hm_a.close()
        hm_b.close()
    assert float(np.max(np.abs(post_a - ref_a[1]) / ref_a[1])) <= RTOL      # A itself was evaluated
    _check("case %s, model B after model A" % name, flp_b, post_b, ref_b)
