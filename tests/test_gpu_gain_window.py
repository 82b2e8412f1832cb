"""The windowed gain pass (k_emis_gain_lane<.., WIN>) and the placement that completes it with the forward pass's
log-scale records (tehmm_place.hip.h: place_item_gain): placement decides no result, so paths and scores stay bit for
bit the oracle's and the posteriors within 1e-6; what it may cost is exact blocks of the chain, and that is bounded.

The route is forced with small chunks and items (256 positions, window 64) so that three intervals of 63 756 positions
hold every kind of chunk: binade crossings from 2^15 to 2^19, a ragged tail, an interval shorter than a chunk."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

pytestmark = pytest.mark.gpu

CS = 256
LENS = [40_000, 23_456, 300]
OFFS = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
ROUTE = {"TEHMM_SPEC_CHUNK": str(CS), "TEHMM_LANE_SUB": "256", "TEHMM_DEFER": "3", "TEHMM_EMIS_SPLIT": "0",
         "TEHMM_GAIN_WINDOW": "64"}
KNOBS = tuple(ROUTE) + ("TEHMM_DEVICE_PLACE", "TEHMM_LANE_VIT", "TEHMM_LANE_P0", "TEHMM_FUSED", "TEHMM_SOFT_TIES",
                        "TEHMM_LANE_WARMUP", "TEHMM_ROWINDEX_REF")


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib, build
    build.build()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


_CASES = {}


def _case(N, stay=None):
    """Model, observations and the oracle's results of one (state count, stickiness): computed once, never modified."""
    key = (N, stay)
    if key not in _CASES:
        from oracle import oracle
        from tehmm_amd import synth
        model = synth.make_model(N, seed=N, stay=stay)
        obs = synth.sample_obs(model, int(OFFS[-1]), seed=11 + N, missing=0.02)
        ref = oracle.eval_batch(obs, OFFS, model.log_probs, model.log_startprob, model.log_transmat)
        for a in (obs,) + tuple(ref):
            a.setflags(write=False)
        _CASES[key] = (model, obs, ref)
    return _CASES[key]


def _route(monkeypatch, **over):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(ROUTE, **over).items():
        monkeypatch.setenv(k, v)


def _eval(model, obs, ratios=None, log_probs=None, viterbi=True, posterior=True):
    from tehmm_amd.engine import HipBatch, HipModel
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs if log_probs is None else log_probs,
                  symbols_per_track=model.symbols_per_track)
    hb = HipBatch(np.array(obs), OFFS, ratios)
    res = hm.eval(hb, viterbi=viterbi, posterior=posterior, use_ratios=ratios is not None)
    out = dict(paths=hb.paths().copy() if viterbi else None, vlp=res["viterbi_logprob"],
               post=hb.posteriors().copy() if posterior else None, flp=res["forward_logprob"], tm=hb.timing())
    hb.close()
    hm.close()
    return out


def _assert_oracle(got, ref):
    ref_paths, ref_vlp, ref_flp, ref_post = ref
    if got["paths"] is not None:
        assert_array_equal(got["paths"], ref_paths)
        assert_array_equal(got["vlp"], ref_vlp)
    if got["post"] is not None:
        assert_allclose(got["flp"], ref_flp, rtol=1e-6)
        assert_allclose(got["post"], ref_post, rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("N", [35, 7])
def test_windowed_gain_pass_vs_oracle(monkeypatch, N):
    """Paths and Viterbi scores bit for bit, posteriors and forward scores at 1e-6, with the window in use."""
    model, obs, ref = _case(N)
    _route(monkeypatch)
    got = _eval(model, obs)
    assert got["tm"]["count:gain_window"] == 64
    assert got["tm"]["count:viterbi_chunk_jumps"] > 0
    _assert_oracle(got, ref)


@pytest.mark.parametrize("stay", [None, 0.995])
def test_windowed_placement_costs_at_most_one_chunk_per_crossing(monkeypatch, stay):
    """Against the full gain pass on the same batch: identical results, and the chain runs at most CS / 32 exact blocks
    more per binade crossing of the batch -- a crossing placed one chunk off costs the chain that chunk, nothing else
    depends on the gains.  An interval's score crosses floor(log2 |score|) - 14 binade boundaries from 2^15 up."""
    model, obs, ref = _case(35, stay)
    got = {}
    for wn in ("64", "0"):
        _route(monkeypatch, TEHMM_GAIN_WINDOW=wn)
        got[wn] = _eval(model, obs)
        assert got[wn]["tm"]["count:gain_window"] == int(wn)
    assert_array_equal(got["64"]["paths"], got["0"]["paths"])
    assert_array_equal(got["64"]["vlp"], got["0"]["vlp"])
    assert_array_equal(got["64"]["post"], got["0"]["post"])
    assert_array_equal(got["64"]["flp"], got["0"]["flp"])
    _assert_oracle(got["64"], ref)
    crossings = sum(max(0, int(np.floor(np.log2(abs(v)))) - 14) for v in got["0"]["vlp"])
    win, full = got["64"]["tm"]["count:viterbi_exact_blocks"], got["0"]["tm"]["count:viterbi_exact_blocks"]
    print("stay=%s: exact blocks %d with the window, %d with the full pass, %d crossings, jumps %d / %d"
          % (stay, win, full, crossings, got["64"]["tm"]["count:viterbi_chunk_jumps"],
             got["0"]["tm"]["count:viterbi_chunk_jumps"]))
    assert crossings >= 9          # (22 to 24 per position: 2^19 in the first interval, 2^18 or 2^19 in the second)
    assert win <= full + (CS // 32) * crossings


@pytest.mark.parametrize("case", ["ratios", "viterbi_only", "emis_split"])
def test_full_pass_where_the_window_does_not_apply(monkeypatch, case):
    """Segment ratios, a call without the posterior (no forward records), the three-wave emission kernel: the full pass."""
    from oracle import oracle
    from tehmm_amd import synth
    model, obs, ref = _case(35)
    _route(monkeypatch, **({"TEHMM_EMIS_SPLIT": "1"} if case == "emis_split" else {}))
    if case == "ratios":
        ratios = np.ascontiguousarray(synth.random_ratios(int(OFFS[-1]), seed=6))
        ref = oracle.eval_batch(obs, OFFS, model.log_probs, model.log_startprob, model.log_transmat, 1.0, ratios)
        got = _eval(model, obs, ratios)
    else:
        got = _eval(model, obs, posterior=case != "viterbi_only")
    assert got["tm"].get("count:gain_window", 0) == 0
    assert got["tm"]["count:viterbi_chunk_jumps"] > 0          # (the chunk-parallel Viterbi itself ran)
    _assert_oracle(got, ref)


def test_impossible_row_inside_and_outside_the_window(monkeypatch):
    """A row no state can emit, inside the gain window of one item (first interval) and ahead of the window of another
    (second interval): either way the item's gain is NaN as in the full pass, and every result is the full pass's."""
    model, obs, _ = _case(35)
    lp = model.log_probs.copy()
    lp[1, :, 2] = -np.inf                                   # symbol 2 of track 1: no state can emit it
    obs = np.array(obs)
    obs[obs[:, 1] == 2, 1] = 1
    obs[20 * 256 + 220, 1] = 2                              # item 20 of the first interval, window = positions 192 .. 255
    obs[int(OFFS[1]) + 30 * 256 + 50, 1] = 2                # item 30 of the second, ahead of the window and its warm-up
    got = {}
    for wn in ("64", "0"):
        _route(monkeypatch, TEHMM_GAIN_WINDOW=wn)
        got[wn] = _eval(model, obs, log_probs=lp)
        assert got[wn]["tm"]["count:gain_window"] == int(wn)
    for k in ("paths", "vlp", "post", "flp"):
        assert_array_equal(got["64"][k], got["0"][k])
    # the third interval has no such row: the oracle's results there
    from oracle import oracle
    sl = slice(int(OFFS[2]), int(OFFS[3]))
    vlp, path = oracle.decode(obs[sl], lp, model.log_startprob, model.log_transmat)
    assert_array_equal(got["64"]["paths"][sl], path)
    assert got["64"]["vlp"][2] == vlp
