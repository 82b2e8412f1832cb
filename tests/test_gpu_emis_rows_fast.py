"""The fast form of the row part of the one-wave emission + gain kernel (tehmm_emis_fast.hip.h) against the form that
calls emis_rows (TEHMM_EMIS_FAST=0) and against the oracle.

A wrong emission row changes no result: the exact chain recomputes its own rows and adopts only what it verifies, so
wrong rows show up as more exact blocks.  Every case therefore holds paths and Viterbi scores bit for bit against the
oracle AND the chain's two counters equal to the old form's on the same input (they are deterministic), and checks that
`count:emis_fast` names the form that was expected to run.

The route is forced with chunks and items of 128 positions (window 32) so that the one-wave kernel and the window run
on batches of about 40 000 positions: five item groups, two workgroups."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

pytestmark = pytest.mark.gpu

CS = 128
ROUTE = {"TEHMM_SPEC_CHUNK": str(CS), "TEHMM_LANE_SUB": "128", "TEHMM_DEFER": "3", "TEHMM_EMIS_SPLIT": "0",
         "TEHMM_GAIN_WINDOW": "32"}
KNOBS = tuple(ROUTE) + ("TEHMM_EMIS_FAST", "TEHMM_DEVICE_PLACE", "TEHMM_LANE_VIT", "TEHMM_LANE_P0", "TEHMM_FUSED",
                        "TEHMM_SOFT_TIES", "TEHMM_LANE_WARMUP", "TEHMM_ROWINDEX_REF")
# two intervals that are no multiple of the item length (last items of 105 and of 3 positions), one shorter than a chunk
LENS = (33_001, 6_915, 300)
BENCH_SYMBOLS = (2, 2, 3, 4, 5, 8, 12, 30, 250, 250)


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib, build
    build.build()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


def _offs(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


_CASES = {}


def _case(N, symbols=BENCH_SYMBOLS, gaussian=(8, 9), lens=LENS, normalize=1.0):
    """Model, observations and the oracle's paths and scores of one configuration: computed once, never modified."""
    key = (N, symbols, gaussian, lens, normalize)
    if key not in _CASES:
        from oracle import oracle
        from tehmm_amd import synth
        offs = _offs(lens)
        model = synth.make_model(N, symbols_per_track=symbols, gaussian_tracks=gaussian, seed=N + len(symbols))
        obs = synth.sample_obs(model, int(offs[-1]), seed=3 + N, missing=0.02)
        ref = oracle.eval_batch(obs, offs, model.log_probs, model.log_startprob, model.log_transmat, normalize,
                                want_post=False)[:2]
        for a in (obs, offs) + tuple(ref):
            a.setflags(write=False)
        _CASES[key] = (model, obs, offs, ref)
    return _CASES[key]


def _route(monkeypatch, **over):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(ROUTE, **over).items():
        monkeypatch.setenv(k, v)


def _eval(model, obs, offs, ratios=None, log_probs=None, normalize=1.0):
    from tehmm_amd.engine import HipBatch, HipModel
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs if log_probs is None else log_probs,
                  normalize=normalize, symbols_per_track=model.symbols_per_track)
    hb = HipBatch(np.array(obs), offs, ratios)
    res = hm.eval(hb, viterbi=True, posterior=True, use_ratios=ratios is not None)
    out = dict(paths=hb.paths().copy(), vlp=res["viterbi_logprob"], tm=hb.timing())
    hb.close()
    hm.close()
    return out


def _both_forms(monkeypatch, model, obs, offs, expect_fast, window="32", **kw):
    """Evaluates with the fast form allowed and with TEHMM_EMIS_FAST=0; asserts which form ran, equal results and equal
    counters of the exact chain; returns the first evaluation."""
    got = {}
    for knob in ("1", "0"):
        _route(monkeypatch, TEHMM_EMIS_FAST=knob, TEHMM_GAIN_WINDOW=window)
        got[knob] = _eval(model, obs, offs, **kw)
    new, old = got["1"], got["0"]
    print("emis_fast %d / %d, window %d, exact blocks %d / %d, jumps %d / %d"
          % (new["tm"]["count:emis_fast"], old["tm"]["count:emis_fast"], new["tm"]["count:gain_window"],
             new["tm"]["count:viterbi_exact_blocks"], old["tm"]["count:viterbi_exact_blocks"],
             new["tm"]["count:viterbi_chunk_jumps"], old["tm"]["count:viterbi_chunk_jumps"]))
    assert new["tm"]["count:emis_fast"] == (1 if expect_fast else 0)
    assert old["tm"]["count:emis_fast"] == 0
    assert new["tm"]["count:gain_window"] == old["tm"]["count:gain_window"]
    assert_array_equal(new["paths"], old["paths"])
    assert_array_equal(new["vlp"], old["vlp"])
    assert new["tm"]["count:viterbi_exact_blocks"] == old["tm"]["count:viterbi_exact_blocks"]
    assert new["tm"]["count:viterbi_chunk_jumps"] == old["tm"]["count:viterbi_chunk_jumps"]
    return new


def _assert_oracle(got, ref):
    assert_array_equal(got["paths"], ref[0])
    assert_array_equal(got["vlp"], ref[1])


@pytest.mark.parametrize("window", ["32", "0"])
@pytest.mark.parametrize("N", [35, 5])
def test_bench_tracks_window_and_full_pass(monkeypatch, N, window):
    """35 and 5 states (rows of 36 and 8 entries), the bench's ten tracks, ragged intervals; windowed and full pass."""
    model, obs, offs, ref = _case(N)
    got = _both_forms(monkeypatch, model, obs, offs, True, window=window)
    assert got["tm"]["count:gain_window"] == int(window)
    assert got["tm"]["count:viterbi_chunk_jumps"] > 0          # (the lane passes' rows were used)
    _assert_oracle(got, ref)


@pytest.mark.parametrize("N,symbols,gaussian", [
    (5, (3, 5, 12, 250), (3,)),                                           # one observation word, every track in LDS
    (35, (3, 5, 12, 250), (3,)),                                          # ... and its last track from the global table
    (35, (2, 2, 3, 4, 5, 8, 12, 30, 250), (8,)),                          # a partial third word
    (35, (2, 2, 3, 3, 4, 5, 8, 12, 20, 30, 250, 250), (10, 11)),          # three full words
])
def test_track_counts(monkeypatch, N, symbols, gaussian):
    model, obs, offs, ref = _case(N, symbols, gaussian)
    got = _both_forms(monkeypatch, model, obs, offs, True)
    assert got["tm"]["count:viterbi_chunk_jumps"] > 0
    _assert_oracle(got, ref)


def test_symbol_zero_and_symbols_beyond_a_track(monkeypatch):
    """Symbol 0 (missing) and symbols behind a track's last one -- the reference's zero padding -- in LDS tracks and in a
    global-table track (200 symbols beside one of 250)."""
    from oracle import oracle
    symbols = (2, 2, 3, 4, 5, 8, 12, 30, 250, 200)
    model, obs, offs, _ = _case(35, symbols, (8, 9))
    obs = np.array(obs)
    rs = np.random.RandomState(5)
    T = len(obs)
    for k, beyond in ((0, 3), (2, 250), (7, 31), (9, 201), (9, 250)):
        obs[rs.randint(0, T, size=T // 50), k] = beyond
    obs[rs.randint(0, T, size=T // 20), rs.randint(0, len(symbols), size=T // 20)] = 0
    assert (obs[:, 9] > 200).any() and (obs[:, 0] == 3).any() and (obs == 0).any()
    ref = oracle.eval_batch(obs, offs, model.log_probs, model.log_startprob, model.log_transmat, want_post=False)[:2]
    got = _both_forms(monkeypatch, model, obs, offs, True)
    _assert_oracle(got, ref)


@pytest.mark.parametrize("window", ["32", "0"])
def test_impossible_row_inside_and_outside_the_window(monkeypatch, window):
    """A row no state can emit inside the gain window of one item and ahead of the window of another: NaN rows and NaN
    gains as in the old form (equal results, equal counters); the interval without such a row is the oracle's."""
    from oracle import oracle
    model, obs, offs, _ = _case(35)
    lp = model.log_probs.copy()
    lp[1, :, 2] = -np.inf                                   # symbol 2 of track 1: no state can emit it
    obs = np.array(obs)
    obs[obs[:, 1] == 2, 1] = 1
    obs[20 * 128 + 110, 1] = 2                              # item 20 of the first interval, window = positions 96 .. 127
    obs[int(offs[1]) + 30 * 128 + 20, 1] = 2                # item 30 of the second, ahead of the window and its warm-up
    got = _both_forms(monkeypatch, model, obs, offs, True, window=window, log_probs=lp)
    sl = slice(int(offs[2]), int(offs[3]))
    vlp, path = oracle.decode(obs[sl], lp, model.log_startprob, model.log_transmat)
    assert_array_equal(got["paths"][sl], path)
    assert got["vlp"][2] == vlp


@pytest.mark.parametrize("window", ["32", "0"])
def test_interval_ends_at_and_behind_a_staging_block(monkeypatch, window):
    """Observation rows are staged in blocks of four positions: an interval that ends with a block, one that ends one
    position behind it, and a last interval that ends with the allocation."""
    model, obs, offs, ref = _case(35, lens=(96 * 128 + 20, 96 * 128 + 21, 3 * 128))
    got = _both_forms(monkeypatch, model, obs, offs, True, window=window)
    assert got["tm"]["count:viterbi_chunk_jumps"] > 0
    _assert_oracle(got, ref)


@pytest.mark.parametrize("case", ["13_tracks", "large_track_first", "normalize", "segment_ratios"])
def test_fall_backs_keep_the_old_form(monkeypatch, case):
    from oracle import oracle
    from tehmm_amd import synth
    kw = {}
    if case == "13_tracks":
        model, obs, offs, ref = _case(35, (2, 2, 3, 3, 4, 5, 8, 12, 20, 30, 250, 250, 2), (10, 11))
    elif case == "large_track_first":
        model, obs, offs, ref = _case(35, (250, 2, 2, 3, 4, 5, 8, 12, 30, 250), (0, 9))
    elif case == "normalize":
        model, obs, offs, ref = _case(35, normalize=0.5)
        kw["normalize"] = 0.5
    else:
        model, obs, offs, _ = _case(35)
        ratios = np.ascontiguousarray(synth.random_ratios(int(offs[-1]), seed=6))
        ref = oracle.eval_batch(obs, offs, model.log_probs, model.log_startprob, model.log_transmat, 1.0, ratios,
                                want_post=False)[:2]
        kw["ratios"] = ratios
    got = _both_forms(monkeypatch, model, obs, offs, False, **kw)
    assert got["tm"]["count:viterbi_chunk_jumps"] > 0          # (the chunk-parallel Viterbi itself ran)
    _assert_oracle(got, ref)
