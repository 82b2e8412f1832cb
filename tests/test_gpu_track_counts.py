"""Every evaluation and E-step route at 33 to 128 tracks (tehmm_model_create takes up to TEHMM_MAX_TRACKS = 128), against
the CPU oracle on the same inputs.  The kernels branch on the track count; DESIGN.md ("What the track count selects")
lists the branches and the ids below that run them:

  * observation words beyond the eighth (track 32 and up) and track info beyond `readlane` (track 64 and up) in the
    sequential E-step's k_estep_accum;
  * FKW, the words per index record of the fused passes: 12 at 33-48 tracks, 24 at 49-78;
  * the fused cut-off: 78 tracks on the fused passes, 79 on the round-1 posterior pipeline and the sequential E-step;
  * the 1024-row one-hot table of the E-step reductions: the spill into LDS histogram groups (fused), the decline (wide);
  * tracks 16 and up outside the prefetched words of k_wide_emis_tile, the KPW loops of the 129+ state kernels;
  * the lane group max(N, K / 4 words) of the emission distribution; LDS staging of some tracks only.

Bars are the project's own: Viterbi paths / scores and emission frames bit for bit, posteriors and forward
log-likelihoods at 1e-6 (BASELINE.json north star, test_chunk_parallel_paths), E-step statistics at 1e-6 and
log-likelihoods at 1e-9 (test_gpu_estep_routes.py), the masked emission column at rtol 1e-12 / atol 1e-10
(test_gpu_emission_dist.py), array-level statistics at 1e-8 (test_array_level_vs_golden).  Every case prints its
observed worst relative error before it asserts."""
import contextlib
import functools
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

pytestmark = pytest.mark.gpu

RTOL = 1e-6

# symbols per track; all multinomial but the 250-bin tracks
TRACKS = {
    "K33": (2, 3, 4) * 11,                     # first track behind the eighth observation word; FKW = 12
    "K48": (2, 3, 4) * 16,                     # the last track count of FKW = 12 ...
    "K49": (2, 3, 4) * 16 + (2,),              # ... the first of FKW = 24
    "K65": (2, 3) * 32 + (250,),               # track 64: LDS-copy track info AND the global-statistics path (lb < 0)
    "K78": (2, 3) * 39,                        # the last track count the fused passes take ...
    "K79": (2, 3) * 39 + (4,),                 # ... the first they decline
    "K127": (2,) * 126 + (5,),                 # KP padding: 127 -> 128
    "K128": (2, 3) * 63 + (250, 4),            # the maximum, a gaussian track among the last words
    "K78_16": (15,) * 78,                      # 78 x 16 = 1248 one-hot rows > 1024 (TEHMM_ESTEP_MAXRT * 16)
    "K128_9": (8,) * 128,                      # 1152 rows
}
GAUSS = {"K65": (64,), "K128": (126,)}
EVAL_LENS = [1, 2, 63, 300, 1025, 2600]
LARGE_LENS = [1, 300, 2600]
ESTEP_LENS = [1500, 0, 700, 1, 1100]           # test_gpu_estep_routes.LENS + an interval that spans a chunk

KNOBS = ("TEHMM_EMIS_SPLIT", "TEHMM_DEVICE_PLACE", "TEHMM_SPEC_CHUNK", "TEHMM_LANE_SUB", "TEHMM_DEFER", "TEHMM_LANE_VIT",
         "TEHMM_LANE_P0", "TEHMM_LANE_PROBE", "TEHMM_FUSED", "TEHMM_GAIN_WINDOW", "TEHMM_ROWINDEX_REF",
         "TEHMM_ESTEP_FUSED", "TEHMM_SOFT_TIES", "TEHMM_ESTEP_WIDE", "TEHMM_WIDE_SUB", "TEHMM_LANE_WARMUP",
         "TEHMM_ESTEP_SMALL", "TEHMM_WIDE_ESTEP_SQ", "TEHMM_WIDE_ESTEP_SERIAL", "TEHMM_WIDE", "TEHMM_WIDE_CP",
         "TEHMM_WIDE_VIT", "TEHMM_WIDE_VIT_WARMUP", "TEHMM_WIDE_TOL", "TEHMM_WIDE_HEAD", "TEHMM_WIDE_POLL")
SMALL_SHAPES = {"TEHMM_SPEC_CHUNK": "256", "TEHMM_LANE_SUB": "64", "TEHMM_WIDE_SUB": "64"}

# evaluation routes: the knobs on top of the small geometry
EVAL_ROUTES = {
    "sequential": {"TEHMM_SPEC_CHUNK": "0"},       # the cooperative one-workgroup kernels
    "chunk": {},                                   # the chunk-parallel default
    "round1": {"TEHMM_FUSED": "0"},                # ... with the round-1 posterior pipeline forced
}
# posterior stage names of eval_timings (tehmm_hip.hip), below 64 states
FUSED_EVAL_KEYS = {"forward_pass", "backward_posterior_pass", "backward_chain"}
ROUND1_EVAL_KEYS = {"forward_backward_speculate", "forward_backward", "posterior_combine"}
SEQ_EVAL_KEYS = {"forward_backward", "posterior_combine"}

# E-step routes and what HipBatch.timing() holds after one on a fresh batch, in order (test_gpu_estep_routes.py)
ROUTE_KNOBS = {
    "fused": {},
    "wide": {"TEHMM_ESTEP_WIDE": "2"},
    "wide_default": {"TEHMM_ESTEP_WIDE": "1"},
    "sequential": {"TEHMM_ESTEP_FUSED": "0", "TEHMM_ESTEP_WIDE": "0"},
}
FUSED_KEYS = ["estep_forward_pass", "estep_backward_pass", "estep_backward_chain", "estep_reduce",
              "count:forward_exact_blocks", "count:forward_chunk_jumps", "count:backward_exact_blocks",
              "count:backward_chunk_jumps"]
WIDE_KEYS = ["estep_emission_rows", "estep_forward_pass", "estep_backward_pass", "estep_reduce",
             "count:wide_estep_attempts", "count:wide_estep_warmup"]
ROUTE_KEYS = {"fused": FUSED_KEYS, "wide": WIDE_KEYS, "wide_default": WIDE_KEYS, "sequential": []}


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib, build
    build.build()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


@contextlib.contextmanager
def knobs(extra):
    """The small geometry plus `extra` (the library reads its knobs at every call), the environment restored after."""
    saved = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(SMALL_SHAPES)
    os.environ.update(extra)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _seg_ratios(total, seed, mean=4.0):
    """Segment-length ratios as emission.getSegmentRatios gives them: length / mean length, many of them 1."""
    rs = np.random.RandomState(seed)
    r = np.clip(rs.geometric(1.0 / mean, size=total), 1, 60).astype(np.float64) / mean
    r[rs.rand(total) < 0.3] = 1.0
    return r


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _rel(a, b, floor):
    """Largest relative error of a against b over the cells of b above `floor`."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.abs(b) > floor
    return float(np.max(np.abs(a - b)[m] / np.abs(b)[m])) if m.any() else 0.0


@functools.lru_cache(maxsize=None)
def inputs(N, kname, lens):
    """(model, obs, offsets, ratios): computed once per shape, shared between the routes and never changed."""
    from tehmm_amd import synth
    model = synth.make_model(N, TRACKS[kname], GAUSS.get(kname, ()), seed=1000 + 7 * N + len(TRACKS[kname]))
    offs = _offsets(lens)
    total = int(offs[-1])
    obs = synth.sample_obs(model, total, seed=5, missing=0.03)
    r = _seg_ratios(total, 7)
    for a in (obs, offs, r, model.log_probs, model.log_transmat, model.log_startprob):
        a.setflags(write=False)
    return model, obs, offs, r


def _model_handle(model):
    from tehmm_amd.engine import HipModel
    return HipModel(model.log_transmat, model.log_startprob, model.log_probs, 1.0, model.symbols_per_track)


# ---------------------------------------------------------------------------------------------------- evaluation
@functools.lru_cache(maxsize=None)
def eval_reference(N, kname, ratios, lens):
    from oracle import oracle
    model, obs, offs, r = inputs(N, kname, lens)
    return oracle.eval_batch(obs, offs, model.log_probs, model.log_startprob, model.log_transmat, 1.0,
                             r if ratios else None, n_threads=8)


def run_eval(N, kname, route, ratios, lens=tuple(EVAL_LENS)):
    """Viterbi and posterior together, twice on one batch (the second call reuses the workspaces): the results of
    each call and the stage names of the last."""
    from tehmm_amd.engine import HipBatch
    model, obs, offs, r = inputs(N, kname, lens)
    out = []
    with knobs(EVAL_ROUTES[route]):
        hm = _model_handle(model)
        hb = HipBatch(obs, offs, r if ratios else None)
        for _call in range(2):
            res = hm.eval(hb, viterbi=True, posterior=True)
            out.append((hb.paths(), res["viterbi_logprob"], res["forward_logprob"], hb.posteriors(N)))
        names = {k for k in hb.timing() if not k.startswith("count:")}
        hb.close()
        hm.close()
    return out, names


def check_eval(N, kname, route, ratios, lens=tuple(EVAL_LENS)):
    """The assertions of test_chunk_parallel_paths; returns the stage names."""
    out, names = run_eval(N, kname, route, ratios, lens)
    p_o, vlp_o, flp_o, post_o = eval_reference(N, kname, ratios, lens)
    for call, (paths, vlp, flp, post) in enumerate(out):
        print("eval N=%d %s %s ratios=%s call %d: path mismatches %d, max rel error of the posteriors (cells > 1e-9) "
              "%.3g, of forward_logprob %.3g" % (N, kname, route, ratios, call, int((paths != p_o).sum()),
                                                 _rel(post, post_o, 1e-9), _rel(flp, flp_o, 0.0)))
    for paths, vlp, flp, post in out:
        assert_array_equal(paths, p_o)
        assert_array_equal(vlp, vlp_o)
        assert_allclose(flp, flp_o, rtol=RTOL)
        assert_allclose(post, post_o, rtol=RTOL, atol=1e-15)
        assert_allclose(post.sum(axis=1), 1.0, rtol=1e-9)
    # (the stage names of the 129+ state kernels: test_gpu_large_states.py)
    assert ({"k_vit_large", "k_fwd_large", "k_bwd_large"} if N > 128 else {"viterbi", "traceback"}) <= names
    return names


def _assert_eval_pipeline(names, kname, route):
    """Which posterior pipeline ran, from the stage names: the fused passes up to 78 tracks, the round-1 pipeline from 79
    and under TEHMM_FUSED=0, the cooperative kernels under TEHMM_SPEC_CHUNK=0."""
    if route == "sequential":
        assert SEQ_EVAL_KEYS <= names
        assert not (names & (FUSED_EVAL_KEYS | {"forward_backward_speculate", "viterbi_speculate"}))
    elif route == "chunk" and len(TRACKS[kname]) <= 78:
        assert FUSED_EVAL_KEYS <= names and not (names & ROUND1_EVAL_KEYS)
    else:
        assert ROUND1_EVAL_KEYS <= names and not (names & FUSED_EVAL_KEYS)


EVAL35 = [(k, route, ratios) for k in ("K33", "K48", "K49", "K78", "K79", "K127", "K128")
          for route, ratios in (("sequential", False), ("chunk", False), ("chunk", True))]
EVAL35.append(("K78", "round1", False))            # both sides of the cut-off run both pipelines (K79: round-1 by default)


@pytest.mark.parametrize("kname,route,ratios", EVAL35,
                         ids=["%s-%s%s" % (k, route, "-ratios" if r else "") for k, route, r in EVAL35])
def test_eval_35_states(kname, route, ratios):
    names = check_eval(35, kname, route, ratios)
    _assert_eval_pipeline(names, kname, route)


EVAL_OTHER = [(3, "K128", False), (63, "K33", False), (63, "K128", False)]
EVAL_OTHER += [(N, k, r) for N in (64, 100) for k in ("K33", "K128") for r in (False, True)]


@pytest.mark.parametrize("N,kname,ratios", EVAL_OTHER,
                         ids=["N%d-%s%s" % (N, k, "-ratios" if r else "") for N, k, r in EVAL_OTHER])
def test_eval_other_state_counts(N, kname, ratios):
    """3 states x 128 tracks, 64 padded states, and the 64-128 state kernels of tehmm_wide.hip.h (tracks 16 and up lie
    outside the prefetched words of k_wide_emis_tile)."""
    check_eval(N, kname, "chunk", ratios)


@pytest.mark.parametrize("kname", ["K33", "K128"])
def test_eval_200_states(kname):
    """tehmm_large.hip.h: the lane3 and coop emission loops over KPW."""
    check_eval(200, kname, "chunk", False, tuple(LARGE_LENS))


# ---------------------------------------------------------------------------------------------------- E-step
@functools.lru_cache(maxsize=None)
def estep_reference(N, kname, ratios):
    from oracle import oracle
    model, obs, offs, r = inputs(N, kname, tuple(ESTEP_LENS))
    ivs = [(int(offs[i]), int(offs[i + 1])) for i in range(len(offs) - 1) if offs[i + 1] > offs[i]]
    return oracle.estep([obs[a:b] for a, b in ivs], model.log_probs, model.log_startprob, model.log_transmat, 1.0,
                        [r[a:b] for a, b in ivs] if ratios else None)


def _estep_twice(N, kname, route, ratios):
    from tehmm_amd.engine import HipBatch
    model, obs, offs, r = inputs(N, kname, tuple(ESTEP_LENS))
    K, _, S = model.log_probs.shape
    out, keys = [], []
    with knobs(ROUTE_KNOBS[route]):
        hm = _model_handle(model)
        hb = HipBatch(obs, offs, r if ratios else None)
        for _call in range(2):
            start, trans, st = np.zeros(N), np.zeros((N, N)), np.zeros((K, N, S))
            lp = hm.estep(hb, ratios, start, trans, st)
            out.append((lp, start, trans, st, hb.interval_logprobs()))
            keys.append(list(hb.timing()))
        hb.close()
        hm.close()
    return out, keys


@functools.lru_cache(maxsize=None)
def run_estep(N, kname, route, ratios):
    """Two E-steps of one fresh batch on one route: [(logprob, start, trans, obs statistics, interval logprobs)] * 2 and
    the timing keys after each call."""
    return _estep_twice(N, kname, route, ratios)


def _check_estep_vs_oracle(got, N, kname, ratios, tag):
    lp, start, trans, st, ilp = got
    ref = estep_reference(N, kname, ratios)
    worst = max(_rel(start, ref["start"], 1e-9), _rel(trans, ref["trans"], 1e-6), _rel(st, ref["obs"], 1e-6))
    print("E-step N=%d %s %s ratios=%s: max rel error of the statistics %.3g, of logprob %.3g"
          % (N, kname, tag, ratios, worst, _rel(lp, ref["logprob"], 0.0)))
    assert_allclose(lp, ref["logprob"], rtol=1e-9)
    assert_allclose(ilp.sum(), ref["logprob"], rtol=1e-9)
    assert_allclose(start, ref["start"], rtol=1e-6, atol=1e-12)
    assert_allclose(trans, ref["trans"], rtol=1e-6, atol=1e-9)
    assert_allclose(st, ref["obs"], rtol=1e-6, atol=1e-9)
    assert ilp.shape == (len(ESTEP_LENS),) and ilp[1] == 0.0                   # the empty interval


ESTEP = [(35, k, "sequential", r) for k in ("K33", "K65", "K128") for r in (False, True)]
ESTEP += [(35, "K33", "fused", False), (35, "K49", "fused", False), (35, "K78", "fused", False),
          (35, "K78_16", "fused", False),                                        # the spill into LDS histogram groups
          (7, "K78", "fused", False)]
ESTEP += [(35, "K33", "wide", False), (35, "K128", "wide", False), (35, "K65", "wide_default", True),
          (70, "K65", "wide_default", False), (70, "K128", "wide_default", False)]


@pytest.mark.parametrize("N,kname,route,ratios", ESTEP,
                         ids=["%s-N%d-%s%s" % (route, N, k, "-ratios" if r else "") for N, k, route, r in ESTEP])
def test_estep_route(N, kname, route, ratios):
    """The intended route ran (the exact timing keys of a fresh batch, in order, after each of two calls), its statistics
    and log-likelihood agree with the oracle's per-sequence E-step, and the second call gives the same bits (ordered
    folds of per-writer partial sums on every route)."""
    out, keys = run_estep(N, kname, route, ratios)
    assert keys[0] == ROUTE_KEYS[route] and keys[1] == ROUTE_KEYS[route]
    _check_estep_vs_oracle(out[0], N, kname, ratios, route)
    _check_estep_vs_oracle(out[1], N, kname, ratios, route + " (second call)")
    for a, b in zip(out[0], out[1]):
        assert_array_equal(np.asarray(a), np.asarray(b))


# ---------------------------------------------------------------------------------------------------- declines
@pytest.mark.parametrize("kname", ["K79", "K128"])
def test_fused_estep_declines_above_78_tracks(kname):
    """estep_fused_wanted: no index records beyond 78 tracks.  Under the fused route's knobs the grouped sequential
    kernels serve the call (no stage of the fused or the item-parallel passes is reported), at the same bars."""
    out, keys = run_estep(35, kname, "fused", False)
    for k in keys:
        assert k != FUSED_KEYS
        assert not ({"estep_backward_chain", "estep_reduce", "estep_emission_rows", "estep_forward_pass"} & set(k))
        assert k == ROUTE_KEYS["sequential"]
    _check_estep_vs_oracle(out[0], 35, kname, False, "fused knobs, declined")
    _check_estep_vs_oracle(out[1], 35, kname, False, "fused knobs, declined (second call)")


def _cells_differing(a, b):
    """'name: differing cells / cells, largest relative difference' of two E-step results, or 'identical'."""
    out = []
    for name, x, y in zip(("logprob", "start", "trans", "obs", "interval logprobs"), a, b):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        ne = x != y
        if ne.any():
            out.append("%s %d / %d, max rel %.3g" % (name, int(ne.sum()), ne.size, _rel(x[ne], y[ne], 0.0)))
    return "; ".join(out) or "identical"


def test_wide_estep_declines_beyond_the_row_table():
    """wide_estep_build_rows: 128 tracks of 9 rows are 1152 one-hot rows, more than the table's 1024.  Below 64 states
    the item-parallel passes decline (TEHMM_ESTEP_WIDE=2, segment ratios: no stage of theirs is reported) and the
    sequential kernels serve the call: the log-likelihood and the per-interval log-probabilities are those of the
    sequential route bit for bit, the statistics meet the oracle at the bars of test_estep_route, on both calls."""
    wide, wkeys = run_estep(35, "K128_9", "wide", True)
    seq, skeys = run_estep(35, "K128_9", "sequential", True)
    for k in wkeys:
        assert "estep_emission_rows" not in k and "estep_reduce" not in k and k != WIDE_KEYS
        assert k == ROUTE_KEYS["sequential"]
    assert skeys[0] == [] and skeys[1] == []
    for call in range(2):
        assert wide[call][0] == seq[call][0]
        assert_array_equal(wide[call][4], seq[call][4])
        _check_estep_vs_oracle(wide[call], 35, "K128_9", True, "wide knobs, declined (call %d)" % call)
        _check_estep_vs_oracle(seq[call], 35, "K128_9", True, "sequential (call %d)" % call)


def test_declined_wide_estep_equals_sequential_bit_for_bit():
    """The same case, statistics included: what the declined call returns equals the sequential route's result bit for
    bit -- the pattern of test_dead_interval_on_every_route, here on finite statistics.  It holds because the sequential
    route is reproducible: every wave of k_estep_accum adds into a slot and an LDS histogram of its own, and
    k_estep_accum_fold adds the slots in ascending order.  (With the waves adding into shared accumulators in arrival
    order, two calls on one batch differed in 10109 of 40320 emission cells and 304 of 1225 transition cells, by up to
    7e-16, and this comparison failed.)"""
    wide, _ = run_estep(35, "K128_9", "wide", True)
    seq, _ = run_estep(35, "K128_9", "sequential", True)
    print("sequential call 0 against call 1: " + _cells_differing(seq[0], seq[1]))
    for call in range(2):
        print("declined call %d against the sequential route's: %s" % (call, _cells_differing(wide[call], seq[call])))
    for call in range(2):
        for a, b in zip(wide[call], seq[call]):
            assert_array_equal(np.asarray(a), np.asarray(b))


def test_wide_estep_unsupported_beyond_the_row_table_at_70_states():
    """... and from 64 states the call fails with TEHMM_ERR_UNSUPPORTED (MultitrackHmm._do_estep then runs the
    per-sequence loop over the array-level entry points), as in test_wide_estep_falls_back.  The next valid E-step of
    the process is served."""
    from tehmm_amd import _lib
    from tehmm_amd.engine import HipBatch
    model, obs, offs, r = inputs(70, "K128_9", tuple(ESTEP_LENS))
    K, _, S = model.log_probs.shape
    with knobs({}):
        hm = _model_handle(model)
        hb = HipBatch(obs, offs)
        start, trans, st = np.zeros(70), np.zeros((70, 70)), np.zeros((K, 70, S))
        with pytest.raises(_lib.TeHmmHipError) as ei:
            hm.estep(hb, False, start, trans, st)
        assert ei.value.code == -3
        assert "estep_emission_rows" not in hb.timing()
        hb.close()
        hm.close()
    out, keys = _estep_twice(70, "K65", "wide_default", False)
    assert keys[0] == WIDE_KEYS
    _check_estep_vs_oracle(out[0], 70, "K65", False, "wide_default after the unsupported call")


# ---------------------------------------------------------------------------------------------------- emission distribution
EDIST_LENS = (65, 1000, 1, 2, 63, 64)           # test_gpu_emission_dist.LENS


def _column(frame, mask):
    with np.errstate(divide="ignore"):
        sums = np.sum(np.exp(frame) * mask, axis=1)
        col = np.log(sums)
    # the derivation of the tolerance (test_gpu_emission_dist.py) needs the sums out of the denormal range
    assert np.all((sums == 0.0) | (sums >= 1e-280))
    return col


def _check_column(got, want):
    inf = np.isneginf(want)
    assert_array_equal(np.isneginf(got), inf)
    assert np.all(np.isfinite(got[~inf]))
    assert_allclose(got[~inf], want[~inf], rtol=1e-12, atol=1e-10)


@pytest.mark.parametrize("with_r", [False, True], ids=["plain", "ratios"])
@pytest.mark.parametrize("N,kname", [(3, "K128"), (12, "K33"), (40, "K128"), (100, "K65")])
def test_emission_distribution(N, kname, with_r):
    """HipBatch.emissions / emission_masksum (tehmm_edist.hip.h): the lane group per row is max(N, K / 4 words), so 3
    states x 128 tracks take the 32-lane instantiation.  Frames bit for bit, the masked column at that file's tolerance.
    The ratios are _seg_ratios at mean 30, i.e. at most 2: a row of the 128-track models is no smaller than
    63 * (log(1 / 5) + log(1 / 9)) + log(1 / 13) + log(4e-4) = -250.2 (the generator's multinomial rows are
    (0.2 + 0.6 u) / sum, its gaussian rows at least 0.1 / 250 before a normalisation by at most 1), so every masked
    sum stays above exp(-501) = 2.6e-218 and clear of the denormal range, which the tolerance needs."""
    from oracle import oracle
    from tehmm_amd.engine import HipBatch
    model, obs, offs, _ = inputs(N, kname, EDIST_LENS)
    ratios = _seg_ratios(int(offs[-1]), 11, mean=30.0)
    assert ratios.max() <= 2.0 and ratios.min() < 1.0
    want = np.concatenate([oracle.emission(obs[a:b], model.log_probs, 1.0, ratios[a:b] if with_r else None)
                           for a, b in zip(offs[:-1], offs[1:])])
    masks = {"ones": np.ones(N), "single": (np.arange(N) == N - 1).astype(np.float64),
             "third": (np.arange(N) % 3 == 0).astype(np.float64)}
    with knobs({}):
        hm = _model_handle(model)
        hb = HipBatch(obs, offs, ratios)
        frame = hb.emissions(hm, use_ratios=with_r)
        cols = {name: hb.emission_masksum(hm, mask, use_ratios=with_r) for name, mask in masks.items()}
        hb.close()
        hm.close()
    print("emission distribution N=%d %s ratios=%s: %d cells differ from the oracle's frame; max abs error of the "
          "masked columns %.3g" % (N, kname, with_r, int((frame != want).sum()),
                                   max(float(np.max(np.abs(cols[n] - _column(want, masks[n])))) for n in masks)))
    assert frame.shape == want.shape
    assert_array_equal(frame, want)
    for name, mask in masks.items():
        _check_column(cols[name], _column(want, mask))


# ---------------------------------------------------------------------------------------------------- array level
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32], ids=["u8", "u16", "i32"])
@pytest.mark.parametrize("kname", ["K127", "K128"])
def test_array_level_emission(kname, dtype):
    """_emission.fastAllLogProbs (tehmm_emission_u8 / _u16 / _i32) at 127 and 128 tracks, bit-equal to the oracle: plain,
    and with the normalisation factor and segment ratios."""
    from oracle import oracle
    from tehmm_amd import _emission
    model, obs, offs, r = inputs(35, kname, tuple(EVAL_LENS))
    o = obs.astype(dtype)
    T, K = o.shape
    for normalize, ratios in ((1.0, None), (3.0 / K, r)):
        frame = np.zeros((T, 35))
        _emission.fastAllLogProbs(o, model.log_probs, frame, normalize, ratios)
        assert_array_equal(frame, oracle.emission(o, model.log_probs, normalize, ratios))


@pytest.mark.parametrize("with_r", [False, True], ids=["plain", "ratios"])
def test_array_level_accumulate_stats_128_tracks(with_r):
    """_emission.fastAccumulateStats at 128 tracks (a 250-bin track among them) against the oracle's accumulation of the
    same posteriors, at the tolerance of test_array_level_vs_golden."""
    from oracle import oracle
    from tehmm_amd import _emission
    model, obs, offs, r = inputs(35, "K128", tuple(EVAL_LENS))
    post = eval_reference(35, "K128", False, tuple(EVAL_LENS))[3]
    ratios = r if with_r else None
    want = oracle.accumulate_obs(obs, np.zeros_like(model.log_probs), post, ratios)
    for dtype in (np.uint8, np.uint16, np.int32):
        stats = np.zeros_like(model.log_probs)
        _emission.fastAccumulateStats(obs.astype(dtype), stats, post, ratios)
        print("fastAccumulateStats K128 %s ratios=%s: max rel error %.3g" % (np.dtype(dtype).name, with_r,
                                                                            _rel(stats, want, 1e-300)))
        assert_allclose(stats, want, rtol=1e-8, atol=1e-300)


# ---------------------------------------------------------------------------------------------------- limits
def test_129_tracks_are_refused_and_128_still_served():
    from tehmm_amd import _lib, synth
    from tehmm_amd.engine import HipModel
    model = synth.make_model(5, (2,) * 129, (), seed=3)
    with pytest.raises(_lib.TeHmmHipError) as ei:
        HipModel(model.log_transmat, model.log_startprob, model.log_probs, 1.0, model.symbols_per_track)
    assert ei.value.code == -3
    assert "tehmm_model_create: N > 1024, K > 128 or S > 256" in str(ei.value)
    names = check_eval(35, "K128", "chunk", False)
    _assert_eval_pipeline(names, "K128", "chunk")
