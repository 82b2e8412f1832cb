"""The three routes of the batch E-step (tehmm_estep_host.inc) on one small batch each: the fused posterior passes, the
item-parallel (wide) passes and the grouped sequential kernels.  Which route ran and what it reports (the timing keys, in
order), its statistics against the oracle, the per-interval log-probabilities between the routes, a dead interval, an
empty one, and same input -> same bits.  tools/estep_dump.py runs the same cases for a bit-for-bit comparison between
two builds."""
import contextlib
import functools
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

pytestmark = pytest.mark.gpu

KNOBS = ("TEHMM_EMIS_SPLIT", "TEHMM_DEVICE_PLACE", "TEHMM_SPEC_CHUNK", "TEHMM_LANE_SUB", "TEHMM_DEFER", "TEHMM_LANE_VIT",
         "TEHMM_ESTEP_FUSED", "TEHMM_SOFT_TIES", "TEHMM_ESTEP_WIDE", "TEHMM_WIDE_SUB", "TEHMM_LANE_WARMUP",
         "TEHMM_ESTEP_SMALL", "TEHMM_WIDE_ESTEP_SQ", "TEHMM_WIDE_ESTEP_SERIAL")
SMALL_SHAPES = {"TEHMM_SPEC_CHUNK": "256", "TEHMM_LANE_SUB": "128", "TEHMM_WIDE_SUB": "64"}
ROUTE_KNOBS = {
    "fused": {},                                                            # the default below 64 states without ratios
    "wide": {"TEHMM_ESTEP_WIDE": "2"},                                      # the item-parallel passes wherever they apply
    "wide_default": {"TEHMM_ESTEP_WIDE": "1"},                              # ... where the fused passes do not apply
    "sequential": {"TEHMM_ESTEP_FUSED": "0", "TEHMM_ESTEP_WIDE": "0"},
}
# what HipBatch.timing() holds after an E-step on a fresh batch, in order
FUSED_KEYS = ["estep_forward_pass", "estep_backward_pass", "estep_backward_chain", "estep_reduce",
              "count:forward_exact_blocks", "count:forward_chunk_jumps", "count:backward_exact_blocks",
              "count:backward_chunk_jumps"]
WIDE_KEYS = ["estep_emission_rows", "estep_forward_pass", "estep_backward_pass", "estep_reduce",
             "count:wide_estep_attempts", "count:wide_estep_warmup"]
ROUTE_KEYS = {"fused": FUSED_KEYS, "wide": WIDE_KEYS, "wide_default": WIDE_KEYS, "sequential": []}
LENS = [1500, 0, 700, 1]                     # an empty interval, a one-row one, tails shorter than an item / a chunk


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib, build
    build.build()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


@contextlib.contextmanager
def knobs(route):
    """The environment of one route at the small shapes (the library reads its knobs at every call), restored after."""
    saved = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(SMALL_SHAPES)
    os.environ.update(ROUTE_KNOBS[route])
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


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (model, log_probs, obs, offs, ratios or None, routes that take it)."""
    from tehmm_amd import synth
    if name == "plain5":             # a 250-bin track: LDS histograms in the fused and the wide reductions
        model = synth.make_model(5, (3, 5, 4, 250), (3,), seed=17)
        lens, ratios, routes = LENS, False, ("fused", "wide", "sequential")
    elif name == "ratios35":
        model = synth.make_model(35, (3, 5, 4, 30, 250), (4,), seed=47)
        lens, ratios, routes = LENS, True, ("wide_default", "sequential")
    elif name == "dead5":            # second interval: a row no state can emit after its first emittable one
        model = synth.make_model(5, (3, 5, 4), (), seed=21)
        lens, ratios, routes = [1500, 700], False, ("fused", "wide", "sequential")
    elif name == "wide70":           # (tools/estep_dump.py only: 80 padded states)
        model = synth.make_model(70, (3, 5, 4), (), seed=82)
        lens, ratios, routes = LENS, False, ("wide_default",)
    else:
        raise KeyError(name)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(offs[-1])
    obs = synth.sample_obs(model, total, seed=5, missing=0.02)
    log_probs = model.log_probs
    if name == "dead5":
        log_probs = model.log_probs.copy()
        log_probs[1, :, 2] = -np.inf                   # symbol 2 of track 1 cannot be emitted by any state
        obs[obs[:, 1] == 2, 1] = 1
        obs[1800, 1] = 2                               # inside the second interval
    r = _seg_ratios(total, 7) if ratios else None
    return model, log_probs, obs, offs, r, routes


@functools.lru_cache(maxsize=None)
def reference(name):
    from oracle import oracle
    model, log_probs, obs, offs, r, _ = case(name)
    ivs = [(int(offs[i]), int(offs[i + 1])) for i in range(len(offs) - 1) if offs[i + 1] > offs[i]]
    return oracle.estep([obs[a:b] for a, b in ivs], log_probs, model.log_startprob, model.log_transmat, 1.0,
                        [r[a:b] for a, b in ivs] if r is not None else None)


@functools.lru_cache(maxsize=None)
def run(name, route):
    """Two E-steps of one fresh batch on one route: [(logprob, start, trans, obs statistics, interval logprobs)] * 2 and
    the timing keys after each call."""
    from tehmm_amd.engine import HipBatch, HipModel
    model, log_probs, obs, offs, r, _ = case(name)
    K, N, S = log_probs.shape
    out, keys = [], []
    with knobs(route):
        hm = HipModel(model.log_transmat, model.log_startprob, log_probs, 1.0, model.symbols_per_track)
        hb = HipBatch(obs, offs, r)
        for _call in range(2):
            start, trans, st = np.zeros(N), np.zeros((N, N)), np.zeros((K, N, S))
            lp = hm.estep(hb, r is not None, start, trans, st)
            out.append((lp, start, trans, st, hb.interval_logprobs()))
            keys.append(list(hb.timing()))
        hb.close()
        hm.close()
    return out, keys


def _check_vs_oracle(name, route):
    lp, start, trans, st, ilp = run(name, route)[0][0]
    ref = reference(name)
    # (tolerances: test_fused_estep_vs_oracle, test_wide_estep_vs_oracle)
    assert_allclose(lp, ref["logprob"], rtol=1e-9)
    assert_allclose(ilp.sum(), ref["logprob"], rtol=1e-9)
    assert_allclose(start, ref["start"], rtol=1e-6, atol=1e-12)
    assert_allclose(trans, ref["trans"], rtol=1e-6, atol=1e-9)
    assert_allclose(st, ref["obs"], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("name,route", [("plain5", "fused"), ("plain5", "wide"), ("plain5", "sequential"),
                                        ("ratios35", "wide_default"), ("ratios35", "sequential")])
def test_route_runs_reports_and_matches_oracle(name, route):
    """The intended route ran -- the exact timing keys of a fresh batch, in order, after each of two calls -- and its
    statistics and log-likelihood agree with the oracle's per-sequence E-step (the empty interval left out there)."""
    _, keys = run(name, route)
    assert keys[0] == ROUTE_KEYS[route] and keys[1] == ROUTE_KEYS[route]
    assert ("estep_backward_chain" in keys[0]) == (route == "fused")
    assert ("estep_emission_rows" in keys[0]) == route.startswith("wide")
    assert ("estep_reduce" in keys[0]) == (route != "sequential")
    _check_vs_oracle(name, route)


@pytest.mark.parametrize("name", ["plain5", "ratios35"])
def test_interval_logprobs_agree_between_routes(name):
    """tehmm_batch_get_interval_logprobs after each route: the same numbers at 1e-9, 0 for the empty interval."""
    routes = case(name)[5]
    ilps = [run(name, route)[0][0][4] for route in routes]
    for ilp in ilps:
        assert ilp.shape == (len(LENS),) and ilp[1] == 0.0 and np.isfinite(ilp).all()
        assert_allclose(ilp, ilps[-1], rtol=1e-9)                 # (the last route: sequential)


def test_dead_interval_on_every_route():
    """An interval with a row no state can emit after its first emittable one: log-likelihood and statistics are NaN and
    so is that interval's log-probability, on the fused and the sequential route; the item-parallel passes decline it
    (TEHMM_ESTEP_WIDE=2), and what the call returns then is the sequential route's result."""
    got = {route: run("dead5", route) for route in case("dead5")[5]}
    assert got["fused"][1][0] == FUSED_KEYS
    assert got["sequential"][1][0] == []
    assert "estep_emission_rows" not in got["wide"][1][0] and "estep_reduce" not in got["wide"][1][0]
    for route, (out, _) in got.items():
        lp, start, trans, st, ilp = out[0]
        assert np.isnan(lp) and np.isnan(start).all() and np.isnan(trans).all() and np.isnan(st).any(), route
        assert np.isfinite(ilp[0]) and np.isnan(ilp[1]), route
    for a, b in zip(got["wide"][0][0], got["sequential"][0][0]):
        assert_array_equal(np.asarray(a), np.asarray(b))
    assert_allclose(got["fused"][0][0][4][0], got["sequential"][0][0][4][0], rtol=1e-9)


@pytest.mark.parametrize("name,route", [("plain5", "fused"), ("plain5", "wide"), ("ratios35", "wide_default")])
def test_statistics_bit_reproducible(name, route):
    """Same batch, same route, two calls: identical statistics, log-likelihood and interval log-probabilities (ordered
    folds of per-writer partial sums, fixed-point LDS histograms) -- test_estep_statistics_bit_reproducible at the small
    shape, and on the item-parallel passes."""
    out, _ = run(name, route)
    for a, b in zip(out[0], out[1]):
        assert_array_equal(np.asarray(a), np.asarray(b))
