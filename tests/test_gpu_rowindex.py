"""GPU tests of the index-record builder of the fused posterior passes (run with -m gpu).

k_fused_rowindex (the default) must write the records of k_fused_rowindex_ref, the executable definition of their
layout (TEHMM_ROWINDEX_REF=1), byte for byte; the results computed from them are checked against the CPU oracle at the
bar of bench.py: forward log-likelihood and every posterior value within 1e-6 relative."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-6
LENS = [1, 63, 300, 257, 1000, 4099, 2560]      # shorter than an item / than a chunk, no multiples of L or the chunk;
                                                # 133 items of 64, 69 of 128: no multiple of 16 or 64
KNOBS = ("TEHMM_SPEC_CHUNK", "TEHMM_LANE_SUB", "TEHMM_LANE_WARMUP", "TEHMM_LANE_VIT", "TEHMM_LANE_P0", "TEHMM_FUSED",
         "TEHMM_ROWINDEX_REF", "TEHMM_DEFER", "TEHMM_ESTEP_FUSED")
SMALL50 = (2, 3, 4, 5, 3) * 10


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib
    _lib.load()
    assert _lib.device_count() >= 1, "no HIP device visible"
    return _lib


def _records(hb):
    from tehmm_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int64(0)
    _lib.check(lib.tehmm_debug_read_rowindex(hb._h, None, 0, ctypes.byref(n)), "tehmm_debug_read_rowindex")
    assert n.value > 0
    out = np.zeros(n.value, dtype=np.uint64)
    m = ctypes.c_int64(0)
    _lib.check(lib.tehmm_debug_read_rowindex(hb._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n.value,
                                             ctypes.byref(m)), "tehmm_debug_read_rowindex")
    assert m.value == n.value
    return out


def _set_env(monkeypatch, item_len, warmup):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TEHMM_SPEC_CHUNK", "256")
    monkeypatch.setenv("TEHMM_LANE_SUB", str(item_len))
    if warmup is not None:
        monkeypatch.setenv("TEHMM_LANE_WARMUP", str(warmup))


def _equal_records(new, ref):
    assert new.size == ref.size
    diff = np.flatnonzero(new != ref)
    print("index records: %d words, %d differ" % (ref.size, diff.size))
    assert diff.size == 0, "first differing word %d: %016x, reference %016x" % (diff[0], new[diff[0]], ref[diff[0]])
    assert new.tobytes() == ref.tobytes()


def _both_builders(monkeypatch, obs, offs, run, collect=None):
    """Check 1, in both orders, each on a batch of its own.

    reset_cache() drops the cache key, not the buffer: a word the second builder of a batch fails to write keeps the
    first one's value and compares equal.  So the default builder also runs FIRST, on a fresh batch whose buffer comes
    straight from the device allocator (the library's block pool is emptied before), and the reference kernel, whose
    grid-stride loop covers every word, second; the results checked against the oracle (collect) are those of that
    first run.  The second batch takes the order the reference kernel first, reset_cache(), the default builder."""
    from tehmm_amd import _lib
    from tehmm_amd.engine import HipBatch
    _lib.trim_pools()
    monkeypatch.delenv("TEHMM_ROWINDEX_REF", raising=False)
    hb = HipBatch(obs, offs)
    try:
        out = run(hb)
        new = _records(hb)
        got = collect(hb) if collect else None
        monkeypatch.setenv("TEHMM_ROWINDEX_REF", "1")
        hb.reset_cache()
        run(hb)
        _equal_records(new, _records(hb))
    finally:
        hb.close()
    hb = HipBatch(obs, offs)
    try:
        run(hb)
        ref = _records(hb)
        hb.reset_cache()
        monkeypatch.delenv("TEHMM_ROWINDEX_REF")
        run(hb)
        _equal_records(_records(hb), ref)
        _equal_records(new, ref)
    finally:
        hb.close()
    return out, got


def _out_of_range(model, obs, seed, tracks=(1, 8), last=255):
    """About 1 % of the symbols of one small track (1: two symbols) and of one 250-bin track (8) replaced by
    values at or beyond the track's symbol count, `last` (255) included."""
    rs = np.random.RandomState(seed)
    obs = obs.copy()
    for k in tracks:
        first_bad = model.symbols_per_track[k] + 1            # rows of the track: symbol 0 (missing) + its symbols
        bad = np.flatnonzero(rs.rand(obs.shape[0]) < 0.01)
        obs[bad, k] = rs.randint(first_bad, last + 1, size=bad.size)
        obs[bad[::5], k] = last
        obs[bad[1::5], k] = first_bad
    return obs


_CASES = {
    # name: (states, symbols per track (a synth configuration or a tuple), item length, out-of-range symbols)
    "a": (35, "CONFIG2", 64, False),
    "b": (35, "CONFIG4", 128, False),
    "c": (35, "CONFIG3B", 64, False),
    "d": (5, (4,), 64, False),
    "e": (7, SMALL50, 64, False),
    "f": (35, "CONFIG2", 64, True),
    "f-small": (35, "CONFIG2", 64, "below S"),     # not in the issue's list: the half of case f the oracle defines
    "g": (60, "CONFIG2", 64, False),
}
_cache = {}


def _case(name):
    """Model, observations and the oracle's results of a case: computed once, shared by its warm-up variants."""
    if name in _cache:
        return _cache[name]
    from oracle import oracle
    from tehmm_amd import synth
    N, sym, item_len, bad = _CASES[name]
    if isinstance(sym, str):
        symbols, gauss = getattr(synth, sym + "_SYMBOLS"), getattr(synth, sym + "_GAUSSIAN")
    else:
        symbols, gauss = sym, ()
    model = synth.make_model(N, symbols, gauss, seed=3 + N)
    offs = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    obs = synth.sample_obs(model, int(offs[-1]), seed=17 + N, missing=0.03)
    ref = None
    if bad == "below S":
        # out-of-range symbols of the small track only, all below S = 251: the oracle reads the zero padding of
        # logProbs for them, which is what the device's zero row holds
        obs = _out_of_range(model, obs, seed=5, tracks=(1,), last=250)
        assert (obs[:, 1] == 250).any()
        bad = False
    if bad:
        # Case f runs check 1 only.  The oracle does not define such symbols the way the device does: it indexes
        # logProbs[(k * N + j) * S + symbol] unchecked (oracle/tehmm_oracle.c), so a symbol between the track's own
        # count and S = 1 + 250 reads the zero padding as the device's zero row does, but 255 >= S reads the NEXT
        # state's (or track's) entries -- and beyond the table for the last one.  There is no reference value.
        obs = _out_of_range(model, obs, seed=5)
        assert (obs[:, 1] == 255).any() and (obs[:, 8] == 255).any()
        assert model.log_probs.shape[2] == 251
    else:
        _, _, flp, post = oracle.eval_batch(obs, offs, model.log_probs, model.log_startprob, model.log_transmat,
                                            1.0, None, want_post=True, n_threads=4)
        post.setflags(write=False)
        ref = (flp, post)
    _cache[name] = (model, offs, obs, ref, item_len)
    return _cache[name]


@pytest.mark.parametrize("name,warmup", [("a", 32), ("a", 64), ("a", 200), ("b", None), ("c", None), ("d", None),
                                         ("e", None), ("f", None), ("f-small", None), ("g", None)])
def test_records_match_reference_kernel_and_oracle(monkeypatch, name, warmup):
    from tehmm_amd.engine import HipModel
    model, offs, obs, ref, item_len = _case(name)
    _set_env(monkeypatch, item_len, warmup)
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs, 1.0, model.symbols_per_track)
    try:
        res, post = _both_builders(monkeypatch, obs, offs, lambda hb: hm.eval(hb, viterbi=False, posterior=True),
                                   lambda hb: np.array(hb.posteriors()))
        flp = np.array(res["forward_logprob"])
    finally:
        hm.close()
    if ref is None:
        assert np.isfinite(post).all()
        return
    flp_o, post_o = ref
    rel_lp = float(np.max(np.abs(flp - flp_o) / np.abs(flp_o)))
    rel_post = float(np.max(np.abs(post - post_o) / post_o))
    print("case %s warm-up %s: forward log-likelihood rel. err %.3g, posterior max rel. err %.3g"
          % (name, warmup, rel_lp, rel_post))
    assert rel_lp <= RTOL
    assert rel_post <= RTOL


def test_estep_route_builds_the_same_records(monkeypatch):
    """The fused E-step builds its records with the same kernel: four chunks of 2 560 positions, 35 states, K = 12."""
    from oracle import oracle
    from tehmm_amd import synth
    from tehmm_amd.engine import HipModel
    _set_env(monkeypatch, 64, None)
    model = synth.make_model(35, synth.CONFIG4_SYMBOLS, synth.CONFIG4_GAUSSIAN, seed=12)
    n, L = 4, 2560
    offs = (np.arange(n + 1) * L).astype(np.int64)
    obs = synth.sample_obs(model, n * L, seed=80, missing=0.03)
    K, N, S = model.log_probs.shape
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs, 1.0, model.symbols_per_track)

    def run(hb):
        st = {"start": np.zeros(N), "trans": np.zeros((N, N)), "obs": np.zeros((K, N, S))}
        st["lp"] = hm.estep(hb, False, st["start"], st["trans"], st["obs"])
        return st

    try:
        stats, _ = _both_builders(monkeypatch, obs, offs, run)
    finally:
        hm.close()
    ref = oracle.estep([obs[offs[i]:offs[i + 1]] for i in range(n)], model.log_probs, model.log_startprob,
                       model.log_transmat, 1.0, None)

    def rel(a, b, floor):
        """the measure of bench.py's E-step check: |a - b| over |b|, entries below `floor` measured against it"""
        return float(np.max(np.abs(np.asarray(a) - b) / np.maximum(np.abs(b), floor)))

    errs = {"logprob": rel(stats["lp"], ref["logprob"], 1e-300), "start": rel(stats["start"], ref["start"], 1e-12),
            "trans": rel(stats["trans"], ref["trans"], 1e-6), "obs": rel(stats["obs"], ref["obs"], 1e-6)}
    print("E-step statistics, max rel. err:", errs)
    for k, v in errs.items():
        assert v <= RTOL, (k, v)
