"""Maximum-posterior decoding, the parts that need no GPU: the C ABI's symbols and argument checks, the multi-rank
gather of the new result keys (two gloo ranks, a stub compute), and the host path of tables that cannot fuse."""
import ctypes
import os
import socket

import numpy as np
import pytest
from numpy.testing import assert_array_equal

NEW_SYMBOLS = ("tehmm_batch_map_decode", "tehmm_batch_get_map_paths", "tehmm_batch_get_map_masksum",
               "tehmm_posterior_argmax")
ERR_ARG, ERR_HIP = -1, -2


@pytest.fixture(scope="module")
def lib():
    from tehmm_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_exported_and_declared(lib):
    from tehmm_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.tehmm_abi_version() == 4
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include",
                               "tehmm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header


def test_bad_arguments(lib):
    from tehmm_amd._lib import f64p, i64p, ptr
    out_i = np.zeros(4, dtype=np.int64)
    out_d = np.zeros(4)
    post = np.zeros((2, 2))
    assert lib.tehmm_batch_map_decode(None, None, ptr(out_d, f64p)) == ERR_ARG
    assert b"tehmm_batch_map_decode" in lib.tehmm_last_error()
    assert lib.tehmm_batch_get_map_paths(None, 0, 1, ptr(out_i, i64p)) == ERR_ARG
    assert lib.tehmm_batch_get_map_masksum(None, 0, 1, ptr(out_d, f64p)) == ERR_ARG
    assert lib.tehmm_posterior_argmax(2, 2, None, ptr(out_i, i64p), ptr(out_d, f64p)) == ERR_ARG
    assert lib.tehmm_posterior_argmax(2, 2, ptr(post, f64p), None, ptr(out_d, f64p)) == ERR_ARG
    assert lib.tehmm_posterior_argmax(-1, 2, ptr(post, f64p), ptr(out_i, i64p), None) == ERR_ARG
    assert lib.tehmm_posterior_argmax(2, 0, ptr(post, f64p), ptr(out_i, i64p), None) == ERR_ARG
    assert lib.tehmm_posterior_argmax(2, 1025, ptr(post, f64p), ptr(out_i, i64p), None) < 0
    assert lib.tehmm_posterior_argmax(0, 2, ptr(post, f64p), ptr(out_i, i64p), None) == 0       # nothing to do


def test_without_a_device_an_error_not_a_crash(lib):
    from tehmm_amd import _lib
    from tehmm_amd._lib import f64p, i64p, ptr
    post = np.random.RandomState(0).rand(5, 300)
    states = np.zeros(5, dtype=np.int64)
    for N in (7, 300):
        p = np.ascontiguousarray(post[:, :N])
        rc = lib.tehmm_posterior_argmax(5, N, ptr(p, f64p), ptr(states, i64p), None)
        if _lib.device_count() > 0:                      # (on a GPU machine the same calls simply work)
            assert rc == 0
            assert_array_equal(states, np.argmax(p, axis=1))
        else:
            assert rc == ERR_HIP
    if _lib.device_count() > 0:
        return
    # no batch can exist without a device, so the batch calls are reached with no handle only
    h = ctypes.c_void_p()
    offs = np.asarray([0, 5], dtype=np.int64)
    obs = np.zeros((5, 2), dtype=np.uint8)
    rc = lib.tehmm_batch_create(1, ptr(offs, i64p), 2, obs.ctypes.data_as(ctypes.c_void_p), None, 0, ctypes.byref(h))
    assert rc == ERR_HIP and not h.value
    assert lib.tehmm_batch_map_decode(h, None, None) == ERR_ARG


# ------------------------------------------------------------------ ShardedEvaluator under two gloo ranks
LENS = [300, 1, 120, 77, 510, 64, 33]


def _stub_compute(tables):
    """What MultitrackHmm._eval_tables(..., map_decode=True) returns, from a deterministic stand-in posterior."""
    out = {"forward_logprob": [], "map_paths": [], "map_logprob": []}
    for t in tables:
        rs = np.random.RandomState(len(t))
        post = rs.dirichlet(np.ones(9), size=len(t))
        out["forward_logprob"].append(-float(len(t)))
        out["map_paths"].append(np.argmax(post, axis=1))
        out["map_logprob"].append(np.max(post, axis=1).sum())
    return out


def _tables():
    return [np.full((L, 2), i, dtype=np.uint8) for i, L in enumerate(LENS)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tehmm_amd.dist import ShardedEvaluator
        mine, res = ShardedEvaluator(_stub_compute).run(_tables())
        q.put((rank, list(mine), res))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world2_gathers_map_paths_and_logprob():
    import torch.multiprocessing as mp
    from tehmm_amd.dist import ShardedEvaluator
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    mine, single = ShardedEvaluator(_stub_compute).run(_tables())        # no process group: one shard holds all
    assert list(mine) == list(range(len(LENS)))
    shards = sorted(got, key=lambda g: g[0])
    assert sorted(shards[0][1] + shards[1][1]) == list(range(len(LENS)))
    assert shards[0][1] and shards[1][1]
    for rank, _, res in shards:
        assert set(res) == {"forward_logprob", "map_paths", "map_logprob"}
        assert_array_equal(res["map_logprob"], np.asarray(single["map_logprob"]))
        assert_array_equal(res["forward_logprob"], np.asarray(single["forward_logprob"]))
        assert len(res["map_paths"]) == len(LENS)
        for i in range(len(LENS)):
            assert res["map_paths"][i].dtype == np.int64
            assert_array_equal(res["map_paths"][i], single["map_paths"][i])


# ------------------------------------------------------------------ tables that cannot fuse keep the host path
def test_decode_of_unfusable_table_is_basehmm_decode_map(monkeypatch):
    """A symbol above 255 keeps a table off the fused path: MultitrackHmm.decode of a "map" model must hand it to
    BaseHMM.decode -> _decode_map unchanged (the array-level calls under it are replaced by NumPy stand-ins: no GPU)."""
    from tehmm_amd import hmm as hmm_mod
    from tehmm_amd.basehmm import BaseHMM
    from tehmm_amd.emission import IndependentMultinomialEmissionModel
    from tehmm_amd.hmm import MultitrackHmm
    N, T = 4, 50
    em = IndependentMultinomialEmissionModel(N, [300, 3])
    h = MultitrackHmm(em, algorithm="map")
    rs = np.random.RandomState(2)
    obs = np.stack([rs.randint(0, 301, size=T), rs.randint(0, 4, size=T)], axis=1).astype(np.uint16)
    obs[7, 0] = 300
    monkeypatch.setattr(hmm_mod.MultitrackHmm, "_device_model",
                        lambda self: pytest.fail("an unfusable table reached the device path"))
    assert not h._can_fuse([obs])
    post = rs.dirichlet(np.ones(N), size=T)
    seen = []

    def fake_score_samples(self, o):
        assert o is obs
        seen.append("score_samples")
        return -12.5, post
    monkeypatch.setattr(BaseHMM, "score_samples", fake_score_samples)
    want = BaseHMM._decode_map(h, obs)
    for got in (h.decode(obs), h.decode(obs, algorithm="viterbi"), h._map_decode_tables([obs])[0]):
        assert got[0] == want[0] == np.max(post, axis=1).sum()
        assert_array_equal(got[1], np.argmax(post, axis=1))
    assert seen == ["score_samples"] * 4
    res = h._eval_tables([obs], viterbi=False, posterior=False, map_decode=True)
    assert res["map_logprob"][0] == want[0] and res["forward_logprob"] == [-12.5] and res["posteriors"] == []
    assert_array_equal(res["map_paths"][0], want[1])
