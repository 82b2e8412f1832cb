"""The emission column of teHmmEval --ed, the parts that need no GPU: the C ABI's symbols and argument checks, the
emission file of output.statesToBed (one-row shift with wrap-around, -inf text), getPosteriorsMask, the multi-rank
gather of the new result key (two gloo ranks, a stub compute) and the array-level path of tables that cannot fuse."""
import math
import os
import socket

import numpy as np
import pytest
from numpy.testing import assert_array_equal

NEW_SYMBOLS = ("tehmm_batch_emission_masksum", "tehmm_batch_get_emissions")
ERR_ARG = -1


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


def test_null_handles_are_argument_errors(lib):
    from tehmm_amd._lib import f64p, ptr
    out = np.zeros(4)
    mask = np.ones(2)
    assert lib.tehmm_batch_emission_masksum(None, None, 0, ptr(mask, f64p), 0, 1, ptr(out, f64p)) == ERR_ARG
    assert b"tehmm_batch_emission_masksum" in lib.tehmm_last_error()
    assert lib.tehmm_batch_get_emissions(None, None, 0, 0, 1, ptr(out, f64p)) == ERR_ARG
    assert b"tehmm_batch_get_emissions" in lib.tehmm_last_error()


# ------------------------------------------------------------------ statesToBed(emissionsPath=...)
def _py2_float(x):
    """str() of a float64 under Python 2: 12 significant digits, ".0" for integral values, inf / nan as words."""
    s = "%.12g" % x
    return s if any(c in s for c in ".en") else s + ".0"


def _reference_lines(chrom, start, end, seg_offsets, mask_offsets, values_per_row, fmt):
    """teHmmEval.py:251-275 restated: the coordinates of every row and the 4th column taken from row i - 1."""
    n = len(seg_offsets)
    lines, seg_dist = [], 0
    for i in range(n):
        cur_start = start + seg_dist
        int_len = (end - (start + seg_offsets[-1])) if i == n - 1 else seg_offsets[i + 1] - seg_offsets[i]
        seg_dist += int_len
        if mask_offsets is not None:
            cur_start += mask_offsets[cur_start - start]
        cur_end = cur_start + int_len
        lines.append("%s\t%d\t%d\t%s\n" % (chrom, cur_start, cur_end, fmt(values_per_row(i - 1))))
    return "".join(lines)


class _Table(object):
    """What statesToBed asks of a segmented, masked TrackTable."""

    def __init__(self, chrom, start, end, seg_offsets, mask_offsets):
        self.chrom, self.start, self.end = chrom, start, end
        self.seg, self.mo = np.asarray(seg_offsets, dtype=np.int64), np.asarray(mask_offsets, dtype=np.int32)

    def __len__(self):
        return len(self.seg)

    def getChrom(self):
        return self.chrom

    def getStart(self):
        return self.start

    def getEnd(self):
        return self.end

    def getSegmentOffsets(self):
        return self.seg

    def getMaskRunningOffsets(self):
        return self.mo


def test_states_to_bed_emission_file(tmp_path, monkeypatch):
    from tehmm_amd import output
    rs = np.random.RandomState(5)
    N, start, end = 4, 1000, 1060
    seg = [0, 3, 4, 10, 25, 26, 40]
    mo = np.cumsum(rs.rand(end - start) < 0.2).astype(np.int32) * 3          # bases cut out before each position
    tab = _Table("chrE", start, end, seg, mo)
    n = len(seg)
    em = -5.0 * rs.rand(n, N)
    em[2] = [-1e100, -1e100, -1.0, -2.0]
    em[n - 1] = [-1e100, -3.0, -1e100, -0.5]          # the LAST row lands on the first line (wrap-around)
    em[4] = 0.0                                        # a Q9-zeroed frame: log(2) under this mask
    mask = np.asarray([1, 0, 1, 0], dtype=np.int8)
    with np.errstate(divide="ignore"):
        col = np.log(np.sum(np.exp(em) * mask, axis=1))
    assert np.isneginf(col[n - 1]) and np.isfinite(col[2]) and col[4] == math.log(2.0)

    def coords(t):                                     # tehmm_bed_coords is a device call: NumPy stand-in
        s = np.zeros(n, dtype=np.int64)
        e = np.zeros(n, dtype=np.int64)
        d = 0
        for i in range(n):
            length = (end - (start + seg[-1])) if i == n - 1 else seg[i + 1] - seg[i]
            s[i] = start + d + mo[d]
            e[i] = s[i] + length
            d += length
        return s, e
    monkeypatch.setattr(output, "bedCoords", coords)
    states = rs.randint(0, N, size=n)
    bed, pd, ed = tmp_path / "s.bed", tmp_path / "pd.bed", tmp_path / "ed.bed"
    psum = rs.rand(n)
    output.statesToBed(tab, states, str(bed), psum, str(pd), append=False, emissionSums=col, emissionsPath=str(ed))

    def plain_python(i):                               # teHmmEval.py:273-275 on row i
        with np.errstate(divide="ignore"):
            return np.log(np.sum(np.exp(em[i]) * mask))
    want = _reference_lines("chrE", start, end, seg, mo, plain_python, _py2_float)
    assert ed.read_text() == want
    lines = want.split("\n")
    assert lines[0].endswith("\t-inf") and lines[5].split("\t")[3] == _py2_float(math.log(2.0))
    assert pd.read_text() == _reference_lines("chrE", start, end, seg, mo, lambda i: psum[i], _py2_float)
    assert len(bed.read_text().strip().split("\n")) == n
    # appending, and no emission file unless both arguments are given
    output.statesToBed(tab, states, emissionSums=col, emissionsPath=str(ed))
    assert ed.read_text() == want + want
    output.statesToBed(tab, states, emissionSums=col)
    output.statesToBed(tab, states, emissionsPath=str(tmp_path / "none.bed"))
    assert not (tmp_path / "none.bed").exists()


def test_inf_text_of_the_native_writer(tmp_path):
    from tehmm_amd import output
    p = tmp_path / "v.bed"
    s = np.asarray([0, 1, 2, 3], dtype=np.int64)
    output._write(str(p), False, "c", s, s + 1, values=[-np.inf, np.inf, -0.0, -745.2])
    assert [ln.split("\t")[3] for ln in p.read_text().strip().split("\n")] == ["-inf", "inf", "-0.0", "-745.2"]


# ------------------------------------------------------------------ getPosteriorsMask
class _Model(object):
    def __init__(self, n, state_map):
        self.n, self.state_map = n, state_map

    def getStateNameMap(self):
        return self.state_map

    def getEmissionModel(self):
        return self

    def getNumStates(self):
        return self.n


def test_get_posteriors_mask():
    from tehmm_amd.output import getPosteriorsMask
    from tehmm_amd.track import CategoryMap
    m = getPosteriorsMask("0,3", _Model(5, None))
    assert m.dtype == np.int8
    assert_array_equal(m, [1, 0, 0, 1, 0])
    assert_array_equal(getPosteriorsMask("4,9,x", _Model(5, None)), [0, 0, 0, 0, 1])     # unknown names are left out
    names = CategoryMap(reserved=0)
    for s in ("Outside", "LTR", "TSD"):
        names.update(s)
    assert_array_equal(getPosteriorsMask("TSD,Outside", _Model(3, names)), [1, 0, 1])
    assert_array_equal(getPosteriorsMask("LTR,nope", _Model(3, names)), [0, 1, 0])


# ------------------------------------------------------------------ ShardedEvaluator under two gloo ranks
LENS = [300, 1, 120, 77, 510, 64, 33]


def _stub_compute(tables):
    """What a compute callback built on MultitrackHmm.emissionColumn returns, from a deterministic stand-in."""
    out = {"emission_masksum": []}
    for t in tables:
        col = -np.random.RandomState(len(t)).rand(len(t)) * 50.0
        col[::7] = -np.inf
        out["emission_masksum"].append(col)
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
def test_world2_gathers_emission_masksum():
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
        assert set(res) == {"emission_masksum"}
        assert len(res["emission_masksum"]) == len(LENS)
        for i, L in enumerate(LENS):
            col = res["emission_masksum"][i]
            assert col.shape == (L,) and col.dtype == np.float64
            assert_array_equal(col, single["emission_masksum"][i])       # -inf rows included


# ------------------------------------------------------------------ tables that cannot fuse keep the array-level path
def test_unfusable_table_keeps_the_array_level_path(monkeypatch):
    """A symbol above 255 keeps a table off the batch path: emissionDistribution and emissionColumn must hand it to
    allLogProbs table by table (the array-level call under it is replaced by a NumPy stand-in: no GPU)."""
    from tehmm_amd import emission as emission_mod
    from tehmm_amd import hmm as hmm_mod
    from tehmm_amd.emission import IndependentMultinomialEmissionModel
    from tehmm_amd.hmm import MultitrackHmm
    N, T = 4, 50
    em = IndependentMultinomialEmissionModel(N, [300, 3], randomize=True, random_state=np.random.RandomState(1))
    h = MultitrackHmm(em)
    rs = np.random.RandomState(2)
    big = np.stack([rs.randint(0, 301, size=T), rs.randint(0, 4, size=T)], axis=1).astype(np.uint16)
    big[7, 0] = 300
    small = np.stack([rs.randint(0, 200, size=9), rs.randint(0, 4, size=9)], axis=1).astype(np.uint16)
    monkeypatch.setattr(hmm_mod.MultitrackHmm, "_device_model",
                        lambda self: pytest.fail("an unfusable table list reached the device path"))
    seen = []

    def fake_fast(obs, logProbs, out, normalize, segRatios):
        assert segRatios is None
        seen.append(len(obs))
        for k in range(obs.shape[1]):
            out += logProbs[k][:, obs[:, k]].T
        out *= normalize
    monkeypatch.setattr(emission_mod, "fastAllLogProbs", fake_fast)

    class _Tables(object):
        def getTrackTableList(self):
            return [big, small]
    assert not h._can_fuse([big, small])
    frames = h.emissionDistribution(_Tables())
    assert seen == [T, 9]
    for obs, f in zip((big, small), frames):
        want = em.logProbs[0][:, obs[:, 0]].T + em.logProbs[1][:, obs[:, 1]].T
        np.testing.assert_allclose(f, want, rtol=1e-15)
    mask = np.asarray([0.0, 1.0, 1.0, 0.0])
    cols = h.emissionColumn(_Tables(), mask)
    assert seen == [T, 9, T, 9]
    for f, c in zip(frames, cols):
        assert_array_equal(c, np.log(np.sum(np.exp(f) * mask, axis=1)))
