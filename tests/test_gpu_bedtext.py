"""The per-row BED text formatted on the device (tehmm_bed_text_write, tehmm_batch_bed_text_write).

Yardstick: the file that tehmm_bed_coords + tehmm_write_bed (output.bedCoords, output._write, output.statesToBed)
produce for the same inputs table by table, compared byte for byte.  Stripes of 512 items (rows and table headers)
end inside tables and, after two tables of 255 rows, exactly at a table boundary."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ERR_ARG = -1
STRIPE = 512


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib, build
    build.build()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


class Tab(object):
    """What output.bedCoords and output.writeBedText read of a TrackTable."""

    def __init__(self, chrom, start, rows, seg=None, mask=None):
        self.chrom, self.start, self.rows = chrom, int(start), int(rows)
        self.seg = None if seg is None else np.asarray(seg, dtype=np.int64)
        self.mask = None if mask is None else np.asarray(mask, dtype=np.int32)
        self.end = self.start + self.rows
        if seg is not None:
            self.end = self.start + int(self.seg[-1]) + 3 if rows else self.start       # the last segment: 3 bases

    def __len__(self):
        return self.rows

    def getChrom(self):
        return self.chrom

    def getStart(self):
        return self.start

    def getEnd(self):
        return self.end

    def getSegmentOffsets(self):
        return self.seg

    def getMaskRunningOffsets(self):
        return self.mask


def seg_offsets(rs, rows, first=0):
    """offsets of segments with lengths 1 to 100"""
    lens = rs.randint(1, 101, size=rows)
    lens[:min(rows, 100)] = np.arange(1, min(rows, 100) + 1)
    return first + np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)


def mask_block(rs, n):
    """running count of cut bases before every kept position"""
    return np.cumsum(rs.choice([0, 0, 0, 1, 17, 1000], size=n)).astype(np.int32)


def reference(path, tables, column, names=None, values=False, headers=None, shift=False):
    from tehmm_amd import output
    open(path, "w").close()
    r0 = 0
    for t, tab in enumerate(tables):
        n = len(tab)
        if headers is not None and headers[t] is not None:
            with open(path, "a") as f:
                f.write(headers[t])
        col = np.asarray(column[r0:r0 + n])
        r0 += n
        if n == 0:
            continue
        starts, ends = output.bedCoords(tab)
        if values:
            output._write(path, True, tab.getChrom(), starts, ends, values=np.roll(col, 1) if shift else col)
        else:
            output._write(path, True, tab.getChrom(), starts, ends, states=col, names=names)
    assert r0 == len(column)


def read(path):
    with open(path, "rb") as f:
        return f.read()


def check(tmp_path, tables, column, tag="x", stripe=STRIPE, **kw):
    """writes both files, compares them and the counters; returns (rows, bytes, host_rows)"""
    from tehmm_amd import output
    want, got = str(tmp_path / (tag + "_want.bed")), str(tmp_path / (tag + "_got.bed"))
    reference(want, tables, column, **kw)
    values = kw.pop("values", False)
    output.writeBedText(got, tables, states=None if values else column, values=column if values else None,
                        stripeRows=stripe, **kw)
    a, b = read(want), read(got)
    if a != b:
        la, lb = a.split(b"\n"), b.split(b"\n")
        bad = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
        pytest.fail("line %d differs: want %r got %r (%d / %d lines)" % (
            bad, la[bad:bad + 1], lb[bad:bad + 1], len(la), len(lb)))
    rows, nbytes, host = output.lastBedTextCounters()
    assert rows == len(column) and nbytes == os.path.getsize(got) == len(a)
    return rows, nbytes, host


NAME_LENS = (0, 1, 7, 40)


def make_names(n):
    return [("s%d" % i + "x" * 40)[:NAME_LENS[i % 4]] for i in range(n)]


@pytest.mark.parametrize("with_headers", [False, True])
@pytest.mark.parametrize("stripe", [STRIPE, 0])
def test_rows_tables_and_stripes(tmp_path, with_headers, stripe):
    rs = np.random.RandomState(1)
    rows = [255, 255, 1, 0, 256, 257, 2049, 1]
    tables = [Tab("chr%d" % (t % 3 + 1), 1000 * t, n) for t, n in enumerate(rows)]
    names = make_names(35)
    col = rs.randint(0, 35, size=sum(rows))
    headers = None
    if with_headers:
        headers = ["#Viterbi Score: %f\n" % (-1234.5 * t) if t % 3 != 2 else None for t in range(len(rows))]
        headers[3] = "# the empty table\n"
    check(tmp_path, tables, col, names=names, headers=headers, stripe=stripe)
    check(tmp_path, tables[2:3], col[:1], names=names, headers=None if headers is None else headers[:1], tag="one")
    check(tmp_path, [], col[:0], tag="none")


def test_append_keeps_the_file(tmp_path):
    from tehmm_amd import output
    path = str(tmp_path / "a.bed")
    with open(path, "w") as f:
        f.write("before\n")
    output.writeBedText(path, [Tab("c", 0, 3)], states=[0, 1, 2], append=True)
    assert read(path) == b"before\nc\t0\t1\t0\nc\t1\t2\t1\nc\t2\t3\t2\n"
    output.writeBedText(path, [Tab("c", 0, 1)], states=[7])
    assert read(path) == b"c\t0\t1\t7\n"


def test_coordinates(tmp_path):
    rs = np.random.RandomState(2)
    tables = [
        Tab("chr1", 5, 12),                                           # 9 -> 10
        Tab("chr1", 93, 12),                                          # 99 -> 100
        Tab("chr1", 999999990, 24),                                   # 999 999 999 -> 1 000 000 000
        Tab("chrBig", 2 ** 32 + 7, 300),
        Tab("chr2", 0, 700, seg=seg_offsets(rs, 700)),
        Tab("chr2", 40000, 300, seg=seg_offsets(rs, 300, first=12)),  # offsets that do not start at 0
        Tab("chr3", 100, 600, mask=mask_block(rs, 600)),
    ]
    seg = seg_offsets(rs, 513)
    tables.append(Tab("chr4", 7, 513, seg=seg, mask=mask_block(rs, int(seg[-1]) + 1)))
    tables.append(Tab("chr4", 2 ** 33, 2, seg=[0, 99], mask=np.arange(100, dtype=np.int32) * 3))
    col = rs.choice([0, 9, 10, 255, 1023], size=sum(len(t) for t in tables))
    check(tmp_path, tables, col)
    check(tmp_path, tables, col, stripe=0, tag="whole")


@pytest.mark.parametrize("n_states", [3, 35, 1024])
def test_names(tmp_path, n_states):
    rs = np.random.RandomState(n_states)
    names = make_names(n_states)
    tables = [Tab("chr1", 10, 700), Tab("c", 0, 1), Tab("chr2", 50, 900)]
    col = rs.randint(0, n_states, size=1601)
    col[:n_states if n_states < 700 else 700] = np.arange(n_states)[:700]
    col[-1] = n_states - 1
    check(tmp_path, tables, col, names=names)


def test_state_without_a_name_leaves_the_file(tmp_path):
    from tehmm_amd import _lib, output
    path = str(tmp_path / "kept.bed")
    with open(path, "w") as f:
        f.write("kept\n")
    col = np.zeros(3000, dtype=np.int64)
    for bad, where in ((5, 2999), (-1, 0), (5, 1700)):
        col[:] = 0
        col[where] = bad
        for append in (False, True):
            with pytest.raises(_lib.TeHmmHipError) as e:
                output.writeBedText(path, [Tab("chr1", 0, 3000)], states=col, names=make_names(5), append=append,
                                    stripeRows=STRIPE)
            assert e.value.code == ERR_ARG
            assert read(path) == b"kept\n"


def curated():
    vals = [1.0, 0.5, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-4, 9.9999999999949e-05, 99999.9999999995,
            999999999999.5, 1e12, 1.0 - 2.0 ** -53, 5e-324, 1.7e308]
    for m in (1, 3, 5, 625, 15625):
        for e in range(-60, 40):
            vals.append(m * 2.0 ** e)
    return np.asarray(vals, dtype=np.float64)


@pytest.mark.parametrize("shift", [False, True])
def test_values(tmp_path, shift):
    rs = np.random.RandomState(3)
    cur = curated()
    uni = rs.random_sample(20000)
    logu = 10.0 ** rs.uniform(-260, 260, 20000) * rs.choice([-1.0, 1.0], 20000)
    # the curated list: true ties of the 12th digit go to the host
    n = len(cur)
    tables = [Tab("chr1", 0, 100), Tab("chr2", 7, n - 100)]
    _, _, host = check(tmp_path, tables, cur, values=True, shift=shift, tag="cur")
    assert 1 <= host < n
    # the uniform block runs on the device
    tables = [Tab("chr1", 0, 7000), Tab("chr2", 99, 1), Tab("chrX", 123456, 12999)]
    _, _, host = check(tmp_path, tables, uni, values=True, shift=shift, tag="uni")
    assert host <= len(uni) // 100
    check(tmp_path, tables, logu, values=True, shift=shift, tag="log")
    check(tmp_path, tables, np.concatenate([cur, uni])[:20000], values=True, shift=shift, stripe=0, tag="mixed")


# ---- the batch form --------------------------------------------------------------------------------------------------
LENS = [300, 1024, 2500]


@pytest.fixture(scope="module")
def batch_case():
    """N -> model, batch (evaluated: Viterbi, posteriors, maximum-posterior states), offsets, tables, observations;
    made once per shape, closed when the module is done"""
    cases = {}
    yield lambda N: cases[N] if N in cases else cases.setdefault(N, _make_case(N))
    for hm, hb, _, _, _ in cases.values():
        hb.close()
        hm.close()


def _make_case(N):
    from tehmm_amd import synth
    from tehmm_amd.engine import HipBatch, HipModel
    sym = (3, 4, 2) if N == 5 else synth.CONFIG2_SYMBOLS
    model = synth.make_model(N, sym, gaussian_tracks=() if N == 5 else synth.CONFIG2_GAUSSIAN, seed=N)
    lp = model.log_probs.copy()
    lp[0, N - 1, 1] = -1e100                                        # a log-zero cell: state N - 1 cannot emit symbol 1
    offs = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    obs = synth.sample_obs(model, int(offs[-1]), seed=N + 1, missing=0.02)
    hm = HipModel(model.log_transmat, model.log_startprob, lp, symbols_per_track=model.symbols_per_track)
    hb = HipBatch(obs, offs)
    hm.eval(hb, viterbi=True, posterior=True, use_ratios=False, map_decode=True)
    rs = np.random.RandomState(N)
    tables = [Tab("chr1", 100, LENS[0]), Tab("chr1", 999999000, LENS[1], seg=seg_offsets(rs, LENS[1])),
              Tab("chr2", 0, LENS[2], mask=mask_block(rs, LENS[2]))]
    return hm, hb, offs, tables, obs


def assemble(path, tables, offs, states=None, names=None, pd=None, ed=None, headers=None):
    from tehmm_amd import output
    open(path, "w").close()
    for t, tab in enumerate(tables):
        a, b = offs[t], offs[t + 1]
        if headers is not None:
            with open(path, "a") as f:
                f.write(headers[t])
        if states is not None:
            output.statesToBed(tab, states[a:b], path, stateNames=names)
        if pd is not None:
            output.statesToBed(tab, None, posteriorSums=pd[a:b], posteriorsPath=path)
        if ed is not None:
            output.statesToBed(tab, None, emissionSums=ed[a:b], emissionsPath=path)


@pytest.mark.parametrize("N", [5, 35])
def test_batch_states_files(tmp_path, batch_case, N):
    from tehmm_amd import output
    hm, hb, offs, tables, _ = batch_case(N)
    names = make_names(N)
    headers = ["#Viterbi Score: %f\n" % (-100.25 * (t + 1)) for t in range(3)]
    want, got = str(tmp_path / "want.bed"), str(tmp_path / "got.bed")
    for src, states in ((output.SRC_VITERBI, hb.paths()), (output.SRC_MAP, hb.map_paths())):
        for nm in (names, None):
            assemble(want, tables, offs, states=states, names=nm, headers=headers)
            output.writeBatchBed(got, hb, src, tables, names=nm, headers=headers, stripeRows=STRIPE)
            assert read(got) == read(want)
            assert output.lastBedTextCounters()[:2] == (int(offs[-1]), os.path.getsize(got))
    assert not np.array_equal(hb.paths(), hb.map_paths())
    # a run of tables that does not start at the batch's first interval, appended
    assemble(want, tables[1:], offs[1:], states=hb.paths(), names=names)
    open(got, "w").close()
    output.writeBatchBed(got, hb, output.SRC_VITERBI, tables[1:], interval0=1, names=names, append=True)
    assert read(got) == read(want)


@pytest.mark.parametrize("N", [5, 35])
def test_batch_value_files(tmp_path, batch_case, N):
    from tehmm_amd import output
    hm, hb, offs, tables, obs = batch_case(N)
    want, got = str(tmp_path / "want.bed"), str(tmp_path / "got.bed")
    mask = np.zeros(N)
    mask[[1, N - 2]] = 1.0                                          # a two-state mask
    assemble(want, tables, offs, pd=hb.posterior_masksum(mask))
    output.writeBatchBed(got, hb, output.SRC_POSTERIOR, tables, mask=mask, stripeRows=STRIPE)
    assert read(got) == read(want)
    only = np.zeros(N)
    only[N - 1] = 1.0                                               # the state with the log-zero cell
    ed = hb.emission_masksum(hm, only)
    assert np.isneginf(ed).sum() == int((obs[:, 0] == 1).sum()) > 0
    assemble(want, tables, offs, ed=ed)
    output.writeBatchBed(got, hb, output.SRC_EMISSION, tables, model=hm, mask=only, stripeRows=STRIPE)
    assert read(got) == read(want)
    assert b"\t-inf\n" in read(got)
    assert output.lastBedTextCounters()[1] == os.path.getsize(got)


def test_batch_sources_need_their_evaluation(tmp_path):
    from tehmm_amd import _lib, output, synth
    from tehmm_amd.engine import HipBatch, HipModel
    model = synth.make_model(5, (3, 4, 2), gaussian_tracks=(), seed=9)
    obs = synth.sample_obs(model, 400, seed=1)
    hm = HipModel(model.log_transmat, model.log_startprob, model.log_probs, symbols_per_track=model.symbols_per_track)
    hb = HipBatch(obs, np.asarray([0, 400], dtype=np.int64))
    path = str(tmp_path / "none.bed")
    tables = [Tab("chr1", 0, 400)]
    for src in (output.SRC_VITERBI, output.SRC_MAP, output.SRC_POSTERIOR):
        with pytest.raises(_lib.TeHmmHipError) as e:
            output.writeBatchBed(path, hb, src, tables, mask=np.ones(5))
        assert e.value.code == ERR_ARG
        assert not os.path.exists(path)
    # the emission column needs no evaluation
    output.writeBatchBed(path, hb, output.SRC_EMISSION, tables, model=hm, mask=np.ones(5))
    want = str(tmp_path / "want.bed")
    assemble(want, tables, [0, 400], ed=hb.emission_masksum(hm, np.ones(5)))
    assert read(path) == read(want)
    hb.close()
