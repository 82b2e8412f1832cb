"""GPU tests of track loading (tehmm_load_tracks_u8, tehmm_amd/trackIO.py, TrackData.loadTrackData): everything is
compared for exact equality with the plain-Python statement (tests/trackio_ref.py) and with what the real reference
returned (tests/golden/trackio.npz)."""
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import trackio_ref as tr
from test_trackio_cpu import CASES, ERR_ARG, assert_equals_fixture

pytestmark = pytest.mark.gpu

_want = {}


def want_of(case):
    """the restatement's answer, computed once per case"""
    if case["name"] not in _want:
        _want[case["name"]] = tr.run_case(case)
    return _want[case["name"]]


@pytest.fixture(scope="module")
def trackIO():
    from tehmm_amd import trackIO
    return trackIO


@pytest.fixture(scope="module")
def tile(trackIO):
    return trackIO.tileRows()


def pairs(vmap):
    return sorted(([k, v] for k, v in vmap.fwd.items()), key=lambda kv: kv[1])


def make_track(t, name, path):
    from tehmm_amd.track import Track
    return Track.fromXMLElement(xml_element(t, name, path))


def xml_element(t, name, path):
    a = dict(name=name, path=path, distribution=t["dist"], valCol=str(t["valCol"]))
    for key in ("scale", "logScale", "shift", "default"):
        if t[key] is not None:
            a[key] = str(t[key])
    if t["delta"]:
        a["delta"] = "True"
    if t["caseSensitive"]:
        a["caseSensitive"] = "True"
    return ET.Element("track", a)


def write_load_case(case, tmp_path):
    root = ET.Element("teModelConfig")
    for name, text in case["files"].items():
        (tmp_path / name).write_text(text)
    for t in case["tracks"]:
        root.append(xml_element(t, t["name"], str(tmp_path / t["file"])))
    xml = str(tmp_path / "tracks.xml")
    ET.ElementTree(root).write(xml)
    return xml


def run_public(trackIO, case, tmp_path):
    """what trackio_ref.run_case makes, through the public functions"""
    from tehmm_amd.track import TrackData
    out = dict()
    if case["type"] in ("bed", "fasta"):
        path = str(tmp_path / ("x.bed" if case["type"] == "bed" else "x.fa"))
        open(path, "w").write(case["bed"] if case["type"] == "bed" else tr.fasta_text(case["records"]))
        track, fresh = make_track(case["track"], "t", path), make_track(case["track"], "t", path)
        for key, t, update in (("row", track, True), ("row_unlearned", fresh, False)):
            out[key] = trackIO.readTrackData(path, case["chrom"], case["start"], case["end"], valCol=t.getValCol(),
                                             valMap=t.getValueMap(), updateValMap=update, useDelta=t.getDelta(),
                                             caseSensitive=t.getCaseSensitive())
        vm = track.getValueMap()
        out["maps"], out["missing"], out["symbols"] = [pairs(vm)], [vm.getMissingVal()], [len(vm)]
        return out
    xml = write_load_case(case, tmp_path)
    learned = None
    for prefix, intervals, segments in (("a_", case["intervals"], None), ("b_", case["intervals2"], None),
                                        ("c_", case["intervals2"], case["segments"])):
        td = TrackData()
        td.loadTrackData(xml, [tuple(iv) for iv in intervals], trackList=learned, segmentIntervals=segments)
        if learned is None:
            learned = td.getTrackList()
        out[prefix + "n"] = td.getNumTrackTables()
        for x, tab in enumerate(td.getTrackTableList()):
            out["%stable%d" % (prefix, x)] = tab.getNumPyArray()
            out["%swhere%d" % (prefix, x)] = [tab.getChrom(), tab.getStart()]
            if tab.getSegmentOffsets() is not None:
                out["%soffsets%d" % (prefix, x)] = np.asarray(tab.getSegmentOffsets())
        maps = [t.getValueMap() for t in td.getTrackList()]
        out[prefix + "maps"] = [pairs(m) for m in maps]
        out[prefix + "missing"] = [m.getMissingVal() for m in maps]
        out[prefix + "symbols"] = td.getNumSymbolsPerTrack()
    return out


# ---- 1. the golden cases through the public functions -------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_public_functions_equal_the_reference(trackIO, case, tmp_path):
    got = run_public(trackIO, case, tmp_path)
    assert_equals_fixture(case["name"], got)
    want = want_of(case)
    assert set(got) == set(want)
    for key, val in want.items():
        if isinstance(val, np.ndarray):
            np.testing.assert_array_equal(got[key], val, err_msg=key)
        else:
            assert got[key] == val, key


def test_output_buffer_is_a_table_column(trackIO, tmp_path):
    from tehmm_amd.track import IntegerTrackTable
    case = CASES[0]
    path = str(tmp_path / "x.bed")
    open(path, "w").write(case["bed"])
    table = IntegerTrackTable(3, case["chrom"], case["start"], case["end"])
    track = make_track(case["track"], "t", path)
    back = trackIO.readBedData(path, case["chrom"], case["start"], case["end"], valCol=3, valMap=track.getValueMap(),
                               updateValMap=True, outputBuf=table.getRow(1))
    np.testing.assert_array_equal(table.getNumPyArray()[:, 1], want_of(case)["row"])
    assert np.shares_memory(back, table.getNumPyArray()) and not table.getNumPyArray()[:, [0, 2]].any()


# ---- 2. adversarial lists ---------------------------------------------------------------------------------------------------
def random_records(rng, T, n, long_share=0.1, max_len=6):
    s = np.sort(rng.randint(0, T, size=n))
    length = np.where(rng.rand(n) < long_share, rng.randint(1, T + 1, size=n), rng.randint(1, max_len + 1, size=n))
    return s, np.minimum(T, s + length), rng.randint(2, 250, size=n), rng.randint(2, 250, size=n)


def random_sequence(rng, T):
    b = rng.randint(ord("A"), ord("z") + 1, size=T).astype(np.uint8)
    b[rng.rand(T) < 0.1] = 0
    if T > 3:
        b[T - 1 - int(rng.randint(3)):] = 0                    # a sequence that ends before the table does
    lut = rng.randint(0, 256, size=256).astype(np.uint8)
    return b, lut


def check(trackIO, T, tracks):
    """tracks: ("records", fill, start, end, sym0, sym) or ("sequence", fill, bytes, lut)"""
    got = trackIO.paintTracks(T, [trackIO.RecordTrack(*t[1:]) if t[0] == "records" else trackIO.SequenceTrack(*t[1:])
                                  for t in tracks])
    assert got.shape == (T, len(tracks)) and got.dtype == np.uint8
    for k, t in enumerate(tracks):
        if t[0] == "records":
            want = tr.paint(T, *(t[1:] + ((), (), (), ())[:6 - len(t)]))
        else:
            want = np.where(t[2] == 0, t[1], t[3][t[2]])
        np.testing.assert_array_equal(got[:, k], want, err_msg="track %d" % k)
    return got


@pytest.mark.parametrize("K", [1, 3, 7, 12])
@pytest.mark.parametrize("rows", ["1", "tile-1", "tile", "3*tile+17"])
def test_shapes_across_the_tile(trackIO, tile, rows, K):
    T = eval(rows, dict(tile=tile))
    rng = np.random.RandomState(1000 * K + T)
    tracks = []
    for k in range(K):
        fill = int(rng.randint(0, 256))
        if k % 3 == 1:
            tracks.append(("sequence", fill) + random_sequence(rng, T))
        elif k % 3 == 2 and k % 2 == 0:
            tracks.append(("records", fill))                    # a track without records
        else:
            tracks.append(("records", fill) + random_records(rng, T, int(rng.randint(1, 2 * T + 2))))
    check(trackIO, T, tracks)


def test_full_span_record_before_five_thousand_short_ones(trackIO, tile):
    T = 20 * tile
    rng = np.random.RandomState(7)
    s = np.sort(rng.randint(0, T, size=5000))
    e = np.minimum(T, s + rng.randint(1, 3, size=5000))
    start, end = np.concatenate([[0], s]), np.concatenate([[T], e])
    assert len(start) > 64 * 64                                 # three levels: records, 64s, 4096s
    sym0, sym = rng.randint(3, 200, size=5001), rng.randint(3, 200, size=5001)
    sym0[0], sym[0] = 201, 202
    got = check(trackIO, T, [("records", 1, start, end, sym0, sym), ("records", 1, s, e, sym0[1:], sym[1:])])
    assert (got[:, 0] == 202).sum() > T // 8 and (got[:, 1] == 1).sum() == (got[:, 0] == 202).sum() + (got[0, 1] == 1)


def test_nested_staircase(trackIO, tile):
    depth = 200
    T = 2 * tile + 50
    assert T > 2 * depth
    start = np.arange(depth)
    end = T - np.arange(depth)
    sym0, sym = 2 + np.arange(depth) % 250, 3 + np.arange(depth) % 250
    got = check(trackIO, T, [("records", 0, start, end, sym0, sym), ("sequence", 4) + random_sequence(
        np.random.RandomState(3), T)])
    assert got[T - 1, 0] == sym[0] and got[T - depth, 0] == sym[depth - 1] and got[depth - 1, 0] == sym0[depth - 1]


def test_equal_starts_unit_records_abutting_and_the_last_row(trackIO, tile):
    T = tile + 5
    # five records on one start, the longest first; unit records; an abutting chain; a record ending on the last row
    start = [3, 3, 3, 3, 3, 10, 11, 12, 20, 25, 30, T - 4, T - 1]
    end = [9, 5, 4, 8, 4, 11, 12, 13, 25, 30, 31, T, T]
    sym0 = list(range(10, 10 + len(start)))
    sym = list(range(50, 50 + len(start)))
    got = check(trackIO, T, [("records", 1, start, end, sym0, sym)])
    assert got[3:9, 0].tolist() == [14, 53, 53, 53, 53, 50] and got[T - 1, 0] == 22 and got[T - 2, 0] == 61
    rng = np.random.RandomState(17)
    s = np.sort(rng.randint(0, 40, size=900)) * 7 % T           # many records per start
    s.sort()
    e = np.minimum(T, s + rng.randint(1, 30, size=900))
    check(trackIO, T, [("records", 0, s, e, rng.randint(1, 255, size=900), rng.randint(1, 255, size=900))])


def test_records_of_several_tables_in_one_call(trackIO, tmp_path):
    from tehmm_amd.track import CategoryMap
    text = "chr1\t5\t40\tA\nchr1\t38\t60\tB\nchr1\t50\t51\tC\nchr2\t0\t100\tD\nchr1\t0\t70\tE\n"
    path = tmp_path / "t.bed"
    path.write_text(text)
    tables = [("chr1", 10, 40), ("chr1", 40, 55), ("chr2", 90, 100), ("chr1", 0, 8)]      # a record ends at 40
    source = trackIO.TrackSource(str(path))
    col = trackIO.ColumnBuilder(CategoryMap(reserved=2), "t")
    vmap = tr.RefMap(reserved=2)
    want, offset = [], 0
    for c, s, e in tables:
        col.add(source, offset, c, s, e, valCol=3, updateValMap=True)
        want.append(tr.bed_row(text, c, s, e, tr.track_options(), vmap, True))
        offset += e - s
    got = trackIO.paintTracks(offset, [col.track(offset)])
    np.testing.assert_array_equal(got[:, 0], np.concatenate(want))
    assert col.valMap.fwd == vmap.fwd and got[29, 0] != got[30, 0]


# ---- 3. bad lists are an argument error, not a fault -----------------------------------------------------------------------
@pytest.mark.parametrize("what, start, end, offender", [
    ("unsorted", [0, 5, 4, 9, 8], [2, 6, 6, 10, 10], 2),
    ("end beyond T", [0, 5, 9], [2, 6, 101], 2),
    ("empty record", [0, 5, 9], [2, 5, 11], 1),
    ("negative start", [-1, 5, 9], [2, 6, 11], 0),
])
def test_bad_records_name_the_lowest_index(trackIO, what, start, end, offender):
    from tehmm_amd._lib import TeHmmHipError
    T = 100
    n = len(start)
    good = ("records", 1, [0, 50], [10, 60], [2, 2], [3, 3])
    with pytest.raises(TeHmmHipError) as err:
        check(trackIO, T, [good, ("records", 1, start, end, [2] * n, [3] * n)])
    assert err.value.code == ERR_ARG and "record %d " % (2 + offender) in str(err.value), what
    check(trackIO, T, [good, good])                             # the next valid call is served
    assert [name for name, _ in trackIO.lastTiming()] == ["upload", "tree", "paint", "download"]


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------
def test_loaded_tables_feed_the_hmm(trackIO, tmp_path):
    from tehmm_amd import synth
    from tehmm_amd.emission import IndependentMultinomialEmissionModel
    from tehmm_amd.hmm import MultitrackHmm
    from tehmm_amd.track import IntegerTrackTable, TrackData
    case = CASES[-1]
    assert case["type"] == "load"
    xml = write_load_case(case, tmp_path)
    intervals = [tuple(iv) for iv in case["intervals"]]
    td = TrackData()
    td.loadTrackData(xml, intervals)
    syms = td.getNumSymbolsPerTrack()
    model = synth.make_model(4, symbols_per_track=syms, gaussian_tracks=(), seed=2)

    def decode(trackData):
        em = IndependentMultinomialEmissionModel(model.n_states, syms)
        em.logProbs = model.log_probs.copy()
        h = MultitrackHmm(em)
        h.transmat_ = model.transmat.copy()
        h.startprob_ = np.exp(model.log_startprob)
        return h.viterbi(trackData)

    tables, _ = tr.load_tables(case["tracks"], case["files"], intervals)
    ref = []
    for tab in tables:
        t = IntegerTrackTable(len(syms), tab["chrom"], tab["start"], tab["start"] + len(tab["data"]))
        for k in range(len(syms)):
            t.writeRow(k, tab["data"][:, k])
        ref.append(t)
    out, ref_out = decode(td), decode(TrackData(ref, td.getTrackList()))
    assert len(out) == len(ref_out) == 3
    for (lp, path), (rlp, rpath), tab in zip(out, ref_out, tables):
        assert len(path) == len(tab["data"]) and np.array_equal(path, rpath) and lp == rlp
