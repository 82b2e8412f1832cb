"""CPU tests of track loading (tehmm_amd/trackIO.py, the additions of tehmm_amd/track.py, tests/trackio_ref.py): the
restatement against what the real reference returned (tests/golden/trackio.npz), the host halves against expectations
written by hand, and the argument errors of tehmm_load_tracks_u8, which are answered before any device call."""
import ctypes
import json
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import trackio_ref as tr
from conftest import load_golden

ERR_ARG = -1
CASES = tr.golden_cases()
GOLDEN = load_golden("trackio")


def meta_of(name):
    return json.loads(bytes(GOLDEN[name + "__meta"]).decode())


def golden_arrays(name):
    return {k.split("__", 1)[1]: v for k, v in GOLDEN.items() if k.startswith(name + "__") and not k.endswith("__meta")}


def assert_equals_fixture(name, result):
    """result: what trackio_ref.run_case makes (arrays and JSON-able values), equal to the fixture key for key"""
    meta, arrays = meta_of(name), golden_arrays(name)
    assert set(result) == set(meta) | set(arrays)
    for key, val in result.items():
        if isinstance(val, np.ndarray):
            assert val.shape == arrays[key].shape, key
            np.testing.assert_array_equal(val, arrays[key], err_msg=key)
        else:
            assert json.loads(json.dumps(val)) == meta[key], key


# ---- the restatement and the fixture --------------------------------------------------------------------------------
def test_fixture_holds_the_seeded_cases():
    assert bytes(GOLDEN["cases"]).decode() == tr.cases_json(CASES)
    kinds = [c["type"] for c in CASES]
    assert kinds.count("bed") >= 8 and kinds.count("fasta") >= 3 and kinds.count("load") == 1


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_the_reference(case):
    assert_equals_fixture(case["name"], tr.run_case(case))


def test_cases_cover_what_they_are_meant_to():
    by = {c["name"]: c for c in CASES}
    m = meta_of("names_reserved2")
    assert m["missing"] == [1] and m["maps"][0][0][1] == 2                  # reserved 2: symbols from 2, missing 1
    m = meta_of("names_default")
    assert m["missing"] == [1] and m["maps"][0][0] == ["0", 1]              # reserved 1: the default is symbol 1
    assert any(float(k) < 0 for k, _ in meta_of("delta_scaled")["maps"][0])  # a delta below zero was binned
    assert set(np.unique(golden_arrays("binary")["row"])) == {1, 2}
    short = by["fasta_short"]
    assert short["end"] > len(dict(map(tuple, short["records"]))[short["chrom"]]) > short["start"]
    folded, cased = meta_of("fasta_folded")["maps"][0], meta_of("fasta_case")["maps"][0]
    assert all(k == k.upper() for k, _ in folded) and any(k != k.upper() for k, _ in cased)
    assert meta_of("load")["a_n"] == 3 and len(meta_of("load")["a_symbols"]) == 5
    b = golden_arrays("load")
    assert (b["b_table0"] == np.asarray(meta_of("load")["b_missing"])).any()
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "trackio.npz")) < 200 * 1024


def test_paint_by_search_equals_painting_in_order():
    rng = np.random.RandomState(5)
    for trial in range(300):
        T = int(rng.randint(1, 40))
        n = int(rng.randint(0, 12))
        s = np.sort(rng.randint(0, T, size=n))                              # equal starts included
        e = np.minimum(T, s + rng.randint(1, 1 + (T if trial % 3 == 0 else 6), size=n))
        a, b = rng.randint(2, 9, size=n), rng.randint(2, 9, size=n)
        np.testing.assert_array_equal(tr.paint(T, 1, s, e, a, b), tr.paint_by_search(T, 1, s, e, a, b))


# ---- BED text -----------------------------------------------------------------------------------------------------------
BED = ("# header\tline\tof\tfour\n"
       "chr1\t10\t20\tA\t1.5\n"
       "short\t7\n"
       "chr1\t5\t12\tB\t2\r\n"
       "chr2\t0\t9\tC\t3\n"
       "#chr1\t0\t1\tD\t4\n"
       "chr1\t18\t30\tA\t5")


@pytest.fixture()
def bed_path(tmp_path):
    p = tmp_path / "x.bed"
    p.write_bytes(BED.encode())
    return str(p)


def test_bed_read_skips_comments_and_short_lines_and_takes_crlf(bed_path):
    from tehmm_amd import trackIO
    assert trackIO.bedRead(bed_path) == [["chr1", "10", "20", "A", "1.5"], ["chr1", "5", "12", "B", "2"],
                                         ["chr2", "0", "9", "C", "3"], ["chr1", "18", "30", "A", "5"]]
    assert tr.bed_records(BED) == trackIO.bedRead(bed_path)


def test_read_bed_intervals_sort_and_range(bed_path):
    from tehmm_amd import trackIO
    assert trackIO.readBedIntervals(bed_path) == [("chr1", 10, 20), ("chr1", 5, 12), ("chr2", 0, 9), ("chr1", 18, 30)]
    assert trackIO.readBedIntervals(bed_path, ncol=4, sort=True) == [
        ("chr1", 5, 12, "B"), ("chr1", 10, 20, "A"), ("chr1", 18, 30, "A"), ("chr2", 0, 9, "C")]
    # a range clips; both records that start before it get its start, and keep file order
    assert trackIO.readBedIntervals(bed_path, ncol=5, chrom="chr1", start=11, end=19) == [
        ("chr1", 11, 19, "A", "1.5"), ("chr1", 11, 12, "B", "2"), ("chr1", 18, 19, "A", "5")]
    assert trackIO.readBedIntervals(bed_path, chrom="chr1", start=20, end=25) == [("chr1", 20, 25)]
    assert trackIO.readBedIntervals(bed_path, chrom="chr3", start=0, end=25) == []
    with pytest.raises(RuntimeError):
        trackIO.readBedIntervals(bed_path + ".none")


def test_bed_file_select_equals_the_rule(bed_path):
    from tehmm_amd import trackIO
    rng = np.random.RandomState(11)
    for c in CASES[:4]:
        p = os.path.join(os.path.dirname(bed_path), c["name"] + ".bed")
        open(p, "w").write(c["bed"])
        bed = trackIO.BedFile(p)
        recs = tr.bed_records(c["bed"])
        for _ in range(25):
            s = int(rng.randint(0, 400))
            e = s + int(rng.randint(1, 200))
            pick, a, b = bed.select(c["chrom"], s, e)
            want = tr.clip_sort(recs, c["chrom"], s, e)
            assert list(zip(a.tolist(), b.tolist())) == [(r[1], r[2]) for r in want]
            assert [bed.fields[i][3:] for i in pick.tolist()] == [r[3:] for r in want]


def test_merged_intervals(tmp_path):
    from tehmm_amd import trackIO
    p = tmp_path / "m.bed"
    p.write_text("chr1\t0\t10\nchr1\t5\t8\nchr1\t9\t15\nchr1\t15\t20\nchr1\t21\t22\nchr2\t3\t4\nchr2\t3\t9\n")
    # nested, overlapping and abutting intervals merge; a gap of one base does not
    assert trackIO.getMergedBedIntervals(str(p)) == [("chr1", 0, 20), ("chr1", 21, 22), ("chr2", 3, 9)]
    q = tmp_path / "u.bed"
    q.write_text("chr1\t30\t40\nchr1\t0\t10\nchr1\t8\t31\n")
    assert trackIO.getMergedBedIntervals(str(q), sort=True) == [("chr1", 0, 40)]
    with pytest.raises(ValueError):
        trackIO.getMergedBedIntervals(str(p), ncol=4)


# ---- symbols --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["names_reserved2", "names_default", "score_scale", "score_log_shift",
                                  "presence_valcol0"])
def test_vectorised_symbols_equal_the_per_record_loop(tmp_path, name):
    from tehmm_amd import trackIO
    from tehmm_amd.track import Track
    case = {c["name"]: c for c in CASES}[name]
    p = tmp_path / "x.bed"
    p.write_text(case["bed"])
    bed = trackIO.BedFile(str(p))
    t = case["track"]
    make = lambda: Track("t", 0, t["dist"], path=str(p), valCol=t["valCol"], scale=t["scale"], logScale=t["logScale"],
                         shift=t["shift"], defaultVal=t["default"])
    fast, slow = make(), make()
    for s, e in ((case["start"], case["end"]), (0, 50), (case["start"] + 17, case["end"] + 60)):
        pick, a, b = bed.select(case["chrom"], s, e)
        got = trackIO.recordSymbols(bed, pick, a, b, case["chrom"], t["valCol"], fast.getValueMap(), True, False, "t")
        want = trackIO.recordSymbolsLoop(bed, pick, a, b, case["chrom"], t["valCol"], slow.getValueMap(), True, False,
                                         "t")
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        assert fast.getValueMap().fwd == slow.getValueMap().fwd
    # and the loop is the restatement's
    vmap = tr.make_map(t)
    clipped = tr.clip_sort(tr.bed_records(case["bed"]), case["chrom"], case["start"], case["end"])
    again = make()
    pick, a, b = bed.select(case["chrom"], case["start"], case["end"])
    sym0, sym = trackIO.recordSymbols(bed, pick, a, b, case["chrom"], t["valCol"], again.getValueMap(), True, False, "t")
    assert list(zip(sym0.tolist(), sym.tolist())) == tr.record_symbols(clipped, t, vmap, True)
    assert again.getValueMap().fwd == vmap.fwd


def test_delta_symbols_equal_the_restatement(tmp_path):
    from tehmm_amd import trackIO
    from tehmm_amd.track import Track
    case = {c["name"]: c for c in CASES}["delta_scaled"]
    p = tmp_path / "x.bed"
    p.write_text(case["bed"])
    t = case["track"]
    track = Track("t", 0, path=str(p), valCol=4, scale=t["scale"], delta=True, defaultVal=t["default"])
    bed = trackIO.BedFile(str(p))
    pick, a, b = bed.select(case["chrom"], case["start"], case["end"])
    sym0, sym = trackIO.recordSymbols(bed, pick, a, b, case["chrom"], 4, track.getValueMap(), True, True, "t")
    vmap = tr.make_map(t)
    want = tr.record_symbols(tr.clip_sort(tr.bed_records(case["bed"]), case["chrom"], case["start"], case["end"]), t,
                             vmap, True)
    assert list(zip(sym0.tolist(), sym.tolist())) == want and track.getValueMap().fwd == vmap.fwd
    assert (sym0 != sym).any()


def test_a_symbol_above_255_names_the_track(tmp_path):
    from tehmm_amd import trackIO
    from tehmm_amd.track import CategoryMap
    p = tmp_path / "many.bed"
    p.write_text("".join("chr1\t%d\t%d\tname%d\n" % (i, i + 1, i) for i in range(300)))
    bed = trackIO.BedFile(str(p))
    pick, a, b = bed.select("chr1", 0, 300)
    with pytest.raises(ValueError, match="wide"):
        trackIO.recordSymbols(bed, pick, a, b, "chr1", 3, CategoryMap(reserved=2), True, False, "wide")


def test_fasta_lut_and_update_order():
    from tehmm_amd import trackIO
    from tehmm_amd.track import CategoryMap
    row = np.frombuffer(b"\0ggTacA\0", dtype=np.uint8)
    vm = CategoryMap(reserved=2)
    trackIO.fastaUpdate(row, vm, False, True)
    assert vm.fwd == {"G": 2, "T": 3, "A": 4, "C": 5}
    lut = trackIO.fastaLut(vm, False, "seq")
    assert [lut[ord(c)] for c in "gGtTaAcCnN"] == [2, 2, 3, 3, 4, 4, 5, 5, 1, 1] and lut[0] == 1
    vm = CategoryMap(reserved=2)
    trackIO.fastaUpdate(row, vm, True, True)
    assert vm.fwd == {"g": 2, "T": 3, "a": 4, "c": 5, "A": 6}
    assert trackIO.fastaLut(vm, True, "seq")[ord("G")] == 1
    assert trackIO.fastaBytes({"c": b"ACGT"}, "c", 2, 7).tolist() == [ord("G"), ord("T"), 0, 0, 0]
    assert trackIO.fastaBytes({"c": b"ACGT"}, "d", 0, 3).tolist() == [0, 0, 0]


# ---- Track, TrackList, the XML list ---------------------------------------------------------------------------------------
def element(**attrib):
    return ET.Element("track", {k: str(v) for k, v in attrib.items()})


def test_track_attributes_and_maps():
    from tehmm_amd.track import BinaryMap, CategoryMap, IdentityValueMap, Track
    t = Track("plain", 3)                                          # as before: no path, no reference map
    assert isinstance(t.getValueMap(), IdentityValueMap) and t.getDist() == "multinomial" and t.getNumber() == 3
    assert (t.getPath(), t.getValCol(), t.getScale(), t.getLogScale(), t.getShift(), t.getDelta(), t.getDefaultVal(),
            t.getCaseSensitive(), t.getPreprocess()) == (None, 3, None, None, None, False, None, False, None)
    t = Track.fromXMLElement(element(name="te", path="te.bed"))
    vm = t.getValueMap()
    assert isinstance(vm, CategoryMap) and vm.getReserved() == 2 and vm.getMissingVal() == 1 and len(vm) == 1
    t = Track.fromXMLElement(element(name="cov", path="c.bed", valCol=4, scale=0.5, shift=1, default=0, delta="True",
                                     caseSensitive="1", preprocess="rm", distribution="gaussian"))
    assert (t.getValCol(), t.getScale(), t.getShift(), t.getDelta(), t.getDefaultVal(), t.getCaseSensitive(),
            t.getPreprocess(), t.getDist()) == (4, 0.5, 1.0, True, "0", True, "rm", "gaussian")
    assert t.getValueMap().getReserved() == 1 and t.getValueMap().getMissingVal() == 1 and len(t.getValueMap()) == 1
    for dist in ("binary", "mask"):
        t = Track.fromXMLElement(element(name="b", path="b.bed", distribution=dist, valCol=4))
        assert isinstance(t.getValueMap(), BinaryMap) and t.getValCol() == 0
    bm = BinaryMap()
    assert (bm.getMap("x"), bm.getMap(None), bm.getMissingVal(), len(bm), bm.getMapBack(2)) == (2, 1, 1, 2, 1)


def test_track_errors():
    from tehmm_amd.track import Track
    with pytest.raises(RuntimeError, match="default"):
        Track.fromXMLElement(element(name="g", path="g.bed", distribution="gaussian"))
    with pytest.raises(RuntimeError, match="delta"):
        Track.fromXMLElement(element(name="d", path="d.bed", logScale=2, delta="true"))
    with pytest.raises(RuntimeError, match="shift"):
        Track.fromXMLElement(element(name="l", path="l.bed", logScale=2, default=0))
    Track.fromXMLElement(element(name="l", path="l.bed", logScale=2, default=0, shift=1))
    with pytest.raises(RuntimeError, match="preprocess"):
        Track.fromXMLElement(element(name="p", path="p.bed", preprocess="other"))
    with pytest.raises(ValueError):
        Track.fromXMLElement(element(name="u", path="u.bed", distribution="poisson"))
    with pytest.raises(KeyError):
        Track.fromXMLElement(element(name="nopath"))


def test_read_track_list(tmp_path):
    from tehmm_amd.track import readTrackList
    root = ET.Element("teModelConfig")
    for a in (dict(name="a", path="a.bed"), dict(name="m", path="m.bed", distribution="mask"),
              dict(name="b", path="b.fa", caseSensitive="true")):
        root.append(element(**a))
    p = str(tmp_path / "tracks.xml")
    ET.ElementTree(root).write(p)
    tl = readTrackList(p)
    assert [t.getName() for t in tl] == ["a", "b"] and [t.getNumber() for t in tl] == [0, 1]
    assert [t.getName() for t in tl.getMaskTracks()] == ["m"] and tl.getMaskTracks()[0].getNumber() == 0
    assert tl.getTrackByName("m") is None and tl.getTrackByName("m", isMask=True).getDist() == "mask"
    assert tl.getTrackByName("b").getCaseSensitive() and tl.getTrackByNumber(1).getName() == "b"
    tl = readTrackList(p, treatMaskAsBinary=True)
    assert [t.getName() for t in tl] == ["a", "m", "b"] and tl.getMaskTracks() == []
    root.append(element(name="al", path="x.maf", distribution="alignment"))
    ET.ElementTree(root).write(p)
    with pytest.raises(NotImplementedError):
        readTrackList(p)


def test_symbols_per_track_fall_back_to_the_maps():
    from tehmm_amd.track import CategoryMap, Track, TrackData, TrackList
    vm = CategoryMap(reserved=2)
    vm.getMap("x", update=True)
    td = TrackData([], TrackList([Track("a", 0, valueMap=vm), Track("b", 1, valueMap=CategoryMap(reserved=1))]))
    assert td.getNumSymbolsPerTrack() == [2, 0]
    assert TrackData([], None, [3, 4]).getNumSymbolsPerTrack() == [3, 4]
    assert TrackData([], TrackList([Track("a", 0)])).getNumSymbolsPerTrack() is None


def test_unoffered_formats(tmp_path):
    from tehmm_amd import trackIO
    from tehmm_amd.track import CategoryMap
    p = tmp_path / "x.bw"
    p.write_bytes(b"")
    with pytest.raises(RuntimeError, match="bigWig"):
        trackIO.readTrackData(str(p), "chr1", 0, 5, valMap=CategoryMap())
    with pytest.raises(RuntimeError, match="not found"):
        trackIO.readTrackData(str(tmp_path / "none.bed"), "chr1", 0, 5, valMap=CategoryMap())
    q = tmp_path / "x.txt"
    q.write_text("chr1\t0\t3\n")
    assert trackIO.readTrackData(str(q), "chr1", 0, 5, valMap=CategoryMap()) is None


# ---- the entry point's argument checks (no device is touched) -----------------------------------------------------------
def _load(lib, T=4, K=2, fill=(1, 1), kind=(0, 1), ro=(0, 1, 1), start=(0,), end=(2,), sym0=(2,), sym=(3,),
          so=(0, 0, 4), seq=b"ACGT", lut=None, null=()):
    from tehmm_amd._lib import i64p, ptr, u8p
    u8 = lambda x: np.ascontiguousarray(np.frombuffer(x, dtype=np.uint8) if isinstance(x, bytes) else x, dtype=np.uint8)
    i64 = lambda x: np.ascontiguousarray(x, dtype=np.int64)
    a = dict(fill=u8(fill), kind=u8(kind), ro=i64(ro), start=i64(start), end=i64(end), sym0=u8(sym0), sym=u8(sym),
             so=i64(so), seq=u8(seq), lut=u8(np.zeros(256) if lut is None else lut),
             data=np.zeros((max(T, 0), max(K, 1)), dtype=np.uint8))
    p = {k: None if k in null else ptr(v, i64p if v.dtype == np.int64 else u8p) for k, v in a.items()}
    return lib.tehmm_load_tracks_u8(T, K, p["fill"], p["kind"], p["ro"], p["start"], p["end"], p["sym0"], p["sym"],
                                    p["so"], p["seq"], p["lut"], p["data"])


@pytest.fixture(scope="module")
def lib():
    from tehmm_amd import _lib
    return _lib.load()


def test_symbols_and_argtypes_are_declared(lib):
    from tehmm_amd import _lib
    for name in ("tehmm_load_tracks_u8", "tehmm_trackio_last_timing", "tehmm_trackio_tile_rows"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.tehmm_abi_version() == 4
    assert lib.tehmm_trackio_tile_rows() >= 8 and lib.tehmm_trackio_tile_rows() % 8 == 0


@pytest.mark.parametrize("what, kw", [
    ("T < 0", dict(T=-1)), ("K < 1", dict(K=0)), ("K > 128", dict(K=129)),
    ("NULL fill", dict(null=("fill",))), ("NULL kind", dict(null=("kind",))), ("NULL rec_offsets", dict(null=("ro",))),
    ("NULL seq_offsets", dict(null=("so",))), ("NULL data", dict(null=("data",))),
    ("NULL rec_start", dict(null=("start",))), ("NULL rec_end", dict(null=("end",))),
    ("NULL rec_sym0", dict(null=("sym0",))), ("NULL rec_sym", dict(null=("sym",))),
    ("NULL seq_bytes", dict(null=("seq",))), ("NULL seq_lut", dict(null=("lut",))),
    ("rec_offsets decrease", dict(ro=(0, 2, 1))), ("rec_offsets start above 0", dict(ro=(1, 1, 1))),
    ("seq_offsets decrease", dict(so=(0, 4, 0))), ("a sequence track without its bytes", dict(so=(0, 0, 3))),
    ("a record track with bytes", dict(so=(0, 4, 8))), ("a sequence track with records", dict(ro=(0, 0, 1))),
    ("a kind of 2", dict(kind=(0, 2))),
])
def test_argument_errors_need_no_device(lib, what, kw):
    assert _load(lib, **kw) == ERR_ARG, what
    assert b"tehmm_load_tracks_u8" in lib.tehmm_last_error()


def test_timing_getter_arguments(lib):
    ms = (ctypes.c_double * 4)()
    names = (ctypes.c_char_p * 4)()
    assert lib.tehmm_trackio_last_timing(4, None, ms) == ERR_ARG
    assert lib.tehmm_trackio_last_timing(-1, names, ms) == ERR_ARG
    assert _load(lib, T=-1) == ERR_ARG and lib.tehmm_trackio_last_timing(4, names, ms) == 0
