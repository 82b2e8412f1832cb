"""GPU tests of the device BED parse (tehmm_bedparse.hip.h, trackIO.parseBed with TEHMM_BED_PARSE=1): lines, fields and
counts against the plain restatement (tests/bedparse_ref.py, itself pinned to trackIO.bedRead by the CPU suite), numbers
against the CPU entry point, codes and everything built on the columns against the host route on the same files.
Every comparison is for equality."""
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import bedparse_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trackIO():
    from tehmm_amd import trackIO
    return trackIO


@pytest.fixture(scope="module")
def tile(trackIO):
    return trackIO.parseTileBytes()


@pytest.fixture(autouse=True)
def device_route(monkeypatch):
    monkeypatch.setenv("TEHMM_BED_PARSE", "1")
    monkeypatch.delenv("TEHMM_BED_PARSE_HASH_BITS", raising=False)


def write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def check_tables(trackIO, tmp_path, data, texts=True):
    """parse data on the device and compare every table with the restatement's"""
    cols = trackIO.parseBed(write(tmp_path, "f.bed", data))
    assert cols.route == "device"
    starts, lens, counts, off, length = ref.tables(data)
    assert cols.n == len(starts) and cols.numLines == ref.numLines(data)
    assert trackIO.parseCounters()["lines"] == cols.numLines and trackIO.parseCounters()["records"] == cols.n
    np.testing.assert_array_equal(cols.lineStart, np.asarray(starts, dtype=np.int64))
    np.testing.assert_array_equal(cols.lineLen, np.asarray(lens, dtype=np.int64))
    np.testing.assert_array_equal(cols.numFields, np.asarray(counts, dtype=np.int32))
    np.testing.assert_array_equal(cols.fieldLen, np.asarray(length, dtype=np.int32).reshape(-1, 6))
    np.testing.assert_array_equal(cols.fieldOff, np.asarray(off, dtype=np.int32).reshape(-1, 6))
    if texts:
        assert list(cols.fields) == ref.fieldTexts(data)
    cols.close()
    return cols


# ---- 1. the rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,data", ref.corpus(), ids=[n for n, _ in ref.corpus()])
def test_corpus(trackIO, tmp_path, name, data):
    check_tables(trackIO, tmp_path, data)


def test_random_files(trackIO, tmp_path):
    for data in ref.randomFiles(200):
        check_tables(trackIO, tmp_path, data)


# ---- 2. boundaries ------------------------------------------------------------------------------------------------------
def fill(nbytes):
    """records of exactly nbytes bytes (at least 32)"""
    assert nbytes >= 32
    full, rest = divmod(nbytes, 16)
    last = 16 + rest
    return b"chr1\t100\t200\tab\n" * (full - 1) + b"c\t1\t2\t" + b"x" * (last - 7) + b"\n"


def prefix(nbytes):
    """dropped lines of exactly nbytes bytes"""
    if nbytes == 0:
        return b""
    return b"\n" if nbytes == 1 else b"#" * (nbytes - 1) + b"\n"


# (what lies before the boundary, what lies from its last byte on): the second part's first byte is byte tile - 1
FEATURES = {
    "crlf": (b"c\t1\t2", b"\r\nc\t3\t4\n"),
    "lone_cr": (b"c\t1\t2", b"\rc\t3\t4\n"),
    "cr_then_crlf": (b"c\t1\t2", b"\r\r\nc\t3\t4\n"),
    "hash_after_terminator": (b"c\t1\t2", b"\n#c\t3\t4\nc\t5\t6\n"),
    "hash_after_cr": (b"c\t1\t2", b"\r#c\t3\t4\rc\t5\t6\r"),
    "tab": (b"c", b"\t1\t2\n"),
    "last_digit": (b"c\t1\t2", b"5\nc\t3\t4\n"),
    "last_digit_cr": (b"c\t1\t2", b"5\r\nc\t3\t4\n"),
}


@pytest.mark.parametrize("feature", sorted(FEATURES))
def test_boundary_sweep(trackIO, tmp_path, tile, feature):
    before, after = FEATURES[feature]
    core = fill(tile - 1 - len(before)) + before + after
    assert core[tile - 1:tile] == after[:1]
    core += fill(tile - 100) + b"c\t7\t8\tend"               # about two tiles, no last terminator
    wave = tile // 4
    shifts = list(range(18)) + [63, 64, 65, wave - 1, wave, wave + 1, tile - 1, tile, tile + 1]
    for shift in shifts:
        check_tables(trackIO, tmp_path, prefix(shift) + core, texts=False)


def test_sizes_around_one_tile(trackIO, tmp_path, tile):
    for n in (tile - 1, tile, tile + 1):
        check_tables(trackIO, tmp_path, fill(n), texts=False)
        check_tables(trackIO, tmp_path, fill(n - 1) + b"\r", texts=False)        # (the last byte is a lone "\r")
        check_tables(trackIO, tmp_path, fill(n - 7) + b"c\t1\t2\t\t", texts=False)   # no terminator, empty last fields


def test_one_line_of_three_tiles(trackIO, tmp_path, tile):
    long = b"c\t1\t2\t" + b"n" * (3 * tile) + b"\tscore\t+\tseventh\r\n"
    for data in (long, fill(40) + long + fill(40), b"#" + long + long):
        cols = check_tables(trackIO, tmp_path, data, texts=False)
    assert cols.n == 1 and cols.numFields[0] == 7


# ---- 3. numbers ---------------------------------------------------------------------------------------------------------
def test_numbers_inside_files(trackIO, tmp_path):
    ints = ref.INT_CERTIFIED + ref.INT_HOST
    floats = ref.FLOAT_CRAFTED + ref.randomFloatTexts(600, seed=3)
    n = max(len(ints), len(floats)) + 5
    rows = [(ints[i % len(ints)], ints[(3 * i + 1) % len(ints)], floats[i % len(floats)]) for i in range(n)]
    data = "".join("c\t%s\t%s\tname\t%s\n" % r for r in rows).encode()
    cols = trackIO.parseBed(write(tmp_path, "n.bed", data))
    assert cols.route == "device" and cols.n == n
    host = {1: 0, 2: 0, 4: 0}
    for col, kind, pos in ((1, trackIO.PARSE_INT, 0), (2, trackIO.PARSE_INT, 1), (4, trackIO.PARSE_FLOAT, 2)):
        val, status = cols.numbers(col, kind)
        for i, r in enumerate(rows):
            v, st = trackIO.parseNumber(r[pos].encode(), kind)
            assert status[i] == st, (col, r[pos])
            host[col] += st != trackIO.CERTIFIED
            if st == trackIO.CERTIFIED:
                assert np.asarray(val[i]).tobytes() == np.asarray(v, dtype=val.dtype).tobytes(), (col, r[pos])
    assert min(host.values()) > 0
    # a column some records lack: status 2
    val, status = trackIO.parseBed(write(tmp_path, "m.bed", b"c\t1\t2\tn\t0.5\nc\t1\t2\nc\t1\t2\tn\t7\n")).numbers(4, 1)
    assert status.tolist() == [0, 2, 0] and val.tolist() == [0.5, 0.0, 7.0]


def outcome(fn):
    try:
        return ("ok", fn())
    except Exception as e:            # noqa: BLE001 -- the exception is the result that is compared
        return (type(e), str(e))


def test_error_parity(trackIO, tmp_path, monkeypatch):
    rows = [["chr1", str(10 * i), str(10 * i + 5), "n"] for i in range(12)]
    rows[6][1] = "12x"
    rows[8][2] = "--"
    p = write(tmp_path, "e.bed", "".join("\t".join(r) + "\n" for r in rows).encode())
    calls = [lambda: trackIO.BedFile(p).start.tolist(), lambda: trackIO.readBedIntervals(p),
             lambda: trackIO.readBedIntervals(p, sort=True), lambda: trackIO.readBedIntervals(p, 4, "chr1", 0, 1000)]
    got = dict()
    for mode in ("0", "1"):
        monkeypatch.setenv("TEHMM_BED_PARSE", mode)
        got[mode] = [outcome(c) for c in calls]
    assert got["0"] == got["1"]
    assert all(kind is ValueError and "12x" in text for kind, text in got["1"])
    # with the bad end in front of the bad start the record order decides which one readBedIntervals meets first
    rows[6][1], rows[3][2] = "60", "--"
    p = write(tmp_path, "e2.bed", "".join("\t".join(r) + "\n" for r in rows).encode())
    for mode in ("0", "1"):
        monkeypatch.setenv("TEHMM_BED_PARSE", mode)
        got[mode] = [outcome(c) for c in calls]
    assert got["0"] == got["1"] and all(kind is ValueError and "--" in text for kind, text in got["1"])


# ---- 4. codes -----------------------------------------------------------------------------------------------------------
def codes_file(tmp_path):
    rng = np.random.default_rng(11)
    values = [f % i for i in range(1000) for f in ("Name%d.5", "Name%d.50", "name%d.5")]
    pick = np.concatenate([rng.permutation(3000), rng.integers(0, 3000, 17000)])
    pick = pick[rng.permutation(20000)]
    chroms = ["chr%d" % c for c in rng.integers(1, 4, 20000)]
    data = "".join("%s\t%d\t%d\t%s\n" % (chroms[i], i, i + 3, values[v]) for i, v in enumerate(pick.tolist())).encode()
    return write(tmp_path, "codes.bed", data)


def test_codes_equal_the_host_route(trackIO, tmp_path, monkeypatch):
    p = codes_file(tmp_path)
    monkeypatch.setenv("TEHMM_BED_PARSE", "0")
    wantCode, wantValues = trackIO.BedFile(p).codes(3)
    assert len(wantValues) == 3000
    monkeypatch.setenv("TEHMM_BED_PARSE", "1")
    bed = trackIO.BedFile(p)
    assert bed.columns.route == "device"
    code, values = bed.codes(3)
    assert values == wantValues and code.dtype == wantCode.dtype
    np.testing.assert_array_equal(code, wantCode)
    assert trackIO.parseCounters()["code_fallbacks"] == 0
    # a 4-bit hash: 3 000 values behind 16 keys; the verification sees it and the host dictionary decides
    monkeypatch.setenv("TEHMM_BED_PARSE_HASH_BITS", "4")
    bed = trackIO.BedFile(p)
    assert bed.columns.route == "device"
    before = trackIO.parseCounters()["code_fallbacks"]
    code, values = bed.codes(3)
    assert trackIO.parseCounters()["code_fallbacks"] == before + 1
    assert values == wantValues
    np.testing.assert_array_equal(code, wantCode)


def test_codes_errors_are_the_host_routes(trackIO, tmp_path, monkeypatch):
    p = write(tmp_path, "v.bed", b"c\t1\t2\ta\nc\t3\t4\t\nc\t5\t6\tb\n")
    q = write(tmp_path, "w.bed", b"c\t1\t2\ta\nc\t3\t4\nc\t5\t6\t\n")
    got = dict()
    for mode in ("0", "1"):
        monkeypatch.setenv("TEHMM_BED_PARSE", mode)
        got[mode] = [outcome(lambda: trackIO.BedFile(p).codes(3)), outcome(lambda: trackIO.BedFile(q).codes(3)),
                     outcome(lambda: trackIO.BedFile(p).codes(4))]
    assert got["0"] == got["1"]
    assert [k for k, _ in got["1"]] == [ValueError] * 3 and "empty value" in got["1"][0][1]


# ---- 5. end to end: host route against device route ---------------------------------------------------------------------
NUMBERS = ["0.25", "1e-1", "3", "2.50", "0.30000000000000004", "7e0", "12.5"]


def e2e_file(tmp_path):
    rng = np.random.default_rng(2)
    lines = ["#track name=x\n"]
    for i in range(20000):
        c = ("chr1", "chr2", "chr10", "chrX")[int(rng.integers(0, 4))]
        s = int(rng.integers(0, 3000))
        n = int(rng.choice([0, 0, 1, 5, 40, 400]))
        lines.append("%s\t%d\t%d\t%s\t%s%s" % (c, s, s + n, "abcdeF"[int(rng.integers(0, 6))],
                                                NUMBERS[int(rng.integers(0, len(NUMBERS)))],
                                                ("\n", "\r\n", "\n", "\tmore\t+\n")[int(rng.integers(0, 4))]))
    return write(tmp_path, "e2e.bed", "".join(lines).encode())


def make_track(dist, valCol, **more):
    from tehmm_amd.track import Track
    a = dict(name="t", path="x", distribution=dist, valCol=str(valCol))
    a.update({k: str(v) for k, v in more.items()})
    return Track.fromXMLElement(ET.Element("track", a))


def e2e_results(trackIO, p):
    from tehmm_amd import masking
    rng = np.random.default_rng(9)
    out = dict()
    bed = trackIO.BedFile(p)
    out["route"] = bed.columns.route
    out["start"], out["end"] = bed.start, bed.end
    out["chroms"] = list(bed.chroms)
    for c in bed.chroms:
        out["idx_" + c], out["s_" + c], out["reach_" + c] = bed.chroms[c]
    out["fields"] = [bed.fields[i] for i in (0, 1, 77, 19999)] + [len(bed.fields)]
    for w in range(50):
        c = ("chr1", "chr2", "chr10", "chrX", "chrNone")[w % 5]
        a = int(rng.integers(0, 3200))
        b = a + int(rng.integers(1, 600))
        out["pick%d" % w], out["os%d" % w], out["oe%d" % w] = bed.select(c, a, b)
        out["val%d" % w] = trackIO.recordValues(bed, out["pick%d" % w], 4, "t")
    for ncol in (3, 4, 5):
        for sort in (False, True):
            out["iv_%d_%d" % (ncol, sort)] = trackIO.readBedIntervals(p, ncol, sort=sort)
            out["ivw_%d_%d" % (ncol, sort)] = trackIO.readBedIntervals(p, ncol, "chr10", 500, 2500, sort=sort)
    out["merged"] = trackIO.getMergedBedIntervals(p, sort=True)
    out["masking_readBed"] = masking.readBed(p)
    cat, num = make_track("multinomial", 3), make_track("multinomial", 4, scale=4)
    for key, t in (("cat", cat), ("num", num)):
        out["row_" + key] = trackIO.readTrackData(p, "chr2", 100, 2900, valCol=t.getValCol(), valMap=t.getValueMap(),
                                                  updateValMap=True)
        out["map_" + key] = sorted(t.getValueMap().fwd.items(), key=lambda kv: kv[1])
    return out


def test_host_route_against_device_route(trackIO, tmp_path, monkeypatch):
    p = e2e_file(tmp_path)
    res = dict()
    for mode in ("0", "1"):
        monkeypatch.setenv("TEHMM_BED_PARSE", mode)
        res[mode] = e2e_results(trackIO, p)
    assert res["0"].pop("route") == "host" and res["1"].pop("route") == "device"
    assert set(res["0"]) == set(res["1"])
    for key, want in res["0"].items():
        got = res["1"][key]
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype, key
            np.testing.assert_array_equal(got, want, err_msg=key)
        else:
            assert got == want, key
    assert len(res["1"]["iv_3_0"]) == 20000 and len(res["1"]["ivw_5_1"]) > 100


# ---- 6. segments --------------------------------------------------------------------------------------------------------
def segment_case(tmp_path, withMask):
    rng = np.random.default_rng(4)
    tables = [("chr2", 1000), ("chr10", 0), ("chr1", 500), ("chr2", 20000), ("chr10", 9000)]
    intervals, segs, track, mask = [], [], [], []
    for c, start in tables:
        pos = start
        for k in range(2000):
            n = int(rng.integers(1, 6))
            segs.append((c, pos, pos + n))
            if k % 3 == 0:
                track.append("%s\t%d\t%d\t%s\n" % (c, pos, pos + n + 2, "xyz"[int(rng.integers(0, 3))]))
            if withMask and k % 50 == 7:                  # (a mask interval is a whole segment: kept or cut as one)
                mask.append("%s\t%d\t%d\n" % (c, pos, pos + n))
            pos += n
        intervals.append((c, start, pos))
    order = rng.permutation(len(segs))
    seg = write(tmp_path, "seg.bed", "".join("%s\t%d\t%d\n" % segs[i] for i in order).encode())
    root = ET.Element("teModelConfig")
    root.append(ET.Element("track", dict(name="a", path=write(tmp_path, "a.bed", "".join(track).encode()),
                                         distribution="multinomial", valCol="3")))
    root.append(ET.Element("track", dict(name="b", path=write(tmp_path, "b.bed", "".join(track[::2]).encode()),
                                         distribution="binary", valCol="0")))
    if withMask:
        root.append(ET.Element("track", dict(name="m", path=write(tmp_path, "m.bed", "".join(mask).encode()),
                                             distribution="mask")))
    xml = str(tmp_path / "tracks.xml")
    ET.ElementTree(root).write(xml)
    return xml, intervals, seg


def loaded(xml, intervals, segments):
    from tehmm_amd.track import TrackData
    td = TrackData()
    td.loadTrackData(xml, intervals, segmentIntervals=segments)
    return ([t.getNumPyArray() for t in td.getTrackTableList()],
            [np.asarray(t.getSegmentOffsets()) for t in td.getTrackTableList()],
            [sorted(t.getValueMap().fwd.items(), key=lambda kv: kv[1]) for t in td.getTrackList()])


@pytest.mark.parametrize("withMask", [False, True], ids=["plain", "masked"])
def test_segments_as_list_and_as_columns(trackIO, tmp_path, withMask):
    xml, intervals, seg = segment_case(tmp_path, withMask)
    asList = trackIO.readBedIntervals(seg, sort=True)
    want = loaded(xml, intervals, asList)
    assert len(want[0]) == 5 and sum(len(o) for o in want[1]) > (9000 if withMask else 9999)
    # (a BedColumns is taken in file order, as a list is: the sorted list as a file)
    cols = trackIO.parseBed(write(tmp_path, "sorted.bed", "".join("%s\t%d\t%d\n" % iv for iv in asList).encode()))
    assert cols.route == "device"
    for segments in (trackIO.readBedColumns(seg, sort=True), cols, trackIO.IntervalColumns.fromTuples(asList, sort=True)):
        got = loaded(xml, intervals, segments)
        assert got[2] == want[2]
        for part in (0, 1):
            assert len(got[part]) == len(want[part])
            for a, b in zip(got[part], want[part]):
                assert a.dtype == b.dtype
                np.testing.assert_array_equal(a, b)


def test_segments_that_do_not_start_at_the_table_still_trip_the_assert(trackIO, tmp_path):
    xml, intervals, seg = segment_case(tmp_path, False)
    first = min(s for c, s, e in trackIO.readBedIntervals(seg) if c == "chr10")
    lines = [ln for ln in open(seg).read().splitlines(True) if not ln.startswith("chr10\t%d\t" % first)]
    short = write(tmp_path, "short.bed", "".join(lines).encode())
    for segments in (trackIO.readBedIntervals(short, sort=True), trackIO.readBedColumns(short, sort=True)):
        with pytest.raises(AssertionError):
            loaded(xml, intervals, segments)
