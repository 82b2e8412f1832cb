"""BED parsing without a device: the line / field rule (bedparse_ref against trackIO.bedRead, the specification), the
number routines of the device parse run on the CPU (tehmm_bed_parse_number executes the code the kernels run), and the
routing of trackIO.parseBed.

Yardsticks: bedRead for lines and fields; Python's int() and float() for numbers, floats compared as uint64; the
certified domains are computed here from the rule (bedparse_ref.intInDomain / floatInDomain), not from the library."""
import os
import struct

import numpy as np
import pytest

import bedparse_ref as ref


@pytest.fixture(scope="module")
def trackIO():
    from tehmm_amd import build, trackIO
    build.build()
    return trackIO


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


# ---- the rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,data", ref.corpus(), ids=[n for n, _ in ref.corpus()])
def test_restatement_equals_bedRead_on_the_corpus(trackIO, tmp_path, name, data):
    assert ref.fieldTexts(data) == trackIO.bedRead(write(tmp_path, name + ".bed", data))


def test_restatement_equals_bedRead_on_random_files(trackIO, tmp_path):
    files = ref.randomFiles(200)
    assert len(files) == 200
    kept = 0
    for i, data in enumerate(files):
        got = ref.fieldTexts(data)
        assert got == trackIO.bedRead(write(tmp_path, "r.bed", data)), (i, data)
        kept += len(got)
    assert kept > 100                                 # (the alphabet does produce records)


def test_restatement_line_count_is_text_mode_with_newline_empty(tmp_path):
    for _, data in ref.corpus():
        p = write(tmp_path, "l.bed", data)
        with open(p, "r", newline="") as f:
            assert ref.numLines(data) == sum(1 for _ in f)


# ---- integers -----------------------------------------------------------------------------------------------------------
def test_integers_certified_domain(trackIO):
    rng = np.random.default_rng(5)
    texts = list(ref.INT_CERTIFIED)
    for _ in range(2000):
        nd = int(rng.integers(1, 19))
        texts.append(str(rng.choice(["", "+", "-"])) + "".join(str(d) for d in rng.integers(0, 10, nd)))
    for t in texts:
        assert ref.intInDomain(t)
        v, st = trackIO.parseNumber(t.encode(), trackIO.PARSE_INT)
        assert st == trackIO.CERTIFIED and v == int(t), t


def test_integers_outside_the_domain_go_to_the_host(trackIO):
    for t in ref.INT_HOST:
        assert not ref.intInDomain(t)
        assert trackIO.parseNumber(t.encode(), trackIO.PARSE_INT)[1] == trackIO.LEFT_TO_HOST, t


# ---- floats -------------------------------------------------------------------------------------------------------------
def check_floats(trackIO, texts):
    certified = 0
    for t in texts:
        v, st = trackIO.parseNumber(t.encode(), trackIO.PARSE_FLOAT)
        if ref.floatInDomain(t):
            assert st == trackIO.CERTIFIED, t            # everything in the domain is certified
            assert bits(v) == bits(float(t)), t          # ... and equals float() bit for bit
            certified += 1
        else:
            assert st == trackIO.LEFT_TO_HOST, t         # nothing outside it is
    return certified


def test_floats_crafted(trackIO):
    inside = {"1e22", "123456789012345", "0.123456789012345", ".5", "5.", "-0.0", "0e999", "3.0", "1.5e-21", "1e-22"}
    outside = {"1e23", "9007199254740993", "1234567890123456", "0.1234567890123456", ".", "e5", "inf", "nan", "0x10",
               "1_0.5", "1.5e-22", "1.5e-23", "", " 1.0"}
    for t in inside:
        assert ref.floatInDomain(t), t
    for t in outside:
        assert not ref.floatInDomain(t), t
    assert inside | outside <= set(ref.FLOAT_CRAFTED)
    assert check_floats(trackIO, ref.FLOAT_CRAFTED) >= len(inside)
    assert bits(trackIO.parseNumber(b"-0.0", trackIO.PARSE_FLOAT)[0]) == 1 << 63
    assert bits(trackIO.parseNumber(b"0e999", trackIO.PARSE_FLOAT)[0]) == 0


def test_floats_random(trackIO):
    texts = ref.randomFloatTexts(100000)
    certified = check_floats(trackIO, texts)
    assert 20000 < certified < 90000                  # both sides of the rule are exercised


# ---- routing ------------------------------------------------------------------------------------------------------------
BED = "chr1\t5\t9\ta\t1.5\nchr2\t0\t4\tb\t2\n#c\nchr1\t2\t7\ta\t3e2\r\nchr10\t1\t1\tc\t4\nshort\t1\nchr2\t3\t8\tb\t5\n"


def legacy_bedfile(trackIO, path):
    """the arrays BedFile built before it stood on BedColumns, from bedRead"""
    fields = trackIO.bedRead(path)
    start = np.asarray([int(r[1]) for r in fields], dtype=np.int64)
    end = np.asarray([int(r[2]) for r in fields], dtype=np.int64)
    groups = dict()
    for i, r in enumerate(fields):
        groups.setdefault(r[0], []).append(i)
    chroms = dict()
    for c, idx in groups.items():
        idx = np.asarray(idx, dtype=np.int64)
        idx = idx[end[idx] > start[idx]]
        idx = idx[np.argsort(start[idx], kind="stable")]
        chroms[c] = (idx, start[idx], np.maximum.accumulate(end[idx]) if len(idx) else end[idx])
    return fields, start, end, chroms


def test_small_file_takes_the_host_route(trackIO, tmp_path, monkeypatch):
    monkeypatch.delenv("TEHMM_BED_PARSE", raising=False)
    monkeypatch.delenv("TEHMM_BED_PARSE_MIN_BYTES", raising=False)
    assert trackIO.BED_PARSE_MIN_BYTES == 1 << 20
    cols = trackIO.parseBed(write(tmp_path, "s.bed", BED.encode()))
    assert cols.route == "host" and cols.n == 5


def test_high_bytes_take_the_host_route_whatever_the_size(trackIO, tmp_path, monkeypatch):
    monkeypatch.delenv("TEHMM_BED_PARSE", raising=False)
    line = "chr1\t1\t2\tnäme\n".encode("utf-8")
    p = write(tmp_path, "h.bed", line * ((1 << 20) // len(line) + 2))
    assert os.path.getsize(p) > 1 << 20
    cols = trackIO.parseBed(p)
    assert cols.route == "host" and cols.fields[0] == trackIO.bedRead(p)[0]


def test_forced_device_route_without_a_device_is_an_error(trackIO, tmp_path, monkeypatch):
    from tehmm_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    monkeypatch.setenv("TEHMM_BED_PARSE", "1")
    with pytest.raises(RuntimeError, match="needs a device"):
        trackIO.parseBed(write(tmp_path, "s.bed", BED.encode()))


def test_host_columns_reproduce_the_bedfile_arrays(trackIO, tmp_path, monkeypatch):
    monkeypatch.setenv("TEHMM_BED_PARSE", "0")
    p = write(tmp_path, "s.bed", BED.encode())
    fields, start, end, chroms = legacy_bedfile(trackIO, p)
    bed = trackIO.BedFile(p)
    assert bed.columns.route == "host"
    assert list(bed.fields) == fields and bed.fields[2] == fields[2]
    assert np.array_equal(bed.start, start) and np.array_equal(bed.end, end)
    assert bed.start.dtype == np.int64 and bed.end.dtype == np.int64
    assert list(bed.chroms) == list(chroms)
    for c in chroms:
        for a, b in zip(bed.chroms[c], chroms[c]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    code, values = bed.codes(3)
    assert code.tolist() == [0, 1, 0, 2, 1] and values == ["a", "b", "c"]
    cols = bed.columns
    assert cols.chromNames == ["chr1", "chr2", "chr10"] and cols.chromCode.tolist() == [0, 1, 0, 2, 1]
    assert cols.numFields.tolist() == [5] * 5 and cols.field(2, 4) == "3e2"
    assert cols.tuples(4) == [(r[0], int(r[1]), int(r[2]), r[3]) for r in fields]
    assert cols.codeFirst(3).tolist() == [0, 1, 3]
    with pytest.raises(ValueError, match="no column 7"):
        bed.codes(7)


def test_interval_columns_window_equals_the_list_filter(trackIO, tmp_path, monkeypatch):
    monkeypatch.setenv("TEHMM_BED_PARSE", "0")
    rng = np.random.default_rng(3)
    rows = []
    for c in ("chr2", "chr10", "chr1"):
        pos = 0
        for _ in range(60):
            n = int(rng.integers(0, 6))
            rows.append((c, pos, pos + n))
            pos += n
    order = rng.permutation(len(rows))
    p = write(tmp_path, "seg.bed", "".join("%s\t%d\t%d\n" % rows[i] for i in order).encode())
    tuples = trackIO.readBedIntervals(p, sort=True)
    for sort in (True, False):
        cols = trackIO.readBedColumns(p, sort=sort)
        ivs = tuples if sort else trackIO.readBedIntervals(p)
        assert cols.tuples() == ivs
        for c in ("chr1", "chr2", "chr10", "chrX"):
            for _ in range(40):
                a = int(rng.integers(0, 150))
                b = a + int(rng.integers(0, 60))
                want = [iv for iv in ivs if iv[0] == c and iv[1] >= a and iv[2] <= b]
                s, e = cols.window(c, a, b)
                assert list(zip(s.tolist(), e.tolist())) == [(iv[1], iv[2]) for iv in want]
