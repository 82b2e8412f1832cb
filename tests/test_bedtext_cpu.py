"""The value formatter of the device BED text, run on the CPU (tehmm_bed_text_format_value executes the code the
device runs), and the argument checks of the two calls that come before any device call.

Yardstick: "%.12g" of the C library (Python's % operator rounds the exact decimal expansion the same way), plus ".0"
where that text holds only digits -- the rule of tehmm_write_bed."""
import ctypes

import numpy as np
import pytest

ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from tehmm_amd import _lib, build
    build.build()
    return _lib.load()


def expected(x):
    s = "%.12g" % x
    if all(c.isdigit() or c == "-" for c in s):
        s += ".0"
    return s


def curated():
    vals = [1.0, 0.5, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-4, 9.9999999999949e-05, 99999.9999999995,
            999999999999.5, 1e12, 1.0 - 2.0 ** -53, 5e-324, 1.7e308, 123456789012.5, 0.1, -2.5e-7, 1e11, 1e-5,
            99999999999.95, 2.2250738585072014e-308, 1e22, 1e23, 1e-287, 1e279, 1e284, 1e-292]
    for m in (1, 3, 5, 625, 15625):
        for e in range(-60, 40):
            vals.append(m * 2.0 ** e)
    return np.asarray(vals, dtype=np.float64)


def fmt(lib, x):
    buf = ctypes.create_string_buffer(32)
    ok = ctypes.c_int(-1)
    assert lib.tehmm_bed_text_format_value(float(x), buf, ctypes.byref(ok)) == 0
    return buf.value.decode(), ok.value


def test_symbols_are_declared(lib):
    from tehmm_amd import _lib
    for name in ("tehmm_bed_text_write", "tehmm_batch_bed_text_write", "tehmm_bed_text_last_counters",
                 "tehmm_bed_text_last_timing", "tehmm_bed_text_format_value"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["tehmm_bed_text_write"][1]) == 18
    assert len(_lib.SIGNATURES["tehmm_batch_bed_text_write"][1]) == 19


def test_curated_values_and_what_goes_to_the_host(lib):
    flagged = {}
    for x in curated():
        text, ok = fmt(lib, x)
        assert text == expected(x), (float(x).hex(), text, expected(x))
        flagged[float(x).hex() if x == x else "nan"] = ok == 0
    # true ties of the 12th digit, subnormals and magnitudes beyond the power table are the host's
    for x in (999999999999.5, 123456789012.5, 2.0 ** -18, 5e-324, 1.7e308, 1e-292, 1e284):
        assert flagged[float(x).hex()], x
    # the specials and plain values are the device's
    for x in (1.0, 0.5, 0.0, -0.0, np.inf, -np.inf, 1e-4, 1e12, 0.1, 1e22, 1e-287, 1e279):
        assert not flagged[float(x).hex()], x
    assert not flagged["nan"]
    assert fmt(lib, -np.nan)[1] == 0


def test_seeded_values_match_and_stay_on_the_device_path(lib):
    rs = np.random.RandomState(20)
    uni = rs.random_sample(40000)
    logu = 10.0 ** rs.uniform(-260, 260, 40000) * rs.choice([-1.0, 1.0], 40000)
    neglog = -rs.exponential(30.0, 20000)
    host = 0
    for block in (uni, logu, neglog):
        for x in block:
            text, ok = fmt(lib, x)
            assert text == expected(x), (float(x).hex(), text, expected(x))
            host += ok == 0
    # a random double lies within 2^-40 of a tie of its 12th digit with probability 2^-39
    assert host == 0


def test_switch_points_of_g(lib):
    vals = []
    for k in range(-8, 16):
        for d in (0.99999999999949, 0.9999999999996, 1.0, 1.00000000000049, 1.0000000000006, 9.9999999999949, 9.999999999996):
            vals.append(d * 10.0 ** k)
            vals.append(-d * 10.0 ** k)
    for x in vals:
        text, _ = fmt(lib, x)
        assert text == expected(x), (float(x).hex(), text, expected(x))


def test_calls_reject_before_any_device_call(lib):
    from tehmm_amd._lib import i64p, ptr
    chroms = (ctypes.c_char_p * 1)(b"chr1")
    one = np.asarray([0], dtype=np.int64)
    offs = np.asarray([0, 1], dtype=np.int64)
    st = np.zeros(1, dtype=np.int64)

    def call(path=b"/nonexistent-dir/x.bed", n=1, kind=1, offsets=offs, stripe=0, n_names=0):
        return lib.tehmm_bed_text_write(path, 0, n, chroms, ptr(one, i64p), ptr(one, i64p), ptr(offsets, i64p), None,
                                        None, None, None, kind, ptr(st, i64p), None, n_names, None, 0, stripe)

    assert call(path=None) == ERR_ARG
    assert call(n=-1) == ERR_ARG
    assert call(kind=7) == ERR_ARG
    assert call(stripe=-1) == ERR_ARG
    assert call(kind=0, n_names=1025) == ERR_ARG
    assert call(offsets=np.asarray([1, 2], dtype=np.int64)) == ERR_ARG
    assert call(offsets=np.asarray([0, -1], dtype=np.int64)) == ERR_ARG
    names, ms = (ctypes.c_char_p * 4)(), (ctypes.c_double * 4)()
    assert lib.tehmm_bed_text_last_timing(4, None, ms) == ERR_ARG
    assert lib.tehmm_bed_text_last_timing(4, names, ms) == 0          # the failed calls above left no timing
    assert lib.tehmm_batch_bed_text_write(None, None, 0, None, 0, 0, 0, None, None, None, None, None, None, None, 0,
                                          None, b"x", 0, 0) == ERR_ARG
