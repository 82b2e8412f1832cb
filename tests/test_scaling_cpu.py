"""CPU tests of track scaling (tehmm_amd/scaling.py, the additive parts of tehmm_amd/track.py): the plain-Python statement
(tests/scaling_ref.py) against what the real reference returned (tests/golden/scaling.npz), the weighted computeScale
against the statement on the expanded array, and the XML that carries the result.  No device call here."""
import json
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import scaling_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "scaling.npz"))
CASES = json.loads(bytes(GOLD["cases"]).decode())
IDS = [c["name"] for c in CASES]
SCALED = [c for c in CASES if c["expect"] is not None]

_want = {}


def want_of(case):
    """the restatement's answer, computed once per case"""
    if case["name"] not in _want:
        _want[case["name"]] = sr.run_case(case)
    return _want[case["name"]]


def fixture_of(name):
    out = json.loads(bytes(GOLD[name + "__meta"]).decode())
    for key in ("data", "linear_counts", "log_counts"):
        out[key] = GOLD["%s__%s" % (name, key)]
    return out


def assert_equals_fixture(name, got):
    """arrays bit for bit, counts integer for integer, parameters as the same floats, attributes as the same text"""
    fix = fixture_of(name)
    assert got["error"] == fix["error"]
    assert got["data"].dtype == fix["data"].dtype == np.float32
    assert got["data"].tobytes() == fix["data"].tobytes()
    for key in ("linear_counts", "log_counts"):
        assert fix[key].dtype == np.int64 and np.asarray(got[key]).tolist() == fix[key].tolist(), key
    assert (got["result"] is None) == (fix["result"] is None)
    if fix["result"] is not None:
        assert got["result"][0] == fix["result"][0]
        assert float(got["result"][1]) == fix["result"][1] and float(got["result"][2]) == fix["result"][2]
    assert got["attrib"] == fix["attrib"]


def test_the_cases_are_the_fixtures_and_cover_the_ground():
    assert sr.cases_json(sr.golden_cases()) == sr.cases_json(CASES)
    results = {c["name"]: fixture_of(c["name"])["result"] for c in CASES}
    kinds = {r[0] for r in results.values() if r}
    assert kinds == {"scale", "logScale"}
    assert any(r and r[0] == "logScale" and r[2] > 0 for r in results.values())           # minVal <= 0: a shift
    assert any(r and r[0] == "scale" and r[1] <= 1e-4 for r in results.values())            # not rounded
    assert any(c["noLog"] for c in CASES) and any(c["track"]["default"] is not None for c in CASES)
    assert {c["track"]["valCol"] for c in CASES} == {0, 3, 4}
    assert any(fixture_of(c["name"])["error"] == "ValueError" for c in CASES)
    assert any(r is None and len(fixture_of(n)["data"]) > 0 for n, r in results.items())   # len(data) <= numBins
    assert any(len({iv[0] for iv in c["intervals"]}) == 2 and len(c["intervals"]) > 2 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_the_reference(case):
    assert_equals_fixture(case["name"], want_of(case))


@pytest.mark.parametrize("case", SCALED, ids=[c["name"] for c in SCALED])
def test_weighted_compute_scale_equals_the_restatement(case):
    from tehmm_amd import scaling
    want = want_of(case)
    values, weights = np.unique(want["data"], return_counts=True)
    np.testing.assert_array_equal(sr.expand(values, weights), np.sort(want["data"]))
    for args in ((values, weights), (want["data"], None)):
        counts = []
        before = args[0].copy()
        got = scaling.computeScale(args[0], case["numBins"], case["noLog"], weights=args[1], counts=counts)
        assert got[0] == want["result"][0] and float(got[1]) == want["result"][1] and float(got[2]) == want["result"][2]
        assert str(got[2]) == want["attrib"]["shift"]                                        # float32 or 0.0, as text
        assert counts[0].tolist() == want["linear_counts"].tolist()
        assert counts[1].tolist() == want["log_counts"].tolist()
        assert args[0].tobytes() == before.tobytes()


def test_hist_variance_keeps_the_assertions():
    from tehmm_amd import scaling
    data = np.asarray([1, 2, 3, 50], dtype=np.float32)
    edges = np.asarray([1, 2, 3, 4], dtype=np.float32)
    with pytest.raises(AssertionError):
        scaling.histVariance(data, edges)                                   # 50 lies above the last edge
    with pytest.raises(AssertionError):
        scaling.histVariance(data, edges, fromLog=True)                     # ... and above it with a bin from 0 too
    low = np.asarray([0.5, 2, 3, 4], dtype=np.float32)
    with pytest.raises(AssertionError):
        scaling.histVariance(low, edges)
    counts = []
    var = scaling.histVariance(low, edges, fromLog=True, weights=np.asarray([5, 1, 1, 2]), counts=counts)
    assert counts[0].tolist() == [0, 1, 3] and var == np.var([0., 1., 3.])  # 0.5 is dropped; 4 closes the last bin


def test_record_values_are_float32_and_must_be_finite_numbers(tmp_path):
    from tehmm_amd import trackIO
    path = tmp_path / "v.bed"
    path.write_text("c\t0\t5\t0.1\t7\nc\t5\t9\t1e-3\tx\nc\t9\t12\t0.1\tinf\nc\t12\t14\t3\t1e39\n")
    bed = trackIO.BedFile(str(path))
    pick = np.arange(4)
    got = trackIO.recordValues(bed, pick, 3, "v")
    assert got.dtype == np.float32 and got.tolist() == [np.float32(0.1), np.float32(1e-3), np.float32(0.1), 3.0]
    assert trackIO.recordValues(bed, pick, 0, "v").tolist() == [1.0] * 4
    with pytest.raises(ValueError):
        trackIO.recordValues(bed, pick, 4, "v")                             # "x" is no number
    for rows in ([0, 2], [0, 3]):
        with pytest.raises(ValueError, match="track v"):
            trackIO.recordValues(bed, np.asarray(rows), 4, "v")             # inf; a number float32 cannot hold


def test_lane_join_adds_every_run_of_a_tile_once():
    """the join of k_trk_rows_won, modelled lane for lane (scaling_ref.lane_join_adds): one add per maximal run of equal
    winners, with its length, whatever the runs look like"""
    rng = np.random.RandomState(0)
    for trial in range(600):
        rows = int(rng.choice([256, 256, 1, 3, 5, 8, 9, 77, 250, 255]))
        kind = trial % 3
        if kind == 0:
            w = np.full(rows, rng.randint(-1, 3))
        elif kind == 1:
            w = rng.randint(-1, 3, size=rows)
        else:
            w = np.concatenate([np.full(int(rng.choice([1, 2, 7, 8, 9, 16, 40, 100])), rng.randint(-1, 4))
                                for _ in range(rows)])[:rows]
        cuts = np.flatnonzero(w[1:] != w[:-1]) + 1
        want = sorted((int(w[a]), int(b - a)) for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [rows]])))
        assert sorted((int(x), int(n)) for x, n in sr.lane_join_adds(w.tolist())) == want, w.tolist()


# ---- the XML that carries the result --------------------------------------------------------------------------------
TRACKS_XML = """<teModelConfig>
<track name="cov" path="cov.bed" distribution="gaussian" valCol="4" default="0" scale="0.25" shift="2.0"/>
<track name="rep" path="rep.bed" preprocess="rm"/>
<track name="seq" path="g.fa" caseSensitive="True"/>
<track name="cpg" path="cpg.bed" distribution="binary"/>
<track name="d" path="d.bed" delta="true" valCol="4" scale="1.5"/>
<track name="gap" path="gap.bed" distribution="mask"/>
</teModelConfig>
"""


def parsed(path):
    return [dict(e.attrib) for e in ET.parse(path).getroot().findall("track")]


def test_xml_round_trip_keeps_every_attribute(tmp_path):
    from tehmm_amd.track import readTrackList
    src = tmp_path / "in.xml"
    src.write_text(TRACKS_XML)
    tracks = readTrackList(str(src))
    out, again = str(tmp_path / "out.xml"), str(tmp_path / "again.xml")
    tracks.saveXML(out)
    assert ET.parse(out).getroot().tag == "teModelConfig"
    got = parsed(out)
    assert [a["name"] for a in got] == ["cov", "rep", "seq", "cpg", "d", "gap"]              # mask tracks come last
    want = {a["name"]: a for a in parsed(str(src))}
    for a in got:
        w = dict(want[a["name"]])
        w.setdefault("distribution", "multinomial")
        w.setdefault("valCol", "3")
        if w["distribution"] in ("binary", "mask"):
            w["valCol"] = "0"
        if "delta" in w:
            w["delta"] = "True"
        assert a == w
    readTrackList(out).saveXML(again)
    assert parsed(again) == got
    back = readTrackList(out)
    cov = back.getTrackByName("cov")
    assert (cov.getScale(), cov.getShift(), cov.getDefaultVal(), cov.getValCol(), cov.getDist()) == (
        0.25, 2.0, "0", 4, "gaussian")
    assert back.getTrackByName("gap", isMask=True).getDist() == "mask" and back.getTrackByName("d").getDelta() is True


def test_setters_and_the_element_follow_the_reference():
    from tehmm_amd.track import Track
    t = Track("t", path="t.bed", scale=0.5, shift=1.0, defaultVal="0")
    t.setLogScale(2.5)
    assert t.getLogScale() == 2.5 and t.getScale() is None and t.getShift() == 1.0
    a = t.toXMLElement().attrib
    assert a["logScale"] == "2.5" and "scale" not in a and a["shift"] == "1.0" and a["default"] == "0"
    t.setScale(0.125)
    assert t.getScale() == 0.125 and t.getLogScale() is None
    t.setShift(np.float32(3.099))
    a = t.toXMLElement().attrib
    assert a["scale"] == "0.125" and "logScale" not in a and a["shift"] == "3.099"
    assert "caseSensitive" not in a and "delta" not in a and "preprocess" not in a
    both = Track("b", path="b.bed")
    both.scale, both.logScale = 2.0, 3.0                                      # logScale wins in the element
    a = both.toXMLElement().attrib
    assert a["logScale"] == "3.0" and "scale" not in a and "shift" not in a
    assert Track("n").toXMLElement().attrib == dict(name="n", distribution="multinomial", valCol="3")


def test_abi_additions_are_detected_by_symbol():
    from tehmm_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(HERE), "include", "tehmm_hip.h")).read()
    for name in ("tehmm_track_rows_won", "tehmm_load_tracks_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
    assert lib.tehmm_abi_version() == 4
