"""CPU-only tests of the segmenter: the plain-Python statement of the chain (tests/segmenter_ref.py) against what the
real reference wrote (tests/golden/segmenter.npz), the option handling of resolveCutLists, and the native writer of
the hex labels.  No GPU compute calls here."""
import json
import logging

import numpy as np
import pytest

import segmenter_ref as sr
from conftest import load_golden


def golden_cases():
    g = load_golden("segmenter")
    cases = []
    for name in g["names"]:
        meta = json.loads(bytes(g[str(name) + "__meta"]).decode())
        meta["name"] = str(name)
        meta["data"] = g[str(name) + "__data"]
        bounds = np.concatenate([[0], np.cumsum(meta["lens"])])
        meta["tables"] = [meta["data"][bounds[t]:bounds[t + 1]] for t in range(len(meta["lens"]))]
        meta["stats_share"] = [float.fromhex(x) for x in meta["stats_share"]]
        cases.append(meta)
    return cases


CASES = golden_cases()


def test_fixture_covers_what_it_should():
    assert len(CASES) >= 12
    assert {c["comp"] for c in CASES} == {"first", "prev"}
    assert {c["thresh"] for c in CASES} >= {0, 1, 2}
    assert {c["maxLen"] for c in CASES} >= {0, 3, 17} and {c["fixLen"] for c in CASES} >= {0, 5}
    assert any(sum(c["cut"]) for c in CASES) and any(sum(c["ignore"]) for c in CASES)
    assert any(len(c["lens"]) > 1 and c["co"] > 0 for c in CASES) and any(c["lens"] == [1] for c in CASES)
    assert all(max(c["lens"]) <= 300 and c["data"].shape[1] <= 6 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_the_reference(case):
    stats = {}
    offsets = [sr.segment_offsets(d, case["ignore"], case["cut"], case["thresh"], case["comp"], case["maxLen"],
                                  case["fixLen"], stats=stats) for d in case["tables"]]
    spans = [(c, s, s + n) for c, s, n in zip(case["chroms"], case["starts"], case["lens"])]
    rows = sr.bed_rows(spans, offsets, co=case["co"])
    assert "".join("%s\t%d\t%d\t%s\n" % r for r in rows) == case["bed"]
    assert sorted(stats) == case["stats_tracks"]
    assert [stats[k][0] for k in sorted(stats)] == case["stats_count"]
    np.testing.assert_allclose([stats[k][1] for k in sorted(stats)], case["stats_share"], rtol=1e-12, atol=0)
    # the early return of the reference without --stats changes nothing
    plain = [sr.segment_offsets(d, case["ignore"], case["cut"], case["thresh"], case["comp"], case["maxLen"],
                                case["fixLen"]) for d in case["tables"]]
    assert all(np.array_equal(a, b) for a, b in zip(plain, offsets))


def test_restatement_rejects_another_comp():
    with pytest.raises(RuntimeError):
        sr.segment_offsets(np.zeros((3, 2), np.uint8), [0, 0], [0, 0], comp="last")


def _tracks():
    from tehmm_amd.track import Track, TrackList
    tl = TrackList([Track("cat", 0), Track("gauss", 1, dist="gaussian"), Track("bin", 2, dist="binary"),
                    Track("msk", 3, dist="mask"), Track("sequence", 4)])
    tl[1].scale = 0.5                                  # a scaled (numeric) track
    return tl


def test_resolve_cut_lists_precedence():
    from tehmm_amd.segmenter import resolveCutLists
    tl = _tracks()
    cut, ign = resolveCutLists(tl)                     # defaults: mask cuts, "sequence" is ignored
    assert cut.tolist() == [0, 0, 0, 1, 0] and ign.tolist() == [0, 0, 0, 0, 1]
    cut, ign = resolveCutLists(tl, cutTracks="cat,bin", ignore=None)
    assert cut.tolist() == [1, 0, 1, 1, 0] and ign.tolist() == [0, 0, 0, 0, 0]
    # the cut-all options leave ignored tracks alone
    cut, ign = resolveCutLists(tl, cutUnscaled=True)
    assert cut.tolist() == [1, 0, 1, 1, 0] and ign.tolist() == [0, 0, 0, 0, 1]
    cut, ign = resolveCutLists(tl, cutMultinomial=True, ignore="cat")
    assert cut.tolist() == [0, 0, 0, 1, 1] and ign.tolist() == [1, 0, 0, 0, 0]
    cut, ign = resolveCutLists(tl, cutNonGaussian=True)
    assert cut.tolist() == [1, 0, 1, 1, 0]
    with pytest.raises(RuntimeError, match="cutTrack nope not found"):
        resolveCutLists(tl, cutTracks="nope")


def test_resolve_cut_lists_cut_and_ignored():
    from tehmm_amd.segmenter import resolveCutLists
    tl = _tracks()
    with pytest.raises(RuntimeError, match=r"Same track \(cat\) cant be cut and ignored"):
        resolveCutLists(tl, cutTracks="cat", ignore="cat")
    with pytest.raises(RuntimeError, match=r"Same track \(msk\) cant be cut and ignored"):
        resolveCutLists(tl, ignore="msk")               # mask tracks are forced to cut first


def test_resolve_cut_lists_unknown_ignore_names(caplog):
    from tehmm_amd.segmenter import resolveCutLists
    from tehmm_amd.track import Track, TrackList
    tl = TrackList([Track("a", 0), Track("b", 1)])
    with caplog.at_level(logging.WARNING, logger="tehmm_amd.segmenter"):
        cut, ign = resolveCutLists(tl)                  # no track called "sequence": silent
        assert not caplog.records and ign.tolist() == [0, 0]
        cut, ign = resolveCutLists(tl, ignore="sequence,zzz,b")
        assert ign.tolist() == [0, 1]
        assert [r.getMessage() for r in caplog.records] == ["ignore track zzz not found"]


def test_segment_offsets_rejects_before_any_device_call():
    from tehmm_amd.segmenter import segmentOffsets
    from tehmm_amd.track import IntegerTrackTable
    d = np.zeros((5, 2), dtype=np.uint8)
    with pytest.raises(RuntimeError, match="--comp must be either first or prev"):
        segmentOffsets([d], [0, 0], [0, 0], comp="last")
    with pytest.raises(TypeError):
        segmentOffsets([d.astype(np.uint16)], [0, 0], [0, 0])
    tab = IntegerTrackTable(2, "c", 0, 5).setData(d)
    tab.setSegmentOffsets([0, 2])
    with pytest.raises(ValueError, match="already segmented"):
        segmentOffsets([tab], [0, 0], [0, 0])


@pytest.mark.parametrize("co", [0, 15, 16, 2 ** 32])
def test_hex_label_writer(co, tmp_path):
    from tehmm_amd import build
    from tehmm_amd.segmenter import writeSegmentsBed
    build.build()
    path = tmp_path / "seg.bed"
    starts = np.asarray([10, 14, 15, 40], dtype=np.int64)
    ends = np.asarray([14, 15, 40, 41], dtype=np.int64)
    writeSegmentsBed(path, "chrX", starts[:3], ends[:3], first_label=co)
    writeSegmentsBed(path, "chrY", starts[3:], ends[3:], first_label=co + 3, append=True)
    want = "".join("%s\t%d\t%d\t%s\n" % (c, a, b, hex(co + i)[2:])
                   for i, (c, a, b) in enumerate(zip(["chrX"] * 3 + ["chrY"], starts, ends)))
    assert path.read_text() == want
