"""GPU tests of track scaling (tehmm_track_rows_won, tehmm_load_tracks_f32, tehmm_amd/scaling.py): everything is compared
for exact equality with the plain-Python statement (tests/scaling_ref.py) and with what the real reference returned
(tests/golden/scaling.npz)."""
import logging
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import scaling_ref as sr
from test_scaling_cpu import CASES, IDS, fixture_of
from test_trackio_cpu import ERR_ARG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trackIO():
    from tehmm_amd import trackIO
    return trackIO


@pytest.fixture(scope="module")
def tile(trackIO):
    return trackIO.tileRows()


# ---- 1. the two device calls on lists built to go wrong ------------------------------------------------------------------
def shaped_tracks(tile):
    """T = 3 tiles + 5 rows over three tables, four tracks of (start, end): see the comments"""
    tables = [2 * tile + 7, 3, tile - 5]
    T = sum(tables)
    t1, t2 = tables[0], tables[0] + tables[1]                  # first rows of the second and third table
    wide = [
        (0, t1),              # table-wide: wins [0, 5), [24, 40), [41, t1) -- separate pieces, and all of the second tile
        (5, 9),
        (8, 12),              # wins nothing: the next record starts with it and outlasts it
        (8, 16),              # run boundary to run boundary
        (16, 24),
        (40, 41),
        (t1, t2),             # the second table, whole
        (t2 + 2, t2 + 3),
        (T - 1, T),           # the last row
    ]
    rng = np.random.RandomState(5)
    s = np.sort(rng.randint(0, T, size=100))
    many = sorted(list(zip(s.tolist(), np.minimum(T, s + rng.randint(1, 12, size=100)).tolist())) + [
        (tile - 8, tile),                 # ends on a tile boundary
        (tile, tile + 3),                 # starts on one
        (2 * tile - 2, 2 * tile + 2),     # crosses one
    ], key=lambda r: r[0])
    assert len(many) > 64                                       # a second level of block maxima
    s = np.sort(rng.randint(0, T, size=150))
    length = np.where(rng.rand(150) < 0.1, rng.randint(1, T + 1, size=150), rng.randint(1, 7, size=150))
    deep = list(zip(s.tolist(), np.minimum(T, s + length).tolist()))
    return T, [wide, many, [], deep]


def random_tracks(T, K, seed):
    rng = np.random.RandomState(seed)
    tracks = []
    for k in range(K):
        n = 0 if k == 1 else int(rng.randint(1, 2 * T + 2))
        s = np.sort(rng.randint(0, T, size=n))
        tracks.append(list(zip(s.tolist(), np.minimum(T, s + rng.randint(1, max(2, T // 2), size=n)).tolist())))
    return T, tracks


def whole_tile_tracks(tile):
    """two tracks that share a wave: a record that has all rows of the second and third tile to itself (and parts of
    their neighbours) beside a track without records, so that every lane of the wave holds one run there"""
    T = 4 * tile + 3
    return T, [[(3, 9), (tile - 10, 3 * tile + 7), (3 * tile + 2, 3 * tile + 5)], []]


def shape(name, tile):
    if name == "3 tiles + 5":
        return shaped_tracks(tile)
    if name == "whole tiles":
        return whole_tile_tracks(tile)
    if name == "whole tiles, one track":
        return 3 * tile, [[(0, 3 * tile), (tile, 2 * tile)]]    # every tile has one winner; the wave's other half is idle
    if name == "3 rows":
        return random_tracks(3, 4, 11)
    return random_tracks(tile + 12, 9, 12)                      # rows a multiple of 4; two turns of eight tracks


SHAPES = ["3 tiles + 5", "3 rows", "tile + 12 rows, 9 tracks", "whole tiles", "whole tiles, one track"]
_ref = {}


def reference_of(name, tile):
    """(T, tracks as FloatTrack arguments, [(won, uncovered)], [float rows]) of a shape, computed once"""
    if name not in _ref:
        T, tracks = shape(name, tile)
        rng = np.random.RandomState(len(name))
        args, counts, rows = [], [], []
        for k, recs in enumerate(tracks):
            start = np.asarray([r[0] for r in recs], dtype=np.int64)
            end = np.asarray([r[1] for r in recs], dtype=np.int64)
            val = (rng.standard_normal(len(recs)) * 10.0 ** rng.randint(-3, 6, size=len(recs))).astype(np.float32)
            fill = np.float32([0.0, -1.5, sr.F32_MAX, 7.25][k % 4])
            args.append((fill, start, end, val))
            counts.append(sr.rows_won(T, start, end))
            rows.append(sr.float_paint(T, start, end, val, fill))
        _ref[name] = (T, args, counts, rows)
    return _ref[name]


@pytest.mark.parametrize("name", SHAPES)
def test_rows_won_equal_the_restatement(trackIO, tile, name):
    T, args, counts, _ = reference_of(name, tile)
    won, uncovered = trackIO.rowsWon(T, [trackIO.FloatTrack(*a) for a in args])
    assert len(won) == len(args) and uncovered.dtype == np.int64
    for k, (want_won, want_unc) in enumerate(counts):
        assert won[k].tolist() == want_won.tolist(), "track %d" % k
        assert int(uncovered[k]) == want_unc
        assert int(won[k].sum()) + int(uncovered[k]) == T
    assert [n for n, _ in trackIO.lastTiming()] == ["upload", "tree", "count", "download"]


def test_the_shaped_lists_hold_what_they_are_for(tile):
    T, args, counts, _ = reference_of(SHAPES[0], tile)
    assert T == 3 * tile + 5 and len(args) == 4
    won = counts[0][0]
    assert won[0] == 5 + 16 + (2 * tile + 7 - 41) and won[0] > tile       # separate pieces, and a whole tile
    assert won[2] == 0 and won[3] == 8                                     # a record that wins nothing
    assert counts[2] == (counts[2][0], T) and len(counts[2][0]) == 0       # a track without records
    assert len(args[1][1]) > 64 and (counts[3][0] == 0).any()


def lanes_with_one_winner(tile, T, tracks):
    """[(tile, first track of the wave, winners)] where every lane of a wave of k_trk_rows_won holds one run: all rows of
    a tile of both tracks of the wave (tracks 2 w and 2 w + 1 of a turn of eight) have one winner each"""
    own = [np.asarray(sr.owners(T, [(s, e, None) for s, e in recs])) for recs in tracks]
    hits = []
    for t in range((T + tile - 1) // tile):
        for k in range(0, len(tracks), 2):
            w = [set(own[j][t * tile:(t + 1) * tile].tolist()) for j in (k, k + 1) if j < len(tracks)]
            if all(len(x) == 1 for x in w):
                hits.append((t, k, [x.pop() for x in w]))
    return hits


def test_the_whole_tile_shapes_reach_the_path_without_a_scan(tile):
    """what the shapes are for, on the host: waves whose lanes all hold one run, with a record as the winner"""
    T, tracks = whole_tile_tracks(tile)
    hits = lanes_with_one_winner(tile, T, tracks)
    assert [(t, w) for t, _, w in hits] == [(1, [1, -1]), (2, [1, -1]), (4, [-1, -1])]
    T, tracks = shape("whole tiles, one track", tile)
    assert [(t, w) for t, _, w in lanes_with_one_winner(tile, T, tracks)] == [(0, [0]), (1, [1]), (2, [0])]
    T, tracks = shaped_tracks(tile)
    assert lanes_with_one_winner(tile, T, tracks) == []          # (the first shape takes the scan everywhere)


def test_winners_of_whole_tiles_are_carried_across_the_tiles_of_a_workgroup(trackIO, tile):
    """More tiles than workgroups (the grid is capped at 65536): workgroup b walks tiles b and b + 65536.  Expected counts
    in closed form.  Track 0: G over all rows, B on the third tile, a short record in tile 65536; track 1: C from tile
    65537 on.  Workgroup 1 sees G, G (the carry grows) beside none, C (flush of the uncovered rows); workgroup 2 sees B, G
    (flush of a record); workgroup 3 ends on the last tile of 5 rows; workgroup 0 meets a tile that needs the scan with a
    carry pending."""
    grid = 65536
    T = (grid + 3) * tile + 5
    short = grid * tile + 10
    track0 = trackIO.FloatTrack(0.0, [0, 2 * tile, short], [T, 3 * tile, short + 5], [1, 2, 3])
    track1 = trackIO.FloatTrack(0.0, [(grid + 1) * tile], [T], [4])
    won, uncovered = trackIO.rowsWon(T, [track0, track1])
    assert won[0].tolist() == [T - tile - 5, tile, 5] and won[1].tolist() == [T - (grid + 1) * tile]
    assert uncovered.tolist() == [0, (grid + 1) * tile]


@pytest.mark.parametrize("name", SHAPES)
def test_float_paint_equals_the_restatement(trackIO, tile, name):
    T, args, _, rows = reference_of(name, tile)
    got = trackIO.paintTracksFloat(T, [trackIO.FloatTrack(*a) for a in args])
    assert got.shape == (len(args), T) and got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
    for k, want in enumerate(rows):
        assert got[k].tobytes() == want.tobytes(), "track %d" % k
    assert [n for n, _ in trackIO.lastTiming()] == ["upload", "tree", "paint", "download"]


# ---- 2. bad lists are an argument error, not a fault -------------------------------------------------------------------------
@pytest.mark.parametrize("what, start, end, offender", [
    ("unsorted", [0, 5, 4, 9, 8], [2, 6, 6, 10, 10], 2),
    ("end beyond T", [0, 5, 9], [2, 6, 101], 2),
    ("empty record", [0, 5, 9], [2, 5, 11], 1),
    ("negative start", [-1, 5, 9], [2, 6, 11], 0),
])
def test_bad_records_name_the_lowest_index(trackIO, what, start, end, offender):
    from tehmm_amd._lib import TeHmmHipError
    T = 100
    good = trackIO.FloatTrack(1.0, [0, 50], [10, 60], [2, 3])
    bad = trackIO.FloatTrack(1.0, start, end, [1] * len(start))
    for call in (trackIO.rowsWon, trackIO.paintTracksFloat):
        with pytest.raises(TeHmmHipError) as err:
            call(T, [good, bad])
        assert err.value.code == ERR_ARG and "record %d " % (2 + offender) in str(err.value), what
        call(T, [good, good])                                   # the next valid call is served


def test_checks_before_the_device(trackIO):
    from tehmm_amd import _lib
    from tehmm_amd._lib import f32p, i64p, ptr
    lib = _lib.load()
    p = lambda a: ptr(a, f32p if a.dtype == np.float32 else i64p)
    ro, one, two = (np.asarray(x, dtype=np.int64) for x in ([0, 1], [0], [2]))
    won, uncovered = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    fill, val, out = np.asarray([-1], dtype=np.float32), np.asarray([3.5], dtype=np.float32), np.zeros(4, np.float32)
    count = lambda T, K, ro_, s, e, a, b: lib.tehmm_track_rows_won(T, K, ro_, s, e, a, b)
    paint = lambda T, K, ro_, s, e, a, b: lib.tehmm_load_tracks_f32(T, K, p(fill), ro_, s, e, a, b)
    for call, a, b in ((count, p(won), p(uncovered)), (paint, p(val), p(out))):
        assert call(-1, 1, p(ro), p(one), p(two), a, b) == ERR_ARG
        assert call(4, 0, p(ro), p(one), p(two), a, b) == ERR_ARG
        assert call(4, 129, p(ro), p(one), p(two), a, b) == ERR_ARG
        assert call(4, 1, None, p(one), p(two), a, b) == ERR_ARG
        assert call(4, 1, p(np.asarray([1, 1], dtype=np.int64)), p(one), p(two), a, b) == ERR_ARG
        assert call(4, 1, p(np.asarray([0, -1], dtype=np.int64)), p(one), p(two), a, b) == ERR_ARG
        assert call(4, 1, p(ro), None, p(two), a, b) == ERR_ARG
        assert call(4, 1, p(ro), p(one), p(two), a, None) == ERR_ARG
        assert b"tehmm_" in lib.tehmm_last_error()
        assert call(4, 1, p(ro), p(one), p(two), a, b) == 0
    assert (won[0], uncovered[0]) == (2, 2) and out.tolist() == [3.5, 3.5, -1, -1]


# ---- 3. the golden cases through the public functions -------------------------------------------------------------------
def make_track(case, path, name="t"):
    from tehmm_amd.track import Track
    t = case["track"]
    a = dict(name=name, path=path, distribution=t["dist"], valCol=str(t["valCol"]))
    for key in ("scale", "logScale", "shift", "default"):
        if t[key] is not None:
            a[key] = str(t[key])
    if t["delta"]:
        a["delta"] = "True"
    return Track.fromXMLElement(ET.Element("track", a))


def scaling_attributes(track):
    a = track.toXMLElement().attrib
    return dict((key, a[key]) for key in ("scale", "logScale", "shift", "default") if key in a)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_public_functions_equal_the_reference(trackIO, case, tmp_path):
    from tehmm_amd import scaling
    fix = fixture_of(case["name"])
    path = str(tmp_path / "x.bed")
    open(path, "w").write(case["bed"])
    intervals = [tuple(iv) for iv in case["intervals"]]
    track = make_track(case, path)
    if fix["error"] == "ValueError":
        for fn in (scaling.readTrackIntoFloatArray, scaling.trackWeights):
            with pytest.raises(ValueError):
                fn(track, intervals)
        with pytest.raises(ValueError):
            scaling.setTrackScale(track, case["numBins"], intervals, case["noLog"])
        assert scaling_attributes(track) == fix["attrib"]
        return
    data = scaling.readTrackIntoFloatArray(track, intervals)
    assert data.dtype == np.float32 and data.tobytes() == fix["data"].tobytes()
    values, weights = scaling.trackWeights(track, intervals)
    assert values.dtype == np.float32 and weights.dtype == np.int64
    assert sr.expand(values, weights).tobytes() == np.sort(fix["data"]).tobytes()
    scaling.setTrackScale(track, case["numBins"], intervals, case["noLog"])
    assert scaling_attributes(track) == fix["attrib"]


def split_bed(intervals):
    """the intervals as a BED whose lines getMergedBedIntervals has to put together again"""
    lines = []
    for chrom, s, e in intervals:
        mid = (s + e) // 2
        lines += ["%s\t%d\t%d" % (chrom, s, mid), "%s\t%d\t%d" % (chrom, mid, e)]
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("names, options, untouched", [
    (["linear_wins", "log_wins", "default_shift_linear", "few_bases", "non_numeric"], [], []),
    (["shift_log", "log_wins"], ["--numBins", "12", "--tracks", "shift_log"], ["log_wins"]),
    (["log_wins_nolog", "linear_wins"], ["--noLog", "--skip", "linear_wins"], ["linear_wins"]),
])
def test_main_writes_the_attributes_of_the_reference(trackIO, names, options, untouched, tmp_path, caplog):
    from tehmm_amd import scaling
    from tehmm_amd.track import readTrackList
    by_name = {c["name"]: c for c in CASES}
    root = ET.Element("teModelConfig")
    for name in names:
        case = by_name[name]
        path = str(tmp_path / (name + ".bed"))
        open(path, "w").write(case["bed"])
        root.append(make_track(case, path, name).toXMLElement())
    root.append(ET.Element("track", dict(name="genome", path=str(tmp_path / "g.fa"))))      # FASTA tracks are passed by
    (tmp_path / "g.fa").write_text(">chr1\nACGT\n")
    xml, out = str(tmp_path / "tracks.xml"), str(tmp_path / "scaled.xml")
    ET.ElementTree(root).write(xml)
    (tmp_path / "all.bed").write_text(split_bed(by_name[names[0]]["intervals"]))
    with caplog.at_level(logging.WARNING, logger="teHmm"):
        assert scaling.main(["setTrackScaling", xml, str(tmp_path / "all.bed"), out] + options) == 0
    done = readTrackList(out)
    assert [t.getName() for t in done] == names + ["genome"]
    for name in names:
        want = fixture_of(name)["attrib"] if name not in untouched else scaling_attributes(make_track(by_name[name], "x"))
        assert scaling_attributes(done.getTrackByName(name)) == want, name
    skipped = [r.getMessage() for r in caplog.records if "Skipping (non-numeric?) track" in r.getMessage()]
    assert len(skipped) == (1 if "non_numeric" in names else 0)


# ---- 4. the call the tool is built on -------------------------------------------------------------------------------------
def test_float_output_buffer_without_a_value_map(trackIO, tmp_path):
    case = CASES[0]
    path = str(tmp_path / "x.bed")
    open(path, "w").write(case["bed"])
    chrom, start, end = case["intervals"][0]
    T, records = sr.interval_records(case["bed"], [case["intervals"][0]], case["track"]["valCol"])
    want = sr.float_paint(T, [r[0] for r in records], [r[1] for r in records], [r[2] for r in records], -7.5)
    assert (want == -7.5).any() and (want != -7.5).any()
    for read in (trackIO.readBedData, trackIO.readTrackData):
        buf = np.full(T, -7.5, dtype=np.float32)
        back = read(path, chrom, start, end, outputBuf=buf, valCol=case["track"]["valCol"], useDelta=make_track)
        assert back is buf and buf.tobytes() == want.tobytes()  # (useDelta: any object that is not True, as the tool's)
    with pytest.raises(ValueError):
        trackIO.readBedData(path, chrom, start, end, outputBuf=np.zeros(T, dtype=np.uint8))      # bytes want a map
    with pytest.raises(ValueError):
        trackIO.readBedData(path, chrom, start, end, outputBuf=np.zeros(T, dtype=np.float32), valCol=3)   # names
