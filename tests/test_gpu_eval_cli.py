"""python -m tehmm_amd.eval end to end on a tiny data set: two chromosomes of about 3 kb, three BED tracks, an XML
track list and models saved with modelIO.  Every output file is compared byte for byte with the file assembled from
loadTrackData, model.viterbi / posteriorDecode / posteriorDistribution / emissionColumn, output.statesToBed (the host
writer) and writeBic; the printed score line is compared too."""
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CHROMS = (("chrA", 3000), ("chrB", 2800))


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib, build
    build.build()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


def _runs(rs, length, values, lo=15, hi=120):
    """[(start, end, value)] covering [0, length) with runs of random lengths"""
    out, at = [], 0
    while at < length:
        n = min(length - at, int(rs.randint(lo, hi)))
        out.append((at, at + n, values[rs.randint(len(values))]))
        at += n
    return out


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """tracks, regions, a trained model without state names and the same model with names and algorithm "map" """
    from tehmm_amd import modelIO, segmenter, train, trackIO
    from tehmm_amd.track import CategoryMap, TrackData
    root = tmp_path_factory.mktemp("evalcli")
    rs = np.random.RandomState(11)
    lines = {"bin": [], "cat": [], "rep": []}
    for chrom, length in CHROMS:
        for s, e, v in _runs(rs, length, [0, 1]):
            if v:
                lines["bin"].append("%s\t%d\t%d\n" % (chrom, s, e))
        for name, vals in (("cat", ["a", "b", "c", None]), ("rep", ["LTR", "LINE", None])):
            for s, e, v in _runs(rs, length, vals):
                if v is not None:
                    lines[name].append("%s\t%d\t%d\t%s\n" % (chrom, s, e, v))
    for name, ls in lines.items():
        (root / (name + ".bed")).write_text("".join(ls))
    xml = root / "tracks.xml"
    xml.write_text('<teModelConfig>\n<track name="bin" path="%s" distribution="binary"/>\n'
                   '<track name="cat" path="%s"/>\n<track name="rep" path="%s"/>\n</teModelConfig>\n'
                   % tuple(str(root / (n + ".bed")) for n in ("bin", "cat", "rep")))
    regions = root / "regions.bed"
    regions.write_text("".join("%s\t0\t%d\n" % c for c in CHROMS))
    d = {"root": root, "xml": str(xml), "regions": str(regions), "model": str(root / "model.npz"),
         "map_model": str(root / "map_model.npz"), "segments": str(root / "segments.bed"),
         "chroms": str(root / "chroms.bed")}
    assert train.main([d["xml"], d["regions"], d["model"], "--numStates", "3", "--iter", "2", "--seed", "1"]) == 0
    m = modelIO.loadModel(d["model"])
    m._algorithm = "map"
    m.stateNameMap = CategoryMap(reserved=0)
    for name in ("outside", "LTR", "inside"):
        m.stateNameMap.update(name)
    modelIO.saveModel(d["map_model"], m)
    td = TrackData()
    td.loadTrackData(d["xml"], trackIO.getMergedBedIntervals(d["regions"], ncol=3), modelIO.loadModel(d["model"]).getTrackList())
    segmenter.segmentTracks(td, d["segments"])
    # jobs: a part of chrA, a line nothing touches, chrB whole, the rest of chrA (given out of order)
    (root / "chroms.bed").write_text("chrB\t0\t5000\nchrA\t1200\t3000\nchrZ\t0\t10\nchrA\t0\t1200\n")
    return d


def expected(d, tag, model_path, regions, segment=False, segLen=0, maxPost=False, pdStates=None, edStates=None,
             slice=0, bic=False):
    """the files and the printed text of one run, assembled with the host writer; returns (paths, text)"""
    from tehmm_amd import eval as te, modelIO, output, trackIO
    from tehmm_amd.track import TrackData
    model = modelIO.loadModel(model_path)
    if segLen > 0:
        model.getEmissionModel().effectiveSegmentLength = segLen
    merged = trackIO.getMergedBedIntervals(regions, ncol=3)
    chopped = list(te.slicedIntervals(merged, slice if slice > 0 else te.MAXINT))
    segIntervals = trackIO.readBedIntervals(regions, sort=True) if segment else None
    td = TrackData()
    td.loadTrackData(d["xml"], chopped, model.getTrackList(), segmentIntervals=segIntervals)
    paths = {k: str(d["root"] / ("%s_want.%s" % (tag, k))) for k in ("bed", "pd", "ed", "bic")}
    for k in ("bed", "pd", "ed"):
        open(paths[k], "w").close()
    post = [None] * td.getNumTrackTables()
    emis = [None] * td.getNumTrackTables()
    if pdStates is not None:
        mask = output.getPosteriorsMask(pdStates, model)
        post = [np.sum(p * mask, axis=1) for p in model.posteriorDistribution(td)]
    if edStates is not None:
        emis = model.emissionColumn(td, output.getPosteriorsMask(edStates, model))
    decoded = model.posteriorDecode(td) if maxPost else model.viterbi(td)
    names = None
    if model.getStateNameMap() is not None:
        names = [model.getStateNameMap().getMapBack(i) for i in range(model.getEmissionModel().getNumStates())]
    total, points = 0, 0
    for i, (lp, states) in enumerate(decoded):
        total += lp
        table = td.getTrackTableList()[i]
        with open(paths["bed"], "a") as f:
            f.write("#Viterbi Score: %f\n" % lp)
        if names is not None:
            states = [model.getStateNameMap().getMap(s) for s in states]
        output.statesToBed(table, states, paths["bed"], posteriorSums=post[i], posteriorsPath=paths["pd"],
                           stateNames=names, emissionSums=emis[i], emissionsPath=paths["ed"])
        points += len(states) * table.getNumTracks()
    text = "Viterbi (log) score: %f\n" % total
    if model.current_iteration is not None:
        text += "Number of EM iterations: %d\n" % model.current_iteration
    if bic:
        output.writeBic(paths["bic"], model, total, points)
    return paths, text, td.getNumTrackTables()


def run(d, tag, model_path, regions, options):
    from tehmm_amd import eval as te
    got = {k: str(d["root"] / ("%s_got.%s" % (tag, k))) for k in ("bed", "pd", "ed", "bic")}
    out = io.StringIO()
    argv = [d["xml"], model_path, regions, "--bed", got["bed"]]
    for opt in options:
        argv.append(got[opt[2:]] if opt in ("@@pd", "@@ed", "@@bic") else opt)
    assert te.main(argv, out=out) == 0
    return got, out.getvalue()


def same(got, want, keys):
    for k in keys:
        with open(got[k], "rb") as f, open(want[k], "rb") as g:
            a, b = f.read(), g.read()
        assert len(b) > 0 and a == b, k


def test_plain(data):
    want, text, n = expected(data, "plain", data["model"], data["regions"])
    got, printed = run(data, "plain", data["model"], data["regions"], [])
    assert n == 2 and printed == text and "Number of EM iterations: 2" in text
    same(got, want, ["bed"])
    with open(got["bed"]) as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("#Viterbi Score: ") and len(lines) == 2 + 3000 + 2800


def test_segment_and_seglen(data):
    kw = dict(segment=True, segLen=100)
    want, text, n = expected(data, "seg", data["model"], data["segments"], **kw)
    got, printed = run(data, "seg", data["model"], data["segments"], ["--segment", "--segLen", "100"])
    assert n == 2 and printed == text
    same(got, want, ["bed"])
    with open(got["bed"]) as f:
        n_lines = len(f.read().splitlines())
    assert 10 < n_lines < 3000                       # one line per segment


def test_max_post_on_a_map_model_with_state_names(data):
    want, text, _ = expected(data, "map", data["map_model"], data["regions"], maxPost=True)
    got, printed = run(data, "map", data["map_model"], data["regions"], ["--maxPost"])
    assert printed == text
    same(got, want, ["bed"])
    with open(got["bed"]) as f:
        assert {l.split("\t")[3] for l in f.read().splitlines() if not l.startswith("#")} <= {"outside", "LTR", "inside"}
    # and on a Viterbi model --maxPost changes nothing (quirk Q14)
    want, text, _ = expected(data, "q14", data["model"], data["regions"], maxPost=True)
    got, printed = run(data, "q14", data["model"], data["regions"], ["--maxPost"])
    assert printed == text
    same(got, want, ["bed"])


@pytest.mark.parametrize("which", ["model", "map_model"])
def test_pd_ed_and_bic_together(data, which):
    pd, ed = ("0,2", "1") if which == "model" else ("LTR,inside", "outside")
    want, text, _ = expected(data, "all_" + which, data[which], data["regions"], pdStates=pd, edStates=ed, bic=True)
    got, printed = run(data, "all_" + which, data[which], data["regions"],
                       ["--pd", "@@pd", "--pdStates", pd, "--ed", "@@ed", "--edStates", ed, "--bic", "@@bic"])
    assert printed == text
    same(got, want, ["bed", "pd", "ed", "bic"])


def test_slice(data):
    want, text, n = expected(data, "slice", data["model"], data["regions"], slice=1000, pdStates="1")
    got, printed = run(data, "slice", data["model"], data["regions"],
                       ["--slice", "1000", "--pd", "@@pd", "--pdStates", "1"])
    assert n == 6 and printed == text
    same(got, want, ["bed", "pd"])


def test_chroms(data, capsys):
    """every output file is the concatenation of the jobs' files in job order, the BIC file included"""
    from tehmm_amd import masking
    opts = dict(pdStates="0", edStates="2", bic=True)
    pieces, texts = [], []
    for n, line in enumerate([("chrA", 0, 1200), ("chrA", 1200, 3000), ("chrB", 0, 5000)]):
        region = str(data["root"] / ("job_%d.bed" % n))
        masking.writeBed([(line[0], line[1], min(line[2], dict(CHROMS)[line[0]]))], region)
        want, text, _ = expected(data, "job%d" % n, data["model"], region, **opts)
        pieces.append(want)
        texts.append(text)
    got, printed = run(data, "chroms", data["model"], data["regions"],
                       ["--chrom", data["chroms"], "--proc", "3", "--pd", "@@pd", "--pdStates", "0", "--ed", "@@ed",
                        "--edStates", "2", "--bic", "@@bic"])
    assert printed == "".join(texts)
    for k in ("bed", "pd", "ed", "bic"):
        joined = b""
        for want in pieces:
            with open(want[k], "rb") as f:
                joined += f.read()
        with open(got[k], "rb") as f:
            assert f.read() == joined and len(joined) > 0, k
