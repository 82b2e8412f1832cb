"""The model of tests/golden/user_params.npz (make_golden_user_params.py) built from this package's classes:
5 named states over a binary, a 4-symbol multinomial and a gaussian track."""
import numpy as np


def make_tracks(g):
    from tehmm_amd.track import BinaryMap, CategoryMap, Track, TrackList
    cmap = CategoryMap(reserved=2)
    for v in g["cat_values"]:
        cmap.getMap(str(v), update=True)
    gmap = CategoryMap(reserved=1, defaultVal="0", scale=0.5)
    for v in g["gauss_values"]:
        gmap.getMap(int(v), update=True)
    gmap.sort()
    return TrackList([Track("bin", 0, "binary", BinaryMap()), Track("cat", 1, "multinomial", cmap),
                      Track("gauss", 2, "gaussian", gmap)])


def make_hmm(g, **kw):
    """The fixture's starting model (tables copied from the fixture, not recomputed)."""
    from tehmm_amd.emission import IndependentMultinomialAndGaussianEmissionModel
    from tehmm_amd.hmm import MultitrackHmm
    from tehmm_amd.track import CategoryMap
    tracks = make_tracks(g)
    names = CategoryMap(reserved=0)
    for s in g["state_names"]:
        names.getMap(str(s), update=True)
    em = IndependentMultinomialAndGaussianEmissionModel(len(g["state_names"]), g["symbols"].tolist(), tracks)
    em.logProbs = g["log_probs"].copy()
    em.gaussParams = g["gauss_params"].copy()
    h = MultitrackHmm(em, state_name_map=names, **kw)
    h.trackList = tracks
    h.transmat_ = g["transmat"].copy()
    h.startprob_ = g["startprob"].copy()
    return h


def lines_of(g, key):
    return [str(x) for x in g[key]]


def write_force_files(g, tmp_path):
    """The three force lists of the fixture as files; the constructor arguments that name them."""
    out = {}
    for key in ("forceUserTrans", "forceUserEmissions", "forceUserStart"):
        p = tmp_path / (key + ".txt")
        p.write_text("".join(lines_of(g, key)))
        out[key] = str(p)
    return out


def forced_cells(h, g):
    """(trans mask, start mask, emission mask) of the fixture's force lists, from the recording parsers."""
    import copy
    rec = {}
    probe = copy.deepcopy(h)
    probe.applyUserTrans(lines_of(g, "forceUserTrans"), record=rec)
    probe.applyUserEmissions(lines_of(g, "forceUserEmissions"), record=rec)
    probe.applyUserStarts(lines_of(g, "forceUserStart"), record=rec)
    return rec["trans_mask"] == 1, rec["start_mask"] == 1, rec["emis_mask"] == 1
