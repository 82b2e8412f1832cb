#!/usr/bin/env python3
"""Golden vectors of the user-parameter files (semi-supervised training), by RUNNING THE REAL REFERENCE (recipe:
make_golden.py; the reference's text never enters the repository).

  user_params   a model of 5 named states over 3 tracks (binary, 4-symbol multinomial, gaussian):
                * applyUserTrans / applyUserStarts / applyUserEmissions (hmm.py:348-488, emission.py:347-470,
                  595-615) case by case: the lines, the tables before and after, numZeroInitEdges, or the type of
                  the exception the reference ends in (the tables are kept as the exception left them);
                * MultitrackHmm.fit with all three force lists for one and for three Baum-Welch iterations on two
                  tables of 600 and 424 rows (layout of em_iteration_r0.npz, results under it1_ / it3_);
                * one iteration with transMatEpsilons and no force list from a matrix that holds a zero (eps_);
                * the statements of teHmmTrain.py's trainModel for --flatEm with init and force files (state names in
                  the order of the transition file, init files, fit, force files once more) with --iter 0 and
                  --iter 3 on two tables of 600 and 400 rows (tool_ files and tables, results under tool0_ / tool3_).
Re-run:  python tests/golden/make_golden_user_params.py
"""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402

STATES = ["s0", "s1", "s2", "s3", "s4"]
SYMBOLS = [2, 4, 8]
CAT_VALUES = ["a", "b", "c"]                      # symbols 2, 3, 4 (1: the unknown value)
GAUSS_VALUES = list(range(0, 16, 2))              # scale 0.5: symbols 1 .. 8

TRANS_CASES = {
    "trans_plain": (["# FROM TO PROB\n", "\n", "s0 s1 0.3\n", "  s2\ts2  0.5\n"], False),
    "trans_fullrow": (["s1 s1 1.0\n"], False),
    "trans_zero": (["s3 s4 0.0\n", "s0 s1 0.3\n"], False),
    "trans_zero_eps": (["s3 s4 0.0\n", "s0 s1 0.3\n"], True),
    "trans_over": (["s0 s1 0.7\n", "s0 s2 0.6\n"], False),
    "trans_unknown": (["sX s1 0.1\n"], False),
}
START_CASES = {
    "start_plain": ["# STATE PROB\n", "s0 0.4\n"],
    "start_zero": ["s1 0.0\n", "s0 0.4\n"],
    "start_over": ["s0 0.7\n", "s1 0.6\n"],
    "start_unknown": ["sX 0.1\n"],
}
EMIS_CASES = {
    "emis_plain": ["# STATE TRACK SYMBOL PROB\n", "\n", "s0 cat a 0.5\n", "s1 bin 1 0.9\n"],
    "emis_binary_names": ["s3 bin None 0.2\n", "s0 bin 0 0.3\n"],
    "emis_fullrow": ["s2 cat a 1.0\n"],
    "emis_additive": ["s3 cat a 0.95\n"],
    "emis_gauss": ["s4 gauss 6.0 2.5\n", "s0 cat b 0.25\n"],
    "emis_unknown": ["s0 cat zzz 0.2\n"],
    "emis_over": ["s0 cat a 0.7\n", "s0 cat b 0.6\n"],
    "emis_noleft": ["s1 bin 1 0.9\n", "s1 bin 0 0.05\n"],
    "emis_badstate": ["sX cat a 0.5\n"],
}
FORCE_TRANS = ["s0 s1 0.3\n", "s3 s4 0.0\n"]
FORCE_EMIS = ["s0 cat a 0.5\n", "s1 bin 1 0.9\n", "s4 gauss 6.0 2.5\n"]
FORCE_START = ["s0 0.4\n"]


def main():
    root = mg.build_reference()
    from teHmm.hmm import MultitrackHmm
    from teHmm.emission import IndependentMultinomialAndGaussianEmissionModel
    from teHmm.track import Track, TrackList, CategoryMap
    from teHmm.common import myLog

    def make_tracks():
        tb, tc, tg = Track(), Track(), Track()
        tb.name, tb.dist = "bin", "binary"
        tb._init()
        tc.name = "cat"
        tc._init()
        for v in CAT_VALUES:
            tc.getValueMap().getMap(v, update=True)
        tg.name, tg.dist, tg.defaultVal, tg.scale = "gauss", "gaussian", "0", 0.5
        tg._init()
        for v in GAUSS_VALUES:
            tg.getValueMap().getMap(v, update=True)
        tg.getValueMap().sort()
        tl = TrackList()
        for t in (tb, tc, tg):
            tl.addTrack(t)
        return tl

    N = len(STATES)
    rs = np.random.RandomState(11)
    params = [[list(r / r.sum()) for r in 0.1 + rs.random_sample((N, n))] for n in SYMBOLS]
    tm = 0.05 + rs.random_sample((N, N)) + 2.0 * np.eye(N)
    tm /= tm.sum(axis=1)[:, None]
    sp = 0.1 + rs.random_sample(N)
    sp /= sp.sum()

    def make_hmm(eps=False, paths=None, **kw):
        tl = make_tracks()
        em = IndependentMultinomialAndGaussianEmissionModel(N, SYMBOLS, tl, params=params)
        names = CategoryMap(reserved=0)
        for s in STATES:
            names.getMap(s, update=True)
        h = MultitrackHmm(em, state_name_map=names, transMatEpsilons=eps, **dict(paths or {}, **kw))
        h.trackList = tl
        h.transmat_ = tm.copy()
        h.startprob_ = sp.copy()
        return h

    def attempt(fn):
        try:
            fn()
            return ""
        except Exception as e:            # noqa: the type is the datum
            return type(e).__name__

    out = {"state_names": np.asarray(STATES), "symbols": np.asarray(SYMBOLS, dtype=np.int64),
           "cat_values": np.asarray(CAT_VALUES), "gauss_values": np.asarray(GAUSS_VALUES, dtype=np.int64)}
    h0 = make_hmm()
    out["transmat"], out["startprob"] = h0.transmat_, h0.startprob_
    out["log_probs"], out["gauss_params"] = h0.emissionModel.logProbs.copy(), h0.emissionModel.gaussParams.copy()

    # ---- applyUserTrans / applyUserStarts
    for name, (lines, eps) in TRANS_CASES.items():
        h = make_hmm(eps=eps)
        out[name + "_lines"] = np.asarray(lines)
        out[name + "_eps"] = int(eps)
        out[name + "_exc"] = np.asarray(attempt(lambda: h.applyUserTrans(lines)))
        out[name + "_after"] = h._log_transmat.copy()
        out[name + "_nzero"] = int(h.numZeroInitEdges)
    for name, lines in START_CASES.items():
        h = make_hmm()
        out[name + "_lines"] = np.asarray(lines)
        out[name + "_exc"] = np.asarray(attempt(lambda: h.applyUserStarts(lines)))
        out[name + "_after"] = h._log_startprob.copy()

    # ---- applyUserEmissions, from a table as maximize() leaves it (-1e6 where nothing was counted)
    before = h0.emissionModel.logProbs.copy()
    before[1, 3, 1:5] = [-1e6, 0.0, -1e6, -1e6]          # s3 emits only "a" on cat
    before[0, 2, 1:3] = [0.0, -1e6]                      # s2 never sees bin covered
    out["emis_before"] = before
    for name, lines in EMIS_CASES.items():
        h = make_hmm()
        h.emissionModel.logProbs = before.copy()
        out[name + "_lines"] = np.asarray(lines)
        out[name + "_exc"] = np.asarray(attempt(lambda: h.applyUserEmissions(lines)))
        out[name + "_after"] = h.emissionModel.logProbs.copy()
        out[name + "_gauss_after"] = h.emissionModel.gaussParams.copy()

    # ---- Baum-Welch with the three force lists (and with transMatEpsilons alone)
    ors = np.random.RandomState(23)
    tables = []
    for T in (600, 424):
        o = np.stack([ors.randint(1, n + 1, size=T) for n in SYMBOLS], axis=1).astype(np.uint8)
        run = np.repeat(ors.randint(1, 9, size=T // 8 + 1), 8)[:T]      # the gaussian track moves in runs
        o[:, 2] = run
        o[ors.random_sample(T) < 0.02, 1] = 0                             # a little missing data
        tables.append(o)
    out["obs0"], out["obs1"] = tables
    paths = {}
    for key, lines in (("forceUserTrans", FORCE_TRANS), ("forceUserEmissions", FORCE_EMIS),
                       ("forceUserStart", FORCE_START)):
        p = os.path.join(root, key + ".txt")
        open(p, "w").write("".join(lines))
        paths[key] = p
        out[key] = np.asarray(lines)
    for tag, n_iter in (("it1", 2), ("it3", 4)):
        h = make_hmm(paths=paths, n_iter=n_iter, thresh=0.0, fixStart=False)
        h.init_params = ""                                # keep our start / trans (basehmm.py:669-673)
        h.fit([t.copy() for t in tables])
        out[tag + "_transmat_after"], out[tag + "_startprob_after"] = h.transmat_, h.startprob_
        out[tag + "_log_transmat_after"], out[tag + "_log_startprob_after"] = h._log_transmat, h._log_startprob
        out[tag + "_log_probs_after"] = h.emissionModel.logProbs.copy()
        out[tag + "_gauss_after"] = h.emissionModel.gaussParams.copy()
        out[tag + "_last_logprob"] = h.last_forward_log_prob
        out[tag + "_nzero"] = int(h.numZeroInitEdges)
    tz = tm.copy()
    tz[1] *= (1.0 - 0.0) / (1.0 - tz[1, 3])
    tz[1, 3] = 0.0
    h = make_hmm(eps=True, n_iter=2, thresh=0.0, fixStart=False)
    h.init_params = ""
    h._log_transmat = np.asarray(myLog(tz.copy()))        # (past the setter: the zero is still there when fit starts)
    out["eps_transmat"] = tz
    h.fit([t.copy() for t in tables])
    out["eps_transmat_after"], out["eps_startprob_after"] = h.transmat_, h.startprob_
    out["eps_log_transmat_after"] = h._log_transmat
    out["eps_log_probs_after"] = h.emissionModel.logProbs.copy()
    out["eps_gauss_after"] = h.emissionModel.gaussParams.copy()
    out["eps_last_logprob"] = h.last_forward_log_prob

    # ---- what teHmmTrain.py's trainModel does with --flatEm, init and force files (teHmmTrain.py:326-414), statement
    # for statement on the reference's classes: a flat emission model, the state names in the order the transition
    # file shows them (:418-430), the init files, fit, the force files once more.  No start force list (the tool has
    # no option for one).  Tables without missing data, so that they survive a trip through BED files; 1 000 rows,
    # below the 1 024 from which the E-step keeps float rows (a log-probability is held to 1e-9 on the fp64 rows).
    ors = np.random.RandomState(29)
    tool_tables = []
    for T in (600, 400):
        o = np.stack([ors.randint(1, n + 1, size=T) for n in SYMBOLS], axis=1).astype(np.uint8)
        o[:, 2] = np.repeat(ors.randint(1, 9, size=T // 8 + 1), 8)[:T]
        tool_tables.append(o)
    tool_tables[0][0:3, 1] = [2, 3, 4]                    # "a", "b", "c" appear in this order
    tool_tables[0][0:8, 2] = np.arange(1, 9)              # every gaussian value occurs, first in ascending order
    out["tool_obs0"], out["tool_obs1"] = tool_tables
    order = [2, 0, 1, 3, 4]                               # the file starts with s2's row: s2 s0 s1 s3 s4
    tfl = np.floor(tm * 1e12) / 1e12                      # rounded down: no row above 1
    tool_files = {
        "init_trans": ["# FROM TO PROB\n"] + ["s%d\ts%d\t%.12f\n" % (i, j, tfl[i, j]) for i in order for j in range(N)],
        "init_emis": ["s%d\tgauss\t%.4f\t%.4f\n" % (j, 2.0 + 2.5 * j, 1.5 + 0.25 * j) for j in range(N)] +
                     ["s1\tcat\tb\t0.6\n", "s2\tbin\t1\t0.2\n", "s3\tcat\tc\t0.4\n"],
        "init_start": ["s1\t0.3\n"],
        "force_trans": list(FORCE_TRANS),
        "force_emis": list(FORCE_EMIS),
    }
    tool_paths = {}
    for key, lines in tool_files.items():
        p = os.path.join(root, "tool_" + key + ".txt")
        open(p, "w").write("".join(lines))
        tool_paths[key] = p
        out["tool_" + key] = np.asarray(lines)

    def tool_model(n_iter):
        tl = make_tracks()
        names = CategoryMap(reserved=0)
        for line in open(tool_paths["init_trans"]):
            if len(line.lstrip()) > 0 and line.lstrip()[0] != "#":
                toks = line.split()
                names.getMap(toks[0], update=True)
                names.getMap(toks[1], update=True)
        rg = np.random.RandomState(1)
        em = IndependentMultinomialAndGaussianEmissionModel(len(names), SYMBOLS, tl, normalizeFac=0, randomize=False,
                                                            effectiveSegmentLength=None, random_state=rg,
                                                            randRange=(0.2, 0.8))
        h = MultitrackHmm(em, n_iter=n_iter, state_name_map=names, fixTrans=False, fixEmission=False, fixStart=False,
                          forceUserEmissions=tool_paths["force_emis"], forceUserTrans=tool_paths["force_trans"],
                          random_state=rg, thresh=0.0, transMatEpsilons=False, maxProb=False, maxProbCut=None)
        h.applyUserTrans(open(tool_paths["init_trans"]).readlines())
        h.trackList = tl
        h.applyUserEmissions(open(tool_paths["init_emis"]).readlines())
        h.applyUserStarts(open(tool_paths["init_start"]).readlines())
        h.validate()
        h.bestCopy = None                                 # train(): hmm.py:155-172
        h.fit([t.copy() for t in tool_tables])
        h.validate()
        h.applyUserTrans(open(tool_paths["force_trans"]).readlines())
        h.applyUserEmissions(open(tool_paths["force_emis"]).readlines())
        return h, names

    for tag, n_iter in (("tool0", 0), ("tool3", 3)):
        h, names = tool_model(n_iter)
        out[tag + "_state_names"] = np.asarray([names.getMapBack(i) for i in range(len(names))])
        out[tag + "_log_transmat"], out[tag + "_log_startprob"] = h._log_transmat, h._log_startprob
        out[tag + "_log_probs"] = h.emissionModel.logProbs.copy()
        out[tag + "_gauss"] = h.emissionModel.gaussParams.copy()
        lp = h.getLastLogProb()
        out[tag + "_last_logprob"] = np.nan if lp is None else lp

    mg.save("user_params", **out)
    shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
