#!/usr/bin/env python3
"""Golden vectors of the grammar model, by RUNNING THE REAL REFERENCE (recipe: make_golden.py -- scratch copy outside
the repository, np.int_t -> np.int64_t, lib2to3, np.float shim -- with cfg.py and _cfg.pyx added to the scratch
package and _cfg cythonized as well; the reference's text never enters the repository).

  cfg.npz   per case NAME the inputs of one MultitrackCfg.decode and what it returned:
              NAME_em [L, M] (allLogProbs rows), NAME_al [L] uint16 (absent: no alignment track), NAME_def,
              NAME_nest (pair states), NAME_lp1 [M, M, M], NAME_lp2 [M, M], NAME_priors [M, 2], NAME_start [M],
              NAME_score, NAME_trace [L], NAME_dp [L, L, M] (only where stored)
            cases: the four decodes of the reference's cfgTest.py (unit_*), the flat initParams model on a constant
            column (ties), a supervisedTrain model (sup: with the HMM tables it was derived from and the training
            data), and random models r_M{M}_L{L} (saPrior 0.95; r1_*: saPrior 1.0, -inf in logPriors).
            init_M5_*: the tables initParams leaves for M = 5 with pair states 1 and 3.
Prints the reference kernel's single-core time on the two longest cases.
Re-run:  python tests/golden/make_golden_cfg.py
"""
import os
import shutil
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402
from make_golden_r2 import DuckTrackData          # noqa: E402

SETUP_CFG = r"""
import numpy
from setuptools import setup, Extension
from Cython.Build import cythonize
exts = [Extension("teHmm._cfg", ["teHmm/_cfg.pyx"], include_dirs=[numpy.get_include()])]
setup(name="teHmm_ref_scratch_cfg", ext_modules=cythonize(exts, language_level=2, quiet=True))
"""

DP_MAX_L = 24
SMALL_M = (1, 2, 3, 5, 8)
SMALL_L = (1, 2, 3, 4, 7, 24)
BIG = ((33, 65), (5, 63), (5, 64), (5, 65), (5, 130), (5, 300), (5, 700))


def add_cfg(root):
    pkg = os.path.join(root, "teHmm")
    for f in ("cfg.py", "_cfg.pyx"):
        shutil.copy(os.path.join(mg.REF, f), os.path.join(pkg, f))
    p = os.path.join(pkg, "_cfg.pyx")
    s = open(p).read().replace("np.int_t", "np.int64_t")
    open(p, "w").write(s)
    subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n", os.path.join(pkg, "cfg.py")],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    open(os.path.join(root, "setup_cfg.py"), "w").write(SETUP_CFG)
    subprocess.check_call([sys.executable, "setup_cfg.py", "-q", "build_ext", "--inplace"], cwd=root,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def main():
    root = mg.build_reference()
    add_cfg(root)
    from teHmm.cfg import MultitrackCfg
    from teHmm.hmm import MultitrackHmm
    from teHmm.emission import IndependentMultinomialEmissionModel, PairEmissionModel
    from teHmm.track import IntegerTrackTable
    out = {}
    times = {}

    def record(name, cfg, obs, al=None, def_sym=0, with_dp=False):
        t0 = time.perf_counter()
        score, trace = cfg.decode(obs, alignmentTrack=al, defAlignmentSymbol=def_sym)
        times[name] = time.perf_counter() - t0
        out[name + "_em"] = np.array(cfg.emLogProbs, dtype=np.float64)
        if al is not None:
            out[name + "_al"] = np.asarray(al[:, 0], dtype=np.uint16)
        out[name + "_def"] = np.asarray(def_sym)
        out[name + "_nest"] = np.asarray(cfg.nestStates, dtype=np.int64)
        out[name + "_lp1"], out[name + "_lp2"] = (np.array(t) for t in cfg.getLogProbTables())
        out[name + "_priors"] = np.array(cfg.pairEmissionModel.logPriors)
        out[name + "_start"] = np.array(cfg.startProbs)
        out[name + "_score"] = np.asarray(score)
        out[name + "_trace"] = np.asarray(trace, dtype=np.float64)
        if with_dp:
            out[name + "_dp"] = np.array(cfg.dp)

    def em_with(M, probs):
        em = IndependentMultinomialEmissionModel(M, [len(probs[0])], zeroAsMissingData=False)
        arr = np.zeros((1, M, len(probs[0])))
        arr[0] = probs
        with np.errstate(divide="ignore"):
            em.logProbs = np.log(arr)
        return em

    # ------------------------------------------------------------------ 1. the decodes of cfgTest.py
    em = IndependentMultinomialEmissionModel(5, [3], zeroAsMissingData=False)
    cfg = MultitrackCfg(em, PairEmissionModel(em, [1.0] * 5))
    record("unit_default", cfg, np.array([[0], [0], [1], [2]], dtype=np.uint8), with_dp=True)
    em = em_with(2, [[0.75, 0.25], [0.05, 0.95]])
    cfg = MultitrackCfg(em, PairEmissionModel(em, [1.0] * 2))
    record("unit_traceback", cfg, np.array([[0], [0], [1], [0]], dtype=np.uint8), with_dp=True)
    em = em_with(3, [[0.75, 0.25], [0.05, 0.95], [0.01, 0.90]])
    cfg = MultitrackCfg(em, PairEmissionModel(em, [1.0] * 3), nestStates=[1])
    obs = np.array([[1], [0], [0], [1]], dtype=np.uint8)
    record("unit_nest_match", cfg, obs, np.array([[1], [0], [0], [1]], dtype=np.uint16), 0, with_dp=True)
    record("unit_nest_nomatch", cfg, obs, np.array([[1], [0], [0], [2]], dtype=np.uint16), 0, with_dp=True)

    # ------------------------------------------------------------------ 2. the flat model on a constant column: ties
    em = IndependentMultinomialEmissionModel(5, [3], zeroAsMissingData=False)
    cfg = MultitrackCfg(em, PairEmissionModel(em, [0.95] * 5), nestStates=[1, 3])
    out["init_M5_lp1"], out["init_M5_lp2"] = (np.array(t) for t in cfg.getLogProbTables())
    out["init_M5_start"] = np.array(cfg.startProbs)
    out["init_M5_helper1"], out["init_M5_helperDim1"] = np.array(cfg.helper1), np.array(cfg.helperDim1)
    out["init_M5_helper2"], out["init_M5_helperDim2"] = np.array(cfg.helper2), np.array(cfg.helperDim2)
    record("ties", cfg, np.ones((40, 1), dtype=np.uint8))

    # ------------------------------------------------------------------ 3. supervisedTrain, M = 4 with one pair state
    rs = np.random.RandomState(17)
    T = 60
    beds, state_of = [], np.zeros(T, dtype=np.int64)
    cuts = [0, 9, 14, 27, 31, 44, 49, 60]
    labels = [0, 1, 2, 1, 0, 3, 0]                # (no transition 1 -> 3, 2 -> 0 ...: zeros in the tables)
    for a, b, s in zip(cuts[:-1], cuts[1:], labels):
        beds.append(("chrC", 100 + a, 100 + b, s))
        state_of[a:b] = s
    obs = np.zeros((T, 2), dtype=np.uint8)
    obs[:, 0] = 1 + (state_of + (rs.rand(T) < 0.15)) % 4
    obs[:, 1] = 1 + ((state_of == 1) ^ (rs.rand(T) < 0.1))
    tab = IntegerTrackTable(2, "chrC", 100, 100 + T)
    tab.data = obs.copy()
    tab.shape = obs.shape
    em = IndependentMultinomialEmissionModel(4, [4, 2])         # (defaults, as teHmmTrain builds it: symbols never
    cfg = MultitrackCfg(em, PairEmissionModel(em, [0.95] * 4), nestStates=[1])      # seen in a state get -1e6)
    cfg.supervisedTrain(DuckTrackData([tab]), beds)
    hmm = MultitrackHmm(em)                       # the tables the productions were split from
    hmm.supervisedTrain(DuckTrackData([tab]), beds)
    out["sup_obs"] = obs
    out["sup_bed"] = np.asarray([(b[1], b[2], b[3]) for b in beds], dtype=np.int64)
    out["sup_table_start"] = np.asarray(100)
    out["sup_log_probs"] = np.array(em.logProbs)
    out["sup_hmm_transmat"] = np.array(hmm.transmat_)
    out["sup_hmm_startprob"] = np.array(hmm.getStartProbs())
    al = np.zeros((T, 1), dtype=np.uint16)
    al[9:14, 0] = [1, 2, 0, 2, 1]
    al[27:31, 0] = [3, 3, 3, 0]
    record("sup", cfg, tab, al, 0)

    # ------------------------------------------------------------------ 4. random models
    def random_case(name, M, L, prior, seed):
        rs = np.random.RandomState(seed)
        nest = sorted(rs.choice(M, size=min(M - 1, max(1, M // 3)) if M > 1 else 0, replace=False).tolist())
        em = em_with(M, rs.dirichlet(np.ones(4), size=M))
        cfg = MultitrackCfg(em, PairEmissionModel(em, [prior] * M), nestStates=nest)
        # productions of every state redrawn at random (a third of them dropped), rows kept summing to one
        lp1, lp2 = cfg.getLogProbTables()
        for x in range(M):
            keep1 = np.isfinite(lp1[x]) & (rs.rand(M, M) < 0.67)
            keep1[x, x] = np.isfinite(lp1[x, x, x])
            keep2 = np.isfinite(lp2[x]) & (rs.rand(M) < 0.67)
            w1, w2 = rs.rand(M, M) * keep1, rs.rand(M) * keep2
            tot = w1.sum() + w2.sum()
            with np.errstate(divide="ignore"):
                lp1[x], lp2[x] = np.log(w1 / tot), np.log(w2 / tot)
        with np.errstate(divide="ignore"):
            cfg.startProbs = np.log(rs.dirichlet(np.ones(M)))
        cfg.createHelperTables()
        cfg.validate()
        obs = rs.randint(0, 4, size=(L, 1)).astype(np.uint8)
        al = rs.randint(0, 4, size=(L, 1)).astype(np.uint16)
        # a few planted repeats so that pair productions do win
        for _ in range(max(1, L // 12)):
            i, j = sorted(rs.randint(0, L, size=2))
            obs[j] = obs[i]
            al[j] = al[i]
        record(name, cfg, obs, al, 0, with_dp=L <= DP_MAX_L)

    seed = 1000
    for M in SMALL_M:
        for L in SMALL_L:
            seed += 1
            random_case("r_M%d_L%d" % (M, L), M, L, 0.95, seed)
    for M, L in ((2, 4), (5, 24)):
        seed += 1
        random_case("r1_M%d_L%d" % (M, L), M, L, 1.0, seed)
    for M, L in BIG:
        seed += 1
        random_case("r_M%d_L%d" % (M, L), M, L, 0.95, seed)

    out["names"] = np.asarray(sorted(k[:-len("_score")] for k in out if k.endswith("_score")))
    mg.save("cfg", **out)
    for name in ("r_M5_L300", "r_M5_L700"):
        print("reference decode (one core) %-12s %.2f s" % (name, times[name]))
    shutil.rmtree(root, ignore_errors=True)
    print("done; reference scratch build removed:", root)


if __name__ == "__main__":
    main()
