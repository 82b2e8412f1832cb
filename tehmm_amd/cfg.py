"""Stochastic context free grammar over the multitrack emission model -- host-side mirror of the reference's
``cfg.py``, with the CYK recurrence (``_cfg.pyx``) on the device (tehmm_cyk_decode).

States listed in ``nestStates`` emit pairs of columns (X -> a a, X -> a Y a), all others one column at a time.
Productions X -> Y Z live in ``logProbs1[X, Y, Z]``, X -> a Y a in ``logProbs2[X, Y]``.  Only supervised training is
offered, as in the reference.
"""
import ctypes

import numpy as np
from numpy.testing import assert_array_almost_equal

from . import _lib
from .common import NEGINF, logger, myLog
from .hmm import MultitrackHmm
from .track import TrackTable


class MultitrackCfg(object):
    def __init__(self, emissionModel, pairEmissionModel, nestStates=[], state_name_map=None):
        self.emissionModel = emissionModel
        self.pairEmissionModel = pairEmissionModel
        self.logProbs1 = None
        self.logProbs2 = None
        self.startProbs = None
        self.defAlignmentSymbol = 0
        self.PAIRFLAG = -2
        self.trackList = None
        self.stateNameMap = state_name_map
        self.M = self.emissionModel.getNumStates()
        self.emittingStates = np.arange(self.M)
        self.nestStates = np.array(nestStates, dtype=np.int64)
        self.hmmStates = np.array([i for i in self.emittingStates if i not in self.nestStates], dtype=np.int64)
        assert len(self.hmmStates) + len(self.nestStates) == self.M
        self.initParams()

    # ---- accessors (cfg.py:78-89); the last three are what the tools around MultitrackHmm ask of a model
    def getLogProbTables(self):
        return self.logProbs1, self.logProbs2

    def getStartProbs(self):
        """Not in log space, to match the HMM."""
        return np.exp(self.startProbs)

    def getTrackList(self):
        return self.trackList

    def getEmissionModel(self):
        return self.emissionModel

    def getStateNameMap(self):
        return self.stateNameMap

    def getLastLogProb(self):
        return None

    # ---- tables (cfg.py:110-217)
    def createTables(self):
        self.logProbs1 = NEGINF + np.zeros((self.M, self.M, self.M), dtype=np.float64)
        self.logProbs2 = NEGINF + np.zeros((self.M, self.M), dtype=np.float64)

    def createHelperTables(self):
        """The productions above -inf of every left state, in ascending order of their right sides: helper1
        [M, maxRow, 2] int32 (padded with -1) with helperDim1 [M], helper2 [M, maxRow] with helperDim2 [M]."""
        M = self.M
        rows1 = [np.argwhere(self.logProbs1[x] > NEGINF) for x in range(M)]
        self.helperDim1 = np.asarray([len(r) for r in rows1], dtype=np.int32)
        self.helper1 = -1 + np.zeros((M, max([len(r) for r in rows1] + [0]), 2), dtype=np.int32)
        for x, r in enumerate(rows1):
            self.helper1[x, :len(r)] = r
        rows2 = [np.flatnonzero(self.logProbs2[x] > NEGINF) for x in range(M)]
        self.helperDim2 = np.asarray([len(r) for r in rows2], dtype=np.int32)
        self.helper2 = -1 + np.zeros((M, max([len(r) for r in rows2] + [0])), dtype=np.int32)
        for x, r in enumerate(rows2):
            self.helper2[x, :len(r)] = r

    def initParams(self):
        """Flat distributions (cfg.py:161-188): a single state X has the M productions X -> X Y; a pair state the 3M - 1
        productions X -> X Y, X -> Y X and X -> a Y a (X -> X X counted once)."""
        self.createTables()
        oneOfAny = myLog(1. / self.M)
        self.startProbs = oneOfAny + np.zeros((self.M,), dtype=np.float64)
        for state in self.hmmStates:
            for nextState in self.emittingStates:
                self.logProbs1[state, state, nextState] = oneOfAny
        oneOfCfgRHS = myLog(1. / (3.0 * self.M - 1.0))
        for state in self.nestStates:
            for nextState in self.emittingStates:
                self.logProbs1[state, state, nextState] = oneOfCfgRHS
                self.logProbs1[state, nextState, state] = oneOfCfgRHS
                self.logProbs2[state, nextState] = oneOfCfgRHS
        self.createHelperTables()
        self.validate()

    def validate(self):
        """Start probabilities and the productions of every state add up to one, in the tables and in the helper
        lists (cfg.py:190-217)."""
        assert_array_almost_equal(np.sum(np.exp(self.startProbs)), 1.)
        for origin in self.emittingStates:
            total = np.sum(np.exp(self.logProbs1[origin])) + np.sum(np.exp(self.logProbs2[origin]))
            assert_array_almost_equal(total, 1.)
            h1 = self.helper1[origin, :self.helperDim1[origin]]
            h2 = self.helper2[origin, :self.helperDim2[origin]]
            total = np.sum(np.exp(self.logProbs1[origin, h1[:, 0], h1[:, 1]])) + np.sum(np.exp(self.logProbs2[origin, h2]))
            assert_array_almost_equal(total, 1.)

    # ---- decoding (cfg.py:219-304) on the device
    def _cyk(self, tables, alignmentTables, defAlignmentSymbol):
        """One tehmm_cyk_decode call over a list of tables: [(score, trace)] in table order."""
        if len(tables) == 0:
            return []
        for t in tables:
            assert (t.getNumPyArray() if isinstance(t, TrackTable) else t).dtype == np.uint8
        em = np.ascontiguousarray(np.concatenate([self.emissionModel.allLogProbs(t) for t in tables]), dtype=np.float64)
        lens = [len(t) for t in tables]
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        al = None
        if alignmentTables is not None:
            assert len(alignmentTables) == len(tables)
            cols = []
            for a, n in zip(alignmentTables, lens):
                a = a.getNumPyArray() if isinstance(a, TrackTable) else np.asarray(a)
                assert a.dtype == np.uint16 and len(a) == n
                cols.append(a.reshape(n, -1)[:, 0])
            al = np.ascontiguousarray(np.concatenate(cols), dtype=np.uint16)
        n = len(tables)
        is_nest = np.zeros(self.M, dtype=np.uint8)
        is_nest[self.nestStates] = 1
        lp1, lp2 = _lib.as_f64(self.logProbs1), _lib.as_f64(self.logProbs2)
        priors, start = _lib.as_f64(self.pairEmissionModel.logPriors), _lib.as_f64(self.startProbs)
        scores = np.zeros(n, dtype=np.float64)
        top = np.zeros(n, dtype=np.int64)
        trace = np.zeros(int(offsets[-1]), dtype=np.float64)
        _lib.check(_lib.load().tehmm_cyk_decode(
            n, _lib.ptr(offsets, _lib.i64p), self.M, _lib.ptr(em, _lib.f64p), _lib.ptr(al, _lib.u16p),
            int(defAlignmentSymbol), _lib.ptr(is_nest, _lib.u8p), _lib.ptr(lp1, _lib.f64p), _lib.ptr(lp2, _lib.f64p),
            _lib.ptr(priors, _lib.f64p), _lib.ptr(start, _lib.f64p), _lib.ptr(scores, _lib.f64p),
            _lib.ptr(top, _lib.i64p), _lib.ptr(trace, _lib.f64p)), "tehmm_cyk_decode")
        return [(scores[t], trace[offsets[t]:offsets[t + 1]].copy()) for t in range(n)]

    def decode(self, obs, alignmentTrack=None, defAlignmentSymbol=0, numThreads=1):
        """(log probability of the best derivation, state of every column as float64), as in the HMM."""
        self.defAlignmentSymbol = defAlignmentSymbol
        return self._cyk([obs], None if alignmentTrack is None else [alignmentTrack], defAlignmentSymbol)[0]

    def viterbi(self, trackData, numThreads=1):
        """(score, states) per table of the TrackData (cfg.py:91-108): all tables in one device call."""
        alignmentTables = trackData.getAlignmentTrackTableList()
        if alignmentTables is not None and len(alignmentTables) == 0:
            alignmentTables = None
        self.defAlignmentSymbol = 0
        out = self._cyk(trackData.getTrackTableList(), alignmentTables, 0)
        if self.stateNameMap is not None:
            out = [(p, [self.stateNameMap.getMapBack(s) for s in states]) for p, states in out]
        return out

    # ---- training (cfg.py:306-346)
    def _tablesFromHmm(self, startprob, transmat):
        """The productions of a trained HMM: P(X -> X Y) = P(X -> Y X) = P(X -> Y) / 2 for a single state X, / 3 with
        P(X -> a Y a) the third share for a pair state (Y = X: the one or two productions keep the whole or half)."""
        assert self.startProbs.shape == np.shape(startprob)
        self.startProbs = np.asarray(myLog(np.asarray(startprob, dtype=np.float64)), dtype=np.float64)
        for lState in self.hmmStates:
            for rState in self.emittingStates:
                hp = transmat[lState, rState]
                if lState != rState:
                    hp = hp / 2.
                self.logProbs1[lState, lState, rState] = myLog(hp)
                self.logProbs1[lState, rState, lState] = myLog(hp)
        for lState in self.nestStates:
            for rState in self.emittingStates:
                hp = transmat[lState, rState]
                hp = hp / 3. if lState != rState else hp / 2.
                self.logProbs1[lState, lState, rState] = myLog(hp)
                self.logProbs1[lState, rState, lState] = myLog(hp)
                self.logProbs2[lState, rState] = myLog(hp)
        self.createHelperTables()

    def supervisedTrain(self, trackData, bedIntervals):
        """Production probabilities from how often two states are adjacent in the training intervals: the HMM's
        supervised training, its transitions then split over the productions."""
        self.trackList = trackData.getTrackList()
        self.initParams()
        hmm = MultitrackHmm(self.emissionModel)
        hmm.supervisedTrain(trackData, bedIntervals)
        self._tablesFromHmm(hmm.getStartProbs(), hmm.transmat_)

    def __str__(self):
        hmmStates, nestStates = [int(s) for s in self.hmmStates], [int(s) for s in self.nestStates]
        states = list(range(self.M))
        if self.stateNameMap is not None:
            states = [self.stateNameMap.getMapBack(s) for s in states]
            hmmStates = [self.stateNameMap.getMapBack(s) for s in self.hmmStates]
            nestStates = [self.stateNameMap.getMapBack(s) for s in self.nestStates]
        s = "\nNumStates = %d:\nSingle:%s\nPair:%s\n" % (self.M, str(hmmStates), str(nestStates))
        s += "\nStart probs =\n%s\n" % str([(states[i], self.startProbs[i]) for i in range(self.M)])
        s += "\nlogTable1 = \n%s\n" % str(self.logProbs1)
        s += "\nlogTable2 = \n%s\n" % str(self.logProbs2)
        em = self.emissionModel
        s += "\nNumber of symbols per track=\n%s\n" % str(em.getNumSymbolsPerTrack())
        s += "\nEmissions =\n"
        emProbs = em.getLogProbs()
        if self.trackList is None:                             # (an untrained model has no track names to print)
            return s
        for state, stateName in enumerate(hmmStates):          # (the reference, too, lists the single states only)
            s += "State %s:\n" % stateName
            for trackNo in range(em.getNumTracks()):
                track = self.trackList.getTrackByNumber(trackNo)
                s += "  Track %d %s (%s):\n" % (track.getNumber(), track.getName(), track.getDist())
                for idx, symbol in enumerate(em.getTrackSymbols(trackNo)):
                    symbolName = track.getValueMap().getMapBack(symbol)
                    prob = np.exp(emProbs[trackNo][state][symbol])
                    if idx <= 2 or prob > 0.01:
                        s += "    %s) %s: %f (log=%f)\n" % (symbol, symbolName, prob, myLog(prob))
        return s
