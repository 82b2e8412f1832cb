"""The step after a decode: judging a prediction against an annotation and naming the states after it
(bin/compareBedStates.py and bin/fitStateNames.py).

The reference counts bases in one interpreter iteration per base and walks both interval lists in Python.  Here the
counting half runs on the device, on interval lists (tehmm_intervals_check, tehmm_compare_base,
tehmm_compare_intervals, tehmm_merge_runs); the arithmetic on the small dicts that come out of it (summaries, the
state-name fit, the fitted BED) stays on the host.  The functions keep the reference's names, arguments and return
values; intervals are tuples ``(chrom, start, end, name[, score])`` as readBedIntervals returns them.

Differences from the reference, all deliberate:
  * checkExactOverlap takes interval lists, not BED paths (BED parsing is not part of this module), and checks BOTH
    lists for order and self-overlap; the reference reads bed1 twice and never looks at bed2's.
  * Chromosomes and states are numbered by first appearance (list 1, then list 2), so "sorted" means that a list
    never returns to a chromosome it has left, not that chromosome names ascend.
  * Where a result of the reference depends on the iteration order of a dict (equal truth sizes or equal F1 in
    getStateMapFromConfMatrix, equal counts in getStateMapFromConfMatrix_simple), this module goes by first
    insertion, as Python 3 does.  The dicts returned by the two comparisons carry their keys in the order in which
    the reference's walk inserts them: the device reports, per cell, where the pair first occurs.
  * summaryRow prints floats as Python 3 does.
--tl / --delMask: cut both lists with masking.cutPair(intervals1, intervals2, tracksXML, delMask) first; that is what
the two tools do before checkExactOverlap.
Not offered: --unique, --model (raises in the reference too), --hm, --plot, --window, BED file parsing, and a variant
that takes a batch's device-resident path.
"""
import ctypes
import itertools

import numpy as np

from . import _lib
from ._lib import i32p, i64p, ptr


class IntervalArrays(object):
    """One interval list as the device takes it: chrom int32, start int64, end int64, label int32."""

    def __init__(self, chrom, start, end, label):
        self.chrom = np.ascontiguousarray(chrom, dtype=np.int32)
        self.start = np.ascontiguousarray(start, dtype=np.int64)
        self.end = np.ascontiguousarray(end, dtype=np.int64)
        self.label = np.ascontiguousarray(label, dtype=np.int32)
        assert self.chrom.ndim == 1 and self.chrom.shape == self.start.shape == self.end.shape == self.label.shape

    def __len__(self):
        return len(self.chrom)

    def args(self):
        return (len(self), ptr(self.chrom, i32p), ptr(self.start, i64p), ptr(self.end, i64p), ptr(self.label, i32p))


def _number(table, key):
    n = table.get(key)
    if n is None:
        n = table[key] = len(table)
    return n


def encodeIntervals(intervals1, intervals2, col):
    """(arrays1, arrays2, chromNames, labelNames): the two lists as IntervalArrays over ONE chrom table and ONE label
    table (label = interval[col]), both numbered by first appearance, list 1 first.  intervals2 may be None."""
    chroms, labels = dict(), dict()
    out = []
    for intervals in (intervals1, intervals2):
        if intervals is None:
            out.append(None)
            continue
        n = len(intervals)
        c, lab = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        s, e = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
        for i, iv in enumerate(intervals):
            c[i] = _number(chroms, iv[0])
            s[i] = iv[1]
            e[i] = iv[2]
            lab[i] = _number(labels, iv[col])
        out.append(IntervalArrays(c, s, e, lab))
    return out[0], out[1], list(chroms), list(labels)


def pathIntervals(trackTable, states, names=None):
    """The interval list of a decoded table, one tuple (chrom, start, end, name) per row, from tehmm_bed_coords: a
    path can be compared without a text BED in between.  names: state number -> name (default: str of the number)."""
    from .output import bedCoords
    starts, ends = bedCoords(trackTable)
    states = np.asarray(states)
    assert states.shape == starts.shape
    chrom = trackTable.getChrom()
    name = (lambda k: str(k)) if names is None else (lambda k: names[k])
    return [(chrom, int(a), int(b), name(int(k))) for a, b, k in zip(starts, ends, states)]


# ---- array level: the four device calls ------------------------------------------------------------------------------
def checkArrays(a, b, L):
    """(which, where, message): which = 0 when both lists are valid and cover the same bases, else the list (1, 2)
    and the index of its first offending interval."""
    which, where = ctypes.c_int(0), ctypes.c_int64(-1)
    lib = _lib.load()
    _lib.check(lib.tehmm_intervals_check(*(a.args() + b.args() + (int(L), ctypes.byref(which),
                                                                   ctypes.byref(where)))), "tehmm_intervals_check")
    msg = lib.tehmm_last_error() if which.value else b""
    return which.value, where.value, (msg or b"").decode()


def baseConfusion(a, b, L, first=False):
    """conf [L][L] int64: conf[x][y] = bases labelled x in list a and y in list b.  With first, also the matrix of
    first occurrences (uint64: index in a << 32 | index in b of the first piece of the cell, all ones where none)."""
    conf = np.zeros((L, L), dtype=np.int64)
    seen = np.zeros((L, L), dtype=np.int64) if first else None
    _lib.check(_lib.load().tehmm_compare_base(*(a.args() + b.args() + (int(L), ptr(conf, i64p), ptr(seen, i64p)))),
               "tehmm_compare_base")
    return (conf, seen.view(np.uint64)) if first else conf


def intervalsOneSided(true, pred, L, threshold, usePredLen, allowMultiple, first=False):
    """(n_hit, len_hit, n_miss, len_miss, conf): the first four [L] by true label, conf[pred label][true label].  With
    first, a sixth: the first occurrence of every cell (uint64: true index << 32 | pred index, all ones where none)."""
    outs = [np.zeros(L, dtype=np.int64) for _ in range(4)]
    conf = np.zeros((L, L), dtype=np.int64)
    seen = np.zeros((L, L), dtype=np.int64) if first else None
    _lib.check(_lib.load().tehmm_compare_intervals(*(true.args() + pred.args() + (
        int(L), float(threshold), 1 if usePredLen else 0, 1 if allowMultiple else 0) + tuple(
            ptr(o, i64p) for o in outs) + (ptr(conf, i64p), ptr(seen, i64p)))), "tehmm_compare_intervals")
    return tuple(outs) + ((conf, seen.view(np.uint64)) if first else (conf,))


def mergeRuns(a, L, lut=None, _cap=None):
    """IntervalArrays of the merged list: labels through lut first, then neighbours of equal chrom and label that
    abut become one."""
    lut = None if lut is None else np.ascontiguousarray(lut, dtype=np.int32)
    assert lut is None or lut.shape == (L,)
    n_out = ctypes.c_int64(0)
    cap = len(a) if _cap is None else int(_cap)
    for _ in range(2):
        oc, ol = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
        os_, oe = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.int64)
        _lib.check(_lib.load().tehmm_merge_runs(*(a.args() + (int(L), ptr(lut, i32p), cap, ptr(oc, i32p),
                                                               ptr(os_, i64p), ptr(oe, i64p), ptr(ol, i32p),
                                                               ctypes.byref(n_out)))), "tehmm_merge_runs")
        if n_out.value <= cap:
            break
        cap = n_out.value
    n = n_out.value
    return IntervalArrays(oc[:n], os_[:n], oe[:n], ol[:n])


def lastTiming():
    """[(pass, milliseconds)] of this thread's last device call of this module."""
    names = (ctypes.c_char_p * 16)()
    ms = (ctypes.c_double * 16)()
    n = _lib.load().tehmm_compare_last_timing(16, names, ms)
    _lib.check(min(n, 0), "tehmm_compare_last_timing")
    return [(names[i].decode(), ms[i]) for i in range(n)]


# ---- the reference's functions ---------------------------------------------------------------------------------------
def checkExactOverlap(intervals1, intervals2):
    """compareBedStates.py:712-764 on interval lists: RuntimeError unless both lists are non-empty, sorted, free of
    self-overlap and cover exactly the same bases.  The message names the first offending interval."""
    if len(intervals1) == 0 or len(intervals2) == 0:
        raise RuntimeError("Interval lists cannot be compared. one or both inputs empty. ")
    a, b, _, labels = encodeIntervals([iv[:3] + (0,) for iv in map(tuple, intervals1)],
                                      [iv[:3] + (0,) for iv in map(tuple, intervals2)], 3)
    which, where, msg = checkArrays(a, b, len(labels))
    if which:
        bad = (intervals1 if which == 1 else intervals2)[where]
        raise RuntimeError("Interval lists cannot be compared. Interval %d of input%d, %s: %s.  Inputs must be both "
                           "sorted, cover the exact same region, and contain no self-overlaps." % (
                               where, which, str(tuple(bad)), msg))


def _first_seen(arrays):
    """labels of a list in the order of their first appearance"""
    vals, idx = np.unique(arrays.label, return_index=True)
    return [int(v) for v in vals[np.argsort(idx, kind="stable")]]


def _conf_dict(conf, seen, names, transpose):
    """{names[o]: {names[i]: cell}} of the non-zero cells (cell = conf[i][o] when transpose else conf[o][i]), keys in
    the order in which the reference's walk inserts them: by the first occurrence of the pair"""
    m, when = (conf.T, seen.T) if transpose else (conf, seen)
    o, i = np.nonzero(m)
    order = np.argsort(when[o, i], kind="stable")
    out = dict()
    for oo, ii in zip(o[order].tolist(), i[order].tolist()):
        out.setdefault(names[oo], dict())[names[ii]] = int(m[oo, ii])
    return out


def compareBaseLevel(intervals1, intervals2, col):
    """compareBedStates.py:176-221: (stats, confMat) with stats[state] = [bases of the state in list 1 only, in list 2
    only, in both] and confMat[state in list 2][state in list 1] = bases.  Keys come in the reference's order."""
    a, b, _, names = encodeIntervals(intervals1, intervals2, col)
    L = len(names)
    conf, seen = baseConfusion(a, b, L, first=True)
    diag = np.diagonal(conf)
    row, colsum = conf.sum(axis=1), conf.sum(axis=0)
    # a state enters stats at its first base, as the state of list 1 before the state of list 2
    entered = sorted(min((int(seen[k].min()), 0), (int(seen[:, k].min()), 1)) + (k,) for k in range(L))
    stats = dict()
    for _, _, k in entered:
        if row[k] or colsum[k]:
            stats[names[k]] = [int(row[k] - diag[k]), int(colsum[k] - diag[k]), int(diag[k])]
    return stats, _conf_dict(conf, seen, names, transpose=True)


def compareIntervalsOneSided(trueIntervals, predIntervals, col, threshold, usePredLenForThreshold,
                             allowMultipleMatches):
    """compareBedStates.py:223-313: (stats, confMat) with stats[true state] = [intervals hit, their bases (float),
    intervals missed, their bases (float)] and confMat[pred state][true state] = overlaps of at least threshold."""
    t, p, _, names = encodeIntervals(trueIntervals, predIntervals, col)
    L = len(names)
    n_hit, len_hit, n_miss, len_miss, conf, seen = intervalsOneSided(
        t, p, L, threshold, usePredLenForThreshold is True, allowMultipleMatches is True, first=True)
    stats = dict()
    for k in _first_seen(t):
        stats[names[k]] = [int(n_hit[k]), float(len_hit[k]), int(n_miss[k]), float(len_miss[k])]
    return stats, _conf_dict(conf, seen, names, transpose=False)


def summarizeBaseComparision(stats, ignore):
    """compareBedStates.py:315-329: (totalRight, totalWrong, {state: (precision, recall)})."""
    eps = np.finfo(float).eps
    totalRight, totalWrong, accMap = 0, 0, dict()
    for state, (fn, fp, tp) in stats.items():
        if state in ignore:
            continue
        totalRight += tp
        totalWrong += fn + fp
        accMap[state] = (float(tp) / (eps + float(tp) + float(fp)), float(tp) / (eps + float(tp) + float(fn)))
    return totalRight, totalWrong, accMap


def _side(stats, state, weighted):
    """(tp, fp, ratio) of one state on one side of the interval comparison"""
    tp, fp = stats[state][0], stats[state][2]
    if weighted is True:
        tp *= stats[state][1]
        fp *= stats[state][3]
    return tp, fp, (float(tp) / float(tp + fp) if tp + fp > 0 else 0.0)


def summarizeIntervalComparison(trueStats, predStats, weighted, ignore):
    """compareBedStates.py:331-387: {state: (precision, recall)} from the two one-sided comparisons, plus "Overall"
    over the states both sides know.  (The weighted totals are sums of whole numbers: their order does not matter
    below 2^53.)"""
    accMap = dict()
    states = [s for s in list(trueStats) + [s for s in predStats if s not in trueStats] if s not in ignore]
    tot = [0, 0, 0, 0]
    for state in states:
        both = state in trueStats and state in predStats
        recall = precision = 0.0
        if state in trueStats:
            tp, fp, recall = _side(trueStats, state, weighted)
            if both:
                tot[0] += tp
                tot[1] += fp
        if state in predStats:
            tp, fp, precision = _side(predStats, state, weighted)
            if both:
                tot[2] += tp
                tot[3] += fp
        accMap[state] = (precision, recall)
    totalRecall = float(tot[0]) / float(tot[0] + tot[1]) if tot[0] + tot[1] > 0 else 0.
    totalPrecision = float(tot[2]) / float(tot[2] + tot[3]) if tot[2] + tot[3] > 0 else 0.
    assert "Overall" not in accMap
    accMap["Overall"] = (totalPrecision, totalRecall)
    return accMap


def summaryRow(accuracy, stats, accMap):
    """compareBedStates.py:390-411: (header, row) of strings: totAcc, then precision, recall and F1 per state."""
    header, row = ["totAcc"], [accuracy]
    for state in sorted(accMap.keys()):
        prec, rec = accMap[state]
        header += ["%s_Prec" % state, "%s_Rec" % state, "%s_F1" % state]
        row += [prec, rec, 2 * ((prec * rec) / (rec + prec)) if prec > 0 and rec > 0 else 0]
    return header, [str(x) for x in row]


def getStateMapFromConfMatrix_simple(forwardMatrix):
    """compareBedStates.py:480-495: {pred state: (true state of the largest count, that count, total count)}; the
    first of equal counts wins."""
    stateMap = dict()
    for predName, counts in forwardMatrix.items():
        best = max(counts.values())
        stateMap[predName] = (next(k for k, v in counts.items() if v == best), best, sum(counts.values()))
    return stateMap


def _subsets(candidates, with_empty):
    if with_empty:
        yield ()
    for size in range(1, len(candidates) + 1):
        for subset in itertools.combinations(candidates, size):
            yield subset


def getStateMapFromConfMatrix(reverseMatrix, truthTgt, truthIgnore, predIgnore, thresh, fdr):
    """compareBedStates.py:497-610, the greedy F1 fit on reverseMatrix[truth state][pred state] = overlap: truth states
    by decreasing size take the set of still unmapped pred states that maximises F1.  A pred state is considered when
    overlap / min(truth size, pred size) >= thresh; at 1 - thresh and above it is a sure bet (always taken), below a
    candidate (every subset is tried; the first of equal F1 wins).  With fdr, the sure bets are the pred states with
    overlap / pred size >= 1 - fdr and there are no candidates.  Returns {pred: [truth, overlap, pred size]}."""
    truthSize, predSize = dict(), dict()
    for truth, row in reverseMatrix.items():
        for pred, overlap in row.items():
            truthSize[truth] = truthSize.get(truth, 0) + overlap
            predSize[pred] = predSize.get(pred, 0) + overlap
    stateMap = dict()
    for truth, size in sorted(truthSize.items(), key=lambda x: x[1], reverse=True):      # stable: ties keep their order
        if truth in truthIgnore or (len(truthTgt) > 0 and truth not in truthTgt):
            continue
        row = reverseMatrix[truth]
        candidates, sure, fdrSure = [], [], []
        for pred, overlap in row.items():
            if pred in stateMap or pred in predIgnore:
                continue
            frac = float(overlap) / float(min(size, predSize[pred]))
            if frac >= thresh:
                (sure if frac >= 1. - thresh else candidates).append(pred)
            if fdr is not None and float(overlap) / float(predSize[pred]) >= 1. - fdr:
                fdrSure.append(pred)
        if fdr is not None:
            candidates, sure = [], fdrSure
        bestF1, bestSet = -1., []
        for subset in _subsets(candidates, len(sure) > 0):
            chosen = list(subset) + sure
            tp, fp, fn, f1 = 0., 0., float(size), 0.
            bases = dict()
            for pred in chosen:
                tp += row[pred]
                fp += predSize[pred] - row[pred]
                fn -= row[pred]
                bases[pred] = tp + fp
            if tp > 0.:
                p, r = tp / (tp + fp), tp / (tp + fn)
                f1 = (2. * p * r) / (p + r)
            if f1 > bestF1:
                bestF1, bestSet = f1, sorted(chosen, reverse=True, key=lambda x: bases[x])
        for pred in bestSet:
            assert pred not in stateMap
            stateMap[pred] = [truth, row[pred], predSize[pred]]
    return stateMap


def filterStateMap(stateMap, args=None, ignore=None, qualThresh=None):
    """fitStateNames.py:198-231 without --unique, in place: a pred state that is ignored, or whose share
    count / total lies below qualThresh, maps to itself as (name, 1, 1).  Takes the reference's args object
    (.ignore, .qualThresh) or the two values."""
    if args is not None:
        if getattr(args, "unique", False):
            raise NotImplementedError("filterStateMap: --unique is not offered")
        ignore = args.ignore if ignore is None else ignore
        qualThresh = args.qualThresh if qualThresh is None else qualThresh
    ignore = () if ignore is None else ignore
    qualThresh = 0.1 if qualThresh is None else qualThresh
    for name, (mapName, mapCount, mapTotal) in list(stateMap.items()):
        if name in ignore or float(mapCount) / float(mapTotal) < qualThresh:
            stateMap[name] = (name, 1, 1)


def writeFittedBed(intervals, stateMap, outBed, col, noMerge, ignoreTgt):
    """fitStateNames.py:241-268: the intervals with column col renamed through stateMap (unless the new name is in
    ignoreTgt) and, without noMerge, abutting neighbours of equal chrom and new name merged (tehmm_merge_runs); a
    merged line keeps the other columns of its first interval.  outBed None: nothing is written.  Returns the
    fitted intervals."""
    fitted = []
    if len(intervals) > 0:
        a, _, chroms, names = encodeIntervals(intervals, None, col)
        L = len(names)
        index = dict((n, k) for k, n in enumerate(names))
        lut = np.arange(L, dtype=np.int32)
        for k in range(L):
            if names[k] in stateMap and stateMap[names[k]][0] not in ignoreTgt:
                lut[k] = _number(index, stateMap[names[k]][0])
        names = list(index)
        if noMerge:
            fitted = [tuple(iv[:col]) + (names[lut[k]],) + tuple(iv[col + 1:]) for iv, k in zip(intervals, a.label)]
        else:
            m = mergeRuns(a, L, lut)
            # the first interval of every run: where the mapped label, the chrom or the abutment breaks
            first = dict()
            if any(len(iv) != 4 for iv in intervals) or col != 3:
                for i in range(len(a) - 1, -1, -1):
                    first[(int(a.chrom[i]), int(a.start[i]))] = i
            for c, s, e, k in zip(m.chrom, m.start, m.end, m.label):
                if first:
                    iv = list(intervals[first[(int(c), int(s))]])
                    iv[2], iv[col] = int(e), names[k]
                    fitted.append(tuple(iv))
                else:
                    fitted.append((chroms[c], int(s), int(e), names[k]))
    if outBed is not None:
        with open(outBed, "w") as f:
            for iv in fitted:
                f.write("\t".join([str(x) for x in iv]) + "\n")
    return fitted


def fitStateNames(tgtIntervals, predIntervals, outBed=None, col=4, intThresh=None, noFrag=False, qualThresh=0.1,
                  ignore=(), ignoreTgt=(), tgt=(), old=False, fdr=None, noMerge=False):
    """bin/fitStateNames.py's main on interval lists: (stateMap, fitted intervals).  col counts from 1 as on the
    command line (4: name, 5: score).  The confusion matrix is the base-level one, or with intThresh the
    interval-level one (fragmented matches unless noFrag); by default it maps target states back to predicted ones
    and the greedy F1 fit (or the fdr cutoff) names the predicted states; with old the roles are swapped and every
    predicted state takes the target state of its largest count."""
    ignore, ignoreTgt, tgt = set(ignore), set(ignoreTgt), set(tgt)
    if old and tgt:
        raise RuntimeError("--tgt option not implemented for --old")
    if old and fdr is not None:
        raise RuntimeError("--old and --fdr options are exclusive")
    assert col == 4 or col == 5
    checkExactOverlap(tgtIntervals, predIntervals)
    first, second = (predIntervals, tgtIntervals) if old else (tgtIntervals, predIntervals)
    if intThresh is not None:
        confMat = compareIntervalsOneSided(second, first, col - 1, intThresh, False, not noFrag)[1]
    else:
        confMat = compareBaseLevel(second, first, col - 1)[1]
    if old:
        stateMap = getStateMapFromConfMatrix_simple(confMat)
    else:
        stateMap = getStateMapFromConfMatrix(confMat, tgt, ignoreTgt, ignore, qualThresh, fdr)
    filterStateMap(stateMap, ignore=ignore, qualThresh=qualThresh)
    return stateMap, writeFittedBed(predIntervals, stateMap, outBed, col - 1, noMerge, ignoreTgt)
