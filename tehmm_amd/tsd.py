"""The producer of the ``tsd`` track: bin/tsdFinder.py (on kmer.py), the overlap clean-up of
bin/removeBedOverlaps.py and their chain in bin/addTsdTrack.py's runTsdFinder.

The reference builds one Python k-mer table per candidate element and merges hit lists in the interpreter.  Here every
element is one lane of a device kernel (tehmm_tsd_find); the clean-up is a segmented running maximum and a compaction
(tehmm_remove_overlaps).  The host keeps what is bookkeeping: matching FASTA records to the chromosomes of the element
list, the name filters, and turning the columns that come back into the reference's 5-tuples
``(chrom, start, end, name, score)``.  Nothing falls back to a CPU implementation.

Differences from the reference, all deliberate:
  * sequences are passed as an ordered mapping name -> bases (readFasta makes one), intervals as lists of tuples;
  * a base other than ACGTNacgtn inside a searched window raises TeHmmHipError (the reference asserts);
  * a chromosome that reappears later in the element list raises ValueError (the reference asserts);
  * search windows are limited to 64 bases (left + overlap - 1, right + overlap - 1), --min to 21 as in the reference;
  * removeBedOverlaps sorts stably by (chromosome name as a string, start); bedtools' order among intervals of equal
    chromosome and start is not specified.
Not offered: --numProc (nothing to parallelise by hand), bigBed input, removeBedOverlaps --rm / --bed12, the XML
rewriting of addTsdTrack.
"""
import collections
import ctypes

import numpy as np

from . import _lib
from ._lib import i32p, i64p, ptr, u8p

NO_MAX_SCORE = -1


def readFasta(path):
    """OrderedDict name -> bases (bytes) of a FASTA file, as trackIO.fastaRead yields them: the name is the whole
    header line behind '>', lines starting with '#' are skipped, blanks and tabs dropped."""
    out = collections.OrderedDict()
    name, parts = None, []

    def close():
        if name is not None:
            seq = b"".join(parts)
            if seq.translate(None, b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz-"):
                raise RuntimeError("Invalid FASTA character found in input sequence %s" % name)
            out[name] = seq
    with open(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                close()
                name, parts = line[1:].rstrip(b"\r\n").decode(), []
            elif name is not None and not line.startswith(b"#"):
                parts.append(line.rstrip(b"\r\n").replace(b" ", b"").replace(b"\t", b""))
    close()
    return out


def _bases(x):
    if isinstance(x, str):
        x = x.encode()
    if isinstance(x, (bytes, bytearray, memoryview)):
        return np.frombuffer(x, dtype=np.uint8)
    a = np.asarray(x)
    assert a.dtype == np.uint8 and a.ndim == 1, "a sequence is bytes or a one-dimensional uint8 array"
    return a


# ---- array level ------------------------------------------------------------------------------------------------------
def findMatches(bases, seqOffsets, seqIndex, start, end, min=4, max=6, all=False, maxScore=None, left=7, right=7,
                overlap=3, _cap=None):
    """(counts [n] int32, columns [6][m] int64) of tehmm_tsd_find: the matches of element x are rows
    sum(counts[:x]) .. of the columns left start, left end, d1, right start, right end, d2."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    seqOffsets = np.ascontiguousarray(seqOffsets, dtype=np.int64)
    seqIndex = np.ascontiguousarray(seqIndex, dtype=np.int32)
    start = np.ascontiguousarray(start, dtype=np.int64)
    end = np.ascontiguousarray(end, dtype=np.int64)
    n = len(seqIndex)
    assert start.shape == end.shape == (n,) and seqOffsets.ndim == 1 and len(seqOffsets) >= 1
    assert len(bases) >= seqOffsets[-1]
    score = NO_MAX_SCORE if maxScore is None else (int(maxScore) if int(maxScore) >= 0 else -2)
    if len(bases) == 0:
        bases = np.zeros(1, dtype=np.uint8)
    counts = np.zeros(n, dtype=np.int32)
    n_out = ctypes.c_int64(0)
    cap = int(_cap) if _cap is not None else (4 * n if all else n)
    lib = _lib.load()
    for _ in range(2):
        cols = np.empty((6, cap), dtype=np.int64)
        _lib.check(lib.tehmm_tsd_find(
            len(seqOffsets) - 1, ptr(bases, u8p), ptr(seqOffsets, i64p), n, ptr(seqIndex, i32p), ptr(start, i64p),
            ptr(end, i64p), int(min), int(max), int(left), int(right), int(overlap), score, 1 if all else 0,
            ptr(counts, i32p), cap, *([ptr(cols[q], i64p) if cap else None for q in range(6)] +
                                      [ctypes.byref(n_out)])), "tehmm_tsd_find")
        if n_out.value <= cap:
            break
        cap = n_out.value
    return counts, cols[:, :n_out.value]


def removeOverlapsArrays(chromId, start, end, _cap=None):
    """(index, newStart) of the intervals tehmm_remove_overlaps keeps, for a list sorted by (chromId, start)."""
    chromId = np.ascontiguousarray(chromId, dtype=np.int32)
    start = np.ascontiguousarray(start, dtype=np.int64)
    end = np.ascontiguousarray(end, dtype=np.int64)
    n = len(chromId)
    assert start.shape == end.shape == (n,)
    cap = n if _cap is None else int(_cap)
    n_out = ctypes.c_int64(0)
    for _ in range(2):
        idx, ns = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.int64)
        _lib.check(_lib.load().tehmm_remove_overlaps(n, ptr(chromId, i32p), ptr(start, i64p), ptr(end, i64p), cap,
                                                     ptr(idx, i64p) if cap else None, ptr(ns, i64p) if cap else None,
                                                     ctypes.byref(n_out)), "tehmm_remove_overlaps")
        if n_out.value <= cap:
            break
        cap = n_out.value
    return idx[:n_out.value], ns[:n_out.value]


def lastTiming():
    """[(pass, milliseconds)] of the device passes of this thread's last tehmm_tsd_find / tehmm_remove_overlaps."""
    names = (ctypes.c_char_p * 16)()
    ms = (ctypes.c_double * 16)()
    n = _lib.load().tehmm_tsd_last_timing(16, names, ms)
    _lib.check(min(n, 0), "tehmm_tsd_last_timing")
    return [(names[i].decode(), ms[i]) for i in range(n)]


# ---- the host half of findTsds: what to search, and what the columns mean -----------------------------------------------
class TsdPlan(object):
    """The records that have elements, concatenated, and the elements in output order (FASTA record order, then list
    order): bases / seqOffsets / seqIndex / start / end as tehmm_tsd_find takes them, chroms[x] the chromosome
    field of element x's interval."""

    def __init__(self, bases, seqOffsets, seqIndex, start, end, chroms):
        self.bases, self.seqOffsets, self.seqIndex, self.start, self.end = bases, seqOffsets, seqIndex, start, end
        self.chroms = chroms

    def __len__(self):
        return len(self.seqIndex)


def buildSeqTable(bedIntervals):
    """chromosome -> (first, behind last) index in bedIntervals (tsdFinder.py:166-190); a chromosome that reappears
    after another raises ValueError."""
    table = collections.OrderedDict()
    prev, first = None, 0
    for i, iv in enumerate(bedIntervals):
        if iv[0] != prev:
            if iv[0] in table:
                raise ValueError("chromosome %r reappears at interval %d: the intervals must be grouped by chromosome"
                                 % (iv[0], i))
            if prev is not None:
                table[prev] = (first, i)
            table[iv[0]] = None
            prev, first = iv[0], i
    if prev is not None:
        table[prev] = (first, len(bedIntervals))
    return table


def planTsds(sequences, bedIntervals, names=None, sequenceNames=None):
    """TsdPlan of findTsds (tsdFinder.py:193-232).  A record serves the chromosome equal to its full name or, failing
    that, to the first whitespace-separated token of its name; records without elements are skipped; names /
    sequenceNames (comma-separated text or a collection) keep only intervals with such a name / such records."""
    split = lambda x: None if x is None else set(x.split(",") if isinstance(x, str) else x)
    nameSet, seqSet = split(names), split(sequenceNames)
    table = buildSeqTable(bedIntervals)
    n = len(bedIntervals)
    start = np.fromiter((iv[1] for iv in bedIntervals), dtype=np.int64, count=n)
    end = np.fromiter((iv[2] for iv in bedIntervals), dtype=np.int64, count=n)
    wanted = np.ones(n, dtype=bool) if nameSet is None else np.fromiter(
        ((iv[3] if len(iv) > 3 else None) in nameSet for iv in bedIntervals), dtype=bool, count=n)
    parts, offsets, picks, owner, chroms = [], [0], [], [], []
    for recName, seq in sequences.items():
        token = recName.split()[0] if recName.split() else recName
        if seqSet is not None and recName not in seqSet and token not in seqSet:
            continue
        seqName = recName if recName in table else token
        if seqName not in table:
            continue
        a, b = table[seqName]
        pick = a + np.flatnonzero(wanted[a:b])
        if len(pick) == 0:
            continue
        picks.append(pick)
        owner.append(np.full(len(pick), len(parts), dtype=np.int32))
        chroms.append(seqName)
        seq = _bases(seq)
        parts.append(seq)
        offsets.append(offsets[-1] + len(seq))
    if not parts:
        empty = np.zeros(0, dtype=np.int64)
        return TsdPlan(np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.int32), empty, empty, [])
    pick = np.concatenate(picks)
    return TsdPlan(np.concatenate(parts), np.asarray(offsets, dtype=np.int64), np.concatenate(owner), start[pick],
                   end[pick], chroms)


def matchTuples(plan, counts, cols, leftName="L_TSD", rightName="R_TSD", id=False):
    """The reference's output (matchesToBedInts, tsdFinder.py:300-323): two 5-tuples per match, left then right;
    with id both names end in _<n>, n counting the matches from 0 in output order."""
    m = cols.shape[1]
    chrom = [plan.chroms[s] for s in np.repeat(plan.seqIndex, counts).tolist()]
    ls, le, d1, rs, re, d2 = (c.tolist() for c in cols)
    if id:
        lname = ["%s_%d" % (leftName, k) for k in range(m)]
        rname = ["%s_%d" % (rightName, k) for k in range(m)]
    else:
        lname, rname = [leftName] * m, [rightName] * m
    out = [None] * (2 * m)
    out[0::2] = zip(chrom, ls, le, lname, d1)
    out[1::2] = zip(chrom, rs, re, rname, d2)
    return out


def writeBedIntervals(intervals, outPath):
    """``chrom\\tstart\\tend\\tname\\tscore`` lines of 5-tuples by the native BED writer (one call per run of a
    chromosome; the name column carries name and score)."""
    from .output import _write
    open(outPath, "w").close()
    n = len(intervals)
    if n == 0:
        return
    chrom = [iv[0] for iv in intervals]
    starts = np.fromiter((iv[1] for iv in intervals), dtype=np.int64, count=n)
    ends = np.fromiter((iv[2] for iv in intervals), dtype=np.int64, count=n)
    table = dict()
    code = np.fromiter((table.setdefault("%s\t%s" % (iv[3], iv[4]), len(table)) for iv in intervals), dtype=np.int64,
                       count=n)
    cuts = [0] + [i for i in range(1, n) if chrom[i] != chrom[i - 1]] + [n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        _write(outPath, True, chrom[a], starts[a:b], ends[a:b], states=code[a:b], names=list(table))


# ---- the reference's functions -----------------------------------------------------------------------------------------
def findTsds(sequences, bedIntervals, min=4, max=6, all=False, maxScore=None, left=7, right=7, overlap=3,
             leftName="L_TSD", rightName="R_TSD", id=False, names=None, sequenceNames=None, outBed=None):
    """bin/tsdFinder.py: the candidate TSDs flanking every interval, as the list of 5-tuples its findTsds returns
    (and, with outBed, as the BED it writes)."""
    plan = planTsds(sequences, bedIntervals, names, sequenceNames)
    tsds = []
    if len(plan) > 0:
        counts, cols = findMatches(plan.bases, plan.seqOffsets, plan.seqIndex, plan.start, plan.end, min=min, max=max,
                                   all=all, maxScore=maxScore, left=left, right=right, overlap=overlap)
        tsds = matchTuples(plan, counts, cols, leftName, rightName, id)
    if outBed is not None:
        writeBedIntervals(tsds, outBed)
    return tsds


def removeBedOverlaps(intervals):
    """bin/removeBedOverlaps.py: sorted (stably, by chromosome name as a string and start), every interval starts no
    earlier than the last kept interval of its chromosome ends, and intervals left empty are dropped."""
    intervals = sorted(intervals, key=lambda iv: (str(iv[0]), int(iv[1])))
    n = len(intervals)
    if n == 0:
        return []
    ids = dict()
    chrom = np.fromiter((ids.setdefault(str(iv[0]), len(ids)) for iv in intervals), dtype=np.int32, count=n)
    start = np.fromiter((iv[1] for iv in intervals), dtype=np.int64, count=n)
    end = np.fromiter((iv[2] for iv in intervals), dtype=np.int64, count=n)
    idx, ns = removeOverlapsArrays(chrom, start, end)
    return [(intervals[i][0], s) + tuple(intervals[i][2:]) for i, s in zip(idx.tolist(), ns.tolist())]


def tsdTrack(sequences, bedIntervals, existing=None, append=False, **options):
    """runTsdFinder of bin/addTsdTrack.py: the TSDs of bedIntervals, with append the intervals of the existing track
    behind them, sorted and cleaned of overlaps."""
    options.pop("outBed", None)
    tsds = findTsds(sequences, bedIntervals, **options)
    if append and existing:
        tsds = tsds + list(existing)
    return removeBedOverlaps(tsds)
