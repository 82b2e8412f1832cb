"""What the reference does with the mask tracks outside the HMM: cutOutMaskIntervals (bin/compareBedStates.py:680-710,
called by segmentTracks --delMask, compareBedStates --tl / --delMask, fitStateNames --tl and interpolateMaskedRegions
--cut) and bin/interpolateMaskedRegions.py.

The reference shells out to sortBed, mergeBed, subtractBed and intersectBed and walks the masks in the interpreter.
Here the interval algebra runs on the device (tehmm_intervals_merge, tehmm_intervals_subtract,
tehmm_intervals_intersect, tehmm_mask_fill); the host keeps the bookkeeping: numbering chromosomes and state names,
carrying the other columns of a record, sorting.  Nothing falls back to a CPU implementation.  Intervals are tuples
``(chrom, start, end[, name, ...])`` as in compare.py.

Where the three workflow places use it:
  * segmentTracks --delMask K:   region = cutOutMaskIntervals(allBed, K, None, tracksXML); merge it (mergeIntervals) and
    hand it to loadTrackData before segmentTracks;
  * compareBedStates --tl XML [--delMask K], fitStateNames --tl XML:   cutPair(bed1, bed2, XML, K) before
    compare.checkExactOverlap;
  * between the decode and the name fit:   interpolateMaskedRegions(...) or main().

Differences from the reference, all deliberate:
  * interval lists in and out instead of temporary files (a BED path is accepted where the reference takes one);
  * chromosomes are ordered by name (byte-wise, the order of sortBed), every sort is stable by (chrom, start): bedtools
    leaves the order among rows of equal (chrom, start) undefined, here input order holds;
  * records with end <= start are dropped, as track loading drops them;
  * subtractIntervals merges its second operand first (bedtools gives the same pieces either way);
  * a mask that overlaps a flanking interval without abutting it raises AssertionError naming the mask (the reference
    asserts without a message).
Kept from the reference: a mask behind the last predicted interval takes the interval BEFORE the last as its left flank
and has no right flank, so it gets the default; with cut the output holds the original rows of the prediction, not
the cut ones, so it has overlapping rows.
"""
import argparse
import ctypes
import re
import sys

import numpy as np

from . import _lib
from ._lib import i32p, i64p, ptr, u8p
from .common import logger

INT64_MAX = 2 ** 63 - 1
SKIPPED, DEFAULT = -2, -1      # what tehmm_mask_fill writes for a mask that is too long / that gets the default


# ---- array level: the four device calls ------------------------------------------------------------------------------
def _cols(c, s, e):
    c = np.ascontiguousarray(c, dtype=np.int32)
    s = np.ascontiguousarray(s, dtype=np.int64)
    e = np.ascontiguousarray(e, dtype=np.int64)
    assert c.ndim == 1 and c.shape == s.shape == e.shape
    return c, s, e


def mergeArrays(chrom, start, end, minLen=0, maxLen=INT64_MAX, _cap=None):
    """(chrom, start, end) of tehmm_intervals_merge for a list sorted by (chrom, start)."""
    c, s, e = _cols(chrom, start, end)
    n = len(c)
    cap = n if _cap is None else int(_cap)
    n_out = ctypes.c_int64(0)
    for _ in range(2):
        oc = np.empty(cap, dtype=np.int32)
        os_, oe = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.int64)
        _lib.check(_lib.load().tehmm_intervals_merge(
            n, ptr(c, i32p), ptr(s, i64p), ptr(e, i64p), int(minLen), int(maxLen), cap, ptr(oc, i32p) if cap else None,
            ptr(os_, i64p) if cap else None, ptr(oe, i64p) if cap else None, ctypes.byref(n_out)),
            "tehmm_intervals_merge")
        if n_out.value <= cap:
            break
        cap = n_out.value
    m = n_out.value
    return oc[:m], os_[:m], oe[:m]


def _pieces(name, a, b, _cap):
    ac, as_, ae = _cols(*a)
    bc, bs, be = _cols(*b)
    cap = len(ac) + len(bc) if _cap is None else int(_cap)
    n_out = ctypes.c_int64(0)
    fn = getattr(_lib.load(), name)
    for _ in range(2):
        src, os_, oe = (np.empty(cap, dtype=np.int64) for _ in range(3))
        _lib.check(fn(len(ac), ptr(ac, i32p), ptr(as_, i64p), ptr(ae, i64p), len(bc), ptr(bc, i32p), ptr(bs, i64p),
                      ptr(be, i64p), cap, ptr(src, i64p) if cap else None, ptr(os_, i64p) if cap else None,
                      ptr(oe, i64p) if cap else None, ctypes.byref(n_out)), name)
        if n_out.value <= cap:
            break
        cap = n_out.value
    m = n_out.value
    return src[:m], os_[:m], oe[:m]


def subtractArrays(a, b, _cap=None):
    """(src, start, end) of tehmm_intervals_subtract; a, b: (chrom, start, end) column triples, b sorted and disjoint."""
    return _pieces("tehmm_intervals_subtract", a, b, _cap)


def intersectArrays(a, b, _cap=None):
    """(src, start, end) of tehmm_intervals_intersect; a, b as in subtractArrays."""
    return _pieces("tehmm_intervals_intersect", a, b, _cap)


def fillArrays(masks, pred, label, L, twoSided=None, oneSided=None, onlyDefault=False, maxLen=INT64_MAX):
    """int32 [len(masks)] of tehmm_mask_fill: SKIPPED, DEFAULT or a label.  masks, pred: column triples; twoSided /
    oneSided: uint8 [L] flags or None (every label / none)."""
    mc, ms, me = _cols(*masks)
    pc, ps, pe = _cols(*pred)
    label = np.ascontiguousarray(label, dtype=np.int32)
    assert label.shape == pc.shape
    flags = []
    for f in (twoSided, oneSided):
        f = None if f is None else np.ascontiguousarray(f, dtype=np.uint8)
        assert f is None or f.shape == (L,)
        flags.append(f)
    out = np.empty(len(mc), dtype=np.int32)
    _lib.check(_lib.load().tehmm_mask_fill(
        len(mc), ptr(mc, i32p), ptr(ms, i64p), ptr(me, i64p), len(pc), ptr(pc, i32p), ptr(ps, i64p), ptr(pe, i64p),
        ptr(label, i32p), int(L), ptr(flags[0], u8p), ptr(flags[1], u8p), 1 if onlyDefault else 0, int(maxLen),
        ptr(out, i32p)), "tehmm_mask_fill")
    return out


def lastTiming():
    """[(pass, milliseconds)] of this thread's last device call of this module."""
    names = (ctypes.c_char_p * 16)()
    ms = (ctypes.c_double * 16)()
    n = _lib.load().tehmm_masking_last_timing(16, names, ms)
    _lib.check(min(n, 0), "tehmm_masking_last_timing")
    return [(names[i].decode(), ms[i]) for i in range(n)]


# ---- lists of tuples -------------------------------------------------------------------------------------------------
def chromTable(*lists):
    """name -> id over the chromosomes of the lists, ids in the byte-wise order of the names (the order of sortBed)."""
    names = set()
    for intervals in lists:
        names.update(iv[0] for iv in intervals)
    return dict((name, k) for k, name in enumerate(sorted(names, key=lambda x: str(x).encode())))


def encode(intervals, table):
    """(chrom, start, end) columns of a list over a chromTable"""
    n = len(intervals)
    return (np.fromiter((table[iv[0]] for iv in intervals), dtype=np.int32, count=n),
            np.fromiter((iv[1] for iv in intervals), dtype=np.int64, count=n),
            np.fromiter((iv[2] for iv in intervals), dtype=np.int64, count=n))


def labelTable(intervals, *nameSets):
    """name -> label over column 4 of the intervals (as str), then the names of the sets, by first appearance."""
    table = dict()
    for iv in intervals:
        table.setdefault(str(iv[3]), len(table))
    for names in nameSets:
        for name in sorted(names):
            table.setdefault(str(name), len(table))
    return table


def sortIntervals(intervals):
    """the list sorted stably by (chrom, start), chromosomes by name; the list itself (as tuples) when it is sorted"""
    intervals = [(iv[0], int(iv[1]), int(iv[2])) + tuple(iv[3:]) for iv in intervals]
    key = lambda iv: (str(iv[0]).encode(), iv[1])
    if all(key(a) <= key(b) for a, b in zip(intervals, intervals[1:])):
        return intervals
    return sorted(intervals, key=key)


def mergeIntervals(intervals, minLength=None, maxLength=None):
    """sortBed | mergeBed | filterBedLengths: (chrom, start, end) of the runs of overlapping or abutting intervals
    whose length lies in [minLength, maxLength] (None: no limit).  Records with end <= start are dropped."""
    intervals = sortIntervals([iv for iv in intervals if int(iv[2]) > int(iv[1])])
    if len(intervals) == 0:
        return []
    table = chromTable(intervals)
    names = list(table)
    c, s, e = mergeArrays(*encode(intervals, table), minLen=0 if minLength is None else minLength,
                          maxLen=INT64_MAX if maxLength is None else maxLength)
    return [(names[k], a, b) for k, a, b in zip(c.tolist(), s.tolist(), e.tolist())]


def _carry(a, pieces):
    src, s, e = (x.tolist() for x in pieces)
    return [(a[i][0], x, y) + tuple(a[i][3:]) for i, x, y in zip(src, s, e)]


def subtractIntervals(a, b):
    """subtractBed -a a -b b: for every record of a, in a's order, its parts that no record of b covers, with the other
    columns of the record.  b is merged first."""
    a = [tuple(iv) for iv in a if int(iv[2]) > int(iv[1])]
    b = mergeIntervals(b) if len(a) > 0 else []
    if len(b) == 0:
        return a
    table = chromTable(a, b)
    return _carry(a, subtractArrays(encode(a, table), encode(b, table)))


def intersectIntervals(a, b):
    """intersectBed -a a -b b: for every record of a, in a's order, its part inside every record of b that overlaps
    it, with the other columns of the record.  b is sorted if needed and must not overlap itself."""
    a = [tuple(iv) for iv in a if int(iv[2]) > int(iv[1])]
    b = sortIntervals([iv for iv in b if int(iv[2]) > int(iv[1])])
    if len(a) == 0 or len(b) == 0:
        return []
    table = chromTable(a, b)
    return _carry(a, intersectArrays(encode(a, table), encode(b, table)))


def _track_list(trackList):
    if isinstance(trackList, str):
        from .track import readTrackList
        return readTrackList(trackList)
    return trackList


def _mask_records(trackList):
    return [iv for t in trackList.getMaskTracks() for iv in _bed_tuples(t.getPath(), 3)]


def _bed_tuples(path, ncol):
    """(chrom, int start, int end) + the text of columns 3 .. ncol - 1 (None: all) of the records of a BED file"""
    from .trackIO import parseBed
    cols = parseBed(path)
    if cols.intsCertified():
        return cols.tuples(ncol)
    return [(r[0], int(r[1]), int(r[2])) + tuple(r[3:ncol]) for r in cols.fields]


def maskIntervals(trackList):
    """All records of the BED files of all mask tracks of a TrackList (or XML path), merged."""
    return mergeIntervals(_mask_records(_track_list(trackList)))


def readBed(path):
    """the records of a BED file as tuples (chrom, int start, int end, other fields as text ...)"""
    return _bed_tuples(path, None)


def writeBed(intervals, path):
    with open(path, "w") as f:
        for iv in intervals:
            f.write("\t".join([str(x) for x in iv]) + "\n")


def cutOutMaskIntervals(intervals, minLength, maxLength, tracksInfo):
    """compareBedStates.py:680-710 on lists: the intervals (a list, or a BED path whose columns are all kept) minus the
    merged records of the mask tracks whose length lies in [minLength + 1, maxLength - 1] (maxLength None: no upper
    limit), sorted stably by (chrom, start).  None when the track list (a TrackList or an XML path) has no mask
    track; RuntimeError when nothing is left."""
    trackList = _track_list(tracksInfo)
    if len(trackList.getMaskTracks()) == 0:
        return None
    if isinstance(intervals, str):
        intervals = readBed(intervals)
    masks = mergeIntervals(_mask_records(trackList), minLength + 1, None if maxLength is None else maxLength - 1)
    out = sortIntervals(subtractIntervals(intervals, masks))
    if len(out) == 0:
        raise RuntimeError("cutOutMaskIntervals removed everything.  Can't continue."
                           " probably best to rerun calling script on bigger region?")
    return out


def cutPair(intervals1, intervals2, tracksInfo, delMask=-1):
    """What compareBedStates --tl [--delMask] and fitStateNames --tl do before checkExactOverlap: both lists with the
    masks longer than delMask cut out, or both untouched when the track list has no mask track."""
    trackList = _track_list(tracksInfo)
    cut1 = cutOutMaskIntervals(intervals1, delMask, None, trackList)
    if cut1 is None:
        return intervals1, intervals2
    return cut1, cutOutMaskIntervals(intervals2, delMask, None, trackList)


def _name_set(x):
    if x is None:
        return set()
    return set(x.split(",")) if isinstance(x, str) else set(str(k) for k in x)


def fillMasks(masks, flank, default="0", tgts=None, oneSidedTgts=None, onlyDefault=False, maxLen=None):
    """The loop of interpolateMaskedRegions.py:117-162: (chrom, start, end, state) for every mask (merged, sorted) not
    longer than maxLen, from the flank list (4 columns, sorted by (chrom, start, end))."""
    tgtSet, oneSet = _name_set(tgts), _name_set(oneSidedTgts)
    if len(masks) == 0 or len(flank) == 0:
        return []
    labels = labelTable(flank, tgtSet, oneSet)
    names = list(labels)
    L = len(names)
    flags = lambda chosen: np.fromiter((name in chosen for name in names), dtype=np.uint8, count=L)
    table = chromTable(masks, flank)
    label = np.fromiter((labels[str(iv[3])] for iv in flank), dtype=np.int32, count=len(flank))
    try:
        got = fillArrays(encode(masks, table), encode(flank, table), label, L, flags(tgtSet) if tgtSet else None,
                         flags(oneSet), onlyDefault, INT64_MAX if maxLen is None else maxLen)
    except _lib.TeHmmHipError as err:
        hit = re.search(r"mask (\d+) overlaps", str(err))
        if hit is None:
            raise
        raise AssertionError("mask interval %s overlaps a flanking interval of the prediction without abutting it"
                             % str(tuple(masks[int(hit.group(1))][:3])))
    return [tuple(m[:3]) + (str(default) if k == DEFAULT else names[k],) for m, k in zip(masks, got.tolist())
            if k != SKIPPED]


def interpolateMaskedRegions(trackList, allIntervals, inIntervals, maxLen=None, default="0", tgts=None,
                             oneSidedTgts=None, onlyDefault=False, cut=False):
    """bin/interpolateMaskedRegions.py on lists: the prediction inIntervals plus one row (chrom, start, end, state) for
    every merged mask not longer than maxLen, sorted and clipped to the merged allIntervals.  The state of a mask comes
    from the intervals that abut it (fillMasks); with cut the flanks are looked up in the prediction with those masks
    cut out, but the rows of the output are still the original ones.  All columns of inIntervals are kept.

    Order: stable by (chrom, start); among rows of equal (chrom, start) the original rows come before the fills and
    input order holds otherwise (bedtools leaves that order undefined)."""
    tgtSet, oneSet = _name_set(tgts), _name_set(oneSidedTgts)
    assert len(tgtSet.intersection(oneSet)) == 0
    trackList = _track_list(trackList)
    inIntervals = [tuple(iv) for iv in inIntervals]
    noMasks = len(trackList.getMaskTracks()) == 0
    pred = inIntervals
    if cut and not noMasks and len(inIntervals) > 0:
        pred = cutOutMaskIntervals(inIntervals, -1, None if maxLen is None else maxLen + 1, trackList)
    flank = sorted((iv[:4] for iv in sortIntervals(pred)), key=lambda iv: (str(iv[0]).encode(), iv[1], iv[2]))
    if noMasks or len(flank) == 0:
        logger.warning("No mask tracks located in track list or prediction empty")
        return inIntervals
    fills = fillMasks(maskIntervals(trackList), flank, default, tgtSet, oneSet, onlyDefault, maxLen)
    return intersectIntervals(sortIntervals(inIntervals + fills), mergeIntervals(allIntervals))


def parseArgs(argv):
    parser = argparse.ArgumentParser(
        formatter_class=argparse.ArgumentDefaultsHelpFormatter,
        description="Fill in masked intervals of an hmm prediction with state corresponding to surrounding intervals.")
    parser.add_argument("tracksXML", help="XML track list (used to id masking tracks")
    parser.add_argument("allBed", help="Target scope.  Masked intervals outside of these regions will not be included")
    parser.add_argument("inBed", help="TE prediction BED file")
    parser.add_argument("outBed", help="Output BED: the input plus the filled gaps")
    parser.add_argument("--maxLen", help="Maximum length of a masked interval to fill (inclusive)", type=int,
                        default=None)
    parser.add_argument("--default", help="Label of a masked region whose label cannot be determined", default="0")
    parser.add_argument("--tgts", help="Only relabel gaps flanked on both sides by the same state of this "
                        "comma-separated list (default: any state)", default=None)
    parser.add_argument("--oneSidedTgts", help="Relabel gaps flanked on at least one side by a state of this "
                        "comma-separated list", default=None)
    parser.add_argument("--onlyDefault", help="Give every masked gap the default state", action="store_true",
                        default=False)
    parser.add_argument("--cut", help="Cut the masked gaps out of the input before looking for flanks",
                        action="store_true", default=False)
    return parser.parse_args(argv)


def main(argv=None):
    """The command line of bin/interpolateMaskedRegions.py: tracksXML allBed inBed outBed [options]."""
    args = parseArgs(sys.argv[1:] if argv is None else argv)
    out = interpolateMaskedRegions(args.tracksXML, readBed(args.allBed), readBed(args.inBed), maxLen=args.maxLen,
                                   default=args.default, tgts=args.tgts, oneSidedTgts=args.oneSidedTgts,
                                   onlyDefault=args.onlyDefault, cut=args.cut)
    writeBed(out, args.outBed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
