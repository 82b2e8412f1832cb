"""Track segmentation (bin/segmentTracks.py): the segments of unsegmented track tables.

A segment is a run of rows that the HMM treats as one observation.  Row i of a table opens a new segment when it
differs from the first row of the running segment (``comp="first"``; from row i - 1 with ``comp="prev"``) in a cut
track or in more than ``thresh`` tracks, when the segment has reached ``maxLen`` rows, or -- with ``fixLen`` -- simply
every ``fixLen`` rows.  The chain over the rows runs on the device (tehmm_segment_offsets_u8);
all tables go in one call.

    intervals = segmentTracks(trackData, "segments.bed", thresh=1)
    for table in trackData.getTrackTableList():
        table.segment(intervals, trackData.getTrackList())

--delMask K (masks longer than K removed from the region, so that they break contiguity): cut the region before the
tables are loaded --
    region = masking.cutOutMaskIntervals(allBed, K, None, tracksXML)      # None: the track list has no mask track
    trackData.loadTrackData(tracksXML, masking.mergeIntervals(region))
and call segmentTracks on that trackData.
"""
import ctypes
import logging

import numpy as np

from . import _lib
from ._lib import i64p, ptr, u8p

logger = logging.getLogger(__name__)


def resolveCutLists(trackList, cutTracks=None, ignore="sequence", cutUnscaled=False, cutMultinomial=False,
                    cutNonGaussian=False):
    """The cut and ignore vectors of segmentTracks.py:125-188, in its order: --cutTracks, mask tracks (always cut),
    --ignore (naming a cut track is an error), then --cutUnscaled / --cutMultinomial / --cutNonGaussian on the tracks
    that are not ignored.  cutTracks and ignore are comma-separated names or None.  A Track attribute this package's
    Track does not carry (scale, shift, logScale) reads as None.  Returns (cut, ignore) as uint8 arrays."""
    n = len(trackList)
    cut = np.zeros(n, dtype=np.uint8)
    if cutTracks is not None:
        for name in cutTracks.split(","):
            track = trackList.getTrackByName(name)
            if track is None:
                raise RuntimeError("cutTrack %s not found" % name)
            cut[track.getNumber()] = 1
    for track in trackList:
        if track.getDist() == "mask":
            cut[track.getNumber()] = 1
    ign = np.zeros(n, dtype=np.uint8)
    if ignore is not None:
        for name in ignore.split(","):
            track = trackList.getTrackByName(name)
            if track is None:
                if name != "sequence":
                    logger.warning("ignore track %s not found" % name)
                continue
            ign[track.getNumber()] = 1
            if cut[track.getNumber()] == 1:
                raise RuntimeError("Same track (%s) cant be cut and ignored" % name)
    for track in trackList:
        k = track.getNumber()
        if ign[k]:
            continue
        unscaled = all(getattr(track, a, None) is None for a in ("scale", "shift", "logScale"))
        if (cutUnscaled and unscaled) or (cutMultinomial and track.getDist() == "multinomial") or \
                (cutNonGaussian and track.getDist() != "gaussian"):
            cut[k] = 1
    return cut, ign


def _table_data(table):
    if hasattr(table, "getSegmentOffsets"):
        if table.getSegmentOffsets() is not None:
            raise ValueError("segmentOffsets: the table is already segmented")
        table = table.getNumPyArray()
    a = np.asarray(table)
    if a.dtype != np.uint8:
        raise TypeError("segmentOffsets: uint8 tables only (got %s)" % a.dtype)
    if a.ndim != 2 or a.shape[0] < 1:
        raise ValueError("segmentOffsets: a table is a [T >= 1][K] array")
    return a


def segmentOffsets(tables, cut, ignore, thresh=1, comp="first", maxLen=0, fixLen=0, stats=False, _cap=None):
    """Segment offsets of every table: a list of int64 arrays, one per table, each starting with 0; segment n of a
    table covers rows [offsets[n], offsets[n + 1]) and the last one runs to the table's end.  tables: TrackTables or
    [T][K] uint8 arrays.  With stats, also returns (count[K], share[K]): count[j] = number of cuts made by the data
    rule at which track j differed, share[j] = sum over those cuts of 1 / (number of differing tracks)."""
    if comp != "first" and comp != "prev":
        raise RuntimeError("--comp must be either first or prev")
    arrs = [_table_data(t) for t in tables]
    if not arrs:
        return ([], (np.zeros(0, np.int64), np.zeros(0))) if stats else []
    K = arrs[0].shape[1]
    if any(a.shape[1] != K for a in arrs):
        raise ValueError("segmentOffsets: tables differ in their number of tracks")
    cut = np.ascontiguousarray(np.asarray(cut) != 0, dtype=np.uint8)
    ign = np.ascontiguousarray(np.asarray(ignore) != 0, dtype=np.uint8)
    if cut.shape != (K,) or ign.shape != (K,):
        raise ValueError("segmentOffsets: cut and ignore hold one entry per track")
    offs = np.concatenate([[0], np.cumsum([a.shape[0] for a in arrs])]).astype(np.int64)
    data = np.ascontiguousarray(arrs[0] if len(arrs) == 1 else np.concatenate(arrs, axis=0))
    n_cuts = np.zeros(len(arrs), dtype=np.int64)
    n_total = ctypes.c_int64(0)
    hist = np.zeros((K, K + 1), dtype=np.uint64) if stats else None
    lib = _lib.load()
    # first guess: a cut every 8 rows (the call reports what it needs when that is too small)
    cap = int(_cap) if _cap is not None else int(offs[-1]) // 8 + len(arrs) + 1024
    for _ in range(2):
        cuts = np.empty(cap, dtype=np.int64)
        _lib.check(lib.tehmm_segment_offsets_u8(
            len(arrs), ptr(offs, i64p), K, ptr(data, u8p), ptr(ign, u8p), ptr(cut, u8p), int(thresh),
            1 if comp == "prev" else 0, int(maxLen), int(fixLen), cap, ptr(cuts, i64p), ptr(n_cuts, i64p),
            ctypes.byref(n_total), None if hist is None else hist.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))),
            "tehmm_segment_offsets_u8")
        if n_total.value <= cap:
            break
        cap = int(n_total.value)
    bounds = np.concatenate([[0], np.cumsum(n_cuts)])
    out = [cuts[bounds[t]:bounds[t + 1]].copy() for t in range(len(arrs))]
    if not stats:
        return out
    count = hist.sum(axis=1).astype(np.int64)
    share = np.zeros(K, dtype=np.float64)
    for dif in range(1, K + 1):                              # ascending dif
        share += hist[:, dif].astype(np.float64) / float(dif)
    return out, (count, share)


def lastCounters():
    """(stripes, stripes_rewalked) of this thread's last segmentOffsets call."""
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().tehmm_segment_last_counters(ctypes.byref(a), ctypes.byref(b)), "tehmm_segment_last_counters")
    return a.value, b.value


def lastTiming():
    """[(pass, milliseconds)] of this thread's last segmentOffsets call (HIP events around the device passes)."""
    names = (ctypes.c_char_p * 16)()
    ms = (ctypes.c_double * 16)()
    n = _lib.load().tehmm_segment_last_timing(16, names, ms)
    _lib.check(min(n, 0), "tehmm_segment_last_timing")
    return [(names[i].decode(), ms[i]) for i in range(n)]


def writeSegmentsBed(path, chrom, starts, ends, first_label=0, append=False):
    """BED lines chrom, start, end, hex label (first_label, first_label + 1, ...) by the native writer."""
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    ends = np.ascontiguousarray(ends, dtype=np.int64)
    assert starts.shape == ends.shape and starts.ndim == 1
    _lib.check(_lib.load().tehmm_write_segments_bed(str(path).encode(), 1 if append else 0, str(chrom).encode(),
                                                    len(starts), ptr(starts, i64p), ptr(ends, i64p),
                                                    int(first_label)), "tehmm_write_segments_bed")


def segmentTracks(trackData, outBed, thresh=1, cutTracks=None, cutUnscaled=False, cutMultinomial=False,
                  cutNonGaussian=False, comp="first", ignore="sequence", maxLen=0, fixLen=0, co=0, statsPath=None):
    """bin/segmentTracks.py on loaded tracks: writes the segment BED ``chrom\\tstart\\tend\\t<hex label>`` (labels count
    on from ``co`` across the tables) and, with statsPath, the --stats file ``name\\tcount\\t%f`` of share / count for
    every track with count > 0.  The stats lines are in ascending track number; the reference writes them in the
    order of a Python 2 dict keyed by track number, which is the same for small numbers but is not promised.
    Returns the segment intervals [(chrom, start, end)] in the form TrackTable.segment takes."""
    tables = trackData.getTrackTableList()
    trackList = trackData.getTrackList()
    cut, ign = resolveCutLists(trackList, cutTracks, ignore, cutUnscaled, cutMultinomial, cutNonGaussian)
    res = segmentOffsets(tables, cut, ign, thresh=thresh, comp=comp, maxLen=maxLen, fixLen=fixLen,
                         stats=statsPath is not None)
    offsets, st = res if statsPath is not None else (res, None)
    intervals = []
    label = int(co)
    for n, (table, offs) in enumerate(zip(tables, offsets)):
        start, end = int(table.getStart()), int(table.getEnd())
        starts = start + offs
        ends = np.concatenate([starts[1:], [end]]).astype(np.int64)
        writeSegmentsBed(outBed, table.getChrom(), starts, ends, first_label=label, append=n > 0)
        label += len(starts)
        chrom = table.getChrom()
        intervals.extend(zip([chrom] * len(starts), starts.tolist(), ends.tolist()))
    if not tables:
        open(outBed, "w").close()
    if statsPath is not None:
        count, share = st
        with open(statsPath, "w") as f:
            for k in range(len(count)):
                if count[k] > 0:
                    f.write("%s\t%d\t%f\n" % (trackList.getTrackByNumber(k).getName(), count[k],
                                              float(share[k]) / float(count[k])))
    return intervals
