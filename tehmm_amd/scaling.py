"""Track scaling: the scale / logScale / shift attributes of numeric tracks (bin/setTrackScaling.py of the reference;
DESIGN.md section 5p).

The reference paints every base of the genome into a float32 array per track in the interpreter, strips the bases no
record covers in a second per-base loop, and computes two histograms of the result.  It never takes the delta branch of
readBedData (it passes the bound method ``track.getDelta`` as useDelta, which ``is not True``; kept here), so a base's
value is the value of the record that wins it, and every statistic of the array is a statistic of the record list
weighted by the rows each record wins.  The device counts those rows (tehmm_track_rows_won); setTrackScale works from
(distinct record values, rows won, uncovered rows, default) and never builds the array.  readTrackIntoFloatArray builds
it with the float paint (tehmm_load_tracks_f32) for those who want it.

Arithmetic: computeScale of the reference mixes float32 scalars with Python floats, so its result depends on NumPy's
promotion rules; the rule here is what the reference returns under NumPy 2 (NEP 50), written with explicit dtypes:
  range = maxVal - minVal                                float32
  binSize = float(range) / float(numBins - 2)            float64 (Python floats)
  minBin = floor(minVal / f32(binSize)) * f32(binSize)   float32, as are all linear edges (edge + f32(binSize))
  linearScale = 1 / binSize                              float64
  shift = f32(1) - minVal when minVal <= 0               float32; data, minVal, maxVal += shift in float32
  ratio = float(maxVal) / float(minVal)                  float64
  logBase = ratio ** (1 / (numBins - 2))                 float64
  minBin = logBase ** floor(f64(log_f32(minVal)) / log(logBase))    the logarithm of minVal is taken in float32
  log edges: edge * logBase                              float64
Bins are np.histogram's: e[b] <= x < e[b + 1] compared in double, the last bin closed on the right, values outside
dropped.  The variance is np.var of the counts as float64.

Differences from the reference, deliberate: a value that is not finite raises ValueError naming the track (main skips
the track, as for text that is no number); main takes its arguments from argv (the reference ignores the parameter).
Kept quirks: shift is always written (0.0 with a linear scale); scaleParam is rounded to 4 decimals only above 1e-4;
nothing changes when the array has numBins values or fewer; the assertions of histVariance -- a track whose values are
all equal (valCol 0 without a default) has binSize 0 and NaN edges and ends in the first of them, an AssertionError
that main does not catch, as in the reference (which also prints NumPy's division warning; not repeated here).
Not offered: applyTrackScaling / scaleVals (CategoryMap applies the attributes at load time), bigWig.
"""
import argparse
import os
import sys

import numpy as np

from . import trackIO
from .common import logger
from .track import readTrackList

FLOAT_MAX = np.finfo(np.float32).max


def trackRecords(track, allIntervals, source=None):
    """The records of a track over the intervals (chrom, start, end) laid end to end: (T, start, end, float32 value),
    in row coordinates and sorted by start.  ValueError for text that is no number or a value that is not finite."""
    source = source or trackIO.TrackSource(track.getPath())
    if source.bed is None:
        raise ValueError("track %s: %s is not a BED file" % (track.getName(), track.getPath()))
    parts, offset = [], 0
    for iv in allIntervals:
        chrom, s, e = iv[0], int(iv[1]), int(iv[2])
        pick, oStart, oEnd = source.bed.select(chrom, s, e)
        parts.append((oStart - s + offset, oEnd - s + offset,
                      trackIO.recordValues(source.bed, pick, track.getValCol(), track.getName())))
        offset += e - s
    cols = [np.concatenate(c) for c in zip(*parts)] if parts else [np.zeros(0, np.int64)] * 2 + [np.zeros(0, np.float32)]
    return offset, cols[0], cols[1], cols[2].astype(np.float32)


def _default(track):
    """(has a default, the value of the bases no record covers) as readTrackIntoFloatArray of the reference"""
    defaultVal = track.getDefaultVal()
    if defaultVal is None:
        return False, FLOAT_MAX
    defaultVal = np.float32(defaultVal)
    assert defaultVal != FLOAT_MAX
    assert not np.isinf(defaultVal)
    return True, defaultVal


def readTrackIntoFloatArray(track, allIntervals):
    """The whole track as one float32 array, a value per base of the intervals.  With a default the bases no record
    covers hold it; without, they are dropped, and so are bases whose value is the largest float32 (the reference marks
    uncovered bases with it)."""
    hasDefault, fill = _default(track)
    T, start, end, val = trackRecords(track, allIntervals)
    data = trackIO.paintTracksFloat(T, [trackIO.FloatTrack(fill, start, end, val)])[0]
    return data if hasDefault else data[data != FLOAT_MAX]


def trackWeights(track, allIntervals):
    """(distinct values: float32, ascending; bases holding each: int64) of the array readTrackIntoFloatArray returns,
    without the array: the rows every record wins, summed per distinct value."""
    hasDefault, fill = _default(track)
    T, start, end, val = trackRecords(track, allIntervals)
    won, uncovered = trackIO.rowsWon(T, [trackIO.FloatTrack(fill, start, end, val)])
    val, won = val[won[0] > 0], won[0][won[0] > 0]
    if hasDefault:
        val, won = np.append(val, fill), np.append(won, uncovered[0])
    else:
        marked = val == FLOAT_MAX
        val, won = val[~marked], won[~marked]
    values, inv = np.unique(val, return_inverse=True)
    weights = np.zeros(len(values), dtype=np.int64)
    np.add.at(weights, inv.reshape(-1), won.astype(np.int64))
    return values[weights > 0].astype(np.float32), weights[weights > 0]


def _histogram(data, weights, edges):
    """(counts per bin: int64, weight below edges[0] or NaN-free above edges[-1]) with np.histogram's bins"""
    x = np.asarray(data, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float64)
    b = np.searchsorted(e, x, side="right") - 1
    b[x == e[-1]] = len(e) - 2
    inside = (x >= e[0]) & (x <= e[-1])
    freq = np.zeros(len(e) - 1, dtype=np.int64)
    np.add.at(freq, b[inside], weights[inside])
    return freq, int(weights[~inside].sum())


def histVariance(data, bins, fromLog=False, weights=None, counts=None):
    """Variance of the histogram counts as a proxy for the quality of the binning.  data with weights: distinct values
    and how often each occurs.  The two assertions of the reference: every value lies inside the bins; or, for log bins
    above 0, inside [0, last edge].  counts: a list that takes the count vector."""
    data = np.asarray(data)
    weights = np.ones(len(data), dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    bins = np.asarray(bins)
    freq, outside = _histogram(data, weights, bins)
    if bins[0] <= 0 or fromLog is False:
        assert outside == 0, "%d values outside the bins %s (all values equal? then there is nothing to scale)" % (
            outside, bins.tolist())
    else:
        tempBins = np.zeros(len(bins) + 1, dtype=np.float64)
        tempBins[1:] = bins
        assert _histogram(data, weights, tempBins)[1] == 0
    if counts is not None:
        counts.append(freq)
    return np.var(freq.astype(np.float64))


def computeScale(data, numBins, noLog, weights=None, counts=None):
    """(scaleType, scaleParam, shift) of the reference's heuristic: the linear or the logarithmic binning into numBins
    symbols whose counts vary less.  data: float32 values; weights: how often each occurs (None: once).  Unlike the
    reference, data is not shifted in place.  Dtypes as in the module docstring.  counts: a list that takes the count
    vectors of the linear and of the logarithmic histogram."""
    f32, f64 = np.float32, np.float64
    data = np.asarray(data, dtype=f32)
    minVal, maxVal = f32(data.min()), f32(data.max())
    spread = f32(maxVal - minVal)

    binSize = float(spread) / float(numBins - 2.0)
    with np.errstate(all="ignore"):
        step = f32(binSize)
        edge = f32(f32(np.floor(f32(minVal / step))) * step)
        linearBins = [edge]
        for _ in range(1, numBins):
            edge = f32(edge + step)
            linearBins.append(edge)
    linearVar = histVariance(data, np.asarray(sorted(linearBins), dtype=f32), weights=weights, counts=counts)
    linearScale = 1.0 / binSize

    shift = 0.
    if minVal <= 0.:
        shift = f32(f32(1.0) - minVal)
        data = (data + shift).astype(f32)
        minVal, maxVal = f32(minVal + shift), f32(maxVal + shift)
    ratio = float(maxVal) / float(minVal)
    logBase = f64(np.power(f64(ratio), f64(1. / float(numBins - 2.00))))
    edge = f64(np.power(logBase, np.floor(f64(np.log(f32(minVal))) / np.log(logBase))))
    logBins = [edge]
    for _ in range(1, numBins):
        edge = f64(edge * logBase)
        logBins.append(edge)
    logVar = histVariance(data, np.asarray(sorted(logBins), dtype=f64), fromLog=True, weights=weights, counts=counts)

    if logVar < linearVar and noLog is False:
        return "logScale", logBase, shift
    return "scale", linearScale, 0.


def setTrackScale(track, numBins, allIntervals, noLog):
    """Set the scaling attributes of the track from its values over the intervals."""
    values, weights = trackWeights(track, allIntervals)
    if int(weights.sum()) > numBins:
        scaleType, scaleParam, shift = computeScale(values, numBins, noLog, weights=weights)
        if scaleParam > 1e-4:                      # round down so the XML does not look too ugly
            scaleParam = float("%.4f" % scaleParam)
        if scaleType == "scale":
            logger.info("Setting track %s scale to %f" % (track.getName(), scaleParam))
            track.setScale(scaleParam)
        elif scaleType == "logScale":
            logger.info("Setting track %s logScale to %f" % (track.getName(), scaleParam))
            track.setLogScale(scaleParam)
        logger.info("Setting track %s shift to %f" % (track.getName(), shift))
        track.setShift(shift)


def main(argv=None):
    if argv is None:
        argv = sys.argv
    parser = argparse.ArgumentParser(
        formatter_class=argparse.ArgumentDefaultsHelpFormatter,
        description="Automatically set the scale attributes of numeric tracks within a given tracks.xml using some "
                    "simple heuristics.")
    parser.add_argument("tracksInfo", help="Path of Tracks Info file containing paths to genome annotation tracks")
    parser.add_argument("allBed", help="Bed file spanning entire genome")
    parser.add_argument("outputTracks", help="Path to write modified tracks XML to.")
    parser.add_argument("--numBins", help="Maximum number of bins after scaling", default=10, type=int)
    parser.add_argument("--tracks", help="Comma-separated list of tracks to process. If not set, all tracks listed as "
                        "having a multinomial distribution (since this is the default value, this includes tracks with "
                        "no distribution attribute) or gaussian distribution will be processed.", default=None)
    parser.add_argument("--skip", help="Comma-separated list of tracks to skip.", default=None)
    parser.add_argument("--noLog", help="Never use log scaling", action="store_true", default=False)
    args = parser.parse_args(argv[1:])

    trackNames = args.tracks.split(",") if args.tracks is not None else []
    skipNames = args.skip.split(",") if args.skip is not None else []
    trackList = readTrackList(args.tracksInfo)
    allIntervals = trackIO.getMergedBedIntervals(args.allBed)
    for track in trackList:
        trackExt = os.path.splitext(track.getPath())[1]
        isFasta = len(trackExt) >= 3 and trackExt[:3].lower() == ".fa"
        if track.getName() not in skipNames and (track.getName() in trackNames or len(trackNames) == 0) and \
                track.getDist() in ("multinomial", "sparse_multinomial", "gaussian") and not isFasta:
            try:
                setTrackScale(track, args.numBins, allIntervals, args.noLog)
            except ValueError as e:
                logger.warning("Skipping (non-numeric?) track %s due to: %s" % (track.getName(), str(e)))
    trackList.saveXML(args.outputTracks)
    return 0


if __name__ == "__main__":
    sys.exit(main())
