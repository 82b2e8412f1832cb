"""The step after the path: what bin/teHmmEval.py writes per row (teHmmEval.py:216-275).

The reference formats one text line per table row in the interpreter (statesToBed), which dominates its
wall-clock at 100 Mb.  Here the coordinates of every row (segment lengths, mask offsets) and the
masked posterior sum are reduced on the device, and the lines are formatted by the library's native
writer (tehmm_write_bed).
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import f64p, i32p, i64p, ptr


def bedCoords(trackTable):
    """(starts, ends) int64 arrays, one entry per row of the table (teHmmEval.py:251-266)."""
    n = len(trackTable)
    offs = trackTable.getSegmentOffsets()
    offs = None if offs is None else np.ascontiguousarray(offs, dtype=np.int64)
    mo = trackTable.getMaskRunningOffsets() if hasattr(trackTable, "getMaskRunningOffsets") else None
    mo = None if mo is None else np.ascontiguousarray(mo, dtype=np.int32)
    starts, ends = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    _lib.check(_lib.load().tehmm_bed_coords(n, int(trackTable.getStart()), int(trackTable.getEnd()),
                                            ptr(offs, i64p), ptr(mo, i32p), 0 if mo is None else len(mo),
                                            ptr(starts, i64p), ptr(ends, i64p)), "tehmm_bed_coords")
    return starts, ends


def _write(path, append, chrom, starts, ends, states=None, names=None, values=None):
    n = len(starts)
    st = None if states is None else np.ascontiguousarray(states, dtype=np.int64)
    vals = None if values is None else np.ascontiguousarray(values, dtype=np.float64)
    arr, n_names = None, 0
    if names is not None:
        n_names = len(names)
        arr = (ctypes.c_char_p * n_names)(*[str(x).encode() for x in names])
    _lib.check(_lib.load().tehmm_write_bed(str(path).encode(), 1 if append else 0, str(chrom).encode(), n,
                                           ptr(starts, i64p), ptr(ends, i64p), ptr(st, i64p), n_names, arr,
                                           ptr(vals, f64p)), "tehmm_write_bed")


def statesToBed(trackTable, states, bedPath=None, posteriorSums=None, posteriorsPath=None, stateNames=None,
                append=True, emissionSums=None, emissionsPath=None):
    """teHmmEval.py:238-275.  states: integer state per row; posteriorSums: the masked posterior sum per
    row (HipBatch.posterior_masksum) -- written one row late, wrapping, as the reference does (quirk Q15:
    row i carries posteriors[i - 1]).  emissionSums: the masked emission column per row
    (HipBatch.emission_masksum, MultitrackHmm.emissionColumn) for the --ed file, with the same one-row shift
    (row i carries emProbs[i - 1]); -inf is written as Python 2 prints that float64."""
    starts, ends = bedCoords(trackTable)
    chrom = trackTable.getChrom()
    if bedPath is not None:
        _write(bedPath, append, chrom, starts, ends, states=states, names=stateNames)
    if posteriorSums is not None and posteriorsPath is not None:
        _write(posteriorsPath, append, chrom, starts, ends, values=np.roll(np.asarray(posteriorSums), 1))
    if emissionSums is not None and emissionsPath is not None:
        _write(emissionsPath, append, chrom, starts, ends, values=np.roll(np.asarray(emissionSums), 1))


# ---- the same lines formatted on the device (tehmm_bed_text_write) -------------------------------------
KIND_NAMES, KIND_INT, KIND_VALUE = 0, 1, 2
SRC_VITERBI, SRC_MAP, SRC_POSTERIOR, SRC_EMISSION = 0, 1, 2, 3
_cpp = ctypes.POINTER(ctypes.c_char_p)


def _describe(table):
    """(chrom, start, end, rows, segOffsets, maskOffsets) of a TrackTable, or such a tuple itself"""
    if isinstance(table, (tuple, list)):
        chrom, start, end, rows, seg, mo = table
    else:
        chrom, start, end, rows = table.getChrom(), table.getStart(), table.getEnd(), len(table)
        seg = table.getSegmentOffsets()
        mo = table.getMaskRunningOffsets() if hasattr(table, "getMaskRunningOffsets") else None
    seg = None if seg is None else np.ascontiguousarray(seg, dtype=np.int64)
    mo = None if mo is None else np.ascontiguousarray(mo, dtype=np.int32)
    if seg is not None and len(seg) != rows:
        raise ValueError("segOffsets holds %d entries for a table of %d rows" % (len(seg), rows))
    return str(chrom).encode(), int(start), int(end), int(rows), seg, mo


def _strings(items):
    return None if items is None else (ctypes.c_char_p * len(items))(
        *[None if x is None else (x if isinstance(x, bytes) else str(x).encode()) for x in items])


class _TableArgs(object):
    """The per-table arrays of the two calls (and the numpy arrays behind their pointers)."""

    def __init__(self, tables, headers):
        d = [_describe(t) for t in tables]
        n = self.n = len(d)
        if headers is not None and len(headers) != n:
            raise ValueError("one header (or None) per table")
        self.chroms = _strings([x[0] for x in d])
        self.start = np.asarray([x[1] for x in d], dtype=np.int64)
        self.end = np.asarray([x[2] for x in d], dtype=np.int64)
        self.row_offsets = np.concatenate([[0], np.cumsum([x[3] for x in d])]).astype(np.int64)
        self.keep = [(x[4], x[5]) for x in d]
        self.seg = self.mask = None
        if any(x[4] is not None for x in d):
            self.seg = (i64p * n)(*[i64p() if x[4] is None else ptr(x[4], i64p) for x in d])
        if any(x[5] is not None for x in d):
            self.mask = (i32p * n)(*[i32p() if x[5] is None else ptr(x[5], i32p) for x in d])
        self.n_mask = np.asarray([0 if x[5] is None else len(x[5]) for x in d], dtype=np.int64)
        self.headers = _strings(headers)


def writeBedText(path, tables, states=None, values=None, names=None, headers=None, shift=False, append=False,
                 stripeRows=0):
    """The lines of a list of tables, formatted on the device: the bytes bedCoords + tehmm_write_bed produce table by
    table.  tables: TrackTables, or tuples (chrom, start, end, rows, segOffsets or None, maskOffsets or None);
    states (int, with names: names[state], else the integer) or values (float64) is the concatenated column of all
    tables; headers: per table a line written verbatim before its rows, or None.  shift: quirk Q15, per table."""
    a = _TableArgs(tables, headers)
    rows = int(a.row_offsets[-1])
    st = vals = None
    if values is not None:
        kind = KIND_VALUE
        vals = np.ascontiguousarray(values, dtype=np.float64)
        assert vals.shape == (rows,)
    else:
        kind = KIND_INT if names is None else KIND_NAMES
        st = np.ascontiguousarray(states, dtype=np.int64)
        assert st.shape == (rows,)
    nm = _strings(None if names is None else list(names))
    _lib.check(_lib.load().tehmm_bed_text_write(
        str(path).encode(), 1 if append else 0, a.n, a.chroms, ptr(a.start, i64p), ptr(a.end, i64p),
        ptr(a.row_offsets, i64p), a.seg, a.mask, ptr(a.n_mask, i64p), a.headers, kind, ptr(st, i64p), ptr(vals, f64p),
        0 if names is None else len(names), nm, 1 if shift else 0, int(stripeRows)), "tehmm_bed_text_write")


def writeBatchBed(path, batch, source, tables, model=None, mask=None, useRatios=False, interval0=0, names=None,
                  headers=None, append=False, stripeRows=0):
    """The same over intervals interval0 .. interval0 + len(tables) of a HipBatch, the column read or computed on the
    device: SRC_VITERBI / SRC_MAP (the state, names[state] with names), SRC_POSTERIOR (the masked posterior sum) or
    SRC_EMISSION (the masked emission column of `model`, a HipModel); the two value columns come with the one-row
    shift of quirk Q15.  No per-row column reaches the host."""
    a = _TableArgs(tables, headers)
    offs = np.asarray(batch.offsets[int(interval0):int(interval0) + a.n + 1], dtype=np.int64)
    if len(offs) != a.n + 1 or not np.array_equal(offs - offs[0], a.row_offsets):
        raise ValueError("the tables are not intervals %d .. %d of the batch" % (interval0, interval0 + a.n))
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.float64)
    if mk is not None and source in (SRC_POSTERIOR, SRC_EMISSION):
        n_states = batch.N if source == SRC_POSTERIOR or model is None else model.N
        if n_states is not None and mk.shape != (n_states,):
            raise ValueError("the mask needs one entry per state")
    nm = _strings(None if names is None else list(names))
    _lib.check(_lib.load().tehmm_batch_bed_text_write(
        None if model is None else model._h, batch._h, int(source), ptr(mk, f64p), 1 if useRatios else 0,
        int(interval0), a.n, a.chroms, ptr(a.start, i64p), ptr(a.end, i64p), a.seg, a.mask, ptr(a.n_mask, i64p),
        a.headers, 0 if names is None else len(names), nm, str(path).encode(), 1 if append else 0, int(stripeRows)),
        "tehmm_batch_bed_text_write")


def lastBedTextCounters():
    """(rows, bytes, rows the host formatted) of this thread's last writeBedText / writeBatchBed"""
    r, b, h = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.load().tehmm_bed_text_last_counters(ctypes.byref(r), ctypes.byref(b), ctypes.byref(h)),
               "tehmm_bed_text_last_counters")
    return r.value, b.value, h.value


def lastBedTextTiming():
    """[(pass, milliseconds)] of this thread's last writeBedText / writeBatchBed"""
    names = (ctypes.c_char_p * 16)()
    ms = (ctypes.c_double * 16)()
    n = _lib.load().tehmm_bed_text_last_timing(16, names, ms)
    _lib.check(min(n, 0), "tehmm_bed_text_last_timing")
    return [(names[i].decode(), ms[i]) for i in range(n)]


def getPosteriorsMask(pdStates, model):
    """teHmmEval.py:294-311: mask[i] == 1 iff state i is named in the comma-separated `pdStates` (--pdStates and
    --edStates); the states of a model without a state-name map are named "0", "1", ...  A name the model does not
    know is reported and left out."""
    import logging
    stateMap = model.getStateNameMap()
    if stateMap is None:
        names = {str(i): i for i in range(model.getEmissionModel().getNumStates())}
        size = len(names)
        has, number = names.__contains__, names.__getitem__
    else:
        size = len(stateMap)
        has, number = stateMap.has, stateMap.getMap
    mask = np.zeros(size, dtype=np.int8)
    for state in pdStates.split(","):
        if not has(state):
            logging.getLogger(__name__).warning(
                "Posterior (or Emission) Distribution state %s not found in model" % state)
        else:
            mask[number(state)] = 1
    return mask


def bic(model, totalScore, totalDatapoints):
    """Bayesian information criterion as teHmmEval.py:216-234 writes it: -2 lnL + k (ln n + ln 2 pi), with
    lnL the summed Viterbi score, n = rows x tracks and k = model.getNumFreeParameters() (0 when the
    model cannot say: the reference swallows the exception).  Returns (bic, k)."""
    lnL = float(totalScore)
    try:
        k = float(model.getNumFreeParameters())
    except Exception:
        k = 0.0
    n = float(totalDatapoints)
    return -2.0 * lnL + k * (np.log(n) + np.log(2 * np.pi)), k


def writeBic(path, model, totalScore, totalDatapoints):
    """The two-line --bic file of teHmmEval.py:216-234."""
    value, k = bic(model, totalScore, totalDatapoints)
    em = model.getEmissionModel()
    with open(path, "w") as f:
        f.write("%f\n" % value)
        f.write("# = -2.0 * lnL + k * (lnN + ln(2 * np.pi))\n"
                "# where lnL=%f  k=%d (%d states)  N=%d (%d obs * %d tracks)  lnN=%f\n" % (
                    float(totalScore), int(k), em.getNumStates(), int(totalDatapoints),
                    totalDatapoints / em.getNumTracks(), em.getNumTracks(), np.log(float(totalDatapoints))))
    return value
