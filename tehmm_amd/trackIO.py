"""Track file IO: BED and FASTA tracks into per-base uint8 rows (trackIO.py of the reference).

The reference shells out to ``intersectBed | sortBed`` once per track and interval and then assigns every base of every
record in the interpreter.  Here a file is parsed and sorted once (BedFile), the records of an interval come from binary
searches, the value map is consulted once per distinct value, and the per-base work -- a "last writer wins" paint -- is
one device call for all tracks and all intervals (tehmm_load_tracks_u8).  Nothing falls back to a CPU implementation.

The rule, for one track over one table [start, end) of chromosome c:
  * records: lines starting with '#' are skipped, fields are split on tabs, lines with fewer than 3 fields are skipped;
  * kept when chrom == c, e > start, s < end and e > s; clipped to oStart = max(start, s), oEnd = min(end, e); sorted
    stably by oStart (file order among equal clipped starts).  This stands in for ``intersectBed -a file -b interval |
    sortBed``: bedtools does not define the order among records of equal start, so where such records overlap the
    reference's result depends on the bedtools build, and this is the order chosen here;
  * every record gives (sym0, sym) through the value map (valCol, useDelta as trackIO.py:173-203: with useDelta the
    first base carries the difference to the previous record's value when the two abut, and the rest carries 0);
  * record r paints sym0 at its first row and sym at the others, in sorted order, over rows that start at the map's
    missing value.
FASTA tracks: row i is the map of base start + i of record c (upper-cased unless caseSensitive); rows past the end of
the sequence keep the missing value.

Differences from the reference, all deliberate: a line's trailing "\\r\\n" is dropped whole (the reference drops one
character); a value map is required for byte rows; a symbol above 255 raises ValueError naming the track (the
reference's result there depends on the NumPy version); bigWig / bigBed need external tools and raise RuntimeError.
Not offered: sort= / ignoreBed12= / needIntersect= of readBedData (records are always clipped and sorted here).

Without a value map and with a float32 outputBuf (what bin/setTrackScaling.py of the reference calls; DESIGN.md section
5p) a BED record's value is np.float32(float(text)), or 1 for valCol 0, and the rows no record covers keep what the
buffer held.  Text that is no number raises ValueError as in the reference; a value that is not finite raises
ValueError naming the track (deliberate).  useDelta=True is not offered there.

BED text itself is read by parseBed into BedColumns: by bedRead and the interpreter (the host
route, the specification) or, for files of 1 MiB and more when there is a device, by the kernels of
tehmm_bedparse.hip.h, which certify what they return and leave the rest to the host's int() / float() / dict.  BedFile,
readBedIntervals and the loaders stand on the columns and return the same either way.
"""
import ctypes
import logging
import operator
import os
import sys

import numpy as np

from . import _lib
from ._lib import f32p, i64p, ptr, u8p

logger = logging.getLogger(__name__)

MAX_SYMBOL = 255
MAX_TRACKS = 128


# ---- BED text ---------------------------------------------------------------------------------------------------------
def bedRead(path):
    """The records of a BED file as lists of text fields (trackIO.py:389-404)."""
    out = []
    with open(path, "r", newline="") as f:
        for line in f:
            if line[:1] == "#":
                continue
            fields = line.rstrip("\n").rstrip("\r").split("\t")
            if len(fields) > 2:
                out.append(fields)
    return out


# ---- BED columns ------------------------------------------------------------------------------------------------------
# The records of a file as columns.  Two routes build them: the host route is bedRead and the
# interpreter's int() / dict, i.e. the specification; the device route parses the file's bytes with the kernels of
# tehmm_bedparse.hip.h and leaves to the host's int() / float() / dict exactly what the device does not certify.
BED_PARSE_MIN_BYTES = 1 << 20       # launch and copy overhead arithmetic, not a measurement
PARSE_INT, PARSE_FLOAT = 0, 1
CERTIFIED, LEFT_TO_HOST, NO_COLUMN = 0, 1, 2
DEVICE_COLS = 6


class _HostRoute(Exception):
    """the device route hands the file to the host route (the reason is logged)"""


class _FieldsView(object):
    """fields[i] of a BedColumns without a list of lists: the text fields of record i, as bedRead returns them"""

    def __init__(self, cols):
        self.cols = cols

    def __len__(self):
        return self.cols.n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self.cols.n))]
        i = operator.index(i)
        if i < 0:
            i += self.cols.n
        if not 0 <= i < self.cols.n:
            raise IndexError("list index out of range")
        return self.cols.line(i).split("\t")

    def __iter__(self):
        for i in range(self.cols.n):
            yield self[i]


class BedColumns(object):
    """The kept records of a BED file, in file order, as columns.  route: "host" or "device"; n: records; numFields
    (int32); start / end (int64: int() of columns 1 and 2); chromCode / chromNames; fields (a sequence of field lists);
    raw (the file's bytes as uint8)."""
    route = None

    def __init__(self, path):
        self.path = path
        self._ints, self._floats, self._codes, self._chroms, self._intervals = dict(), dict(), dict(), None, dict()

    # -- numbers ------------------------------------------------------------------------------------------------------
    def ints(self, col):
        """int() of every record's column col (int64); the first text that is no integer raises as int() does"""
        if col not in self._ints:
            self._ints[col] = self._int_column(col)
        return self._ints[col]

    @property
    def start(self):
        return self.ints(1)

    @property
    def end(self):
        self.ints(1)                                  # (starts first: the order in which a bad number is met)
        return self.ints(2)

    def floats(self, col):
        """(float64 values, bool: certified equal to float(text)) of column col; the rest is the caller's float()"""
        if col not in self._floats:
            self._floats[col] = self._float_column(col)
        return self._floats[col]

    def intsCertified(self):
        """True: the device certified every start and end (the vectorised consumers need no int() of their own)"""
        return False

    # -- codes --------------------------------------------------------------------------------------------------------
    def codes(self, col):
        """(code per record, distinct raw values in order of first appearance) of a text column, as BedFile.codes"""
        return self._strict_codes(col)[:2]

    def codeFirst(self, col):
        """the record in which each distinct value of codes(col) first appears"""
        return self._strict_codes(col)[2]

    def _strict_codes(self, col):
        if col not in self._codes:
            code, values, first, missing, empty = self._code_column(col)
            if missing:
                raise ValueError("%s: a record has no column %d" % (self.path, col))
            if empty:
                raise ValueError("%s: an empty value in column %d" % (self.path, col))
            self._codes[col] = (code, values, first)
        return self._codes[col]

    def _chrom_codes(self):
        if self._chroms is None:
            code, values, _, _, _ = self._code_column(0)
            self._chroms = (code, values)
        return self._chroms

    @property
    def chromCode(self):
        return self._chrom_codes()[0]

    @property
    def chromNames(self):
        return self._chrom_codes()[1]

    def _dict_codes(self, col):
        """the host dictionary over the field texts: (code, values, first records, missing, empty)"""
        table, first = dict(), []

        def walk():
            for i in range(self.n):
                v = self.field(i, col)
                c = table.get(v)
                if c is None:
                    c = table[v] = len(table)
                    first.append(i)
                yield c
        try:
            code = np.fromiter(walk(), dtype=np.int64, count=self.n)
        except IndexError:
            return None, None, None, 1, 0
        return code, list(table), np.asarray(first, dtype=np.int64), 0, int("" in table)

    # -- tuples -------------------------------------------------------------------------------------------------------
    def tuples(self, ncol=None, order=None):
        """[(chrom, int start, int end) + the text of columns 3 .. ncol - 1 (None: all)] of the records, or of the
        records `order` in that order"""
        s, e = self.start, self.end
        idx = np.arange(self.n, dtype=np.int64) if order is None else np.asarray(order, dtype=np.int64)
        names = self.chromNames
        chrom = [names[c] for c in self.chromCode[idx].tolist()]
        if ncol == 3:
            return list(zip(chrom, s[idx].tolist(), e[idx].tolist()))
        fields = self.fields
        return [(c, a, b) + tuple(fields[i][3:ncol]) for c, a, b, i in
                zip(chrom, s[idx].tolist(), e[idx].tolist(), idx.tolist())]

    def intervals(self, sort=False):
        """IntervalColumns of the records (TrackTable.segment takes them)"""
        if sort not in self._intervals:
            self._intervals[sort] = IntervalColumns(self.chromNames, self.chromCode, self.start, self.end, sort=sort)
        return self._intervals[sort]

    def close(self):
        pass


class _HostBedColumns(BedColumns):
    """bedRead and the interpreter: the specification"""
    route = "host"

    def __init__(self, path):
        super(_HostBedColumns, self).__init__(path)
        self.fields = bedRead(path)
        self.n = len(self.fields)
        self.numFields = np.fromiter((len(r) for r in self.fields), dtype=np.int32, count=self.n)
        self._raw = None

    @property
    def raw(self):
        if self._raw is None:
            self._raw = np.fromfile(self.path, dtype=np.uint8)
        return self._raw

    def line(self, i):
        return "\t".join(self.fields[i])

    def field(self, i, col):
        return self.fields[i][col]

    def _int_column(self, col):
        return np.fromiter((int(r[col]) for r in self.fields), dtype=np.int64, count=self.n)

    def _float_column(self, col):
        return np.zeros(self.n, dtype=np.float64), np.zeros(self.n, dtype=bool)

    def _code_column(self, col):
        return self._dict_codes(col)


class _DeviceBedColumns(BedColumns):
    """the parse of tehmm_bed_parse_open; the handle keeps text and tables on the device for later columns"""
    route = "device"

    def __init__(self, path):
        super(_DeviceBedColumns, self).__init__(path)
        lib = _lib.load()
        self._handle = None
        self.raw = _read_pinned(path)
        h = _lib.vp()
        rc = lib.tehmm_bed_parse_open(_lib.vp(self.raw.ctypes.data), len(self.raw), ctypes.byref(h))
        if rc == -3:
            raise _HostRoute(lib.tehmm_last_error().decode())
        _lib.check(rc, "tehmm_bed_parse_open")
        self._handle = h
        lines, n, high = _lib.c_i64(0), _lib.c_i64(0), _lib.c_i64(0)
        _lib.check(lib.tehmm_bed_parse_counts(h, ctypes.byref(lines), ctypes.byref(n), ctypes.byref(high)),
                   "tehmm_bed_parse_counts")
        if high.value > 0:
            self.close()
            raise _HostRoute("bytes >= 0x80: decoding them is the locale's business")
        self.n, self.numLines = int(n.value), int(lines.value)
        self.lineStart, self.lineLen = np.empty(self.n, dtype=np.int64), np.empty(self.n, dtype=np.int64)
        self.numFields = np.empty(self.n, dtype=np.int32)
        self.fieldOff = np.empty((self.n, DEVICE_COLS), dtype=np.int32)
        self.fieldLen = np.empty((self.n, DEVICE_COLS), dtype=np.int32)
        _lib.check(lib.tehmm_bed_parse_get_table(h, ptr(self.lineStart, i64p), ptr(self.lineLen, i64p),
                                                 ptr(self.numFields, _lib.i32p), ptr(self.fieldOff, _lib.i32p),
                                                 ptr(self.fieldLen, _lib.i32p)), "tehmm_bed_parse_get_table")
        self.fields = _FieldsView(self)
        self._text = None
        self._status = dict()

    def close(self):
        if getattr(self, "_handle", None) is not None:
            _lib.load().tehmm_bed_parse_close(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def text(self):
        """the file as one str (no byte is >= 0x80: offsets are the bytes'), decoded when text is first asked for"""
        if self._text is None:
            self._text = self.raw.tobytes().decode("ascii")
        return self._text

    def line(self, i):
        a = int(self.lineStart[i])
        return self.text()[a:a + int(self.lineLen[i])]

    def field(self, i, col):
        if col >= DEVICE_COLS:
            return self.fields[i][col]
        n = int(self.fieldLen[i, col])
        if n < 0:
            raise IndexError("list index out of range")
        a = int(self.lineStart[i]) + int(self.fieldOff[i, col])
        return self.text()[a:a + n]

    def numbers(self, col, kind):
        """(values, status bytes) of the device's routine over column col (0 .. 5), nothing added by the host"""
        val = np.zeros(self.n, dtype=np.int64 if kind == PARSE_INT else np.float64)
        status = np.zeros(self.n, dtype=np.uint8)
        _lib.check(_lib.load().tehmm_bed_parse_get_numbers(
            self._handle, col, kind, ptr(val, i64p) if kind == PARSE_INT else None,
            ptr(val, _lib.f64p) if kind == PARSE_FLOAT else None, ptr(status, u8p)), "tehmm_bed_parse_get_numbers")
        return val, status

    def _int_column(self, col):
        if col >= DEVICE_COLS:
            return np.fromiter((int(r[col]) for r in self.fields), dtype=np.int64, count=self.n)
        val, status = self._device_ints(col)
        val = val.copy()
        for i in np.flatnonzero(status != CERTIFIED).tolist():      # file order: the first error is bedRead's first
            val[i] = int(self.field(i, col))
        return val

    def _device_ints(self, col):
        if col not in self._status:
            self._status[col] = self.numbers(col, PARSE_INT)
        return self._status[col]

    def _float_column(self, col):
        if col >= DEVICE_COLS:
            return np.zeros(self.n, dtype=np.float64), np.zeros(self.n, dtype=bool)
        val, status = self.numbers(col, PARSE_FLOAT)
        return val, status == CERTIFIED

    def intsCertified(self):
        return all(bool((self._device_ints(col)[1] == CERTIFIED).all()) for col in (1, 2))

    def _code_column(self, col):
        if col >= DEVICE_COLS:
            return self._dict_codes(col)
        code, first = np.zeros(self.n, dtype=np.int64), np.zeros(self.n, dtype=np.int64)
        nd, missing, empty, fell = _lib.c_i64(0), _lib.c_i64(0), _lib.c_i64(0), _lib.c_int(0)
        _lib.check(_lib.load().tehmm_bed_parse_get_codes(
            self._handle, col, ptr(code, i64p), ptr(first, i64p), ctypes.byref(nd), ctypes.byref(missing),
            ctypes.byref(empty), ctypes.byref(fell)), "tehmm_bed_parse_get_codes")
        if missing.value:
            return None, None, None, int(missing.value), int(empty.value)
        if fell.value:                                # two values behind one hash: the host dictionary decides
            logger.info("%s: column %d coded by the host dictionary (hash collision)" % (self.path, col))
            return self._dict_codes(col)
        first = first[:int(nd.value)].copy()
        return code, [self.field(i, col) for i in first.tolist()], first, 0, int(empty.value)


def _read_pinned(path):
    """the bytes of a file in a tehmm_host_alloc block (the upload is one DMA)"""
    size = os.path.getsize(path)
    buf = _lib.pinned_empty(size, np.uint8)
    got = 0
    with open(path, "rb", buffering=0) as f:
        view = memoryview(buf)
        while got < size:
            k = f.readinto(view[got:])
            if not k:
                break
            got += k
    return buf[:got]


def parseBed(path):
    """BedColumns of a BED file.  TEHMM_BED_PARSE=0: the host route; =1: the device route (an error without a device);
    unset: the device route for files of at least TEHMM_BED_PARSE_MIN_BYTES bytes (default 1 MiB) when there is a
    device.  A file with a byte >= 0x80, or one whose text and columns exceed the workspace budget, takes the host
    route from the device route, with the reason logged."""
    mode = os.environ.get("TEHMM_BED_PARSE", "")
    if mode not in ("", "0", "1"):
        raise ValueError("TEHMM_BED_PARSE is 0 or 1")
    device = False
    if mode == "1":
        if _lib.device_count() < 1:
            raise RuntimeError("TEHMM_BED_PARSE=1: the device route needs a device and there is none")
        device = True
    elif mode == "":
        minBytes = int(os.environ.get("TEHMM_BED_PARSE_MIN_BYTES", BED_PARSE_MIN_BYTES))
        device = os.path.getsize(path) >= minBytes and _lib.device_count() > 0
    if device:
        try:
            return _DeviceBedColumns(path)
        except _HostRoute as e:
            logger.info("%s: parsed on the host (%s)" % (path, e))
    return _HostBedColumns(path)


def parseCounters():
    """lines, records, host_ints, host_floats, code_fallbacks since this thread's last device parse was opened"""
    v = [_lib.c_i64(0) for _ in range(5)]
    _lib.check(_lib.load().tehmm_bed_parse_last_counters(*[ctypes.byref(x) for x in v]), "tehmm_bed_parse_last_counters")
    return dict(zip(("lines", "records", "host_ints", "host_floats", "code_fallbacks"), (int(x.value) for x in v)))


def parseTiming():
    """[(pass, milliseconds)] of the device passes since this thread's last device parse was opened"""
    names = (ctypes.c_char_p * 64)()
    ms = (ctypes.c_double * 64)()
    n = _lib.load().tehmm_bed_parse_last_timing(64, names, ms)
    _lib.check(min(n, 0), "tehmm_bed_parse_last_timing")
    return [(names[i].decode(), ms[i]) for i in range(n)]


def parseNumber(text, kind):
    """(value, status) of the device's number routine run on the CPU (tehmm_bed_parse_number); text: bytes"""
    iv, fv, st = _lib.c_i64(0), _lib.c_dbl(0.0), _lib.c_int(0)
    _lib.check(_lib.load().tehmm_bed_parse_number(text, len(text), kind, ctypes.byref(iv), ctypes.byref(fv),
                                                  ctypes.byref(st)), "tehmm_bed_parse_number")
    return (iv.value if kind == PARSE_INT else fv.value), st.value


def parseTileBytes():
    return int(_lib.load().tehmm_bed_parse_tile_bytes())


class IntervalColumns(object):
    """Intervals (chrom, start, end) as arrays, in list order, or with sort stably by (chrom name, start) as
    readBedIntervals(sort=True) orders them; window() is what TrackTable.segment asks of its segment list."""

    def __init__(self, chromNames, chromCode, start, end, sort=False):
        code = np.asarray(chromCode, dtype=np.int64)
        start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
        self.sorted = bool(sort)
        self.chromNames = list(chromNames)
        if sort:
            rank = np.zeros(len(self.chromNames), dtype=np.int64)
            rank[np.asarray(sorted(range(len(self.chromNames)), key=lambda c: self.chromNames[c]), dtype=np.int64)] = \
                np.arange(len(self.chromNames))
            order = np.lexsort((start, rank[code])) if len(code) else np.zeros(0, dtype=np.int64)
            code, start, end = code[order], start[order], end[order]
            self.order = order
            byRank = rank[code]
            self._slices = dict()
            for c, name in enumerate(self.chromNames):
                self._slices[name] = (int(np.searchsorted(byRank, rank[c], side="left")),
                                      int(np.searchsorted(byRank, rank[c], side="right")))
        else:
            self.order = np.arange(len(code), dtype=np.int64)
            self._index = {name: c for c, name in enumerate(self.chromNames)}
        self.chromCode, self.start, self.end = code, start, end

    @classmethod
    def fromTuples(cls, intervals, sort=False):
        table = dict()
        code = np.fromiter((table.setdefault(iv[0], len(table)) for iv in intervals), dtype=np.int64,
                           count=len(intervals))
        start = np.fromiter((int(iv[1]) for iv in intervals), dtype=np.int64, count=len(intervals))
        end = np.fromiter((int(iv[2]) for iv in intervals), dtype=np.int64, count=len(intervals))
        return cls(list(table), code, start, end, sort=sort)

    def __len__(self):
        return len(self.start)

    def tuples(self):
        return list(zip([self.chromNames[c] for c in self.chromCode.tolist()], self.start.tolist(), self.end.tolist()))

    def window(self, chrom, start, end):
        """(starts, ends) of the intervals of chrom with start >= `start` and end <= `end`, in list order"""
        if self.sorted:
            if chrom not in self._slices:
                z = np.zeros(0, dtype=np.int64)
                return z, z
            a, b = self._slices[chrom]
            lo = a + int(np.searchsorted(self.start[a:b], start, side="left"))
            hi = a + int(np.searchsorted(self.start[a:b], end, side="right"))   # (an interval inside ends by `end`)
            s, e = self.start[lo:hi], self.end[lo:hi]
            keep = e <= end
        else:
            c = self._index.get(chrom, -1)
            keep = (self.chromCode == c) & (self.start >= start) & (self.end <= end)
            s, e = self.start, self.end
        return s[keep], e[keep]


def readBedColumns(bedPath, sort=False):
    """The intervals of readBedIntervals(bedPath, 3, sort=sort) as IntervalColumns"""
    if not os.path.isfile(bedPath):
        raise RuntimeError("Bed interval file %s not found" % bedPath)
    cols = parseBed(bedPath)
    if cols.intsCertified():
        return cols.intervals(sort=sort)
    return IntervalColumns.fromTuples(_bed_intervals(cols, bedPath, 3, None, None, None, sort))


def _clip(records, chrom, start, end):
    """rule step 2 on tuples / lists whose first three fields are chrom, start, end: [(oStart, oEnd, record)]"""
    kept = [(max(start, int(r[1])), min(end, int(r[2])), r) for r in records
            if r[0] == chrom and int(r[2]) > start and int(r[1]) < end and int(r[2]) > int(r[1])]
    kept.sort(key=lambda x: x[0])
    return kept


def readBedIntervals(bedPath, ncol=3, chrom=None, start=None, end=None, sort=False):
    """Tuples (chrom, start, end[, name[, score]]) of a BED file, or of its part inside chrom:start-end (clipped and
    sorted by clipped start as in the module docstring).  sort: stable by (chrom, start)."""
    if not os.path.isfile(bedPath):
        raise RuntimeError("Bed interval file %s not found" % bedPath)
    assert ncol in (3, 4, 5)
    cols = parseBed(bedPath)
    if not cols.intsCertified():
        return _bed_intervals(cols, bedPath, ncol, chrom, start, end, sort)
    short = np.flatnonzero(cols.numFields < ncol)
    if len(short):
        raise ValueError("%s: a line has %d fields, ncol = %d" % (bedPath, int(cols.numFields[short[0]]), ncol))
    order = cols.intervals(sort=True).order if sort else np.arange(cols.n, dtype=np.int64)
    if chrom is None:
        return cols.tuples(ncol, order)
    assert start is not None and end is not None
    start, end = int(start), int(end)
    names = cols.chromNames
    s, e = cols.start[order], cols.end[order]
    keep = (cols.chromCode[order] == (names.index(chrom) if chrom in names else -1)) & (e > start) & (s < end) & (e > s)
    order, oStart, oEnd = order[keep], np.maximum(start, s[keep]), np.minimum(end, e[keep])
    by = np.argsort(oStart, kind="stable")
    rows = cols.tuples(ncol, order[by])
    return [(chrom, a, b) + r[3:] for a, b, r in zip(oStart[by].tolist(), oEnd[by].tolist(), rows)]


def _bed_intervals(cols, bedPath, ncol, chrom, start, end, sort):
    """readBedIntervals over field lists, record by record: the host route, and the device route's way for a file with
    a start or end that the device did not certify (every int() then runs where and when it always did)"""
    recs = cols.fields
    for r in recs:
        if len(r) < ncol:
            raise ValueError("%s: a line has %d fields, ncol = %d" % (bedPath, len(r), ncol))
    if sort:
        recs = sorted(recs, key=lambda r: (r[0], int(r[1])))
    if chrom is not None:
        assert start is not None and end is not None
        rows = [(chrom, s, e, r) for s, e, r in _clip(recs, chrom, int(start), int(end))]
    else:
        rows = [(r[0], int(r[1]), int(r[2]), r) for r in recs]
    return [(c, s, e) + tuple(r[3:ncol]) for c, s, e, r in rows]


def getMergedBedIntervals(bedPath, ncol=3, sort=False):
    """Overlapping and abutting intervals merged (what ``bedtools merge`` does by default); like bedtools it wants the
    file sorted, or sort=True."""
    if ncol > 3:
        raise ValueError("getMergedBedIntervals: merged intervals carry no name or score (ncol = %d)" % ncol)
    out = []
    for c, s, e in readBedIntervals(bedPath, 3, sort=sort):
        if out and out[-1][0] == c and s <= out[-1][2]:
            if e > out[-1][2]:
                out[-1] = (c, out[-1][1], e)
        else:
            out.append((c, s, e))
    return out


class BedFile(object):
    """A BED file parsed once: per chromosome the records stably sorted by start, with the running maximum of their
    ends, so that the records of any interval are two binary searches and a short filter."""

    def __init__(self, path):
        if not os.path.isfile(path):
            raise RuntimeError("Track file not found %s\n" % path)
        self.path = path
        self.columns = parseBed(path)
        self.fields = self.columns.fields
        start, end = self.columns.start, self.columns.end
        code, names = self.columns.chromCode, self.columns.chromNames
        byCode = np.argsort(code, kind="stable")          # the records of each chromosome, in file order
        cut = np.concatenate([[0], np.cumsum(np.bincount(code, minlength=len(names)))]).astype(np.int64)
        self.start, self.end = start, end
        self.chroms = dict()
        for c, name in enumerate(names):
            idx = byCode[cut[c]:cut[c + 1]].astype(np.int64)
            idx = idx[end[idx] > start[idx]]
            idx = idx[np.argsort(start[idx], kind="stable")]
            self.chroms[name] = (idx, start[idx], np.maximum.accumulate(end[idx]) if len(idx) else end[idx])

    def select(self, chrom, start, end):
        """(record index, oStart, oEnd) of rule step 2, as int64 arrays"""
        if chrom not in self.chroms:
            z = np.zeros(0, dtype=np.int64)
            return z, z, z
        idx, s, reach = self.chroms[chrom]
        first = int(np.searchsorted(reach, start, side="right"))      # nothing before it ends above start
        lo = int(np.searchsorted(s, start, side="right"))             # [first, lo): clipped start = the table's start
        hi = int(np.searchsorted(s, end, side="left"))
        lo = max(min(lo, hi), first)
        early = idx[first:lo]
        early = np.sort(early[self.end[early] > start])               # equal clipped starts: file order
        pick = np.concatenate([early, idx[lo:hi]])
        return pick, np.maximum(self.start[pick], start), np.minimum(self.end[pick], end)

    def codes(self, col):
        """(code per record, distinct raw values) of a text column; a record without the column raises"""
        return self.columns.codes(col)


def _check_symbols(sym, name):
    if len(sym) and (sym.max() > MAX_SYMBOL or sym.min() < 0):
        raise ValueError("track %s: symbol %d does not fit the uint8 table" % (name, int(sym.max())))


def recordSymbols(bed, pick, oStart, oEnd, chrom, valCol, valMap, updateValMap, useDelta, name):
    """rule step 3: (sym0, sym) int64 arrays of the selected records, the map updated in the reference's order"""
    n = len(pick)
    if valCol is not None and int(valCol) not in (0, 3, 4):
        raise ValueError("track %s: valCol is 0, 3 or 4" % name)
    col = 3 if valCol is None else int(valCol)
    if not useDelta:
        if n == 0:
            z = np.zeros(0, dtype=np.int64)
            return z, z
        if col == 0:
            sym = np.full(n, int(valMap.getMap(1, update=updateValMap)), dtype=np.int64)
        else:
            code, values = bed.codes(col)
            uniq, first, inv = np.unique(code[pick], return_index=True, return_inverse=True)
            table = np.zeros(len(uniq), dtype=np.int64)
            for u in np.argsort(first, kind="stable").tolist():      # distinct values in order of first appearance
                table[u] = int(valMap.getMap(values[int(uniq[u])], update=updateValMap))
            sym = table[inv.reshape(-1)]
        _check_symbols(sym, name)
        return sym, sym
    return recordSymbolsLoop(bed, pick, oStart, oEnd, chrom, col, valMap, updateValMap, useDelta, name)


def recordSymbolsLoop(bed, pick, oStart, oEnd, chrom, col, valMap, updateValMap, useDelta, name):
    """the reference's per-record loop (trackIO.py:173-203); the vectorised path above must agree with it"""
    n = len(pick)
    sym0, sym = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    prevEnd, prevVal = None, 0
    for x, (i, s, e) in enumerate(zip(pick.tolist(), oStart.tolist(), oEnd.tolist())):
        if col == 0:
            val = 1
        else:
            fields = bed.fields[i]
            if len(fields) <= col or fields[col] == "":
                raise ValueError("track %s: a record has no value in column %d" % (name, col))
            val = fields[col]
        val0 = val
        if useDelta:
            if prevEnd is not None and s == prevEnd:
                try:
                    val0 = float(val) - float(prevVal)
                except (TypeError, ValueError):
                    val0 = int(val != prevVal)
            prevVal, prevEnd = val, e
            val = 0
        sym[x] = int(valMap.getMap(val, update=updateValMap))
        sym0[x] = int(valMap.getMap(val0, update=updateValMap))
    _check_symbols(sym, name)
    _check_symbols(sym0, name)
    return sym0, sym


# ---- FASTA ------------------------------------------------------------------------------------------------------------
def fastaBytes(sequences, chrom, start, end):
    """bases start .. end of record chrom as T bytes, 0 where there is no base"""
    out = np.zeros(end - start, dtype=np.uint8)
    seq = sequences.get(chrom)
    if seq is not None and start < len(seq):
        part = np.frombuffer(seq, dtype=np.uint8)[max(start, 0):end]
        out[:len(part)] = part
    return out


def fastaUpdate(rowBytes, valMap, caseSensitive, updateValMap):
    """with updateValMap, new symbols in order of first appearance along the row"""
    if not updateValMap:
        return
    b = rowBytes[rowBytes != 0]
    if not caseSensitive:
        b = np.frombuffer(b.tobytes().upper(), dtype=np.uint8)
    uniq, first = np.unique(b, return_index=True)
    for u in np.argsort(first, kind="stable").tolist():
        valMap.getMap(chr(int(uniq[u])), update=True)


def fastaLut(valMap, caseSensitive, name):
    """byte -> symbol of a FASTA track as the map stands now (unknown bases: the missing value)"""
    lut = np.zeros(256, dtype=np.int64)
    for b in range(1, 256):
        c = chr(b)
        lut[b] = int(valMap.getMap(c if caseSensitive else c.upper(), update=False))
    lut[0] = int(valMap.getMissingVal())
    _check_symbols(lut, name)
    return lut.astype(np.uint8)


# ---- the device call ---------------------------------------------------------------------------------------------------
class RecordTrack(object):
    """one column of a paint: records in row coordinates, sorted by start"""
    kind = 0

    def __init__(self, fill, start=None, end=None, sym0=None, sym=None):
        z = np.zeros(0, dtype=np.int64)
        self.fill = int(fill)
        self.start = z if start is None else np.asarray(start, dtype=np.int64)
        self.end = z if end is None else np.asarray(end, dtype=np.int64)
        self.sym0 = z if sym0 is None else np.asarray(sym0)
        self.sym = z if sym is None else np.asarray(sym)


class SequenceTrack(object):
    """one column of a paint: T bytes (0 = no base) and their byte -> symbol table"""
    kind = 1

    def __init__(self, fill, seqBytes, lut):
        self.fill = int(fill)
        self.bytes = np.ascontiguousarray(seqBytes, dtype=np.uint8)
        self.lut = np.ascontiguousarray(lut, dtype=np.uint8)


def tileRows():
    """rows of a tile of the paint kernel"""
    return int(_lib.load().tehmm_trackio_tile_rows())


def paintTracks(T, tracks):
    """uint8 [T, K] of tehmm_load_tracks_u8 for a list of RecordTrack / SequenceTrack"""
    T, K = int(T), len(tracks)
    fill = np.asarray([t.fill for t in tracks], dtype=np.uint8)
    kind = np.asarray([t.kind for t in tracks], dtype=np.uint8)
    recs = [t if t.kind == 0 else RecordTrack(0) for t in tracks]
    seqs = [t for t in tracks if t.kind == 1]
    ro = np.concatenate([[0], np.cumsum([len(t.start) for t in recs])]).astype(np.int64)
    so = np.concatenate([[0], np.cumsum([T if t.kind == 1 else 0 for t in tracks])]).astype(np.int64)
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), dtype=dt)
    start, end = cat([t.start for t in recs], np.int64), cat([t.end for t in recs], np.int64)
    sym0, sym = cat([t.sym0 for t in recs], np.uint8), cat([t.sym for t in recs], np.uint8)
    assert len(start) == len(end) == len(sym0) == len(sym) == ro[-1]
    for t in seqs:
        assert t.bytes.shape == (T,) and t.lut.shape == (256,)
    sb, lut = cat([t.bytes for t in seqs], np.uint8), cat([t.lut for t in seqs], np.uint8)
    data = np.empty((T, K), dtype=np.uint8)
    some = lambda a: ptr(a, u8p if a.dtype == np.uint8 else i64p) if len(a) else None
    _lib.check(_lib.load().tehmm_load_tracks_u8(
        T, K, ptr(fill, u8p), ptr(kind, u8p), ptr(ro, i64p), some(start), some(end), some(sym0), some(sym),
        ptr(so, i64p), some(sb), some(lut), ptr(data, u8p) if T else None), "tehmm_load_tracks_u8")
    return data


class FloatTrack(object):
    """one numeric track: records in row coordinates, sorted by start, a float32 value each"""

    def __init__(self, fill=0.0, start=None, end=None, val=None):
        z = np.zeros(0, dtype=np.int64)
        self.fill = np.float32(fill)
        self.start = z if start is None else np.ascontiguousarray(start, dtype=np.int64)
        self.end = z if end is None else np.ascontiguousarray(end, dtype=np.int64)
        self.val = np.zeros(0, dtype=np.float32) if val is None else np.ascontiguousarray(val, dtype=np.float32)
        assert len(self.start) == len(self.end) == len(self.val)


def _record_lists(tracks):
    ro = np.concatenate([[0], np.cumsum([len(t.start) for t in tracks])]).astype(np.int64)
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), dtype=dt)
    return ro, cat([t.start for t in tracks], np.int64), cat([t.end for t in tracks], np.int64), cat


def rowsWon(T, tracks):
    """(rows won by every record: one int64 array per track, uncovered rows: int64 [K]) of tehmm_track_rows_won for a
    list of tracks with .start / .end"""
    T, K = int(T), len(tracks)
    ro, start, end, _ = _record_lists(tracks)
    won, uncovered = np.zeros(int(ro[-1]), dtype=np.int64), np.zeros(K, dtype=np.int64)
    some = lambda a: ptr(a, i64p) if len(a) else None
    _lib.check(_lib.load().tehmm_track_rows_won(T, K, ptr(ro, i64p), some(start), some(end), some(won),
                                                ptr(uncovered, i64p)), "tehmm_track_rows_won")
    return [won[ro[k]:ro[k + 1]] for k in range(K)], uncovered


def paintTracksFloat(T, tracks):
    """float32 [K, T] of tehmm_load_tracks_f32 for a list of FloatTrack (one contiguous row array per track)"""
    T, K = int(T), len(tracks)
    ro, start, end, cat = _record_lists(tracks)
    fill, val = np.asarray([t.fill for t in tracks], dtype=np.float32), cat([t.val for t in tracks], np.float32)
    out = np.empty((K, T), dtype=np.float32)
    some = lambda a: ptr(a, f32p if a.dtype == np.float32 else i64p) if len(a) else None
    _lib.check(_lib.load().tehmm_load_tracks_f32(T, K, ptr(fill, f32p), ptr(ro, i64p), some(start), some(end),
                                                 some(val), ptr(out, f32p) if T else None), "tehmm_load_tracks_f32")
    return out


def recordValues(bed, pick, valCol, name):
    """float32 value of the selected records without a value map: np.float32(float(text)), 1 for valCol 0"""
    if valCol is not None and int(valCol) not in (0, 3, 4):
        raise ValueError("track %s: valCol is 0, 3 or 4" % name)
    col = 3 if valCol is None else int(valCol)
    if col == 0 or len(pick) == 0:
        return np.ones(len(pick), dtype=np.float32)
    code, values = bed.codes(col)
    uniq, inv = np.unique(code[pick], return_inverse=True)
    first = bed.columns.codeFirst(col)[uniq]          # a value's float is that of the record it first appears in
    fval, certified = bed.columns.floats(col)
    with np.errstate(over="ignore"):
        table = np.asarray([np.float32(fval[r] if certified[r] else float(values[int(u)]))
                            for u, r in zip(uniq.tolist(), first.tolist())], dtype=np.float32)
    if not np.isfinite(table).all():
        raise ValueError("track %s: a value that is not finite (%s)" % (name, table[~np.isfinite(table)][0]))
    return table[inv.reshape(-1)]


def lastTiming():
    """[(pass, milliseconds)] of the device passes of this thread's last tehmm_load_tracks_u8, tehmm_track_rows_won or
    tehmm_load_tracks_f32"""
    names = (ctypes.c_char_p * 16)()
    ms = (ctypes.c_double * 16)()
    n = _lib.load().tehmm_trackio_last_timing(16, names, ms)
    _lib.check(min(n, 0), "tehmm_trackio_last_timing")
    return [(names[i].decode(), ms[i]) for i in range(n)]


# ---- one track over a list of tables -----------------------------------------------------------------------------------
class TrackSource(object):
    """A track file read once; columns of any number of tables come from it."""

    def __init__(self, path):
        if not os.path.isfile(path):
            raise RuntimeError("Track file not found %s\n" % path)
        self.path = path
        ext = os.path.splitext(path)[1]
        self.bed = self.sequences = None
        if ext in (".bw", ".bigwig", ".wg", ".bb", ".bigbed"):
            raise RuntimeError("%s: bigWig / bigBed tracks need bigWigToBedGraph / bigBedToBed, which are not offered; "
                               "convert the file to BED" % path)
        if ext == ".bed":
            self.bed = BedFile(path)
        elif ext[:3].lower() == ".fa":
            from .tsd import readFasta
            self.sequences = readFasta(path)
        else:
            sys.stderr.write("Warning: non-BED, non-FASTA file skipped %s\n" % path)


class ColumnBuilder(object):
    """The records (or bytes) of one table column, gathered table after table in the call's row space."""

    def __init__(self, valMap, name):
        self.valMap, self.name = valMap, name
        self.parts, self.seq_parts = [], []
        self.caseSensitive = False

    def add(self, source, offset, chrom, start, end, valCol=None, updateValMap=False, useDelta=False,
            caseSensitive=False):
        """the table chrom:start-end lies at rows offset .. offset + end - start; updates the map as the reference"""
        if source.bed is not None:
            pick, oStart, oEnd = source.bed.select(chrom, start, end)
            sym0, sym = recordSymbols(source.bed, pick, oStart, oEnd, chrom, valCol, self.valMap, updateValMap,
                                      useDelta, self.name)
            self.parts.append((oStart - start + offset, oEnd - start + offset, sym0, sym))
        elif source.sequences is not None:
            row = fastaBytes(source.sequences, chrom, start, end)
            fastaUpdate(row, self.valMap, caseSensitive, updateValMap)
            self.caseSensitive = caseSensitive
            self.seq_parts.append((offset, row))

    def track(self, T):
        fill = int(self.valMap.getMissingVal())
        if not 0 <= fill <= MAX_SYMBOL:
            raise ValueError("track %s: missing value %d does not fit the uint8 table" % (self.name, fill))
        if self.seq_parts:
            assert not self.parts
            b = np.zeros(T, dtype=np.uint8)
            for offset, row in self.seq_parts:
                b[offset:offset + len(row)] = row
            return SequenceTrack(fill, b, fastaLut(self.valMap, self.caseSensitive, self.name))
        cols = [np.concatenate(c) for c in zip(*self.parts)] or [None] * 4
        return RecordTrack(fill, *cols)


# ---- the reference's functions -----------------------------------------------------------------------------------------
def _finish(row, outputBuf):
    if outputBuf is None:
        return row
    outputBuf[...] = row
    return outputBuf


def _one_float(source, chrom, start, end, kwargs, name):
    """the float rows of one BED track: painted over what outputBuf holds (NaN marks the rows nothing covers; record
    values are finite)"""
    if source.bed is None:
        raise ValueError("a value map is required: %s is not a BED file" % name)
    if kwargs.get("useDelta") is True:
        raise ValueError("track %s: useDelta is not offered without a value map" % name)
    pick, oStart, oEnd = source.bed.select(chrom, start, end)
    track = FloatTrack(np.nan, oStart - start, oEnd - start, recordValues(source.bed, pick, kwargs.get("valCol"), name))
    row = paintTracksFloat(end - start, [track])[0]
    outputBuf = kwargs["outputBuf"]
    covered = ~np.isnan(row)
    outputBuf[covered] = row[covered]
    return outputBuf


def _one(trackPath, chrom, start, end, kwargs, want):
    valMap = kwargs.get("valMap")
    outputBuf = kwargs.get("outputBuf")
    floatRows = valMap is None and outputBuf is not None and outputBuf.dtype == np.float32
    if valMap is None and not floatRows:
        raise ValueError("a value map is required: the rows are bytes")
    for key in kwargs:
        if key not in ("valCol", "valMap", "updateValMap", "useDelta", "caseSensitive", "outputBuf"):
            raise TypeError("unexpected keyword argument %r" % key)
    source = TrackSource(trackPath)
    if want == "bed" and source.bed is None or want == "fasta" and source.sequences is None:
        raise RuntimeError("%s is not a %s file" % (trackPath, want))
    if source.bed is None and source.sequences is None:
        return None
    if floatRows:
        return _one_float(source, chrom, int(start), int(end), kwargs, os.path.basename(trackPath))
    col = ColumnBuilder(valMap, os.path.basename(trackPath))
    col.add(source, 0, chrom, int(start), int(end), valCol=kwargs.get("valCol"),
            updateValMap=bool(kwargs.get("updateValMap", False)), useDelta=bool(kwargs.get("useDelta", False)),
            caseSensitive=bool(kwargs.get("caseSensitive", False)))
    T = int(end) - int(start)
    return _finish(paintTracks(T, [col.track(T)])[:, 0], kwargs.get("outputBuf"))


def readBedData(bedPath, chrom, start, end, **kwargs):
    """One value per base of chrom:start-end from a BED file (trackIO.py:67-212): a uint8 array, or outputBuf filled."""
    return _one(bedPath, chrom, start, end, kwargs, "bed")


def readFastaData(faPath, chrom, start, end, **kwargs):
    """One value per base of chrom:start-end from a FASTA file (trackIO.py:305-360)."""
    return _one(faPath, chrom, start, end, kwargs, "fasta")


def readTrackData(trackPath, chrom=None, start=None, end=None, **kwargs):
    """Dispatch on the extension as trackIO.py:23-63: .bed, .fa*; other files are skipped with a warning (None)."""
    if not os.path.isfile(trackPath):
        raise RuntimeError("Track file not found %s\n" % trackPath)
    return _one(trackPath, chrom, start, end, kwargs, None)
