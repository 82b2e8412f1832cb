"""The data contract the hot path consumes: TrackTable / IntegerTrackTable (track.py:352-662).

A table is a uint8 [T, K] array, one row per position (``getNumPyArray``), with optional segment offsets and
``getSegmentLengthsAsRatio``.  ``readTrackList`` reads the XML track list, ``TrackData.loadTrackData`` turns it and its
BED / FASTA files into tables: all tables of a call are painted by one device call (trackIO.py),
then masked and segmented by the calls below.
"""
import logging
import xml.etree.ElementTree as ET

import numpy as np

logger = logging.getLogger("tehmm_amd")

INTEGER_ARRAY_TYPE = np.uint8   # track.py:23


class TrackTable(object):
    def __init__(self, numTracks, chrom, start, end):
        assert end > start
        self.numTracks = numTracks
        self.chrom = chrom
        self.start = start
        self.end = end
        self.origEnd = end
        self.segOffsets = None
        self.maskArray = None
        self.shape = (len(self), self.getNumTracks())

    def __len__(self):
        if self.segOffsets is None:
            return self.end - self.start
        return len(self.segOffsets)

    def getNumTracks(self):
        return self.numTracks

    def getChrom(self):
        return self.chrom

    def getStart(self):
        return self.start

    def getEnd(self):
        return self.end

    def getNumPyArray(self):
        raise RuntimeError("Not implemented")

    def getSegmentOffsets(self):
        return self.segOffsets

    def setSegmentOffsets(self, segOffsets):
        """Attach segment offsets to an already-compressed table (one row per segment)."""
        self.segOffsets = None if segOffsets is None else np.asarray(segOffsets, dtype=np.int64)
        self.shape = (len(self), self.getNumTracks())

    def getSegmentLength(self, i):
        """track.py:497-502."""
        if i == len(self.segOffsets) - 1:
            return self.end - (self.start + self.segOffsets[-1])
        elif i < len(self.segOffsets) - 1:
            return self.segOffsets[i + 1] - self.segOffsets[i]

    def getOverlapInTableCoords(self, bedInterval, startHint=None):
        """track.py:390-432: overlap of a genome-coordinate BED interval with this table, in TABLE
        coordinates (segment indices when the table is segmented), or None.  Binary search instead
        of the reference's linear scan from startHint (same result)."""
        assert len(bedInterval) > 2
        chrom, start, end = bedInterval[0], bedInterval[1], bedInterval[2]
        if not (self.chrom == chrom and self.start < end and self.end > start):
            return None
        overlap = [self.chrom, max(self.start, start), min(self.end, end)] + list(bedInterval[3:])
        if self.segOffsets is not None:
            offs = np.asarray(self.segOffsets, dtype=np.int64)
            genStart, genEnd = overlap[1] - self.start, overlap[2] - self.start
            if genStart < offs[0]:
                return None                                    # starts before the first segment
            first = int(np.searchsorted(offs, genStart, side="right")) - 1
            last = int(np.searchsorted(offs, genEnd, side="left")) - 1     # segment holding genEnd - 1
            if last < first:
                return None
            overlap[1], overlap[2] = first, last + 1
        else:
            overlap[1] -= self.start
            overlap[2] -= self.start
        return overlap

    def segment(self, segIntervals, trackList, interpolate=True):
        """track.py:449-495: keep one row per segment interval (chrom, start, end, ...).  Offsets (and
        the skipping of fully masked segments) are computed here; the O(T) work -- per-segment mode of
        the categorical tracks, mean of the gaussian ones, the gather -- is one device call
        (tehmm_segment_table_u8)."""
        import ctypes
        from . import _lib
        from ._lib import f64p, i64p, ptr, u8p
        first_end = self.origEnd if self.maskArray is not None else self.end
        if hasattr(segIntervals, "intervals"):          # BedColumns: its intervals in file order
            segIntervals = segIntervals.intervals(sort=False)
        if hasattr(segIntervals, "window"):             # IntervalColumns: binary searches instead of the scan
            segStart, segEnd = segIntervals.window(self.chrom, self.start, first_end)
            assert len(segStart) and segStart[0] == self.start and segEnd[-1] == first_end
            offs = (segStart - self.start).astype(np.int64)
        else:
            ivs = [iv for iv in segIntervals if iv[0] == self.chrom and iv[1] >= self.start and iv[2] <= first_end]
            assert ivs and ivs[0][1] == self.start and ivs[-1][2] == first_end
            offs = np.asarray([int(iv[1]) - self.start for iv in ivs], dtype=np.int64)
        if self.maskArray is not None:
            run = self.getMaskRunningOffsets(reverseTransform=True)
            kept = self.maskArray[offs]                 # a segment is either all kept or all cut
            offs = (offs - run[offs])[kept]
        self.segOffsets = offs
        if len(offs) == 0:
            self.shape = (0, self.getNumTracks())
            return
        data = np.ascontiguousarray(self.data, dtype=np.uint8)
        T, K = data.shape
        is_g = np.zeros(K, dtype=np.uint8)
        mapback = np.zeros((K, 256), dtype=np.float64)
        if interpolate:
            for track in trackList:
                if track.getDist() == "gaussian":
                    is_g[track.getNumber()] = 1
                    mapback[track.getNumber()] = track.getValueMap().getMapBackTable(np.uint8)
        out = np.zeros((len(offs), K), dtype=np.uint8)
        means = np.zeros((len(offs), K), dtype=np.float64)
        if interpolate:
            _lib.check(_lib.load().tehmm_segment_table_u8(
                T, K, ptr(data, u8p), len(offs), ptr(offs, i64p), ptr(is_g, u8p), ptr(mapback, f64p),
                ptr(out, u8p), ptr(means, f64p)), "tehmm_segment_table_u8")
            for track in trackList:                     # O(segments): may create new symbols
                if track.getDist() == "gaussian":
                    k, vm = track.getNumber(), track.getValueMap()
                    out[:, k] = [vm.getMap(mv, update=True) for mv in means[:, k]]
        else:
            out = data[offs]
        del ctypes
        self.data = out
        self.shape = (len(self), self.getNumTracks())

    def getSegmentLengthsAsRatio(self, effectiveSegmentLength):
        """track.py:504-513, vectorised: segment length / effective segment length."""
        if self.segOffsets is None:
            return None
        eff = float(effectiveSegmentLength)
        assert eff >= 1
        offs = np.asarray(self.segOffsets, dtype=np.int64)
        ends = np.concatenate([offs[1:], [self.end - self.start]])
        return (ends - offs).astype(np.float64) / eff


class IntegerTrackTable(TrackTable):
    def __init__(self, numTracks, chrom, start, end, dtype=INTEGER_ARRAY_TYPE):
        super(IntegerTrackTable, self).__init__(numTracks, chrom, start, end)
        self.data = np.zeros((end - start, numTracks), dtype=dtype)
        self.iinfo = np.iinfo(dtype)
        self.maskArray = None

    def __getitem__(self, index):
        return self.data[index]

    def writeRow(self, row, rowArray):
        """Write one track (row) of values, clamping to the dtype range (track.py:563-580)."""
        assert row < self.getNumTracks()
        assert len(rowArray) == len(self)
        self.data[:, row] = np.clip(np.asarray(rowArray), self.iinfo.min, self.iinfo.max)

    def getNumPyArray(self):
        return self.data

    def getRow(self, row):
        return self.data[:, row]

    def initRow(self, row, val):
        self.data[:, row] = val

    def setData(self, data):
        data = np.ascontiguousarray(data, dtype=self.data.dtype)
        assert data.ndim == 2 and data.shape[1] == self.numTracks
        self.data = data
        return self

    def setMaskTable(self, maskTable):
        """track.py:622-645: cut out every position a (binary) mask track covers; the flags, the running
        offsets (_track.runSum) and the compaction are one device call (tehmm_mask_table_u8)."""
        from . import _lib
        from ._lib import i32p, i64p, ptr, u8p
        self.maskArray = None
        if maskTable is None:
            return
        data = np.ascontiguousarray(self.data, dtype=np.uint8)
        mask = np.ascontiguousarray(maskTable.data, dtype=np.uint8)
        T, K = data.shape
        assert mask.shape[0] == T
        keep = np.zeros(T, dtype=np.uint8)
        run_full = np.zeros(T, dtype=np.int32)
        out = np.zeros((T, K), dtype=np.uint8)
        run_masked = np.zeros(T, dtype=np.int32)
        nk = np.zeros(1, dtype=np.int64)
        _lib.check(_lib.load().tehmm_mask_table_u8(T, K, ptr(data, u8p), mask.shape[1], ptr(mask, u8p),
                                                   ptr(keep, u8p), ptr(run_full, i32p), ptr(out, u8p),
                                                   ptr(run_masked, i32p), ptr(nk, i64p)), "tehmm_mask_table_u8")
        n = int(nk[0])
        self.maskArray = keep.astype(bool)
        self._run_full, self._run_masked = run_full, run_masked[:n].copy()
        self.data = out[:n].copy()
        self.shape = self.data.shape
        self.origEnd = self.end
        self.end = self.start + n

    def hasMask(self):
        return self.maskArray is not None

    def getMaskRunningOffsets(self, reverseTransform=False):
        """track.py:650-662: number of cut bases before every position (of the uncut table when
        reverseTransform, else of the kept rows)."""
        if not self.hasMask():
            return None
        return self._run_full if reverseTransform else self._run_masked


class CategoryMap(object):
    """Value <-> symbol dictionary of a track (track.py:668-799): symbols are handed out in order of
    first appearance starting at `reserved`; numeric tracks bin their values first
    (key = str(int(scale * (value + shift))) or str(int(log_base(value + shift))))."""

    def __init__(self, reserved=1, defaultVal=None, scale=None, logScale=None, shift=None):
        self.fwd, self.back = {}, {}
        self.reserved = reserved
        self.scale = None if logScale is not None else scale
        self.logBase = logScale
        self.shift = None if shift is None else float(shift)
        self.defaultVal = defaultVal
        self.missingVal = max(0, reserved - 1)
        if defaultVal is not None:
            self.missingVal = int(self.getMap(defaultVal, update=True))

    def _key(self, x):
        y = x if self.shift is None else float(x) + self.shift
        if self.scale is not None:
            return str(int(self.scale * float(y)))
        if self.logBase is not None:
            return str(int(np.log(float(y)) / np.log(self.logBase)))
        return y

    def _unkey(self, key):
        y = key
        if self.scale is not None:
            y = float(key) / float(self.scale)
        elif self.logBase is not None:
            y = float(self.logBase) ** float(key)
        return y if self.shift is None else float(y) - self.shift

    def update(self, value):
        key = self._key(value)
        if key not in self.fwd:
            sym = len(self.fwd) + self.reserved
            self.fwd[key], self.back[sym] = sym, key

    def has(self, value):
        return self._key(value) in self.fwd

    def getMap(self, value, update=False):
        key = self._key(value)
        if update and key is not None and key not in self.fwd:
            self.update(value)
        return self.fwd.get(key, self.missingVal)

    def getMapBack(self, sym):
        if sym in self.back:
            return self._unkey(self.back[sym])
        if self.defaultVal is not None:
            return self._unkey(self.back[self.getMap(self.defaultVal)])
        return None

    def getMapBackTable(self, dtype):
        table = np.full(int(np.iinfo(dtype).max) + 1, float(np.iinfo(np.int64).max), dtype=np.float64)
        for sym in range(len(table)):
            v = self.getMapBack(sym)
            if v is not None:
                table[sym] = v
        return table

    def getMissingVal(self):
        return self.missingVal

    def getReserved(self):
        return self.reserved

    def __len__(self):
        return len(self.fwd) + max(0, self.reserved - 1)

    def sort(self):
        """Re-number so that symbols ascend with the (numeric where possible) keys."""
        keys = list(self.fwd)
        try:
            order = sorted(keys, key=float)
        except (TypeError, ValueError):
            order = sorted(keys)
        self.fwd = {k: i + self.reserved for i, k in enumerate(order)}
        self.back = {v: k for k, v in self.fwd.items()}


class BinaryMap(CategoryMap):
    """Value map of binary and mask tracks (track.py:816-832): 1 = nothing there, 2 = covered."""

    def __init__(self):
        super(BinaryMap, self).__init__()

    def getMap(self, value, update=False):
        return 2 if value is not None else 1

    def getMapBack(self, sym):
        return sym - 1

    def getMissingVal(self):
        return 1

    def __len__(self):
        return 2


class IdentityValueMap(object):
    """Value map of a numeric (binned) track: symbol s (1-based, 0 = missing) <-> value s - 1.
    Stands in for CategoryMap (track.py:668-760) where only getMapBack is needed (the gaussian
    re-fit of the M-step, emission.py:520-545)."""

    def __init__(self, scale=1.0, shift=0.0):
        self.scale = float(scale)
        self.shift = float(shift)

    def getMapBack(self, symbol):
        return (float(symbol) - 1.0) * self.scale + self.shift

    def getMap(self, value, update=False):
        return int(round((float(value) - self.shift) / self.scale)) + 1


DISTRIBUTIONS = ("binary", "multinomial", "sparse_multinomial", "alignment", "gaussian", "mask")
PREPROCESSORS = ("rm", "rmu", "ltr_finder", "termini", "overlap")


class Track(object):
    """The per-track metadata (track.py:27-229).  With a path (a track of the XML list) and no value map, the map is
    built as the reference's Track._init does: a CategoryMap with 2 reserved symbols, or 1 with a default value (which
    a gaussian track must have); a BinaryMap for binary and mask tracks, which also take their value from the record's
    presence (valCol 0)."""

    def __init__(self, name=None, number=-1, dist="multinomial", valueMap=None, path=None, valCol=3, scale=None,
                 logScale=None, shift=None, delta=False, defaultVal=None, caseSensitive=False, preprocess=None):
        self.name = name
        self.number = number
        self.dist = dist
        self.path = path
        self.valCol = valCol
        self.scale = scale
        self.logScale = logScale
        self.shift = shift
        self.delta = delta
        self.defaultVal = defaultVal
        self.caseSensitive = caseSensitive
        self.preprocess = preprocess
        if valueMap is not None:
            self.valueMap = valueMap
        elif path is not None:
            self.valueMap = self._referenceMap()
        else:
            self.valueMap = IdentityValueMap()

    def _referenceMap(self):
        if self.dist not in ("multinomial", "binary", "alignment", "gaussian", "mask"):
            raise ValueError("track %s: distribution %r is not one of multinomial, binary, alignment, gaussian, mask"
                             % (self.name, self.dist))
        if self.delta and self.logScale is not None:
            raise RuntimeError("track %s: delta attribute not compatible with logScale" % self.name)
        if self.dist in ("binary", "mask"):
            self.valCol = 0
            return BinaryMap()
        if self.dist == "alignment":
            return CategoryMap(reserved=1)
        reserved = 2
        if self.defaultVal is not None:
            reserved = 1
        elif self.dist == "gaussian":
            raise RuntimeError("\"default\" attribute must be specified for gaussian distribution (track %s)"
                               % self.name)
        return CategoryMap(reserved=reserved, defaultVal=self.defaultVal, scale=self.scale, logScale=self.logScale,
                           shift=self.shift)

    @classmethod
    def fromXMLElement(cls, elem, number=-1):
        """A <track> element of the list (track.py:101-146)."""
        a = elem.attrib
        truth = lambda key: a.get(key, "").lower() in ("1", "true")
        number_of = lambda key, kind: kind(a[key]) if key in a else None
        name = a["name"]
        dist = a.get("distribution", "multinomial")
        if dist not in DISTRIBUTIONS:
            raise ValueError("track %s: unknown distribution %r" % (name, dist))
        logScale, shift = number_of("logScale", float), number_of("shift", float)
        # (a default is a number, as in the reference: float() raises on anything else)
        if "default" in a and float(a["default"]) <= 0. and logScale is not None and (
                shift is None or shift + float(a["default"]) <= 0):
            raise RuntimeError("track %s: default set to %s in conjunction with logScale requires shift attribute set "
                               "to at least %f" % (name, a["default"], 1. - float(a["default"])))
        if "preprocess" in a and a["preprocess"] not in PREPROCESSORS:
            raise RuntimeError("track %s: preprocess set to invalid value %s.  must be rm, rmu, ltr_finder, termini or "
                               "overlap" % (name, a["preprocess"]))
        return cls(name, number, dist, path=a["path"], valCol=int(a.get("valCol", 3)), scale=number_of("scale", float),
                   logScale=logScale, shift=shift, delta=truth("delta"), defaultVal=a.get("default"),
                   caseSensitive=truth("caseSensitive"), preprocess=a.get("preprocess"))

    def getName(self):
        return self.name

    def getNumber(self):
        return self.number

    def getDist(self):
        return self.dist

    def getValueMap(self):
        return self.valueMap

    def getPath(self):
        return self.path

    def getValCol(self):
        return self.valCol

    def getScale(self):
        return self.scale

    def getLogScale(self):
        return self.logScale

    def getShift(self):
        return self.shift

    def getDelta(self):
        return self.delta

    def getDefaultVal(self):
        return self.defaultVal

    def getCaseSensitive(self):
        return self.caseSensitive

    def getPreprocess(self):
        return self.preprocess

    # the setters the scaling tool uses (track.py:202-217); the value map built at construction is not rebuilt, as in
    # the reference: the attributes take effect in the list read back from the saved XML
    def setScale(self, scale):
        self.scale = scale
        self.logScale = None

    def setLogScale(self, logScale):
        self.logScale = logScale
        self.scale = None

    def setShift(self, shift):
        self.shift = shift

    def toXMLElement(self):
        """The <track> element of this track (track.py:148-173): logScale wins over scale, false flags are left out."""
        elem = ET.Element("track")
        put = lambda key, val: elem.attrib.__setitem__(key, str(val))
        if self.name is not None:
            put("name", self.name)
        if self.path is not None:
            put("path", self.path)
        if self.dist is not None:
            put("distribution", self.dist)
        if self.valCol is not None:
            put("valCol", self.valCol)
        if self.logScale is not None:
            put("logScale", self.logScale)
        elif self.scale is not None:
            put("scale", self.scale)
        if self.shift is not None:
            put("shift", self.shift)
        if self.caseSensitive is not None and self.caseSensitive is not False:
            put("caseSensitive", self.caseSensitive)
        if self.delta is True:
            put("delta", "True")
        if self.defaultVal is not None:
            put("default", self.defaultVal)
        if self.preprocess is not None:
            put("preprocess", self.preprocess)
        return elem


class TrackList(list):
    """The tracks of a model, by number; mask tracks (track.py:235-346) are kept beside them."""

    def getTrackByNumber(self, n):
        return self[n]

    def getMaskTracks(self):
        return self.__dict__.setdefault("maskTrackList", [])

    def getTrackByName(self, name, isMask=False):
        for t in (self.getMaskTracks() if isMask else self):
            if t.getName() == name:
                return t
        return None

    def getAlignmentTrack(self):
        """The one alignment track (track.py:277-278), kept apart from the tracks a model emits; None without one."""
        return self.__dict__.get("alignmentTrack")

    def addTrack(self, track, treatMaskAsBinary=False, allowAlignment=False):
        """track.py:280-294: the track's number becomes its position in its list.  An alignment track is read by the
        grammar model alone: only a caller that says so (allowAlignment) gets one, at most one, number 0."""
        names = [t.getName() for t in self] + [t.getName() for t in self.getMaskTracks()]
        if self.getAlignmentTrack() is not None:
            names.append(self.getAlignmentTrack().getName())
        if track.getDist() == "alignment":
            if not allowAlignment:
                raise NotImplementedError("track %s: alignment tracks belong to the grammar model (--cfg); no other "
                                          "path reads them" % track.getName())
            if self.getAlignmentTrack() is not None:
                raise RuntimeError("Only one track with alignment distribution permitted")
            if track.getName() in names:
                raise ValueError("track name %s appears twice" % track.getName())
            track.number = 0
            self.__dict__["alignmentTrack"] = track
            return
        if track.getName() in names:
            raise ValueError("track name %s appears twice" % track.getName())
        target = self.getMaskTracks() if track.getDist() == "mask" and not treatMaskAsBinary else self
        track.number = len(target)
        target.append(track)

    def saveXML(self, path):
        """track.py:322-332: the tracks, then the mask tracks, below a teModelConfig root, pretty-printed"""
        import xml.dom.minidom
        root = ET.Element("teModelConfig")
        for track in list(self) + self.getMaskTracks():
            root.append(track.toXMLElement())
        if self.getAlignmentTrack() is not None:
            root.append(self.getAlignmentTrack().toXMLElement())
        with open(path, "w") as f:
            f.write(xml.dom.minidom.parseString(ET.tostring(root)).toprettyxml())


def readTrackList(xmlPath, treatMaskAsBinary=False, allowAlignment=False):
    """The TrackList of an XML track list: the <track> elements below its root (track.py:308-320)."""
    tracks = TrackList()
    for child in ET.parse(xmlPath).getroot().findall("track"):
        tracks.addTrack(Track.fromXMLElement(child), treatMaskAsBinary, allowAlignment)
    return tracks


class TrackData(object):
    """Container of the TrackTables of a set of intervals (track.py:838-977)."""

    def __init__(self, trackTableList=None, trackList=None, numSymbolsPerTrack=None):
        self.trackTableList = list(trackTableList) if trackTableList is not None else []
        self.trackList = trackList
        self.numSymbolsPerTrack = numSymbolsPerTrack
        self.alignmentTrackTableList = []

    def getTrackTableList(self):
        return self.trackTableList

    def getAlignmentTrackTableList(self):
        """One 1-row uint16 table per interval when the track list holds an alignment track, else empty."""
        return self.alignmentTrackTableList

    def getTrackList(self):
        return self.trackList

    def getNumTracks(self):
        return self.trackTableList[0].getNumTracks() if self.trackTableList else 0

    def getNumTrackTables(self):
        return len(self.trackTableList)

    def getNumSymbolsPerTrack(self):
        if self.numSymbolsPerTrack is None and self.trackList is not None and all(
                hasattr(t.getValueMap(), "__len__") for t in self.trackList):
            return [len(t.getValueMap()) for t in self.trackList]      # no list given: what the value maps hold
        return self.numSymbolsPerTrack

    def loadTrackData(self, trackListPath, intervals, trackList=None, segmentIntervals=None, interpolateSegments=True,
                      applyMasking=True, treatMaskAsBinary=False, allowAlignment=False):
        """track.py:874-955: the tables of the intervals (chrom, start, end, ...) from the files of an XML track list.
        trackList None: the list is the XML's and its value maps learn the values, in (interval, track) order; else the
        given (learned) list maps them, unseen values go to the missing value, and tracks it does not know are skipped
        with a warning.  Every file is parsed once; all tables are painted by one device call (mask tracks by a
        second), then masked (setMaskTable) and, with segmentIntervals, segmented (segment; tables left empty by the
        mask are dropped).  Only when a gaussian track can learn symbols while segments are interpolated is the paint
        done table by table, so that its map sees the values in the reference's order."""
        from . import trackIO
        assert len(intervals) > 0
        inputList = readTrackList(trackListPath, treatMaskAsBinary, allowAlignment)
        init = trackList is None
        self.trackList = inputList if init else trackList
        self.numSymbolsPerTrack = None
        self.trackTableList = []
        self.alignmentTrackTableList = []
        numTracks = len(self.trackList)
        if numTracks < 1 or numTracks > trackIO.MAX_TRACKS:
            raise ValueError("%d tracks: a table holds 1 to %d" % (numTracks, trackIO.MAX_TRACKS))
        plan = []                                      # (input track, the track whose map and number count, is mask)
        for isMask, group in ((False, inputList), (True, inputList.getMaskTracks())):
            for inputTrack in group:
                selfTrack = self.trackList.getTrackByName(inputTrack.getName(), isMask)
                if selfTrack is None and not isMask:
                    logger.warning("track %s not learned\n" % inputTrack.getName())
                    continue
                plan.append((inputTrack, inputTrack if selfTrack is None else selfTrack, isMask))
        sources = dict()
        for inputTrack, _, _ in plan:
            if inputTrack.getPath() not in sources:
                sources[inputTrack.getPath()] = trackIO.TrackSource(inputTrack.getPath())
        numMask = len(inputList.getMaskTracks())
        for interval in intervals:
            assert len(interval) >= 3 and interval[2] > interval[1]
        oneByOne = init and segmentIntervals is not None and interpolateSegments and any(
            t.getDist() == "gaussian" for t in self.trackList)
        groups = [[iv] for iv in intervals] if oneByOne else [list(intervals)]
        for group in groups:
            offsets = np.concatenate([[0], np.cumsum([int(iv[2]) - int(iv[1]) for iv in group])]).astype(np.int64)
            T = int(offsets[-1])
            columns = [None] * numTracks
            maskColumns = [None] * numMask
            for x, iv in enumerate(group):
                for inputTrack, selfTrack, isMask in plan:
                    cols = maskColumns if isMask else columns
                    k = selfTrack.getNumber()
                    if cols[k] is None:
                        cols[k] = trackIO.ColumnBuilder(selfTrack.getValueMap(), selfTrack.getName())
                    cols[k].add(sources[inputTrack.getPath()], int(offsets[x]), iv[0], int(iv[1]), int(iv[2]),
                                valCol=inputTrack.getValCol(), updateValMap=init, useDelta=inputTrack.getDelta(),
                                caseSensitive=inputTrack.getCaseSensitive())
            blank = trackIO.RecordTrack(0)             # a column nothing is read into stays 0, as in the reference
            data = trackIO.paintTracks(T, [blank if c is None else c.track(T) for c in columns])
            mask = trackIO.paintTracks(T, [blank if c is None else c.track(T) for c in maskColumns]) if numMask else None
            for x, iv in enumerate(group):
                a, b = int(offsets[x]), int(offsets[x + 1])
                table = IntegerTrackTable(numTracks, iv[0], int(iv[1]), int(iv[2])).setData(data[a:b].copy())
                if applyMasking and mask is not None:
                    table.setMaskTable(IntegerTrackTable(numMask, iv[0], int(iv[1]), int(iv[2])).setData(
                        mask[a:b].copy()))
                if segmentIntervals is not None and table.getNumPyArray().shape[0] == 0:
                    continue
                if segmentIntervals is not None:
                    table.segment(segmentIntervals, self.trackList, interpolate=interpolateSegments)
                self.trackTableList.append(table)
        # the alignment track (track.py:957-968): one uint16 row per interval, its own value map learning every value
        # (the grammar model only compares its symbols with each other and with the default symbol 0)
        inputTrack = inputList.getAlignmentTrack()
        selfTrack = self.trackList.getAlignmentTrack()
        if allowAlignment and inputTrack is not None and selfTrack is not None:
            if segmentIntervals is not None or any(t.hasMask() for t in self.trackTableList):
                raise RuntimeError("an alignment track cannot follow rows that a mask or segments have cut out")
            for iv in intervals:
                row = trackIO.readTrackData(inputTrack.getPath(), iv[0], int(iv[1]), int(iv[2]),
                                            valCol=inputTrack.getValCol(), valMap=selfTrack.getValueMap(),
                                            updateValMap=True)
                table = IntegerTrackTable(1, iv[0], int(iv[1]), int(iv[2]), dtype=np.uint16)
                table.writeRow(0, row)
                self.alignmentTrackTableList.append(table)
