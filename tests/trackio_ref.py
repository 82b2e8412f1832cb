"""Plain, slow Python statement of what tehmm_amd/trackIO.py and TrackData.loadTrackData compute,
used by the tests as the thing to be equal to, and the seeded cases they and tests/golden/make_golden_trackio.py run on.

The rule for one track over one table [start, end) of chromosome c:
  1. records: lines starting with '#' are skipped, fields are split on tabs, lines with fewer than 3 fields are skipped;
  2. kept when chrom == c, e > start and s < end; clipped to oStart = max(start, s), oEnd = min(end, e); sorted stably
     by oStart, i.e. file order among equal clipped starts.  This stands in for the reference's ``intersectBed -a file
     -b interval | sortBed``.  bedtools does not define the order among records of equal start: where such records
     overlap, the reference's own result depends on the bedtools at hand, and the order stated here is a choice;
  3. every record gives (sym0, sym) through the track's value map, the map asked for val first and val0 second;
  4. rows start at the map's missing value; record r writes sym0 at row oStart - start and sym at the rows behind it
     up to oEnd - start - 1, in sorted order.  Said as a search (paint_by_search): row p takes its value from the
     largest i in sorted order with oStart_i <= p < oEnd_i, sym0_i if p == oStart_i and sym_i otherwise.
FASTA tracks: row i is the map of base start + i of record c, upper-cased unless caseSensitive; rows past the end of
the sequence keep the missing value; with update, new symbols in order of first appearance.
"""
import json
import math

import numpy as np


# ---- value maps (track.py:668-832 of the reference, restated) -----------------------------------------------------------
class RefMap(object):
    def __init__(self, reserved=1, defaultVal=None, scale=None, logScale=None, shift=None):
        self.fwd = dict()
        self.reserved = reserved
        self.scale = None if logScale is not None else scale
        self.logScale = logScale
        self.shift = None if shift is None else float(shift)
        self.missing = max(0, reserved - 1)
        if defaultVal is not None:
            self.missing = self.get(defaultVal, True)

    def key(self, x):
        y = x
        if self.shift is not None:
            y = float(y) + self.shift
        if self.scale is not None:
            return str(int(self.scale * float(y)))
        if self.logScale is not None:
            return str(int(math.log(float(y)) / math.log(self.logScale)))
        return y

    def get(self, x, update=False):
        k = self.key(x)
        if update and k not in self.fwd:
            self.fwd[k] = len(self.fwd) + self.reserved
        return self.fwd.get(k, self.missing)

    def size(self):
        return len(self.fwd) + max(0, self.reserved - 1)

    def pairs(self):
        return sorted(([k, v] for k, v in self.fwd.items()), key=lambda kv: kv[1])


class RefBinaryMap(RefMap):
    def __init__(self):
        RefMap.__init__(self)
        self.missing = 1

    def get(self, x, update=False):
        return 2 if x is not None else 1

    def size(self):
        return 2


TRACK_DEFAULTS = dict(dist="multinomial", valCol=3, scale=None, logScale=None, shift=None, delta=False, default=None,
                      caseSensitive=False)


def track_options(**kw):
    t = dict(TRACK_DEFAULTS)
    t.update(kw)
    if t["dist"] in ("binary", "mask"):
        t["valCol"] = 0
    return t


def make_map(t):
    """the map the reference's Track._init gives a track (track.py:67-99)"""
    if t["dist"] in ("binary", "mask"):
        return RefBinaryMap()
    assert t["dist"] == "multinomial" or (t["dist"] == "gaussian" and t["default"] is not None)
    return RefMap(reserved=1 if t["default"] is not None else 2, defaultVal=t["default"], scale=t["scale"],
                  logScale=t["logScale"], shift=t["shift"])


# ---- the rule ---------------------------------------------------------------------------------------------------------
def bed_records(text):
    out = []
    for line in text.split("\n"):
        if line[:1] == "#":
            continue
        fields = line.rstrip("\r").split("\t")
        if len(fields) > 2:
            out.append(fields)
    return out


def clip_sort(records, chrom, start, end):
    """[[chrom, oStart, oEnd, fields behind...]] of rule step 2"""
    kept = [[r[0], max(start, int(r[1])), min(end, int(r[2]))] + list(r[3:]) for r in records
            if r[0] == chrom and int(r[2]) > start and int(r[1]) < end and int(r[2]) > int(r[1])]
    return sorted(kept, key=lambda r: r[1])


def record_symbols(clipped, t, vmap, update):
    """[(sym0, sym)] of rule step 3 (trackIO.py:173-203 of the reference)"""
    out = []
    prev, prevVal = None, 0
    for r in clipped:
        val = 1 if t["valCol"] == 0 else r[t["valCol"]]
        val0 = val
        if t["delta"]:
            if prev is not None and r[1] == prev[2] and r[0] == prev[0]:
                try:
                    val0 = float(val) - float(prevVal)
                except (TypeError, ValueError):
                    val0 = int(val != prevVal)
            prevVal, prev = val, r
            val = 0
        sym = vmap.get(val, update)
        out.append((vmap.get(val0, update), sym))
    return out


def paint(T, fill, starts, ends, sym0, sym):
    """rule step 4 as the reference does it: record after record"""
    row = np.full(T, fill, dtype=np.int64)
    for s, e, a, b in zip(starts, ends, sym0, sym):
        row[s] = a
        row[s + 1:e] = b
    return row


def paint_by_search(T, fill, starts, ends, sym0, sym):
    """rule step 4 as a search: the last covering record wins"""
    row = np.full(T, fill, dtype=np.int64)
    for p in range(T):
        for i in range(len(starts) - 1, -1, -1):
            if starts[i] <= p < ends[i]:
                row[p] = sym0[i] if p == starts[i] else sym[i]
                break
    return row


def bed_row(text, chrom, start, end, t, vmap, update):
    clipped = clip_sort(bed_records(text), chrom, start, end)
    syms = record_symbols(clipped, t, vmap, update)
    return paint(end - start, vmap.missing, [r[1] - start for r in clipped], [r[2] - start for r in clipped],
                 [s[0] for s in syms], [s[1] for s in syms])


def fasta_row(records, chrom, start, end, t, vmap, update):
    row = np.full(end - start, vmap.missing, dtype=np.int64)
    for name, seq in records:
        if name == chrom:
            for i in range(start, min(end, len(seq))):
                c = seq[i] if t["caseSensitive"] else seq[i].upper()
                row[i - start] = vmap.get(c, update)
            break
    return row


def fasta_text(records, width=50):
    return "".join(">%s\n%s" % (n, "".join(s[i:i + width] + "\n" for i in range(0, len(s), width))) for n, s in records)


def fasta_records(text):
    out = []
    for line in text.split("\n"):
        if line[:1] == ">":
            out.append([line[1:], ""])
        elif out:
            out[-1][1] += line
    return out


def load_tables(tracks, files, intervals, maps=None, segments=None):
    """TrackData.loadTrackData of the reference (track.py:874-955) for multinomial, binary and mask tracks:
    (tables, maps).  tracks: [dict(name, file, **track_options)], mask tracks go to the mask table.  maps None: new
    maps learn in (interval, track) order; else {name: map} maps without learning and tracks without one are skipped.
    segments: sorted (chrom, start, end) tiling every table; a table keeps the mode of every segment at its first row."""
    update = maps is None
    if update:
        maps = dict((t["name"], make_map(t)) for t in tracks)
    plain = [t for t in tracks if t["dist"] != "mask"]
    masks = [t for t in tracks if t["dist"] == "mask"]
    columns = [t["name"] for t in plain if t["name"] in maps]
    tables = []
    for chrom, start, end in intervals:
        data = np.zeros((end - start, len(columns)), dtype=np.uint8)
        cover = np.zeros((end - start, len(masks)), dtype=np.uint8)
        for t in plain + masks:
            if t["name"] not in maps and t["dist"] != "mask":
                continue
            vmap = maps.get(t["name"]) or make_map(t)
            text = files[t["file"]]
            if t["file"].endswith(".bed"):
                row = bed_row(text, chrom, start, end, t, vmap, update)
            else:
                row = fasta_row(fasta_records(text), chrom, start, end, t, vmap, update)
            if t["dist"] == "mask":
                cover[:, masks.index(t)] = row
            else:
                data[:, columns.index(t["name"])] = row
        keep = cover.sum(axis=1) <= len(masks)
        data = data[keep]
        offsets = None
        if segments is not None:
            if len(data) == 0:
                continue
            cut = np.concatenate([[0], np.cumsum(~keep)])      # bases cut before every position
            offsets, rows = [], []
            for c, s, e in segments:
                if c == chrom and s >= start and e <= end and keep[s - start]:
                    a = s - start - cut[s - start]
                    offsets.append(a)
            for x, a in enumerate(offsets):
                b = offsets[x + 1] if x + 1 < len(offsets) else len(data)
                rows.append([np.bincount(data[a:b, k]).argmax() for k in range(data.shape[1])])
            data = np.asarray(rows, dtype=np.uint8).reshape(len(offsets), len(columns))
            offsets = np.asarray(offsets, dtype=np.int64)
        tables.append(dict(chrom=chrom, start=start, data=data, offsets=offsets))
    return tables, maps


# ---- seeded cases -------------------------------------------------------------------------------------------------------
NAMES = ["LTR", "LINE", "SINE", "DNA", "Simple", "Low", "Sat", "Other", "x|y"]


def random_bed(rng, chroms, length, n, names=NAMES, scores=False, tile=False):
    """n records, unsorted, overlapping and nested, none with the clipped start of another on its chromosome unless
    they are identical in value (the fixture does not cover the order among equal clipped starts)"""
    lines, used = ["# a comment line", "short\tline"], set()
    pos = dict((c, 0) for c in chroms)
    for _ in range(n):
        c = chroms[int(rng.randint(len(chroms)))]
        if tile:                                            # abutting records, for delta tracks
            s = pos[c] + (0 if rng.rand() < 0.7 else int(rng.randint(1, 9)))
            e = s + int(rng.randint(1, 12))
            pos[c] = e
        else:
            s = int(rng.randint(0, length))
            e = s + int(rng.randint(1, 1 + (length // 3 if rng.rand() < 0.1 else 15)))
        if (c, s) in used:
            continue
        used.add((c, s))
        name = names[int(rng.randint(len(names)))]
        score = "%.3f" % (rng.rand() * 40) if scores else "%d" % rng.randint(0, 30)
        lines.append("%s\t%d\t%d\t%s\t%s\t+" % (c, s, e, name, score))
    order = rng.permutation(len(lines) - 2) if not tile else np.arange(len(lines) - 2)
    return "\n".join(lines[:2] + [lines[2 + int(i)] for i in order]) + "\n"


def avoid_equal_clipped_starts(text, intervals):
    """drop records that would share a clipped start with an earlier one inside one of the intervals"""
    out, seen = [], set()
    for line in text.split("\n"):
        f = line.split("\t")
        if line[:1] != "#" and len(f) > 2:
            keys = set((c, max(s, int(f[1]))) for c, s, e in intervals if c == f[0] and int(f[2]) > s and int(f[1]) < e)
            if keys & seen:
                continue
            seen |= keys
        out.append(line)
    return "\n".join(out)


def golden_cases():
    rng = np.random.RandomState(20240611)
    cases = []

    def bed(name, interval, text, **opt):
        cases.append(dict(name=name, type="bed", track=track_options(**opt), chrom=interval[0], start=interval[1],
                          end=interval[2], bed=avoid_equal_clipped_starts(text, [interval])))

    bed("names_reserved2", ("chr1", 40, 400), random_bed(rng, ["chr1", "chr2"], 450, 90))
    bed("names_default", ("chr2", 0, 300), random_bed(rng, ["chr1", "chr2"], 350, 70, names=["0", "3", "7", "11"]),
        default="0")
    bed("score_scale", ("chr1", 10, 310), random_bed(rng, ["chr1"], 320, 80, scores=True), valCol=4, scale=0.25,
        default="0")
    bed("score_log_shift", ("chr1", 0, 256), random_bed(rng, ["chr1"], 256, 60, scores=True), valCol=4, logScale=2.0,
        shift=1.0)
    bed("presence_valcol0", ("chr1", 5, 200), random_bed(rng, ["chr1"], 220, 40), valCol=0)
    bed("delta_scaled", ("chr1", 3, 330), random_bed(rng, ["chr1", "chr2"], 0, 120, scores=True, tile=True), valCol=4,
        scale=0.5, delta=True, default="0")
    bed("binary", ("chr2", 20, 280), random_bed(rng, ["chr1", "chr2"], 300, 50), dist="binary")
    bed("mask", ("chr1", 0, 150), random_bed(rng, ["chr1"], 150, 12), dist="mask")
    bed("empty_interval", ("chr3", 0, 64), random_bed(rng, ["chr1"], 100, 10))

    alphabet = np.asarray(list("ACGTacgtNn"))
    seqs = [["chr1 description", "".join(alphabet[rng.randint(len(alphabet), size=90)])],
            ["chr1", "".join(alphabet[rng.randint(len(alphabet), size=333)])],
            ["chr2", "".join(alphabet[rng.randint(len(alphabet), size=120)])]]
    for name, interval, cs in (("fasta_folded", ("chr1", 7, 300), False), ("fasta_case", ("chr1", 0, 333), True),
                               ("fasta_short", ("chr2", 100, 260), False), ("fasta_absent", ("chr9", 0, 40), False)):
        cases.append(dict(name=name, type="fasta", track=track_options(caseSensitive=cs), records=seqs,
                          chrom=interval[0], start=interval[1], end=interval[2]))

    # a whole load: 5 tracks and a mask track over 3 intervals, then a second set of intervals through the learned list
    intervals = [["chr1", 30, 330], ["chr1", 400, 520], ["chr2", 0, 270]]
    intervals2 = [["chr1", 330, 400], ["chr1", 520, 700], ["chr2", 200, 380]]
    both = [tuple(iv) for iv in intervals + intervals2]
    files = {
        "te.bed": avoid_equal_clipped_starts(random_bed(rng, ["chr1", "chr2"], 700, 260), both),
        "cov.bed": avoid_equal_clipped_starts(random_bed(rng, ["chr1", "chr2"], 700, 200, scores=True), both),
        "tiles.bed": avoid_equal_clipped_starts(random_bed(rng, ["chr1", "chr2"], 0, 300, scores=True, tile=True), both),
        "hits.bed": avoid_equal_clipped_starts(random_bed(rng, ["chr1", "chr2"], 700, 60), both),
        "genome.fa": fasta_text([["chr1", "".join(alphabet[rng.randint(len(alphabet), size=650)])],
                                 ["chr2", "".join(alphabet[rng.randint(4, size=300)])]]),
        "holes.bed": avoid_equal_clipped_starts(random_bed(rng, ["chr1", "chr2"], 700, 30), both),
    }
    tracks = [dict(name="te", file="te.bed", **track_options()),
              dict(name="cov", file="cov.bed", **track_options(valCol=4, scale=0.2, default="0")),
              dict(name="dcov", file="tiles.bed", **track_options(valCol=4, scale=0.5, delta=True, default="0")),
              dict(name="hit", file="hits.bed", **track_options(dist="binary")),
              dict(name="seq", file="genome.fa", **track_options()),
              dict(name="holes", file="holes.bed", **track_options(dist="mask"))]
    cuts = dict()
    for c, s, e in both:
        cuts.setdefault(c, set()).update([s, e])
    for f in bed_records(files["holes.bed"]):
        cuts.setdefault(f[0], set()).update([int(f[1]), int(f[2])])
    for c in cuts:
        top = max(cuts[c])
        cuts[c].update(int(x) for x in rng.randint(0, top, size=top // 6))
    segments = [[c, a, b] for c in sorted(cuts) for a, b in zip(sorted(cuts[c])[:-1], sorted(cuts[c])[1:])]
    cases.append(dict(name="load", type="load", tracks=tracks, files=files, intervals=intervals,
                      intervals2=intervals2, segments=segments))
    return cases


def cases_json(cases):
    return json.dumps(cases, sort_keys=True)


def run_case(case):
    """what the fixture stores for a case, by the rule: {key: array or JSON-able}"""
    out = dict()

    def put_maps(prefix, names, maps):
        out[prefix + "maps"] = [maps[n].pairs() for n in names]
        out[prefix + "missing"] = [maps[n].missing for n in names]
        out[prefix + "symbols"] = [maps[n].size() for n in names]

    if case["type"] in ("bed", "fasta"):
        vmap = make_map(case["track"])
        args = (case["chrom"], case["start"], case["end"], case["track"], vmap, True)
        row = bed_row(case["bed"], *args) if case["type"] == "bed" else fasta_row(case["records"], *args)
        out["row"] = row
        again = make_map(case["track"])            # the same file through a map that may not learn: all missing
        args = args[:4] + (again, False)
        out["row_unlearned"] = bed_row(case["bed"], *args) if case["type"] == "bed" else fasta_row(case["records"], *args)
        put_maps("", ["t"], {"t": vmap})
        return out
    names = [t["name"] for t in case["tracks"] if t["dist"] != "mask"]
    stages = [("a_", case["intervals"], None, None), ("b_", case["intervals2"], "learned", None),
              ("c_", case["intervals2"], "learned", case["segments"])]
    learned = None
    for prefix, intervals, use, segments in stages:
        tables, maps = load_tables(case["tracks"], case["files"], [tuple(iv) for iv in intervals],
                                   maps=learned if use else None, segments=segments)
        if use is None:
            learned = maps
        out[prefix + "n"] = len(tables)
        for x, tab in enumerate(tables):
            out["%stable%d" % (prefix, x)] = tab["data"]
            out["%swhere%d" % (prefix, x)] = [tab["chrom"], tab["start"]]
            if tab["offsets"] is not None:
                out["%soffsets%d" % (prefix, x)] = tab["offsets"]
        put_maps(prefix, names, maps)
    return out
