"""Plain, slow Python statement of what tehmm_amd/scaling.py computes (bin/setTrackScaling.py of the reference; DESIGN.md
section 5p), used by the tests as the thing to be equal to, and the seeded cases they and
tests/golden/make_golden_scaling.py run on.

The rule for one numeric track over the merged intervals of the genome, laid end to end:
  1. per interval, the records are those of tests/trackio_ref.py rule steps 1 and 2 (clipped, sorted stably by clipped
     start); a record's value is np.float32(float(text of column valCol)), or 1 for valCol 0; text that is no number
     raises ValueError.  The delta attribute is never looked at (the tool passes a bound method where readBedData
     tests ``is True``);
  2. every base starts at np.float32(default), or at the largest float32 without a default; record after record
     writes its value over its bases, so the last record covering a base wins it;
  3. without a default every base that holds the largest float32 is dropped -- bases no record covers, and bases won
     by a record of exactly that value;
  4. when more than numBins bases are left, compute_scale picks the scale; its arithmetic is NumPy 2's (a Python float
     next to a float32 scalar is rounded to float32), spelt out below with a dtype on every step;
  5. scaleParam above 1e-4 is rounded to four decimals; the track gets scale (and loses logScale) or logScale (and
     loses scale), and always shift: 0.0 with a linear scale, else the float32 that was added (or 0.0).
Histogram bins are np.histogram's: edges e[0] .. e[n], bin b holds e[b] <= x < e[b + 1], the last bin also x == e[n];
compared in double; values outside count nowhere.
"""
import json

import numpy as np

import trackio_ref as tr

F32_MAX = np.finfo(np.float32).max


# ---- rule steps 1 - 3 ------------------------------------------------------------------------------------------------
def record_value(fields, valCol):
    return np.float32(1) if valCol == 0 else np.float32(float(fields[valCol]))


def interval_records(text, intervals, valCol):
    """(T, [(row start, row end, value)]) of the intervals laid end to end"""
    out, offset = [], 0
    for chrom, s, e in intervals:
        for r in tr.clip_sort(tr.bed_records(text), chrom, s, e):
            out.append((r[1] - s + offset, r[2] - s + offset, record_value(r, valCol)))
        offset += e - s
    return offset, out


def owners(T, records):
    """per base the index of the record that wins it, or -1"""
    own = [-1] * T
    for i, (s, e, _) in enumerate(records):
        for p in range(s, e):
            own[p] = i
    return own


def rows_won(T, start, end):
    """(rows won per record, uncovered rows) of one track, base by base"""
    own = owners(T, [(int(s), int(e), None) for s, e in zip(start, end)])
    won = [0] * len(start)
    for o in own:
        if o >= 0:
            won[o] += 1
    return np.asarray(won, dtype=np.int64), own.count(-1)


def float_paint(T, start, end, val, fill):
    out = np.full(T, np.float32(fill), dtype=np.float32)
    for s, e, v in zip(start, end, val):
        out[int(s):int(e)] = np.float32(v)
    return out


def float_array(text, intervals, valCol, default):
    fill = F32_MAX if default is None else np.float32(default)
    T, records = interval_records(text, intervals, valCol)
    data = np.full(T, fill, dtype=np.float32)
    for p, o in enumerate(owners(T, records)):
        if o >= 0:
            data[p] = records[o][2]
    if default is None:
        data = np.asarray([x for x in data if x != F32_MAX], dtype=np.float32)
    return data


def lane_join_adds(winners):
    """A model of how k_trk_rows_won joins the rows of one track in one tile (up to 256 winners), lane for lane: 32 lanes
    of 8 rows; a lane adds the runs of equal winners strictly inside its rows at once, an inclusive scan over the lanes
    (element: first winner, last winner, one run?, length of the last run) joins the first and last runs of neighbouring
    lanes, and only the lane in which a run ends adds it.  Returns the adds [(winner, rows)] in no particular order."""
    rows, adds, lanes = len(winners), [], []
    for run in range(32):
        w = list(winners[run * 8:run * 8 + 8]) if run * 8 < rows else []
        hw = tw = -2
        hl = tl = 0
        uni = True
        for u, x in enumerate(w):
            if u == 0 or x == tw:
                tw, tl = x, tl + 1
                continue
            if uni:
                hw, hl, uni = tw, tl, False
            else:
                adds.append((tw, tl))
            tw, tl = x, 1
        if w and uni:
            hw, hl = tw, tl
        lanes.append(dict(nq=len(w), hw=hw, tw=tw, hl=hl, tl=tl, uni=uni))
    scan = [dict(hw=x["hw"], tw=x["tw"], tl=x["tl"], uni=x["uni"]) for x in lanes]
    d = 1
    while d < 32:
        old = [dict(x) for x in scan]
        for i in range(d, 32):
            a, p = old[i - d], scan[i]
            if p["uni"]:
                if a["tw"] == p["hw"]:
                    p["tl"] += a["tl"]
                    p["uni"] = a["uni"]
                else:
                    p["uni"] = False
            p["hw"] = a["hw"]
        d *= 2
    for i, x in enumerate(lanes):
        if x["nq"] == 0:
            continue
        if not x["uni"]:
            adds.append((x["hw"], x["hl"] + (scan[i - 1]["tl"] if i > 0 and scan[i - 1]["tw"] == x["hw"] else 0)))
        if i == 31 or lanes[i + 1]["hw"] != x["tw"]:
            adds.append((x["tw"], scan[i]["tl"]))
    return adds


# ---- rule step 4 -----------------------------------------------------------------------------------------------------
def hist_counts(data, edges):
    e = [float(x) for x in edges]
    n = len(e) - 1
    freq = [0] * n
    for x in data:
        x = float(x)
        for b in range(n):
            if e[b] <= x < e[b + 1] or (b == n - 1 and x == e[n]):
                freq[b] += 1
                break
    return np.asarray(freq, dtype=np.int64)


def hist_variance(data, edges, fromLog=False):
    freq = hist_counts(data, edges)
    if float(edges[0]) <= 0 or not fromLog:
        assert int(freq.sum()) == len(data)
    else:
        assert int(hist_counts(data, [0.0] + list(edges)).sum()) == len(data)
    return np.var(freq.astype(np.float64)), freq


def compute_scale(data, numBins, noLog):
    """(scaleType, scaleParam, shift, linear counts, log counts); data is left as it is"""
    f32, f64 = np.float32, np.float64
    data = np.array(data, dtype=f32)
    minVal, maxVal = f32(min(data)), f32(max(data))
    spread = f32(maxVal - minVal)                                     # float32 - float32
    binSize = float(spread) / float(numBins - 2.0)                    # Python floats: double
    step = f32(binSize)                                               # a Python float beside a float32: rounded first
    edge = f32(f32(np.floor(f32(minVal / step))) * step)
    linearBins = [edge]
    for _ in range(1, numBins):
        edge = f32(edge + step)
        linearBins.append(edge)
    linearVar, linearCounts = hist_variance(data, sorted(linearBins))
    linearScale = 1.0 / binSize

    shift = 0.
    if minVal <= 0.:
        shift = f32(f32(1.0) - minVal)
        data = np.asarray([f32(x + shift) for x in data], dtype=f32)
        minVal = f32(minVal + shift)
        maxVal = f32(maxVal + shift)
    ratio = float(maxVal) / float(minVal)
    logBase = f64(np.power(f64(ratio), f64(1. / float(numBins - 2.00))))
    logMin = np.log(f32(minVal))                                      # float32 in, float32 out
    assert logMin.dtype == f32
    edge = f64(np.power(logBase, np.floor(f64(logMin) / np.log(logBase))))
    logBins = [edge]
    for _ in range(1, numBins):
        edge = f64(edge * logBase)
        logBins.append(edge)
    logVar, logCounts = hist_variance(data, sorted(logBins), fromLog=True)
    if logVar < linearVar and not noLog:
        return "logScale", logBase, shift, linearCounts, logCounts
    return "scale", linearScale, 0., linearCounts, logCounts


# ---- rule step 5 and the cases -----------------------------------------------------------------------------------------
def scaled_attributes(track, result):
    """the scaling attributes of the <track> element, as text: what the track had, then what the tool sets"""
    a = dict()
    for key in ("scale", "logScale", "shift", "default"):
        if track[key] is not None:
            a[key] = str(track[key])
    if a.get("logScale") is not None:
        a.pop("scale", None)
    if result is not None:
        scaleType, scaleParam, shift = result[:3]
        if scaleParam > 1e-4:
            scaleParam = float("%.4f" % scaleParam)
        a.pop("scale", None)
        a.pop("logScale", None)
        a[scaleType] = str(scaleParam)
        a["shift"] = str(shift)
    return a


def run_case(case):
    """what the fixture holds of a case"""
    t = case["track"]
    out = dict(error=None, data=np.zeros(0, dtype=np.float32), result=None,
               linear_counts=np.zeros(0, dtype=np.int64), log_counts=np.zeros(0, dtype=np.int64))
    try:
        out["data"] = float_array(case["bed"], case["intervals"], t["valCol"], t["default"])
    except ValueError:
        out["error"] = "ValueError"
    if out["error"] is None and len(out["data"]) > case["numBins"]:
        r = compute_scale(out["data"], case["numBins"], case["noLog"])
        out["result"] = [r[0], float(r[1]), float(r[2])]
        out["linear_counts"], out["log_counts"] = r[3], r[4]
        out["attrib"] = scaled_attributes(t, r)
    else:
        out["attrib"] = scaled_attributes(t, None)
    return out


def expand(values, weights):
    return np.repeat(np.asarray(values, dtype=np.float32), np.asarray(weights, dtype=np.int64))


INTERVALS = [["chr1", 0, 300], ["chr1", 400, 520], ["chr2", 10, 200]]


def bed_text(rng, values, fmt, maxLen=12, chroms=(("chr1", 540), ("chr2", 230)), extra=(), names=False):
    """one record per value, scattered over the chromosomes (records overlap and cross the interval ends); column 3 the
    value (names: a name), column 4 the value"""
    lines = []
    for i, v in enumerate(values):
        chrom, size = chroms[int(rng.randint(len(chroms)))]
        s = int(rng.randint(0, size))
        e = s + 1 + int(rng.randint(maxLen))
        text = fmt % v
        lines.append("%s\t%d\t%d\t%s\t%s" % (chrom, s, e, "n%d" % i if names else text, text))
    lines.extend(extra)
    return "\n".join(lines) + "\n"


def golden_cases():
    """The seeded cases.  expect: the scale type the reference must choose (the generator checks it), None when
    nothing is set."""
    rng = np.random.RandomState(20141)
    t = lambda **kw: tr.track_options(**kw)
    cases = []

    def add(name, bed, track, expect, numBins=10, noLog=False, intervals=INTERVALS):
        cases.append(dict(name=name, bed=bed, track=track, expect=expect, numBins=numBins, noLog=noLog,
                          intervals=[list(iv) for iv in intervals]))

    uniform = rng.uniform(10, 100, size=150)
    # one record of exactly the largest float32: its bases are dropped with the uncovered ones
    add("linear_wins", bed_text(rng, uniform, "%.3f", names=True,
                                extra=["chr1\t100\t140\tx\t3.4028234663852886e+38"]),
        t(valCol=4), "scale")
    spread = np.exp(rng.uniform(0, 9, size=150))
    logbed = bed_text(rng, spread, "%.4g")
    add("log_wins", logbed, t(valCol=3), "logScale")
    add("log_wins_nolog", logbed, t(valCol=3), "scale", noLog=True)
    add("shift_log", bed_text(rng, np.exp(rng.uniform(0, 9, size=150)) - 3.25, "%.4g", names=True), t(valCol=4), "logScale",
        numBins=12)
    add("default_shift_linear", bed_text(rng, rng.uniform(0, 50, size=200), "%.2f", maxLen=20),
        t(valCol=3, default="0"), "scale")
    add("default_negative_log", bed_text(rng, np.exp(rng.uniform(0, 8, size=300)) - 1.5, "%.5g", maxLen=6, names=True),
        t(valCol=4, default="-1.5", dist="gaussian"), "logScale", numBins=8)
    add("presence_default", bed_text(rng, np.ones(60), "%d", maxLen=8), t(valCol=0, default="0"), "scale", numBins=5)
    add("few_bases", "chr1\t5\t8\t2.5\t1\nchr2\t20\t22\t7\t3\n", t(valCol=3), None)
    add("non_numeric", bed_text(rng, rng.randint(0, 5, size=40), "LTR%d"), t(valCol=3), None)
    add("tiny_scale", bed_text(rng, rng.uniform(0, 5e6, size=150), "%.1f", names=True), t(valCol=4), "scale",
        intervals=[["chr2", 0, 230], ["chr1", 20, 500]])
    add("one_interval", bed_text(rng, rng.uniform(1, 9, size=80), "%.3f", chroms=(("chr1", 300),)),
        t(valCol=3, scale=0.5, delta=True), "scale", numBins=6, intervals=[["chr1", 0, 300]])
    return cases


def cases_json(cases):
    return json.dumps(cases, sort_keys=True)
