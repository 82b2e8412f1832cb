"""Plain, slow Python statement of what tehmm_amd/tsd.py computes on the device, used by the
tests as the thing to be equal to, and the seeded cases they and tests/golden/make_golden_tsd.py run on.

The finder is stated by its rules, not by the reference's list merge: every k-mer hit (i, j) of the query window in
the table window knows h, the number of consecutive hits before it on its diagonal; a piece opens where h is a multiple
of `per` and is k + min(per - 1, hits behind it) long.  The clean-up is stated twice: as the reference's chain and as
the running maximum the kernels use.
"""
import numpy as np

DEFAULTS = dict(min=4, max=6, all=False, maxScore=None, left=7, right=7, overlap=3, leftName="L_TSD",
                rightName="R_TSD", id=False, names=None, sequenceNames=None)
VALID = set("acgtn")


class InvalidBase(Exception):
    """a base other than ACGTNacgtn inside a searched window (the reference asserts); .element is its index"""

    def __init__(self, element):
        Exception.__init__(self, "element %d" % element)
        self.element = element


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def windows(s, e, length, k, left, right, overlap):
    """(l1, r1, l2, r2) or None when the element yields nothing"""
    ov = max(0, min(overlap, (e - s) // 2 - 2))
    l1, r1 = max(0, s - left), s - 1 + ov
    l2, r2 = e - ov, min(e - 1 + right, length - 1)
    if r1 - l1 < k or r2 - l2 < k:
        return None
    return l1, r1, l2, r2


def pieces(q, c, k, mx):
    """[[i, i + L, j, j + L]] in the reference's list order (i, then j)"""
    per = max(k, mx - k) - k + 1
    nq, nc = len(q) - k + 1, len(c) - k + 1
    hits = [[q[i:i + k] == c[j:j + k] for j in range(nc)] for i in range(nq)]
    hit = lambda i, j: 0 <= i < nq and 0 <= j < nc and hits[i][j]
    before = {}                                      # (i, j) of a hit -> consecutive hits before it on its diagonal
    out = []
    for i in range(nq):
        for j in range(nc):
            if not hits[i][j]:
                continue
            h = before[(i, j)] = before.get((i - 1, j - 1), -1) + 1
            if h % per:
                continue
            after = 0
            while after < per - 1 and hit(i + after + 1, j + after + 1):
                after += 1
            L = k + after
            out.append([i, i + L, j, j + L])
    return out


def element_matches(seq, s, e, o):
    """rows (left start, left end, d1, right start, right end, d2) of one element; seq is lower-case text"""
    win = windows(s, e, len(seq), o["min"], o["left"], o["right"], o["overlap"])
    if win is None:
        return []
    l1, r1, l2, r2 = win
    q, c = seq[l1:r1], seq[l2:r2]
    if not set(q) | set(c) <= VALID:
        raise InvalidBase(-1)
    rows = []
    for i, i2, j, j2 in pieces(q, c, o["min"], o["max"]):
        d1, d2 = abs(s - (l1 + i2)), abs(e - (l2 + j))
        if o["maxScore"] is None or max(d1, d2) <= o["maxScore"]:
            rows.append((l1 + i, l1 + i2, d1, l2 + j, l2 + j2, d2))
    if not o["all"] and len(rows) > 1:
        best = rows[0]
        for r in rows[1:]:
            if (max(r[2], r[5]), -(r[1] - r[0])) < (max(best[2], best[5]), -(best[1] - best[0])):
                best = r
        rows = [best]
    return rows


def plan(sequences, intervals, o):
    """[(record index, record name, chromosome, interval index)] in output order: records in their order, each
    serving the chromosome named like it or like its first token; raises ValueError on a reappearing chromosome"""
    split = lambda x: None if x is None else set(x.split(",") if isinstance(x, str) else x)
    names, seqs = split(o["names"]), split(o["sequenceNames"])
    table, prev = dict(), None
    for i, iv in enumerate(intervals):
        if iv[0] != prev:
            if iv[0] in table:
                raise ValueError(iv[0])
            table[iv[0]] = []
            prev = iv[0]
        table[iv[0]].append(i)
    out = []
    for r, (rec, _) in enumerate(sequences):
        token = rec.split()[0]
        if seqs is not None and rec not in seqs and token not in seqs:
            continue
        chrom = rec if rec in table else token
        for i in table.get(chrom, []):
            iv = intervals[i]
            if names is None or (iv[3] if len(iv) > 3 else None) in names:
                out.append((r, rec, chrom, i))
    return out


def find_tsds(sequences, intervals, **kw):
    """the list of 5-tuples tsdFinder.py's findTsds returns; sequences is a list of (name, bases as bytes)"""
    o = options(**kw)
    lower = {}
    out, n = [], 0
    for x, (r, rec, chrom, i) in enumerate(plan(sequences, intervals, o)):
        if r not in lower:
            lower[r] = bytes(sequences[r][1]).decode("latin-1").lower()
        iv = intervals[i]
        try:
            rows = element_matches(lower[r], iv[1], iv[2], o)
        except InvalidBase:
            raise InvalidBase(x)
        for ls, le, d1, rs, re, d2 in rows:
            tag = "_%d" % n if o["id"] else ""
            out.append((iv[0], ls, le, o["leftName"] + tag, d1))
            out.append((iv[0], rs, re, o["rightName"] + tag, d2))
            n += 1
    return out


def lowest_invalid(sequences, intervals, **kw):
    """index (in output order) of the lowest element with an invalid base in a searched window, or None"""
    o = options(**kw)
    for x, (r, rec, chrom, i) in enumerate(plan(sequences, intervals, o)):
        try:
            element_matches(bytes(sequences[r][1]).decode("latin-1").lower(), intervals[i][1], intervals[i][2], o)
        except InvalidBase:
            return x
    return None


# ---- the clean-up ----------------------------------------------------------------------------------------------------
def sort_intervals(intervals):
    return sorted(intervals, key=lambda iv: (str(iv[0]), int(iv[1])))


def remove_overlaps_chain(intervals):
    """removeBedOverlaps.py:76-95 as written, on a sorted list"""
    out, prev = [], None
    for iv in intervals:
        start = iv[1]
        if prev is not None and iv[0] == prev[0] and start < prev[2]:
            start = prev[2]
        if iv[2] > start:
            iv = (iv[0], start) + tuple(iv[2:])
            out.append(iv)
            prev = iv
    return out


def remove_overlaps_running_max(intervals):
    """the same through the maximum of ALL earlier ends of the chromosome"""
    out, chrom, top = [], None, None
    for iv in intervals:
        if iv[0] != chrom:
            chrom, top = iv[0], None
        start = iv[1] if top is None else max(iv[1], top)
        if iv[2] > start:
            out.append((iv[0], start) + tuple(iv[2:]))
        top = iv[2] if top is None else max(top, iv[2])
    return out


# ---- seeded cases ----------------------------------------------------------------------------------------------------
def random_bases(rs, n, letters="acgt", upper=0.3, n_runs=0):
    seq = np.frombuffer(letters.encode(), dtype=np.uint8)[rs.randint(len(letters), size=n)].copy()
    for _ in range(n_runs):
        a = rs.randint(max(n - 1, 1))
        seq[a:a + rs.randint(1, 12)] = ord("n")
    up = rs.rand(n) < upper
    seq[up] -= 32
    return seq.tobytes()


def random_elements(rs, chrom, length, n, max_len=40, short=0.5, name=None):
    """n elements on a sequence of `length` bases, sorted by start; half of them 0 - 9 bases long; the first at base 0
    and the last three at and past the sequence end"""
    starts = np.sort(rs.randint(0, max(length, 1), size=n))
    out = []
    for x, s in enumerate(starts.tolist()):
        size = rs.randint(0, 10) if rs.rand() < short else rs.randint(10, max_len + 1)
        iv = (chrom, s, s + size)
        if name is not None:
            iv += (name if isinstance(name, str) else name[rs.randint(len(name))],)
        out.append(iv)
    if n >= 6:
        out[0] = (chrom, 0, rs.randint(0, 12)) + out[0][3:]
        out[1] = (chrom, min(2, length), min(2, length) + 8) + out[1][3:]
        out[-3] = (chrom, max(length - 12, 0), max(length - 2, 0)) + out[-3][3:]
        out[-2] = (chrom, max(length - 9, 0), length) + out[-2][3:]
        out[-1] = (chrom, max(length - 5, 0), length + 7) + out[-1][3:]
        out.sort(key=lambda iv: iv[1])
    return out


def golden_cases():
    """[(name, sequences [(record name, bytes)], intervals, option overrides)]: small enough for the reference's own
    functions, wide enough to reach every rule (see test_tsd_cpu.test_fixture_covers_what_it_should)"""
    rs = np.random.RandomState(20142)
    cases = []
    seq2 = random_bases(rs, 1500, "ac", n_runs=20)
    seq4 = random_bases(rs, 2500, "acgt", n_runs=10)
    seq5 = random_bases(rs, 1200, "acgtn")
    cases.append(("defaults_two_letters", [("chrA", seq2)], random_elements(rs, "chrA", 1500, 160), {}))
    cases.append(("defaults_four_letters", [("chrB", seq4)], random_elements(rs, "chrB", 2500, 200), {}))
    cases.append(("defaults_all", [("chrA", seq2)], random_elements(rs, "chrA", 1500, 120), dict(all=True)))
    cases.append(("five_letters_all_id", [("chrN", seq5)], random_elements(rs, "chrN", 1200, 120),
                  dict(all=True, id=True, min=3, max=5)))
    # no extension (max < 2k) and extension with saturation (max >= 2k + 1), runs several times longer than per
    one = random_bases(rs, 400, "a", upper=0.5)
    cases.append(("no_extension", [("c", seq2)], random_elements(rs, "c", 1500, 100), dict(min=4, max=7, all=True)))
    cases.append(("extension", [("c", seq2)], random_elements(rs, "c", 1500, 100),
                  dict(min=3, max=9, all=True, left=12, right=12)))
    cases.append(("extension_one_letter", [("c", one)], random_elements(rs, "c", 400, 24, max_len=30),
                  dict(min=2, max=7, all=True, left=14, right=13, overlap=4)))
    cases.append(("extension_one_letter_best", [("c", one)], random_elements(rs, "c", 400, 40, max_len=30),
                  dict(min=2, max=7, left=14, right=13, overlap=4)))
    # k = 1, and the densest element there is: 64-long windows of one letter, 4096 matches
    cases.append(("k1", [("c", seq4)], random_elements(rs, "c", 2500, 80), dict(min=1, max=1, all=True)))
    cases.append(("k1_max3_best", [("c", seq4)], random_elements(rs, "c", 2500, 80), dict(min=1, max=3)))
    cases.append(("k1_dense_64", [("c", one)], [("c", 150, 190), ("c", 200, 232)],
                  dict(min=1, max=1, all=True, left=62, right=62, overlap=3)))
    # k = 21 on windows of 64 and below
    two = random_bases(rs, 900, "at", upper=0.2)
    runs = np.frombuffer(two, dtype=np.uint8).copy()
    for a in range(50, 850, 160):
        runs[a:a + 90] = runs[a + 100:a + 190]        # long exact repeats 100 bases apart
    runs = runs.tobytes()
    cases.append(("k21", [("c", runs)], [("c", a + 90 + d, a + 100 + d) for a in range(50, 850, 160)
                                         for d in (-3, 0, 2)] + [("c", 880, 890)],
                  dict(min=21, max=50, all=True, left=60, right=60, overlap=5)))
    cases.append(("k21_best", [("c", runs)], [("c", a + 90 + d, a + 100 + d) for a in range(50, 850, 160)
                                              for d in (-3, 0, 2)], dict(min=21, max=21, left=65, right=65, overlap=0)))
    # maxScore
    cases.append(("max_score_0", [("chrA", seq2)], random_elements(rs, "chrA", 1500, 300, short=0.2),
                  dict(maxScore=0, min=3, max=6)))
    cases.append(("max_score_3_all", [("chrA", seq2)], random_elements(rs, "chrA", 1500, 100),
                  dict(maxScore=3, all=True)))
    # several records, elements grouped by chromosome but not in record order; names with a second token; a record
    # without elements; a chromosome without a record; name filters
    recs = [("chr2 second", random_bases(rs, 700, "ac")), ("chrU", random_bases(rs, 90, "ac")),
            ("chr1", random_bases(rs, 800, "acg")), ("chr3 x y", random_bases(rs, 300, "ct")), ("chr 4", seq5[:200])]
    ivs = (random_elements(rs, "chr1", 800, 60, name=["LTR", "LINE", "SINE"]) +
           random_elements(rs, "chr3 x y", 300, 30, name=["LTR", "LINE"]) +
           random_elements(rs, "chrMissing", 300, 8, name="LTR") +
           random_elements(rs, "chr2", 700, 50, name=["LTR", "SINE"]) +
           random_elements(rs, "chr", 200, 20, name="LINE"))
    cases.append(("records", recs, ivs, dict(id=True)))
    cases.append(("records_names", recs, ivs, dict(names="LTR,SINE", id=True, leftName="left", rightName="right")))
    cases.append(("records_sequences", recs, ivs, dict(sequenceNames="chr1,chr3 x y,chr", all=True)))
    # element counts around a wave
    for n in (1, 63, 64, 65):
        cases.append(("n_%d" % n, [("w", seq2)], random_elements(rs, "w", 1500, n), dict(min=3, max=6)))
    # an invalid base: outside every searched window nothing happens, inside one the reference asserts
    bad = bytearray(random_bases(rs, 600, "ac"))
    bad[300] = ord("x")
    bad[301] = ord("-")
    far = [("b", s, s + 10) for s in (20, 100, 200, 284, 320, 400, 500)]      # searched: up to base 299, from 313 on
    cases.append(("invalid_unsearched", [("b", bytes(bad))], far, {}))
    cases.append(("invalid_searched", [("b", bytes(bad))], far[:4] + [("b", 290, 297), ("b", 302, 330)] + far[4:], {}))
    return cases


def big_cases():
    """cases for the device only (the restatement still runs them in seconds): more than one workgroup, and dense
    elements on both sides of a scan block boundary"""
    rs = np.random.RandomState(7)
    cases = []
    seq = bytearray(random_bases(rs, 60000, "acgt", n_runs=200))
    seq[30000:30400] = b"aAaa" * 100
    seq = bytes(seq)
    ivs = random_elements(rs, "g", 60000, 2049)
    cases.append(("block_plus_one", [("g", seq)], ivs, {}))
    # elements at the start of the sequence have a query window of a few bases: cheap fill around the dense ones
    dense = [("g", 1 + x % 4, 1 + x % 4 + x % 3) for x in range(2100)]
    for x in range(2040, 2056):                       # 16 elements inside the one-letter stretch, across item 2048
        dense[x] = ("g", 30150 + (x - 2040), 30150 + (x - 2040) + 40)
    cases.append(("dense_across_blocks", [("g", seq)], dense, dict(min=1, max=1, all=True, left=62, right=62, overlap=3)))
    two = random_bases(rs, 90000, "ag", n_runs=50)
    cases.append(("two_letters_all", [("t", two)], random_elements(rs, "t", 90000, 3000),
                  dict(min=3, max=8, all=True, left=20, right=20, overlap=6)))
    return cases


def overlap_lists():
    """[(name, intervals)] for the clean-up: contained intervals, chains, zero-length results, many chromosomes"""
    rs = np.random.RandomState(99)
    out = [("contained", [("c", 0, 100, "a", 1), ("c", 10, 20, "b", 2), ("c", 30, 100, "c", 3), ("c", 50, 120, "d", 4),
                          ("c", 120, 120, "e", 5), ("c", 119, 121, "f", 6), ("d", 5, 9, "g", 7), ("d", 5, 9, "h", 8)])]
    for n in (1, 63, 64, 65, 2048, 2049, 6000):
        ivs = []
        chroms = max(1, n // 700)
        for q in range(n):
            c = "chr%d" % rs.randint(chroms)
            s = rs.randint(0, 40 * n // chroms + 10)
            ivs.append((c, s, s + rs.randint(0, 60) * (rs.rand() < 0.9) + rs.randint(0, 600) * (rs.rand() < 0.05),
                        "iv%d" % q, q))
        out.append(("n_%d" % n, ivs))
    # a chromosome change exactly at items 2048 and 4096 of the sorted list
    ivs = [("a", 3 * q, 3 * q + 5, "x", q) for q in range(2048)] + [("b", 2 * q, 2 * q + 4, "y", q) for q in range(2048)]
    ivs += [("c", 7, 9, "z", 0), ("c", 8, 9, "z", 1)]
    out.append(("change_at_block", ivs))
    return out
