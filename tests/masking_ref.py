"""A plain front-to-back statement of tehmm_amd/masking.py and the entry points behind it: no searches, no scans.
Every function walks its lists the way the reference's tools (sortBed, mergeBed, filterBedLengths, subtractBed,
intersectBed and the loop of bin/interpolateMaskedRegions.py:117-162) do.  Also the seeded case generators of the
masking tests and the predicates that say which branches a case contains."""
import numpy as np

SKIPPED, DEFAULT = -2, -1


class Overlap(AssertionError):
    """the reference's assertion: a candidate flank overlaps the mask without abutting it"""

    def __init__(self, mask_index):
        AssertionError.__init__(self, "mask %d" % mask_index)
        self.mask = mask_index


def chrom_key(name):
    return str(name).encode()


def sort_intervals(intervals):
    """stable by (chrom name byte-wise, start)"""
    return sorted([tuple(iv) for iv in intervals], key=lambda iv: (chrom_key(iv[0]), iv[1]))


def chrom_ids(*lists):
    names = sorted({iv[0] for l in lists for iv in l}, key=chrom_key)
    return {n: k for k, n in enumerate(names)}


def columns(intervals, table):
    return (np.asarray([table[iv[0]] for iv in intervals], dtype=np.int32),
            np.asarray([iv[1] for iv in intervals], dtype=np.int64),
            np.asarray([iv[2] for iv in intervals], dtype=np.int64))


# ---- merge -------------------------------------------------------------------------------------------------------------
def merge(intervals, min_len=0, max_len=None):
    """mergeBed on a sorted list, then filterBedLengths: (chrom, start, end)"""
    runs = []
    for iv in intervals:
        c, s, e = iv[0], iv[1], iv[2]
        if runs and runs[-1][0] == c and s <= runs[-1][2]:
            runs[-1][2] = max(runs[-1][2], e)
        else:
            runs.append([c, s, e])
    return [tuple(r) for r in runs if r[2] - r[1] >= min_len and (max_len is None or r[2] - r[1] <= max_len)]


# ---- subtract and intersect ----------------------------------------------------------------------------------------
def by_chrom(b_list):
    """chrom -> its b, in list order (so that walking the b of an a does not walk the other chroms')"""
    out = {}
    for b in b_list:
        out.setdefault(b[0], []).append(b)
    return out


def subtract(a_list, b_list):
    """[(index of a, start, end)]: for every a the parts no b covers, left to right.  b: sorted and disjoint."""
    out = []
    groups = by_chrom(b_list)
    for i, a in enumerate(a_list):
        at = a[1]
        for b in groups.get(a[0], ()):
            if b[2] <= at or b[1] >= a[2]:
                continue
            if b[1] > at:
                out.append((i, at, b[1]))
            at = b[2]
        if at < a[2]:
            out.append((i, at, a[2]))
    return out


def intersect(a_list, b_list):
    """[(index of a, start, end)]: for every a its part inside every b that overlaps it, in b's order"""
    out = []
    groups = by_chrom(b_list)
    for i, a in enumerate(a_list):
        for b in groups.get(a[0], ()):
            if b[2] > a[1] and b[1] < a[2]:
                out.append((i, max(a[1], b[1]), min(a[2], b[2])))
    return out


def carry(a_list, pieces):
    return [(a_list[i][0], s, e) + tuple(a_list[i][3:]) for i, s, e in pieces]


# ---- the flank loop ------------------------------------------------------------------------------------------------
def intersect_size(x, y):
    if x[0] != y[0]:
        return 0
    if x[1] > y[1]:
        x, y = y, x
    return max(0, min(x[2], y[2]) - y[1])


def fill(masks, ivs, tgt=(), one=(), only_default=False, max_len=None):
    """One entry per mask: SKIPPED, DEFAULT or the state name.  masks: merged and sorted; ivs: (chrom, start, end,
    name) sorted as tuples.  The pointer only moves forward; once it has stopped on the last index with nothing at
    or above the mask, the right flank is gone for good (Python 2 orders None below every tuple) and the left flank
    is the interval before the last.  Raises Overlap for the first mask the reference asserts on."""
    tgt, one = set(tgt), set(one)
    key = lambda iv: (chrom_key(iv[0]), iv[1], iv[2])
    out = []
    idx = 0
    right = ivs[idx]
    for x, m in enumerate(masks):
        if max_len is not None and m[2] - m[1] > max_len:
            out.append(SKIPPED)
            continue
        while right is None or key(right) < key(m):
            if idx == len(ivs) - 1:
                right = None
                break
            idx += 1
            right = ivs[idx]
        left = ivs[idx - 1] if idx > 0 else None
        ls = rs = None
        if left is not None:
            if left[0] == m[0] and left[2] == m[1]:
                ls = str(left[3])
            elif intersect_size(left, m) != 0:
                raise Overlap(x)
        if right is not None:
            if right[0] == m[0] and right[1] == m[2]:
                rs = str(right[3])
            elif intersect_size(right, m) != 0:
                raise Overlap(x)
        state = DEFAULT
        if only_default:
            pass
        elif ls is not None and ls == rs:
            if len(tgt) == 0 or ls in tgt:
                state = ls
        elif ls in one:
            state = ls
        elif rs in one:
            state = rs
        out.append(state)
    return out


def fill_branches(masks, ivs, tgt=(), one=(), max_len=None):
    """the set of branches of the loop the case takes (no overlap cases)"""
    tgt, one = set(tgt), set(one)
    key = lambda iv: (chrom_key(iv[0]), iv[1], iv[2])
    seen, behind, p = set(), 0, 0
    for m in masks:
        if max_len is not None and m[2] - m[1] > max_len:
            seen.add("too_long")
            continue
        while p < len(ivs) and key(ivs[p]) < key(m):      # (masks ascend: the pointer never goes back)
            p += 1
        if p == 0:
            seen.add("before_first")
        if p == len(ivs):
            behind += 1
            continue
        left = ivs[p - 1] if p > 0 else None
        right = ivs[p]
        ls = left[3] if left is not None and left[0] == m[0] and left[2] == m[1] else None
        rs = right[3] if right[0] == m[0] and right[1] == m[2] else None
        if ls is not None and ls == rs:
            seen.add("equal_flagged" if len(tgt) == 0 or ls in tgt else "equal_unflagged")
        elif ls in one:
            seen.add("one_left")
        elif rs in one:
            seen.add("one_right")
        elif ls is None and rs is None:
            seen.add("no_flank")
    if behind >= 2:
        seen.add("two_behind_last")
    return seen


FILL_BRANCHES = {"too_long", "before_first", "equal_flagged", "equal_unflagged", "one_left", "one_right", "no_flank",
                 "two_behind_last"}


# ---- the Python layer ------------------------------------------------------------------------------------------------
def cut_out(intervals, mask_records, min_length, max_length):
    """cutOutMaskIntervals with mask tracks present"""
    masks = merge(sort_intervals([r for r in mask_records if r[2] > r[1]]), min_length + 1,
                  None if max_length is None else max_length - 1)
    intervals = [tuple(iv) for iv in intervals if iv[2] > iv[1]]
    out = sort_intervals(carry(intervals, subtract(intervals, masks)))
    if not out:
        raise RuntimeError("cutOutMaskIntervals removed everything")
    return out


def interpolate(mask_records, all_intervals, in_intervals, max_len=None, default="0", tgt=(), one=(),
                only_default=False, cut=False):
    in_intervals = [tuple(iv) for iv in in_intervals]
    pred = in_intervals
    if cut:
        pred = cut_out(in_intervals, mask_records, -1, None if max_len is None else max_len + 1)
    flank = sorted([iv[:4] for iv in pred], key=lambda iv: (chrom_key(iv[0]), iv[1], iv[2]))
    masks = merge(sort_intervals([r for r in mask_records if r[2] > r[1]]))
    if not flank:
        return in_intervals
    states = fill(masks, flank, tgt, one, only_default, max_len) if masks else []
    fills = [m + (str(default) if s == DEFAULT else s,) for m, s in zip(masks, states) if s != SKIPPED]
    rows = sort_intervals([iv for iv in in_intervals if iv[2] > iv[1]] + fills)
    scope = merge(sort_intervals([iv for iv in all_intervals if iv[2] > iv[1]]))
    return carry(rows, intersect(rows, scope))


# ---- hand-sized cases that hold every branch ---------------------------------------------------------------------------
CHROMS = ["chr1", "chr10", "chr2"]      # name order differs from numeric order


def merge_case():
    """(records, min_len, max_len): nested, overlapping, abutting and separate masks, one filtered at each limit"""
    recs = [("chr2", 0, 100), ("chr2", 10, 20),           # nested -> 100 long
            ("chr1", 5, 30), ("chr1", 20, 50),            # overlapping -> 45 long
            ("chr1", 60, 70), ("chr1", 70, 95),           # abutting -> 35 long
            ("chr10", 0, 3),                              # separate, below min
            ("chr10", 10, 500),                           # separate, above max
            ("chr10", 600, 640),                          # separate, kept
            ("chr1", 200, 210), ("chr1", 200, 205)]       # equal start
    return recs, 10, 100


def merge_branches(recs):
    s = sort_intervals(recs)
    seen = set()
    end = None
    for p, q in zip(s, s[1:]):
        if p[0] != q[0]:
            end = None
            continue
        end = p[2] if end is None else max(end, p[2])
        if q[2] <= end and q[1] < end:
            seen.add("nested")
        elif q[1] < end:
            seen.add("overlapping")
        elif q[1] == end:
            seen.add("abutting")
        else:
            seen.add("separate")
            end = None
    return seen


def pieces_case():
    """(A, B) for subtract and intersect"""
    B = [("chr1", 100, 200), ("chr1", 300, 400), ("chr1", 400, 450), ("chr1", 600, 700),      # 300-450 abut
         ("chr2", 50, 60), ("chr3", 0, 10)]                                                     # chr3 is not in A
    A = [("chr1", 0, 50, "no_b"),
         ("chr1", 120, 180, "covered"),
         ("chr1", 100, 250, "cut_at_start"),
         ("chr1", 50, 200, "cut_at_end"),
         ("chr1", 0, 1000, "spans_all"),
         ("chr1", 150, 650, "overlaps_previous"),
         ("chr10", 0, 500, "chrom_not_in_b"),
         ("chr2", 55, 58, "covered2"),
         ("chr2", 40, 70, "inner")]
    return A, B


def pieces_branches(A, B):
    seen = set()
    for a in A:
        hits = [b for b in B if b[0] == a[0] and b[2] > a[1] and b[1] < a[2]]
        if not any(b[0] == a[0] for b in B):
            seen.add("a_chrom_absent")
        elif not hits:
            seen.add("no_b")
        if hits and not [p for p in subtract([a], B)]:
            seen.add("covered")
        if hits and hits[0][1] == a[1]:
            seen.add("cut_at_start")
        if hits and hits[-1][2] == a[2]:
            seen.add("cut_at_end")
    if any(not any(a[0] == b[0] for a in A) for b in B):
        seen.add("b_chrom_absent")
    names = sorted({iv[0] for iv in A + B}, key=chrom_key)
    if names != sorted(names, key=lambda n: int(n[3:])):
        seen.add("name_order")
    if any(p[0] == q[0] and p[2] > q[1] and q[2] > p[1] for i, p in enumerate(A) for q in A[i + 1:]):
        seen.add("overlapping_a")
    return seen


PIECES_BRANCHES = {"a_chrom_absent", "no_b", "covered", "cut_at_start", "cut_at_end", "b_chrom_absent", "name_order",
                   "overlapping_a"}


def fill_case():
    """(masks, ivs, tgt, one, max_len) with every branch of FILL_BRANCHES"""
    ivs = [("chr1", 100, 200, "A"), ("chr1", 210, 300, "A"),      # mask 200-210: equal, flagged
           ("chr1", 320, 400, "B"),                              # mask 300-320: A | B, nothing one-sided -> default
           ("chr1", 410, 500, "B"),                              # mask 400-410: equal, B not in tgt
           ("chr1", 505, 600, "L"),                              # mask 500-505: B | L -> one-sided by the right
           ("chr1", 620, 700, "C"),                              # mask 600-620: L | C -> one-sided by the left
           ("chr1", 5000, 5100, "A"),                            # mask 700-5000: too long; mask 800-.. merged in
           ("chr10", 50, 60, "A"), ("chr10", 60, 70, "A"),
           ("chr2", 10, 20, "A"), ("chr2", 30, 40, "A")]          # mask chr2 20-30 sits before the LAST interval
    masks = [("chr1", 10, 20),                                    # before the first interval
             ("chr1", 200, 210), ("chr1", 300, 320), ("chr1", 400, 410), ("chr1", 500, 505), ("chr1", 600, 620),
             ("chr1", 700, 5000),
             ("chr1", 5200, 5210),                                # no flank
             ("chr2", 20, 30),                                    # equal flagged, right flank is the last interval
             ("chr2", 40, 45), ("chr2", 100, 110), ("chr3", 0, 5)]     # behind the last interval: default, all three
    return masks, ivs, ("A",), ("L",), 1000


def overlap_case():
    """(masks, ivs): masks 1 and 2 overlap their left candidate without abutting it"""
    ivs = [("chr1", 0, 100, "A"), ("chr1", 150, 300, "B"), ("chr1", 500, 600, "A")]
    masks = [("chr1", 100, 150), ("chr1", 200, 260), ("chr1", 280, 320), ("chr1", 400, 410)]
    return masks, ivs


def golden_cases():
    """[(name, [records of every mask track], allBed, inBed, options)]: what tests/golden/make_golden_masking.py runs
    the reference's main() on.  Python 3 cannot order None against a tuple, so no case has a second mask behind the
    last predicted interval."""
    masks, ivs, tgt, one, max_len = fill_case()
    masks = [m for m in masks if m not in (("chr2", 100, 110), ("chr3", 0, 5))]
    scope = [("chr1", 0, 6000), ("chr10", 0, 100), ("chr2", 0, 200)]
    cases = [("hand", [masks[0::2], masks[1::2]], scope, ivs,
              dict(maxLen=max_len, default="0", tgts=",".join(tgt), oneSidedTgts=",".join(one)))]
    rs = np.random.RandomState(11)
    raw = random_masks(rs, 90, merged=False)
    pred = random_prediction(rs, merge(sort_intervals(raw)))
    scope = [(c, 0, 10 ** 6) for c in CHROMS]
    cases.append(("random", [raw[:50], raw[50:]], scope, pred, dict(maxLen=25, default="X", oneSidedTgts="L")))
    cases.append(("random_tgts", [raw[:50], raw[50:]], scope, pred, dict(maxLen=60, default="X", tgts="A,B",
                                                                         oneSidedTgts="C,L")))
    cases.append(("only_default", [raw], scope, pred, dict(maxLen=25, default="d", onlyDefault=True)))
    cases.append(("no_max_len", [raw], scope, pred, dict()))
    whole = []
    for c in CHROMS:                                         # a prediction that covers the masks: --cut
        cuts = sorted(set([0, 4000] + [int(x) for x in rs.randint(1, 4000, size=40)]))
        whole += [(c, a, b, "ABCL"[rs.randint(4)]) for a, b in zip(cuts, cuts[1:])]
    cases.append(("cut", [raw], scope, whole, dict(maxLen=20, default="0", oneSidedTgts="L", cut=True)))
    return cases


# ---- seeded generators ---------------------------------------------------------------------------------------------
def first_seed(make, ok, start, tries=200):
    """make(RandomState(seed)) for the first seed from start on whose case holds what ok asks for: a case is never
    used on the strength of its seed alone"""
    for seed in range(start, start + tries):
        case = make(np.random.RandomState(seed))
        if ok(case):
            return case
    raise AssertionError("no seed in [%d, %d) gives a case with every branch" % (start, start + tries))


def merged_masks(rs, n, last="chr2"):
    """exactly n merged masks: merging shrinks a random list, so it is topped up behind the end of the last chrom"""
    masks = random_masks(rs, n)
    e = max([m[2] for m in masks if m[0] == last] + [0])
    for _ in range(n - len(masks)):
        s = e + 1 + int(rs.randint(1, 40))
        e = s + int(rs.randint(1, 60))
        masks.append((last, s, e))
    return sort_intervals(masks)


def random_masks(rs, n, chroms=CHROMS, span=40, merged=True):
    """n raw mask records; with merged, the merged list (sorted, disjoint, never abutting)"""
    recs = []
    for c in chroms:
        at = int(rs.randint(0, 50))
        for _ in range(n // len(chroms) + 1):
            at += int(rs.randint(0, span))
            recs.append((c, at, at + int(rs.randint(1, span))))
    recs = [recs[i] for i in rs.permutation(len(recs))[:n]]
    return merge(sort_intervals(recs)) if merged else recs


def random_disjoint(rs, n, chroms=CHROMS + ["chr7"], span=30):
    """n sorted disjoint intervals, about a third of them abutting their predecessor"""
    out = []
    per = [n // len(chroms) + (1 if k < n % len(chroms) else 0) for k in range(len(chroms))]
    for c, m in zip(sorted(chroms, key=chrom_key), per):
        at = int(rs.randint(0, 20))
        for _ in range(m):
            at += 0 if rs.randint(3) == 0 else int(rs.randint(1, span))
            e = at + int(rs.randint(1, span))
            out.append((c, at, e))
            at = e
    return out


def random_any(rs, n, B, chroms=CHROMS + ["chr30"], span=200):
    """n intervals in any order, overlapping, with a name column; about a quarter start exactly where a b of their
    chrom starts, a quarter end where one ends, and a few lie inside one b"""
    by = {}
    for b in B:
        by.setdefault(b[0], []).append(b)
    limit = max(b[2] for b in B) + span
    out = []
    for k in range(n):
        c = chroms[rs.randint(len(chroms))]
        s = int(rs.randint(0, limit))
        e = s + int(rs.randint(1, span))
        how = rs.randint(8)
        if c in by and how < 5:
            b = by[c][rs.randint(len(by[c]))]
            if how < 2:
                s, e = b[1], b[1] + int(rs.randint(1, span))
            elif how < 4:
                s, e = max(0, b[2] - int(rs.randint(1, span))), b[2]
            else:
                s, e = b[1] + (b[2] - b[1]) // 3, b[2] - (b[2] - b[1]) // 3
            if e <= s:
                e = s + 1
        out.append((c, s, e, "r%d" % k))
    return out


def random_prediction(rs, masks, states=("A", "B", "C", "L"), gap=3, open_ends=False):
    """A prediction shaped like a decode on the masked genome: between consecutive masks of a chrom one to three
    intervals that tile the space (so most masks are abutted on both sides), some spaces left open at one end.  With
    open_ends nothing lies before the first mask of the first chrom or behind the third last mask of the last."""
    out = []
    by = {}
    for m in masks:
        by.setdefault(m[0], []).append(m)
    order = sorted(by, key=chrom_key)
    for c in order:
        at = max(0, by[c][0][1] - 7)
        spaces = by[c] + [(c, by[c][-1][2] + 50, 0)]
        if open_ends and c == order[0]:
            at, spaces = spaces[0][2], spaces[1:]
        if open_ends and c == order[-1]:
            spaces = spaces[:-3]
        for m in spaces:
            lo, hi = at, m[1]
            if hi - lo >= 2 and rs.randint(6) == 0:
                lo += 1                                      # does not abut the previous mask
            if hi - lo >= 2 and rs.randint(6) == 0:
                hi -= 1                                      # does not abut the next mask
            cuts = sorted(set([lo, hi] + [int(x) for x in rs.randint(lo, hi + 1, size=int(rs.randint(0, gap)))]))
            for a, b in zip(cuts, cuts[1:]):
                out.append((c, a, b, states[rs.randint(len(states))]))
            at = m[2]
    return out
