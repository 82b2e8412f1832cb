"""Plain, slow Python statement of what tehmm_amd/compare.py computes on the device, used by
the tests as the thing to be equal to.  Intervals are tuples (chrom, start, end, name[, ...]).  Nothing here searches:
every function goes through the lists from front to back, which is exactly what the kernels do not do.
"""
import numpy as np


def _ids(lists, pick):
    table = {}
    for l in lists:
        for iv in l:
            table.setdefault(pick(iv), len(table))
    return table


def check_lists(iv1, iv2):
    """(which, where): (0, -1) when both lists are valid and cover the same bases, else the offending list (1, 2) and
    the index of its first offending interval.  Order: validity of list 1, validity of list 2, region boundaries of
    list 1 that are none of list 2, region boundaries of list 2 that are none of list 1."""
    chrom = _ids([iv1, iv2], lambda iv: iv[0])          # numbered by first appearance, list 1 first
    for which, l in ((1, iv1), (2, iv2)):
        for i, iv in enumerate(l):
            if not iv[1] < iv[2]:
                return which, i
            if i > 0:
                a, b = chrom[l[i - 1][0]], chrom[iv[0]]
                if b < a or (a == b and iv[1] < l[i - 1][2]):
                    return which, i
    def boundaries(l):
        starts, ends = set(), set()
        for i, iv in enumerate(l):
            if i == 0 or l[i - 1][0] != iv[0] or l[i - 1][2] != iv[1]:
                starts.add((iv[0], iv[1]))
            if i == len(l) - 1 or l[i + 1][0] != iv[0] or l[i + 1][1] != iv[2]:
                ends.add((iv[0], iv[2]))
        return starts, ends
    for which, x, y in ((1, iv1, iv2), (2, iv2, iv1)):
        ys, ye = boundaries(y)
        for i, iv in enumerate(x):
            if i == 0 or x[i - 1][0] != iv[0] or x[i - 1][2] != iv[1]:
                if (iv[0], iv[1]) not in ys:
                    return which, i
            if i == len(x) - 1 or x[i + 1][0] != iv[0] or x[i + 1][1] != iv[2]:
                if (iv[0], iv[2]) not in ye:
                    return which, i
    return 0, -1


def base_confusion(iv1, iv2, col):
    """{(name in list 1, name in list 2): bases}, by stepping through both lists piece by piece."""
    out = {}
    i = j = 0
    while i < len(iv1) and j < len(iv2):
        a, b = iv1[i], iv2[j]
        lo, hi = max(a[1], b[1]), min(a[2], b[2])
        assert a[0] == b[0] and hi > lo
        key = (a[col], b[col])
        out[key] = out.get(key, 0) + hi - lo
        i += a[2] == hi                                   # with equal covers a gap ends an interval of both lists
        j += b[2] == hi
    assert i == len(iv1) and j == len(iv2)
    return out


def compare_base_level(iv1, iv2, col):
    """(stats, confMat) as the reference's compareBaseLevel returns them."""
    cells = base_confusion(iv1, iv2, col)
    stats, conf = {}, {}
    for (s1, s2), n in cells.items():
        for s in (s1, s2):
            stats.setdefault(s, [0, 0, 0])
        if s1 == s2:
            stats[s1][2] += n
        else:
            stats[s1][0] += n
            stats[s2][1] += n
        conf.setdefault(s2, {})[s1] = n
    return stats, conf


def overlap(a, b):
    return max(0, min(a[2], b[2]) - max(a[1], b[1])) if a[0] == b[0] else 0


def compare_intervals_one_sided(true, pred, col, threshold, use_pred_len, allow_multiple):
    """(stats, confMat) as the reference's compareIntervalsOneSided returns them: stats[true name] = [hits, bases of
    the hits (float), misses, bases of the misses (float)], confMat[pred name][true name] = overlaps >= threshold."""
    stats, conf = {}, {}
    first = 0
    for t in true:
        while first < len(pred) and overlap(t, pred[first]) == 0:
            first += 1
        best, total = 0.0, 0.0
        j = first
        while j < len(pred) and overlap(t, pred[j]) > 0:
            p = pred[j]
            frac = float(overlap(t, p)) / float((p[2] - p[1]) if use_pred_len else (t[2] - t[1]))
            if p[col] == t[col]:
                best = max(best, frac)
                total = total + frac                      # in list order: the sum is order-bound
            if frac >= threshold:
                row = conf.setdefault(p[col], {})
                row[t[col]] = row.get(t[col], 0) + 1
            j += 1
        st = stats.setdefault(t[col], [0, 0.0, 0, 0.0])
        k = 0 if (total if allow_multiple else best) >= threshold else 2
        st[k] += 1
        st[k + 1] += float(t[2] - t[1])
    return stats, conf


def merge_runs(intervals, col, rename=None):
    """The intervals with column col renamed through the dict rename, abutting neighbours of equal chrom and new name
    merged; a merged interval keeps the other columns of its first member."""
    out = []
    for iv in intervals:
        iv = list(iv)
        if rename is not None:
            iv[col] = rename.get(iv[col], iv[col])
        if out and out[-1][0] == iv[0] and out[-1][col] == iv[col] and out[-1][2] == iv[1]:
            out[-1][2] = iv[2]
        else:
            out.append(iv)
    return [tuple(iv) for iv in out]


def fitted_bed(intervals, state_map, col, no_merge, ignore_tgt):
    """(fitted intervals, BED text) of the reference's writeFittedBed."""
    rename = {k: v[0] for k, v in state_map.items() if v[0] not in ignore_tgt}
    if no_merge:
        fitted = [tuple(iv[:col]) + (rename.get(iv[col], iv[col]),) + tuple(iv[col + 1:]) for iv in intervals]
    else:
        fitted = merge_runs(intervals, col, rename)
    return fitted, "".join("\t".join(str(x) for x in iv) + "\n" for iv in fitted)


# ---- seeded lists -----------------------------------------------------------------------------------------------------
def random_pair(rs, n_regions, n_labels, mean_len=20, chroms=1, start=100, breaks=0.1, gap=50):
    """Two valid lists over the same cover: `chroms` chromosomes of n_regions regions each (gaps between them), each
    region cut independently for the two lists at a share `breaks` of its bases; names "s<k>" drawn from n_labels."""
    iv1, iv2 = [], []
    for c in range(chroms):
        pos = start
        for _ in range(n_regions):
            length = int(rs.randint(1, 2 * mean_len))
            for out in (iv1, iv2):
                cuts = [pos] + [pos + int(x) for x in np.flatnonzero(rs.rand(length - 1) < breaks) + 1] + [pos + length]
                for a, b in zip(cuts[:-1], cuts[1:]):
                    out.append(("chr%d" % (c + 1), a, b, "s%d" % rs.randint(n_labels)))
            pos += length + int(rs.randint(1, gap))
    return iv1, iv2
