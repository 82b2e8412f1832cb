"""Plain-Python statement of the segmentation chain (bin/segmentTracks.py:200-277), the yardstick of the segmenter
tests.  One interpreter step per row, like the reference; nothing here is shared with tehmm_amd/segmenter.py.

segment_offsets(d, ...)   offsets of one table's segments (the first is 0), optionally the --stats numbers
bed_rows(...)             the BED rows of a run over several tables (the label counter carries over)
"""
import numpy as np


def segment_offsets(d, ignore, cut, thresh=1, comp="first", maxLen=0, fixLen=0, stats=None):
    """d: [T][K] table.  stats: None, or a dict {track: [count, share]} that the data-rule cuts add into, in row
    order (the same order of additions as the reference's running sums)."""
    if comp not in ("first", "prev"):
        raise RuntimeError("--comp must be either first or prev")
    rows = [bytes(r) for r in np.ascontiguousarray(d, dtype=np.uint8)]
    live = [j for j in range(len(ignore)) if ignore[j] == 0]
    cutset = set(j for j in live if cut[j] == 1)
    prev = comp == "prev"
    offsets = [0]
    pi = 0
    cur = 0
    for i in range(1, len(rows)):
        cur += 1
        if fixLen > 0:
            c = cur >= fixLen
        elif maxLen > 0 and cur >= maxLen:
            c = True
        else:
            a, b = rows[i], rows[pi]
            if a == b:
                c = False
            else:
                D = [j for j in live if a[j] != b[j]]
                c = len(D) > thresh or any(j in cutset for j in D)
                if c and stats is not None:
                    for j in D:
                        st = stats.setdefault(j, [0, 0.0])
                        st[0] += 1
                        st[1] += 1.0 / float(len(D))
        if c:
            offsets.append(i)
            pi = i
            cur = 0
        if prev:
            pi = i
    return np.asarray(offsets, dtype=np.int64)


def bed_rows(tables, offsets, co=0):
    """tables: [(chrom, start, end)]; offsets: one array per table.  Returns [(chrom, start, end, label)]."""
    out = []
    count = int(co)
    for (chrom, start, end), offs in zip(tables, offsets):
        ends = list(offs[1:]) + [end - start]
        for a, b in zip(offs, ends):
            out.append((chrom, int(start + a), int(start + b), hex(count)[2:]))
            count += 1
    return out


def run_structured(rs, T, K, keep=0.9, n_values=4):
    """Seeded table in which every track keeps its value from one row to the next with probability `keep`."""
    change = rs.random_sample((T, K)) >= keep
    change[0] = True
    fresh = rs.randint(0, n_values, size=(T, K))
    last = np.maximum.accumulate(np.where(change, np.arange(T)[:, None], 0), axis=0)      # row of the last draw
    return np.ascontiguousarray(fresh[last, np.arange(K)[None, :]], dtype=np.uint8)
