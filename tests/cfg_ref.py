"""Plain NumPy restatement of the CYK decode of the grammar model: what tehmm_cyk_decode and
tehmm_cyk_get_dp have to return, bit for bit.

For size = 2..L, every cell (i, j = i + size - 1) and every state x, candidates are visited in the order
  splits   q (the productions x -> r1 r2 above -inf, ascending (r1, r2)) outer, k = i..j-1 inner:
           (logProbs1[x, r1, r2] + dp[i, k, r1]) + dp[k+1, j, r2]
  pairs    only for size > 2, ascending r over logProbs2[x, r] > -inf:
           (((logProbs2[x, r] + dp[i+1, j-1, r]) + em[i, x]) + em[j, x]) + logPriors[x, match(i, j)]
and a candidate replaces the cell only when strictly greater, so among equal values the first one visited wins.  The
diagonal holds em[i, x] for single states; the size-2 cell of a pair state starts as
(em[i, x] + em[i+1, x]) + logPriors[x, match(i, i+1)].  match(i, j) = an alignment row is given and
al[i] != defAlignmentSymbol and al[i] == al[j].

The cells of one diagonal are independent, so the code below handles a whole diagonal at once: per production one
array of candidates [cell, k], its first maximum along k, and a strict `>` against the running best.
"""
import numpy as np
from numpy.lib.stride_tricks import as_strided

PAIRFLAG = -2


def golden_case(z, name):
    """The arguments of cyk() of case `name` of tests/golden/cfg.npz, as a dict."""
    M = z[name + "_em"].shape[1]
    is_nest = np.zeros(M, dtype=np.uint8)
    is_nest[z[name + "_nest"].astype(np.int64)] = 1
    return dict(em=z[name + "_em"], al=z[name + "_al"] if name + "_al" in z.files else None,
                def_sym=int(z[name + "_def"]), is_nest=is_nest, lp1=z[name + "_lp1"], lp2=z[name + "_lp2"],
                priors=z[name + "_priors"], log_start=z[name + "_start"])


def helper_lists(lp1, lp2):
    M = lp1.shape[0]
    h1 = [[(r1, r2, lp1[x, r1, r2]) for r1 in range(M) for r2 in range(M) if lp1[x, r1, r2] > -np.inf]
          for x in range(M)]
    h2 = [[(r, lp2[x, r]) for r in range(M) if lp2[x, r] > -np.inf] for x in range(M)]
    return h1, h2


def cyk(em, al, def_sym, is_nest, lp1, lp2, priors, log_start):
    """em [L, M], al [L] or None -> (score, top, trace float64 [L], dp [L, L, M] with -inf below the diagonal).
    Raises ValueError when the derivation reaches a cell without a winner."""
    em = np.ascontiguousarray(em, dtype=np.float64)
    L, M = em.shape
    h1, h2 = helper_lists(lp1, lp2)
    # diagonal-major tables: D[x, t, i] is cell (i, i + t) of state x
    D = np.full((M, L, L), -np.inf)
    TB = np.full((M, L, L, 3), -1, dtype=np.int32)
    s0, s1 = D.strides[1], D.strides[2]

    def match(t, n):
        if al is None:
            return np.zeros(n, dtype=np.int64)
        a = np.asarray(al[:n], dtype=np.int64)
        return ((a != def_sym) & (a == np.asarray(al[t:t + n], dtype=np.int64))).astype(np.int64)

    for x in range(M):
        if not is_nest[x]:
            D[x, 0, :] = em[:, x]
        elif L > 1:
            D[x, 1, :L - 1] = (em[:-1, x] + em[1:, x]) + priors[x, match(1, L - 1)]
            TB[x, 1, :L - 1] = (PAIRFLAG, 0, 0)
    for size in range(2, L + 1):
        n = L - size + 1
        cells = np.arange(n)
        new = []
        for x in range(M):
            best = D[x, size - 1, :n].copy()
            tb = TB[x, size - 1, :n].copy()
            for r1, r2, lp in h1[x]:
                A = D[r1, :size - 1, :n].T                                    # [cell i, k - i] = dp[i, k, r1]
                B = as_strided(D[r2, size - 2:, 1:], shape=(n, size - 1), strides=(s1, s1 - s0))     # dp[k+1, j, r2]
                cand = (lp + A) + B
                a = cand.argmax(axis=1)                                       # first maximum along k
                m = cand[cells, a]
                up = m > best
                best[up] = m[up]
                tb[up, 0] = (cells + a)[up]
                tb[up, 1] = r1
                tb[up, 2] = r2
            if size > 2:
                pr = priors[x, match(size - 1, n)]
                for r, lp in h2[x]:
                    m = (((lp + D[r, size - 3, 1:1 + n]) + em[:n, x]) + em[size - 1:, x]) + pr
                    up = m > best
                    best[up] = m[up]
                    tb[up] = (PAIRFLAG, r, r)
            new.append((best, tb))
        for x, (best, tb) in enumerate(new):
            D[x, size - 1, :n] = best
            TB[x, size - 1, :n] = tb
    tops = log_start + D[:, L - 1, 0]
    top = int(np.argmax(tops))
    score = tops[top]
    trace = -1 + np.zeros(L)
    stack = [(0, L - 1, top)]
    while stack:
        i, j, state = stack.pop()
        if i == j:
            trace[i] = state
            continue
        k, r1, r2 = (int(v) for v in TB[state, j - i, i])
        if k == PAIRFLAG:
            trace[i] = trace[j] = state
            if j - i + 1 > 2:
                stack.append((i + 1, j - 1, r1))
        elif k < 0:
            raise ValueError("no derivation: cell (%d, %d) of state %d has no winner" % (i, j, state))
        else:
            stack.append((i, k, r1))
            stack.append((k + 1, j, r2))
    dp = np.full((L, L, M), -np.inf)
    for t in range(L):
        dp[np.arange(L - t), np.arange(t, L), :] = D[:, t, :L - t].T
    return score, top, trace, dp
