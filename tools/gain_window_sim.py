"""Binade placement from a windowed gain pass, simulated on the CPU (numpy only).

The gain pass P0 only tells the placement how far the Viterbi score falls over each item.  This script measures how well
that fall is estimated when P0 runs on the last Wn positions of an item only:

  estimator:      gain ~= dF(item) + (g_w - dF(window)) * L / Wn     (tehmm_place.hip.h: place_item_gain)
  extrapolation:  gain ~= g_w * L / Wn

g_w: max-plus gain over the window from a zero start WU positions ahead of it (float32, as the kernel); dF: change of the
forward score (the log-scale records of the forward pass).  Printed: the largest CUMULATIVE error over the sequence, in
positions -- the distance by which a binade crossing would be misplaced -- for both, and for the full pass (Wn = L).

usage: python tools/gain_window_sim.py [--stay 0.995] [--sparse 0.5] [--states 35] [--positions 300000] [--item 512]
                                       [--warmup 32] [WN ...]            (default windows: 64 128 256)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tehmm_amd import synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stay", type=float, default=None)
    ap.add_argument("--sparse", type=float, default=0.0)
    ap.add_argument("--states", type=int, default=35)
    ap.add_argument("--positions", type=int, default=300_000)
    ap.add_argument("--item", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("windows", type=int, nargs="*", default=[64, 128, 256])
    a = ap.parse_args()
    m = synth.make_model(a.states, synth.CONFIG2_SYMBOLS, synth.CONFIG2_GAUSSIAN, seed=0, sparse=a.sparse, stay=a.stay)
    T, L, WU, N = a.positions, a.item, a.warmup, a.states
    obs = synth.sample_obs(m, T, seed=5)
    b = np.zeros((T, N))
    for k in range(m.n_tracks):
        b += m.log_probs[k][:, obs[:, k]].T
    lt, A = m.log_transmat, m.transmat
    # the exact chains: Viterbi maximum M[t] and forward score F[t]
    V = m.log_startprob + b[0]
    al = np.exp(V - V.max())
    M, F = np.empty(T), np.empty(T)
    M[0] = V.max()
    F[0] = V.max() + np.log(al.sum())
    al /= al.sum()
    for t in range(1, T):
        V = (V[:, None] + lt).max(0) + b[t]
        M[t] = V.max()
        mx = b[t].max()
        al = (al @ A) * np.exp(b[t] - mx)
        c = al.sum()
        al /= c
        F[t] = F[t - 1] + np.log(c) + mx
    rate = -M[-1] / T
    print("states %d stay %s sparse %g: Viterbi %.3f per position, Viterbi - forward %.4f per position"
          % (N, a.stay, a.sparse, -rate, (M[-1] - F[-1]) / T))
    items = np.arange(1, T // L)                          # (the first item has no warm-up ahead of it)
    end = (items + 1) * L - 1
    true = M[end] - M[end - L]
    with np.errstate(over="ignore"):                      # (sparse models: -1e100 becomes -inf, as in the kernel's table)
        ltf, bf = lt.astype(np.float32), b.astype(np.float32)

    def window_gain(wn):                                  # all items at once: W [item][state]
        W = np.zeros((len(items), N), dtype=np.float32)
        g0 = None
        for s in range(L - wn - WU, L):
            if s == L - wn:
                g0 = W.max(1)
            W = (W[:, :, None] + ltf[None]).max(1) + bf[items * L + s]
        return (W.max(1) - g0).astype(np.float64)

    def report(tag, est):
        cum = np.cumsum(est - true)
        print("  %-28s largest cumulative error %7.1f positions (final %+.1f)" % (tag, np.abs(cum).max() / rate, cum[-1] / rate))

    report("full pass (Wn = %d)" % L, window_gain(L))     # (warmed up on the item before)
    for wn in a.windows:
        if not (0 < wn and wn + WU <= L):
            print("  Wn = %d: no room for the warm-up inside an item of %d" % (wn, L))
            continue
        gw = window_gain(wn)
        dF, dFw = F[end] - F[end - L], F[end] - F[end - wn]
        report("Wn = %d, estimator" % wn, dF + (gw - dFw) * L / wn)
        report("Wn = %d, extrapolation" % wn, gw * L / wn)


if __name__ == "__main__":
    main()
