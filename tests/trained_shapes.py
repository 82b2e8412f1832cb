"""Emission tables as training leaves them, for tests/test_trained_shapes_cpu.py and tests/test_gpu_trained_shapes.py.

synth.make_model draws multinomial rows (0.2 + 0.6 u) / sum and gaussian rows over a 10 % uniform floor: no state is ever
more than about 4x off the best state of a track and no cell is a log-zero.  A trained table is different.  The M-step
(emission.maximize on the host, k_mstep_emis on the device) writes myLog(0) = -1e6 into every (track, state, symbol) cell
whose count is zero, applyUserEmissions writes -1e100 for a forced zero, and trained rows are peaked.  plant() turns the
generator's table into such a one, observations() samples from it and writes a designated symbol vector -- the cover row
-- at fixed positions of every multi-chunk interval: on it every state meets a planted cell, the states spread over
different tracks.  The linear product the fused passes form below 64 states (tehmm_fused.hip.h),
    q_t[j] = prod_k exp(lp[k][j][s] - max_j lp[k][.][s]),
is then 0 for every state at once, where the reference's log-domain row is ordinary: about -1e6 in every state.

forward_backward_ld restates the reference's formulas in np.longdouble; the CPU test holds the fp64 oracle against it, so
that the expected values of the GPU tests are known not to be an artefact of fp64 at a magnitude of 1e7.

Not covered: rows after the first emittable one on which every state sits at or below -1e20 without being -inf (a cover
row of "m1e100" that also hit state 0).  The reference's lattices collapse to -1e100 in every state there and what it
returns afterwards is the rounding noise of its own operation order; the "m1e100" tables avoid such rows by construction.
"""
import dataclasses
import functools

import numpy as np

CHUNK = 256                                   # TEHMM_SPEC_CHUNK of the small shapes (test_gpu_estep_routes.SMALL_SHAPES)
LOG_ZERO = {"m1e6": -1e6, "m1e100": -1e100, "peaked": -20.0, "unseen": -1e6}
F32_EPS = float(np.finfo(np.float32).eps)
MINDBL = -1e20                                # _emission.pyx: a row is emittable when some state is above this
ZEROLOGPROB = -1e200                          # _hmm.pyx: lattice values at or below this become -inf
UNDERFLOW = 1e-280                            # k_fused_fwd / k_fused_bwd: "the product underflowed" below this
SYM10 = (3, 5, 4, 8, 6, 3, 7, 4, 5, 8)        # 10 tracks of 3 .. 8 symbols
LENS = [1500, 0, 700, 1]                      # test_gpu_estep_routes.LENS
LENS2 = [1500, 700]


# ------------------------------------------------------------------------------------------------ the planted table
def eligible_tracks(model, skip=()):
    return [k for k, sk in enumerate(model.symbols_per_track) if sk >= 3 and k not in skip]


def cover_row(model):
    """The designated symbol vector (one symbol 1 .. S_k per track): a function of the track list alone."""
    return np.asarray([1 + (3 * k + 1) % sk for k, sk in enumerate(model.symbols_per_track)], dtype=np.uint8)


def designated(model, kind, skip=()):
    """bool [K, N]: the (track, state) pairs whose planted cells include the track's cover symbol.
    m1e6: state j in track E[j mod len(E)], E the eligible tracks -- every state once, neighbours in different tracks,
    and no track in which every state is planted (the per-row scale of k_build_ptab would absorb that one).
    m1e100: the same without state 0.  peaked: every state but state k mod N in EVERY track, so that a state meets the
    value in all tracks but about K / N of them.  unseen: none (the whole column is set instead)."""
    K, N = model.n_tracks, model.n_states
    E = eligible_tracks(model, skip)
    d = np.zeros((K, N), dtype=bool)
    if kind in ("m1e6", "m1e100"):
        assert len(E) >= 2
        for j in range(N):
            d[E[j % len(E)], j] = True
        if kind == "m1e100":
            d[:, 0] = False
        assert not d.all(axis=1).any()
    elif kind == "peaked":
        assert N >= 2
        for k in E:
            d[k] = np.arange(N) != k % N
    elif kind != "unseen":
        raise KeyError(kind)
    return d


def plant(model, kind, seed, skip=()):
    """The generator's table as training leaves it -> log_probs [K, N, S].  Per (track, state) of every track with at
    least 3 symbols (`skip`: tracks left alone, the gaussian ones) a third of the symbols get probability 0, the rest is
    renormalised, the zero cells get LOG_ZERO[kind].  "unseen": instead, the cover symbol of the first eligible track
    gets probability 0 in every state."""
    rs = np.random.RandomState(seed)
    cov = cover_row(model)
    des = designated(model, kind, skip)
    P = model.probs.copy()
    zero = np.zeros(P.shape, dtype=bool)
    E = eligible_tracks(model, skip)
    if kind == "unseen":
        zero[E[0], :, cov[E[0]]] = True
    else:
        for k in E:
            sk = model.symbols_per_track[k]
            others = np.asarray([s for s in range(1, sk + 1) if s != cov[k]])
            for j in range(model.n_states):
                n = sk // 3
                if des[k, j]:
                    zero[k, j, cov[k]] = True
                    n -= 1
                zero[k, j, rs.choice(others, size=n, replace=False)] = True
    P[zero] = 0.0
    for k, sk in enumerate(model.symbols_per_track):
        P[k, :, 1:1 + sk] /= P[k, :, 1:1 + sk].sum(axis=1, keepdims=True)
    lp = model.log_probs.copy()
    live = (P > 0) & ~zero
    lp[live] = np.log(P[live])
    lp[zero] = LOG_ZERO[kind]
    lp[:, :, 0] = 0.0
    for k, sk in enumerate(model.symbols_per_track):
        lp[k, :, 1 + sk:] = model.log_probs[k, :, 1 + sk:]          # (padding symbols as the generator left them)
    return np.ascontiguousarray(lp)


def planted_cells(model, log_probs):
    """bool [K, N, S]: the cells plant() set (they are the only ones at or below -20 + 1e-9)."""
    m = log_probs <= -20.0
    for k, sk in enumerate(model.symbols_per_track):
        m[k, :, 1 + sk:] = False
    m[:, :, 0] = False
    return m


def planted_model(model, log_probs):
    """The SynthModel sample_obs needs: planted cells have probability 0 (e^-20 included), symbol 0 stays "missing"."""
    P = np.zeros_like(model.probs)
    P[:, :, 0] = 1.0
    for k, sk in enumerate(model.symbols_per_track):
        row = np.exp(log_probs[k, :, 1:1 + sk])
        row[log_probs[k, :, 1:1 + sk] <= -20.0] = 0.0
        P[k, :, 1:1 + sk] = row / row.sum(axis=1, keepdims=True)
    return dataclasses.replace(model, log_probs=log_probs, probs=P)


# ------------------------------------------------------------------------------------------------ the observations
def cover_positions(length, chunk=CHUNK):
    """Where the cover row goes in an interval of `length` rows, {role: row}; nothing in a single-chunk interval.
    Seven rows: the running sums stay near 1e7."""
    if length <= chunk:
        return {}
    n_chunks = (length + chunk - 1) // chunk
    mid = (n_chunks // 2) * chunk
    pos = {"first": 0, "inside": 100, "chunk_end": chunk - 1, "chunk_start": chunk, "ratio": mid + 60, "middle": mid + 188,
           "last": length - 1}
    assert len(set(pos.values())) == 7 and max(pos.values()) == length - 1 and pos["middle"] < length - 1
    return pos


def cover_rows_of(lens):
    """Batch row numbers of every cover row, ascending."""
    out, t0 = [], 0
    for n in lens:
        out += [t0 + p for p in cover_positions(n).values()]
        t0 += n
    return np.asarray(sorted(out), dtype=np.int64)


def control_observations(model, log_probs, lens, seed):
    """sample_obs of the planted model over the whole batch, 2 % missing: no cover row."""
    from tehmm_amd import synth
    return synth.sample_obs(planted_model(model, log_probs), int(np.sum(lens)), seed=seed, missing=0.02)


def observations(model, log_probs, lens, seed):
    """control_observations with the cover row written at cover_positions of every multi-chunk interval."""
    obs = control_observations(model, log_probs, lens, seed)
    obs[cover_rows_of(lens)] = cover_row(model)
    return obs


def seg_ratios(lens, seed, mean=4.0):
    """Segment ratios as test_gpu_estep_routes._seg_ratios draws them (length / mean length, many of them 1); the cover
    row "ratio" of every interval gets 2.5, the cover row "middle" exactly 1."""
    total = int(np.sum(lens))
    rs = np.random.RandomState(seed)
    r = np.clip(rs.geometric(1.0 / mean, size=total), 1, 60).astype(np.float64) / mean
    r[rs.rand(total) < 0.3] = 1.0
    t0 = 0
    for n in lens:
        pos = cover_positions(n)
        if pos:
            r[t0 + pos["ratio"]] = 2.5
            r[t0 + pos["middle"]] = 1.0
        t0 += n
    return r


def linear_product(log_probs, obs):
    """q [T, N] = prod_k exp(lp[k][j][s] - max_j lp[k][.][s]), fp64, tracks in order: the emission row of the fused passes."""
    K, N, _ = log_probs.shape
    q = np.ones((obs.shape[0], N))
    for k in range(K):
        col = log_probs[k][:, obs[:, k]].T                           # [T, N]
        q *= np.exp(col - col.max(axis=1, keepdims=True))
    return q


def log_rows(log_probs, obs, normalize=1.0):
    """The reference's emission rows [T, N] (no leading-rows rule: the builder asserts row 0 is emittable)."""
    x = np.zeros((obs.shape[0], log_probs.shape[1]))
    for k in range(log_probs.shape[0]):
        x += log_probs[k][:, obs[:, k]].T
    return x * normalize


# ------------------------------------------------------------------------------------------------ long double
def _lse(w, axis):
    m = w.max(axis=axis, keepdims=True)
    return (np.log(np.exp(w - m).sum(axis=axis, keepdims=True)) + m).squeeze(axis)


def forward_backward_ld(obs, log_probs, log_startprob, log_transmat, normalize=1.0, ratios=None, estep=False):
    """One interval in np.longdouble, log domain, from the reference's formulas.
    estep=False: what teHmmEval computes -- score_samples without ratios (forward log-likelihood, posteriors with the
    float32-eps renormalisation) and decode (emission rows without ratios, Viterbi with them and its from-state-0 quirk).
    estep=True: the Baum-Welch statistics of the interval, ratios applied everywhere.
    -> dict of longdouble scalars / arrays ("path": int64)."""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63, "np.longdouble is not the 80-bit format here"
    obs = np.asarray(obs)
    T, K = obs.shape
    lp, pi, lt = log_probs.astype(ld), log_startprob.astype(ld), log_transmat.astype(ld)
    N = lp.shape[1]
    diag = np.diagonal(lt).copy()
    frame = np.zeros((T, N), dtype=ld)
    for k in range(K):
        frame += lp[k][:, obs[:, k]].T
    frame *= ld(normalize)
    assert frame[0].max() > MINDBL                                    # (no leading rows to zero)
    r = None if ratios is None else np.asarray(ratios, dtype=np.float64).astype(ld)
    out = {}
    with np.errstate(divide="ignore", under="ignore"):
        if not estep:
            # decode: _hmm.pyx:201-259
            V = pi + frame[0]
            if r is not None and r[0] > 1:
                V = V + diag * (r[0] - 1)
            tb = np.zeros((T, N), dtype=np.int64)
            for t in range(1, T):
                c = V[:, None] + lt + frame[t][None, :]
                if r is not None:
                    if r[t] > 1:
                        c[1:] += (diag * (r[t] - 1))[None, :]
                    c[0] += diag * r[t]
                    c[0, 0] -= lt[0, 0]
                tb[t] = np.argmax(c, axis=0)                          # (first maximum = lowest from-state)
                V = c.max(axis=0)
            path = np.zeros(T, dtype=np.int64)
            path[T - 1] = int(np.argmax(V))
            for t in range(T - 1, 0, -1):
                path[t - 1] = tb[t, path[t]]
            out["viterbi_logprob"], out["path"] = V[path[T - 1]], path
            rf = None                                                 # score_samples: no ratios anywhere
        else:
            frame = frame * r[:, None] if r is not None else frame
            rf = r
        fwd = np.zeros((T, N), dtype=ld)
        fwd[0] = pi + frame[0]
        if rf is not None and rf[0] > 1:
            fwd[0] += diag * (rf[0] - 1)
        for t in range(1, T):
            w = fwd[t - 1][:, None] + lt
            if rf is not None and rf[t] > 1:
                w = w + (diag * (rf[t] - 1))[None, :]
            v = _lse(w, 0) + frame[t]
            v[v <= ZEROLOGPROB] = -np.inf
            fwd[t] = v
        bwd = np.zeros((T, N), dtype=ld)
        bwd[T - 1] = np.log(ld(1) / ld(N))
        for t in range(T - 2, -1, -1):
            w = lt + (frame[t + 1] + bwd[t + 1])[None, :]
            if rf is not None and rf[t + 1] > 1:
                w = w + (diag * (rf[t + 1] - 1))[None, :]
            v = _lse(w, 1)
            v[v <= ZEROLOGPROB] = -np.inf
            bwd[t] = v
        logprob = _lse(fwd[T - 1], 0)
        g = fwd + bwd
        post = np.exp(g - _lse(g, 1)[:, None])
        out["logprob"] = logprob
        if not estep:
            post = post + ld(F32_EPS)
            out["post"] = post / post.sum(axis=1, keepdims=True)
            return out
        trans = np.zeros((N, N), dtype=ld)
        for t in range(T - 1):                                        # _hmm.pyx:62-117, summed directly
            x = fwd[t][:, None] + lt + (frame[t + 1] + bwd[t + 1])[None, :] - logprob
            if rf is not None and rf[t + 1] > 1:
                x = x + (diag * (rf[t + 1] - 1))[None, :]
                trans[np.arange(N), np.arange(N)] += np.exp(fwd[t + 1] + bwd[t + 1] + np.log(rf[t + 1] - 1) - logprob)
            trans += np.exp(x)
        st = np.zeros(lp.shape, dtype=ld)
        wp = post if rf is None else post * rf[:, None]
        for k in range(K):
            for s in np.unique(obs[:, k]):
                st[k, :, s] = wp[obs[:, k] == s].sum(axis=0)
        out.update(start=post[0], trans=trans, obs=st)
        return out


# ------------------------------------------------------------------------------------------------ the cases
@dataclasses.dataclass(frozen=True)
class Spec:
    n_states: int
    symbols: tuple
    gaussian: tuple
    kind: str
    normalize: float = 1.0
    ratios: bool = False
    seed: int = 0
    estep_routes: tuple = ()                  # the E-step routes of test_gpu_estep_routes.ROUTE_KNOBS this case runs on
    evaluate: bool = True
    eval_lens: tuple = tuple(LENS2)
    plant_skip: tuple = ()                    # tracks plant() leaves alone besides the gaussian ones


def _specs():
    from tehmm_amd import synth
    c2, g2 = tuple(synth.CONFIG2_SYMBOLS), tuple(synth.CONFIG2_GAUSSIAN)
    k64 = (4,) * 64
    all3 = ("fused", "wide", "sequential")
    return {
        "n5-m1e6": Spec(5, SYM10, (), "m1e6", seed=105, estep_routes=all3),
        "n5-m1e100": Spec(5, SYM10, (), "m1e100", seed=106),
        "n5-unseen": Spec(5, SYM10, (), "unseen", seed=107),
        "n19-m1e6": Spec(19, SYM10, (), "m1e6", seed=119),
        "n32-m1e6": Spec(32, SYM10, (), "m1e6", seed=132),
        "n35c2-m1e6": Spec(35, c2, g2, "m1e6", seed=135, estep_routes=("fused",)),
        "n35c2-m1e100": Spec(35, c2, g2, "m1e100", seed=136),
        "n35c2-emfac-m1e6": Spec(35, c2, g2, "m1e6", normalize=0.7, seed=137),
        "n5k64-peaked": Spec(5, k64, (), "peaked", seed=164, estep_routes=all3),
        # e^-20 (against e^-1.2 or so in the state that is spared) in 39 or 40 of the tracks: the product does not reach 0,
        # its largest entry is a denormal of fewer than 20 bits (4e-321 here: ten)
        "n5k64-denormal": Spec(5, k64, (), "peaked", seed=165, estep_routes=("fused",), plant_skip=tuple(range(49, 64))),
        "n35-ratios-m1e6": Spec(35, SYM10, (), "m1e6", ratios=True, seed=235, estep_routes=("wide_default", "sequential")),
        # (the item-parallel posterior passes take batches of 4096 rows and up: the same two intervals twice)
        "n70-m1e6": Spec(70, SYM10, (), "m1e6", seed=170, estep_routes=("wide_default",), eval_lens=tuple(LENS2) * 2),
        "n70-m1e100": Spec(70, SYM10, (), "m1e100", seed=171, eval_lens=tuple(LENS2) * 2),
        "n130-m1e6": Spec(130, (3, 5, 4), (), "m1e6", seed=230),
    }


SPECS = _specs()
EVAL_CASES = [n for n, s in SPECS.items() if s.evaluate]
ESTEP_CASES = [n for n, s in SPECS.items() if s.estep_routes]


@dataclasses.dataclass(frozen=True)
class Case:
    spec: Spec
    model: object                             # the generator's SynthModel (transitions, start, track list)
    log_probs: np.ndarray                     # the planted table
    lens: tuple
    offs: np.ndarray
    obs: np.ndarray                           # with cover rows
    control: np.ndarray                       # without
    ratios: object                            # [total] or None
    cover: np.ndarray                         # batch rows of the cover rows

    def intervals(self):
        return [(int(a), int(b)) for a, b in zip(self.offs[:-1], self.offs[1:]) if b > a]


@functools.lru_cache(maxsize=None)
def case(name, estep=False):
    """The case of SPECS[name], read-only: evaluation runs on the spec's eval_lens (LENS2), the E-step on LENS (an empty
    and a one-row interval as well).  Asserts the builder conditions: they are what makes the case mean something."""
    from tehmm_amd import synth
    sp = SPECS[name]
    lens = tuple(LENS) if estep else sp.eval_lens
    model = synth.make_model(sp.n_states, sp.symbols, sp.gaussian, seed=sp.seed)
    lp = plant(model, sp.kind, sp.seed + 1, skip=sp.gaussian + sp.plant_skip)
    obs = observations(model, lp, lens, sp.seed + 2)
    ctl = control_observations(model, lp, lens, sp.seed + 2)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    r = seg_ratios(lens, sp.seed + 3) if sp.ratios else None
    cov = cover_rows_of(lens)
    for a in (lp, obs, ctl, offs, cov) + ((r,) if r is not None else ()):
        a.setflags(write=False)
    c = Case(sp, model, lp, lens, offs, obs, ctl, r, cov)
    check_builder(c)
    return c


def check_builder(c):
    """The conditions a case must satisfy (a failure is a bug in the builder, not something to skip)."""
    sp, lp = c.spec, c.log_probs
    total = int(c.offs[-1])
    assert 0 < len(c.cover) and all(len(cover_positions(n)) <= 8 for n in c.lens)
    rest = np.ones(total, dtype=bool)
    rest[c.cover] = False
    assert (c.obs[rest] == c.control[rest]).all() and (c.obs[c.cover] == cover_row(c.model)).all()
    cells = planted_cells(c.model, lp)
    assert cells.any() and (lp[cells] == LOG_ZERO[sp.kind]).all()
    for k, sk in enumerate(c.model.symbols_per_track):               # still distributions (validate())
        np.testing.assert_allclose(np.exp(lp[k, :, 1:1 + sk]).sum(axis=1), 1.0, rtol=0, atol=1e-6)
    q_cov = linear_product(lp, c.obs[c.cover]).sum(axis=1)
    x_cov = log_rows(lp, c.obs[c.cover], sp.normalize).max(axis=1)
    assert (x_cov > MINDBL).all()                                     # the reference treats every cover row as emittable
    if sp.kind in ("m1e6", "peaked"):
        assert (q_cov < UNDERFLOW).all()
        hit = cells[np.arange(len(sp.symbols)), :, cover_row(c.model)]            # [K, N]
        assert hit.any(axis=0).all() and not hit.all(axis=1).any()
        if sp.kind == "m1e6":
            assert (hit.sum(axis=0) == 1).all() and len(set(np.argmax(hit, axis=0)[:len(sp.symbols)])) > 1
        else:
            assert len(sp.symbols) >= 64 and (hit.sum(axis=0) > 33).all()          # e^-20 more than 33 times: < 1e-280
            if sp.plant_skip:                                          # ... and not 0: fewer than 20 bits are left
                q_max = linear_product(lp, c.obs[c.cover]).max(axis=1)
                assert (hit.sum(axis=0) < 41).all() and (q_max > 0.0).all() and (q_max < 2.0 ** (20 - 1074)).all()
            else:
                assert (q_cov == 0.0).all()
    else:
        assert (q_cov >= UNDERFLOW).all()                             # state 0 / the per-row scale keeps the product alive
        if sp.kind == "m1e100":
            assert (log_rows(lp, c.obs[c.cover])[:, 1:] <= -1e99).all()
    assert (linear_product(lp, c.obs[rest]).sum(axis=1) >= UNDERFLOW).all()
    assert (linear_product(lp, c.control).sum(axis=1) >= UNDERFLOW).all()
    if c.ratios is not None:
        t0 = 0
        for n in c.lens:
            pos = cover_positions(n)
            if pos:
                assert c.ratios[t0 + pos["ratio"]] > 1.0 and c.ratios[t0 + pos["middle"]] == 1.0
            t0 += n


# ------------------------------------------------------------------------------------------------ expected values
@functools.lru_cache(maxsize=None)
def oracle_eval(name, control=False):
    """oracle.eval_batch on the case's (control) observations: (paths, viterbi logprobs, forward logprobs, posteriors)."""
    from oracle import oracle
    c = case(name)
    out = oracle.eval_batch(c.control if control else c.obs, c.offs, c.log_probs, c.model.log_startprob,
                            c.model.log_transmat, c.spec.normalize, c.ratios, want_post=True, n_threads=4)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_estep(name, control=False):
    """oracle.estep over the non-empty intervals, per interval (the total is their sum in order): list of dicts."""
    from oracle import oracle
    c = case(name, True)
    obs = c.control if control else c.obs
    out = []
    for a, b in c.intervals():
        out.append(oracle.estep([obs[a:b]], c.log_probs, c.model.log_startprob, c.model.log_transmat, c.spec.normalize,
                                [c.ratios[a:b]] if c.ratios is not None else None))
    return out


def estep_total(per_interval):
    """The sums oracle.estep forms over a list of sequences, in its order."""
    tot = {k: np.zeros_like(per_interval[0][k]) for k in ("start", "trans", "obs")}
    lp = 0.0
    for d in per_interval:
        for k in tot:
            tot[k] += d[k]
        lp += d["logprob"]
    tot["logprob"] = lp
    return tot


def logprob_bound(planted, control, n_rows):
    """The absolute bound on a log-likelihood (or Viterbi score) of `n_rows` positions whose expected value is `planted`
    and whose control-case value is `control`: 1e-9 |control| -- the project's bar on the part of the sum that carries
    information -- plus one ulp of the planted value per position -- one rounding of the running sum per step."""
    return 1e-9 * abs(float(control)) + float(np.spacing(abs(float(planted)))) * int(n_rows)


def map_rows(post, rel=1e-5):
    """bool [T]: rows whose top two posteriors differ by more than `rel` relative -- where the maximum-posterior state is
    decided beyond the error the posterior tolerance allows."""
    top = np.sort(post, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) > rel * top[:, 1]
