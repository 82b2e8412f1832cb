"""Every evaluation and E-step route on emission tables as training leaves them (tests/trained_shapes.py): log-zero cells
of -1e6 and -1e100, rows whose linear product underflows in every state at once (a log-zero per state, 64 tracks of e^-20),
a symbol no state has seen.  Run with -m gpu.

On the cover rows of "m1e6" and "peaked" the fused passes' product form is 0 for every state: k_fused_fwd / k_fused_bwd
poison the item, k_fb_fix recomputes its blocks from the log table, the E-step reductions count those positions from the
rows the exact chain wrote, the quantised Viterbi pass leaves through its "below the range" exit.  The oracle's row is
ordinary there, so every number is compared with the oracle's -- posteriors and statistics at the suite's tolerances,
paths exactly -- and the counters show that the rescue ran.  A log-likelihood of -7e6 is compared absolutely
(trained_shapes.logprob_bound): tests/test_trained_shapes_cpu.py holds the oracle itself to that bound against long double.

What these cases found (both in the backward half of the fused passes, fixed with them): a chunk whose FIRST row
underflows handed the backward chain an all-zero start row (k_fb_stitch took the chunk for verified: the lane pass meets
the zero one step later, in the previous chunk) -- NaN posteriors and NaN statistics from that chunk back to the interval's
start; and a row total that ended as a denormal ("n5k64-denormal": ten bits left) passed k_fused_bwd's `t > 0` and was
rescaled as if it were a number -- posteriors off by 11 % on the row before it, infinite transition statistics in the
fused E-step.

Observed on an MI355X (maxima over the cases; every test prints its own): paths equal and Viterbi scores bit-equal
everywhere; forward log-likelihood off by at most 1.4e-7 on -7.0e6 (allowed 2.1e-5), 1.2e-9 on -1.1e5 ("peaked");
posteriors within 1.2e-7 relative, cover rows included; E-step statistics within 1e-6 relative on every route, planted
cells within 1.9e-7 absolute of masses up to 9.2; exact blocks planted / control on the fused "m1e6" and "peaked" cases
29 / 17 forward, 29 / 9 backward, 69 / 69 Viterbi (all there are: see the assertion and the 40 000-row test), equal on
"unseen" and "m1e100"."""
import functools

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import trained_shapes as ts
from test_gpu_estep_routes import ROUTE_KEYS, knobs

pytestmark = pytest.mark.gpu

FUSED_STAGES = {"forward_pass", "backward_posterior_pass", "backward_chain"}
EXACT_COUNTERS = ("count:forward_exact_blocks", "count:backward_exact_blocks", "count:viterbi_exact_blocks")


@pytest.fixture(scope="module", autouse=True)
def hip():
    from tehmm_amd import _lib, build
    build.build()
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")


# ---------------------------------------------------------------------------------------------------- evaluation
@functools.lru_cache(maxsize=None)
def evaluate(name, control=False):
    """HipModel.eval(viterbi, posterior) at the small shapes on the case's planted (control) observations."""
    from tehmm_amd.engine import HipBatch, HipModel
    c = ts.case(name)
    N = c.spec.n_states
    with knobs("fused"):                                              # (no route knob: the library's own choice)
        hm = HipModel(c.model.log_transmat, c.model.log_startprob, c.log_probs, c.spec.normalize,
                      c.model.symbols_per_track)
        hb = HipBatch(c.control if control else c.obs, c.offs, c.ratios)
        try:
            res = hm.eval(hb, viterbi=True, posterior=True, use_ratios=c.ratios is not None)
            out = {"vlp": np.array(res["viterbi_logprob"]), "flp": np.array(res["forward_logprob"]),
                   "tm": dict(hb.timing()), "paths": np.array(hb.paths()), "post": np.array(hb.posteriors(N))}
            if not control:
                onehot = np.zeros(N)
                onehot[N - 1] = 1.0
                out["sum_onehot"] = hb.posterior_masksum(onehot)
                out["sum_ones"] = hb.posterior_masksum(np.ones(N))
                hb.map_decode()
                out["map_paths"] = np.array(hb.map_paths())
        finally:
            hb.close()
            hm.close()
    return out


def _assert_route(name, tm):
    """The pipeline the case was built for, from the stage names and counters of the call."""
    sp = ts.SPECS[name]
    N = sp.n_states
    if N > 128:
        assert {"k_vit_large", "k_fwd_large", "k_bwd_large"} <= set(tm)
    elif N >= 64:
        assert "count:wide_chunk_parallel_warmup" in tm and "count:viterbi_exact_blocks" in tm
        assert not (FUSED_STAGES & set(tm))
    else:
        assert FUSED_STAGES <= set(tm) and "count:wide_chunk_parallel_warmup" not in tm
        # the tail rows of the product at 20 and 36 padded states, linear domain only (test_gpu_fused_tail.py)
        tail = sp.normalize == 1.0 and (N // 4 * 4 + 4) in (20, 36)
        assert tm["count:fused_tail"] == int(tail)
        assert all(k in tm for k in EXACT_COUNTERS)


@pytest.mark.parametrize("name", ts.EVAL_CASES)
def test_evaluation_matches_oracle(name):
    c = ts.case(name)
    got, ctl = evaluate(name), evaluate(name, control=True)
    paths_o, vlp_o, flp_o, post_o = ts.oracle_eval(name)
    paths_c, vlp_c, flp_c, post_c = ts.oracle_eval(name, control=True)
    _assert_route(name, got["tm"])
    _assert_route(name, ctl["tm"])
    n_rows = np.diff(c.offs)
    b_f = np.asarray([ts.logprob_bound(flp_o[i], flp_c[i], n_rows[i]) for i in range(len(n_rows))])
    b_v = np.asarray([ts.logprob_bound(vlp_o[i], vlp_c[i], n_rows[i]) for i in range(len(n_rows))])
    counters = {k: (got["tm"].get(k), ctl["tm"].get(k)) for k in got["tm"] if k.startswith("count:")}
    rel = np.abs(got["post"] - post_o) / post_o
    print("%s: path mismatches %d; Viterbi score off by %s (allowed %s); forward log-likelihood off by %s (allowed %s); "
          "posterior max rel. err %.3g, on cover rows %.3g; counters planted / control %s"
          % (name, int((got["paths"] != paths_o).sum()), np.abs(got["vlp"] - vlp_o), b_v, np.abs(got["flp"] - flp_o), b_f,
             float(np.nanmax(rel)), float(np.nanmax(rel[c.cover])), counters))
    bad = np.flatnonzero(~np.isfinite(got["post"]).all(axis=1) | (rel > 1e-6).any(axis=1))
    print("%s: %d rows with a posterior that is not finite or off by more than 1e-6: %s" % (name, len(bad), bad[:40]))
    # the planted observations against the oracle
    assert_array_equal(got["paths"], paths_o)
    assert np.isfinite(got["vlp"]).all() and (np.abs(got["vlp"] - vlp_o) <= b_v).all()
    assert np.isfinite(got["flp"]).all() and (np.abs(got["flp"] - flp_o) <= b_f).all()
    assert np.isfinite(got["post"]).all()
    assert_allclose(got["post"], post_o, rtol=1e-6, atol=1e-15)
    assert_allclose(got["post"].sum(axis=1), 1.0, rtol=1e-9)
    decided = ts.map_rows(post_o)
    assert (~decided).sum() < 0.01 * len(decided)
    assert_array_equal(got["map_paths"][decided], np.argmax(post_o, axis=1)[decided])
    assert_allclose(got["sum_onehot"], post_o[:, -1], rtol=1e-6, atol=1e-15)
    assert_allclose(got["sum_ones"], post_o.sum(axis=1), rtol=1e-6, atol=1e-15)
    # the control observations: the same table without the rows that underflow
    assert_array_equal(ctl["paths"], paths_c)
    assert_allclose(ctl["vlp"], vlp_c, rtol=1e-9)
    assert_allclose(ctl["flp"], flp_c, rtol=1e-9)
    assert_allclose(ctl["post"], post_c, rtol=1e-6, atol=1e-15)
    # the case did what it was built for: the exact chains walked the underflowed rows / had nothing more to do
    if c.spec.n_states < 64 and c.spec.normalize == 1.0:
        if c.spec.kind in ("m1e6", "peaked"):
            for k in EXACT_COUNTERS[:2]:
                assert got["tm"][k] > ctl["tm"][k], k
            # The Viterbi chain cannot walk more than everything, and on the control it already does: the quantised
            # pass speculates only where |V| >= 2^15 (TEHMM_SPEC_MIN_E), which 1 500 ordinary rows never reach.  Strictly
            # more blocks than the control, or every block of the batch (32 positions each); what the pass does with a
            # planted table where it does speculate: test_quantised_viterbi_leaves_a_trained_table_to_the_exact_chain.
            k = EXACT_COUNTERS[2]
            every = sum((int(n) + 31) // 32 for n in n_rows)
            assert got["tm"][k] > ctl["tm"][k] or got["tm"][k] == ctl["tm"][k] == every, k
        elif c.spec.kind == "unseen":
            for k in EXACT_COUNTERS:
                assert got["tm"][k] == ctl["tm"][k], k


def test_quantised_viterbi_leaves_a_trained_table_to_the_exact_chain():
    """The quantised Viterbi pass at a length where it does speculate (|V| >= 2^15 from row 1 600 or so at the bench
    shape): one interval of 40 000 rows.  On the generator's table the chain jumps over chunks the pass computed.  On the
    planted table nearly every row holds a state 1e6 below the best one -- a live state below the range of the quantised
    values -- so the pass leaves through that exit everywhere (on the cover rows a chunk also crosses four binades):
    the chain walks every block, strictly more than on the generator's table, and the path and the score equal the
    oracle's on both.  (The small evaluation cases cannot show this: 1 500 rows never reach 2^15 on their control.)"""
    from oracle import oracle
    from tehmm_amd import synth
    from tehmm_amd.engine import HipBatch, HipModel
    c = ts.case("n35c2-m1e6")
    T = 40000
    offs = np.asarray([0, T], dtype=np.int64)
    obs = ts.control_observations(c.model, c.log_probs, [T], 77)
    rows = [k * ts.CHUNK + 100 for k in (143, 144, 145)]
    obs[rows] = ts.cover_row(c.model)
    assert (ts.linear_product(c.log_probs, obs[rows]).sum(axis=1) == 0.0).all()
    runs = {"planted": (c.log_probs, obs), "generator": (c.model.log_probs, synth.sample_obs(c.model, T, seed=77, missing=0.02))}
    got, ref = {}, {}
    with knobs("fused"):
        for name, (lp, o) in runs.items():
            hm = HipModel(c.model.log_transmat, c.model.log_startprob, lp, 1.0, c.model.symbols_per_track)
            hb = HipBatch(o, offs)
            try:
                res = hm.eval(hb, viterbi=True, posterior=False)
                got[name] = (np.array(hb.paths()), float(res["viterbi_logprob"][0]), dict(hb.timing()))
            finally:
                hb.close()
                hm.close()
            ref[name] = oracle.decode(o, lp, c.model.log_startprob, c.model.log_transmat)
    for name in got:
        tm = got[name][2]
        print("%s table: Viterbi score %.10g (oracle %.10g), path mismatches %d, exact blocks %d, chunk jumps %d"
              % (name, got[name][1], ref[name][0], int((got[name][0] != ref[name][1]).sum()),
                 tm["count:viterbi_exact_blocks"], tm["count:viterbi_chunk_jumps"]))
    for name in got:
        assert_array_equal(got[name][0], ref[name][1])
        assert abs(got[name][1] - ref[name][0]) <= ts.logprob_bound(ref[name][0], ref["generator"][0], T)
    assert got["generator"][2]["count:viterbi_chunk_jumps"] > 0
    assert got["planted"][2]["count:viterbi_chunk_jumps"] == 0
    assert got["planted"][2]["count:viterbi_exact_blocks"] == (T + 31) // 32
    assert got["planted"][2]["count:viterbi_exact_blocks"] > got["generator"][2]["count:viterbi_exact_blocks"]


# ---------------------------------------------------------------------------------------------------- E-step
@functools.lru_cache(maxsize=None)
def run_estep(name, route):
    """Two E-steps of one fresh batch on one route (test_gpu_estep_routes.run): [(logprob, start, trans, obs statistics,
    interval logprobs)] * 2 and the timing after each call."""
    from tehmm_amd.engine import HipBatch, HipModel
    c = ts.case(name, True)
    K, N, S = c.log_probs.shape
    out, tms = [], []
    with knobs(route):
        hm = HipModel(c.model.log_transmat, c.model.log_startprob, c.log_probs, c.spec.normalize, c.model.symbols_per_track)
        hb = HipBatch(c.obs, c.offs, c.ratios)
        try:
            for _call in range(2):
                start, trans, st = np.zeros(N), np.zeros((N, N)), np.zeros((K, N, S))
                lp = hm.estep(hb, c.ratios is not None, start, trans, st)
                out.append((lp, start, trans, st, hb.interval_logprobs()))
                tms.append(dict(hb.timing()))
        finally:
            hb.close()
            hm.close()
    return out, tms


def _interval_bounds(name):
    """Per interval of LENS: (the oracle's log-likelihood, the bound on it); the empty interval: (0, 0)."""
    c = ts.case(name, True)
    per, per_c = ts.oracle_estep(name), ts.oracle_estep(name, control=True)
    ref, bound, i = np.zeros(len(c.lens)), np.zeros(len(c.lens)), 0
    for x, n in enumerate(c.lens):
        if n > 0:
            ref[x] = per[i]["logprob"]
            bound[x] = ts.logprob_bound(per[i]["logprob"], per_c[i]["logprob"], n)
            i += 1
    return ref, bound


@pytest.mark.parametrize("name,route", [(n, r) for n in ts.ESTEP_CASES for r in ts.SPECS[n].estep_routes])
def test_estep_route_matches_oracle(name, route):
    c = ts.case(name, True)
    out, tms = run_estep(name, route)
    lp, start, trans, st, ilp = out[0]
    ref = ts.estep_total(ts.oracle_estep(name))
    ilp_o, bound = _interval_bounds(name)
    cells = ts.planted_cells(c.model, c.log_probs)
    print("%s on %s: log-likelihood %.10g off by %.3g (allowed %.3g), intervals off by %s; max abs. err start %.3g trans "
          "%.3g emission %.3g, planted cells %.3g (they hold at most %.3g); counters %s"
          % (name, route, lp, abs(lp - ref["logprob"]), bound.sum(), np.abs(ilp - ilp_o), np.abs(start - ref["start"]).max(),
             np.abs(trans - ref["trans"]).max(), np.abs(st - ref["obs"]).max(), np.abs(st - ref["obs"])[cells].max(),
             ref["obs"][cells].max(), {k: v for k, v in tms[0].items() if k.startswith("count:")}))
    for tm in tms:
        assert list(tm) == ROUTE_KEYS[route]
    for a in (lp, start, trans, st, ilp):
        assert np.isfinite(a).all()
    assert abs(lp - ref["logprob"]) <= bound.sum()
    assert abs(ilp.sum() - ref["logprob"]) <= bound.sum()
    assert (np.abs(ilp - ilp_o) <= bound).all() and ilp[1] == 0.0
    # (tolerances: test_gpu_estep_routes._check_vs_oracle)
    assert_allclose(start, ref["start"], rtol=1e-6, atol=1e-12)
    assert_allclose(trans, ref["trans"], rtol=1e-6, atol=1e-9)
    assert_allclose(st, ref["obs"], rtol=1e-6, atol=1e-9)
    # every planted cell: the mass its state has on the cover rows (all states equally impossible there) and nothing
    # else -- a position the exact chain rescued is counted once and only once
    assert_allclose(st[cells], ref["obs"][cells], rtol=1e-6, atol=1e-12)
    if route == "fused":
        assert tms[0]["count:forward_exact_blocks"] > 0 and tms[0]["count:backward_exact_blocks"] > 0
    # same batch, same route, again: the same bits
    for a, b in zip(out[0], out[1]):
        assert_array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("name", [n for n in ts.ESTEP_CASES if len(ts.SPECS[n].estep_routes) > 1])
def test_interval_logprobs_agree_between_routes(name):
    routes = ts.SPECS[name].estep_routes
    _, bound = _interval_bounds(name)
    ilps = [run_estep(name, r)[0][0][4] for r in routes]
    for r, ilp in zip(routes, ilps):
        print("%s: %s against %s: intervals differ by %s (allowed %s)" % (name, r, routes[-1], np.abs(ilp - ilps[-1]), bound))
        assert np.isfinite(ilp).all() and (np.abs(ilp - ilps[-1]) <= bound).all()


# ---------------------------------------------------------------------------------------------------- training
def test_device_training_writes_and_reads_log_zeros(monkeypatch):
    """Two iterations of tehmm_estep_batch_device + tehmm_model_mstep at 5 states over (3, 5, 4, 250) symbols, one symbol
    of track 1 absent from the batch (and a few bins of the 250-symbol track, for lack of rows): k_mstep_emis writes
    exactly -1e6 into their cells, the next E-steps run on that table.  Against BaseHMM.fit's per-sequence loop over the
    array-level entry points with the host M-step (tolerances: test_device_em_100_states_matches_host_loop)."""
    from tehmm_amd import synth
    from tehmm_amd.basehmm import BaseHMM
    from tehmm_amd.emission import IndependentMultinomialEmissionModel
    from tehmm_amd.engine import DeviceStats, HipBatch, HipModel
    from tehmm_amd.hmm import MultitrackHmm
    N, sym, absent = 5, [3, 5, 4, 250], 3
    truth = synth.make_model(N, tuple(sym), (3,), seed=3)
    init = synth.make_model(N, tuple(sym), (3,), seed=4)
    seqs = [synth.sample_obs(truth, T, seed=50 + i, missing=0.02) for i, T in enumerate(ts.LENS2)]
    for s in seqs:
        s[s[:, 1] == absent, 1] = absent - 1
    never = np.ones((len(sym), init.log_probs.shape[2]), dtype=bool)                 # [K, S]: symbols not in the batch
    for k, sk in enumerate(sym):
        never[k, np.unique(np.concatenate([s[:, k] for s in seqs]))] = False
        never[k, 1 + sk:] = False
    never[:, 0] = False
    assert never[1, absent] and never[1].sum() == 1 and never[0].sum() == 0 and never[3].sum() > 0

    em = IndependentMultinomialEmissionModel(N, sym)
    em.logProbs = init.log_probs.copy()
    host = MultitrackHmm(em, n_iter=3, thresh=0.0, fixStart=False)
    host.transmat_ = init.transmat.copy()
    host.init_params = ""
    host_hist = []
    with knobs("fused"):
        monkeypatch.setenv("TEHMM_DEVICE_EM", "0")
        # the handle of the device loop, from the parameters the host loop starts from
        hm = HipModel(host._log_transmat, host._log_startprob, em.logProbs, normalize=em.normalizeFac,
                      symbols_per_track=em.getNumSymbolsPerTrack())

        def per_sequence_estep(obs, stats):
            host_hist.append(BaseHMM._do_estep(host, obs, stats))
            return host_hist[-1]

        host._do_estep = per_sequence_estep
        host.fit(seqs)                                                # E M E M E
        offs = np.concatenate([[0], np.cumsum(ts.LENS2)]).astype(np.int64)
        hb = HipBatch(np.concatenate(seqs, axis=0), offs)
        stats = DeviceStats(hm)
        dev_hist, params = [], []
        try:
            for it in range(3):
                stats.zero()
                hm.estep_device(hb, False, stats)
                dev_hist.append(stats.head()[0])
                if it < 2:
                    hm.mstep(stats, True, True, True, 1.0, 1.0, em.fudge)
                    params.append(hm.get_params(init.log_probs))
        finally:
            stats.close()
            hb.close()
            hm.close()
    lt1, pi1, lp1 = params[0]
    lt2, pi2, lp2 = params[1]
    for lp in (lp1, lp2):
        assert (lp[1, :, absent] == -1e6).all()
        assert (lp[:, :, :][never[:, None, :].repeat(N, axis=1)] == -1e6).all()
        seen = ~never[:, None, :].repeat(N, axis=1)
        assert (lp[seen] > -1e3).all()                                # nothing else is a log-zero
    print("device against host loop: log-likelihood history %s / %s; max abs. difference transitions %.3g start %.3g "
          "logProbs %.3g" % (dev_hist, host_hist, np.abs(lt2 - host._log_transmat).max(),
                             np.abs(pi2 - host._log_startprob).max(), np.abs(lp2 - host.emissionModel.logProbs).max()))
    assert len(host_hist) == 3 and np.isfinite(dev_hist).all()
    assert_allclose(dev_hist, host_hist, rtol=1e-9)
    assert_allclose(lt2, host._log_transmat, rtol=1e-6, atol=1e-9)
    assert_allclose(pi2, host._log_startprob, rtol=1e-6, atol=1e-9)
    assert_allclose(lp2, host.emissionModel.logProbs, rtol=1e-6, atol=1e-9)
