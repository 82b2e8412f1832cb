"""The cases of tests/trained_shapes.py on the CPU: every case the GPU tests use satisfies its builder conditions (the
linear product underflows on the cover rows of "m1e6" and "peaked" and nowhere else, the reference's log-domain rows are
emittable), and the fp64 oracle agrees with a long-double restatement of the same formulas inside the bounds the GPU
tests then hold the kernels to -- so the expected values are no artefact of fp64 running sums at a magnitude of 1e7."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import trained_shapes as ts


def _ld(c, a, b, control=False, estep=False):
    obs = c.control if control else c.obs
    return ts.forward_backward_ld(obs[a:b], c.log_probs, c.model.log_startprob, c.model.log_transmat, c.spec.normalize,
                                  None if c.ratios is None else c.ratios[a:b], estep=estep)


def test_plant_kinds():
    """What plant() promises, on the smallest table: a third of the symbols per (track, state), exact values, cover row."""
    from tehmm_amd import synth
    model = synth.make_model(5, ts.SYM10, (), seed=1)
    cov = ts.cover_row(model)
    for kind in ("m1e6", "m1e100", "peaked"):
        lp = ts.plant(model, kind, 2)
        cells = ts.planted_cells(model, lp)
        assert_array_equal(cells.sum(axis=2), np.asarray(ts.SYM10)[:, None] // 3 * np.ones((1, 5), dtype=int))
        assert (lp[cells] == ts.LOG_ZERO[kind]).all() and np.isfinite(lp).all()
        hit = cells[np.arange(10), :, cov]
        assert hit[:, 1:].any(axis=0).all() and hit[:, 0].any() == (kind != "m1e100")
        assert not np.array_equal(lp, ts.plant(model, kind, 3))
        assert_array_equal(lp, ts.plant(model, kind, 2))
    lp = ts.plant(model, "unseen", 2)
    cells = ts.planted_cells(model, lp)
    assert cells.sum() == 5 and cells[0, :, cov[0]].all()
    assert (ts.linear_product(lp, cov[None, :]) > 0.01).any()          # the per-row scale absorbs the column


def test_cover_positions():
    assert ts.cover_positions(1500) == {"first": 0, "inside": 100, "chunk_end": 255, "chunk_start": 256, "ratio": 828,
                                        "middle": 956, "last": 1499}
    assert ts.cover_positions(700) == {"first": 0, "inside": 100, "chunk_end": 255, "chunk_start": 256, "ratio": 316,
                                       "middle": 444, "last": 699}
    assert ts.cover_positions(256) == {} and ts.cover_positions(1) == {} and ts.cover_positions(0) == {}
    assert_array_equal(ts.cover_rows_of([700, 0, 1, 700])[[0, 6, 7, 13]], [0, 699, 701, 1400])


@pytest.mark.parametrize("name", ts.EVAL_CASES)
def test_oracle_evaluation_against_long_double(name):
    c = ts.case(name)                                                 # (asserts the builder conditions)
    paths, vlp, flp, post = ts.oracle_eval(name)
    _, vlp_c, flp_c, _ = ts.oracle_eval(name, control=True)
    assert np.isfinite(vlp).all() and np.isfinite(flp).all() and np.isfinite(post).all()
    worst = {"flp": 0.0, "vlp": 0.0, "post_rel": 0.0}
    for i, (a, b) in enumerate(c.intervals()):
        ref = _ld(c, a, b)
        d_f = float(abs(np.longdouble(flp[i]) - ref["logprob"]))
        d_v = float(abs(np.longdouble(vlp[i]) - ref["viterbi_logprob"]))
        b_f, b_v = ts.logprob_bound(flp[i], flp_c[i], b - a), ts.logprob_bound(vlp[i], vlp_c[i], b - a)
        p = ref["post"].astype(np.float64)
        rel = float(np.max(np.abs(post[a:b] - p) / p))
        print("%s interval %d: forward log-likelihood %.10g (control %.10g) off by %.3g of %.3g allowed; Viterbi score "
              "%.10g off by %.3g of %.3g; posterior max rel. err %.3g"
              % (name, i, flp[i], flp_c[i], d_f, b_f, vlp[i], d_v, b_v, rel))
        assert d_f <= b_f and d_v <= b_v
        assert_array_equal(paths[a:b], ref["path"])
        assert_allclose(post[a:b], p, rtol=1e-6, atol=1e-15)
        worst = {"flp": max(worst["flp"], d_f), "vlp": max(worst["vlp"], d_v), "post_rel": max(worst["post_rel"], rel)}
    # the rows on which the GPU test does not compare the maximum-posterior state: under 1 %
    undecided = int((~ts.map_rows(post)).sum())
    print("%s: maxima %s; %d of %d rows without a decided maximum-posterior state" % (name, worst, undecided, len(post)))
    assert undecided < 0.01 * len(post)
    # the planted case sits a cover row's worth of log-zeros below its control
    n_cov = [len(ts.cover_positions(n)) for n in c.lens]
    if c.spec.kind in ("m1e6", "unseen"):
        assert_allclose(flp - flp_c, [-1e6 * n * c.spec.normalize for n in n_cov], rtol=1e-3)


@pytest.mark.parametrize("name", ts.ESTEP_CASES)
def test_oracle_estep_against_long_double(name):
    c = ts.case(name, True)
    per, per_c = ts.oracle_estep(name), ts.oracle_estep(name, control=True)
    cells = ts.planted_cells(c.model, c.log_probs)
    for i, (a, b) in enumerate(c.intervals()):
        ref = _ld(c, a, b, estep=True)
        got = per[i]
        d = float(abs(np.longdouble(got["logprob"]) - ref["logprob"]))
        bound = ts.logprob_bound(got["logprob"], per_c[i]["logprob"], b - a)
        err = {k: float(np.max(np.abs(got[k] - ref[k].astype(np.float64)))) for k in ("start", "trans", "obs")}
        print("%s E-step interval %d (%d rows): log-likelihood %.10g off by %.3g of %.3g allowed; max abs. err %s; planted "
              "cells hold at most %.3g" % (name, i, b - a, got["logprob"], d, bound, err, got["obs"][cells].max()))
        assert d <= bound
        assert_allclose(got["start"], ref["start"].astype(np.float64), rtol=1e-6, atol=1e-12)
        assert_allclose(got["trans"], ref["trans"].astype(np.float64), rtol=1e-6, atol=1e-9)
        assert_allclose(got["obs"], ref["obs"].astype(np.float64), rtol=1e-6, atol=1e-9)
        assert_allclose(got["obs"][cells], ref["obs"].astype(np.float64)[cells], rtol=1e-6, atol=1e-12)
    tot = ts.estep_total(per)
    assert np.isfinite(tot["logprob"]) and np.isfinite(tot["obs"]).all()
    # a planted cell collects posterior mass on cover rows only (every state is equally impossible there): elsewhere its
    # state sits 1e6 (20 a track) below the others
    if c.spec.kind == "m1e6":
        cov = ts.cover_row(c.model)
        off_cover = cells.copy()
        off_cover[np.arange(len(cov)), :, cov] = False
        assert (tot["obs"][off_cover] == 0.0).all()
