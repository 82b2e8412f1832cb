#!/usr/bin/env python3
"""Headline benchmark: genome positions/sec for Viterbi + posterior (teHmmEval's hot path),
35 states x 10 tracks, on N MI355X -- one process per GPU, intervals sharded, no data-path
collective ("weak" scaling: every rank evaluates its own 100 Mb shard).

  python bench.py [--gpus N] [--steps K] [--warmup W]        # N > 1: starts the N ranks itself
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
      --master-port P bench.py --gpus N ...                  # or under an external launcher

One "step" = one tehmm_eval_batch(VITERBI | POSTERIOR) over the rank's whole batch of intervals,
observations already resident in HBM, results left in HBM (paths int64 + posteriors f64).  Every timed
step is a FIRST evaluation of its batch as far as derived data go (tehmm_batch_reset_cache drops the
table-row index records of the fused passes): teHmmEval evaluates a batch once.
`--scaling strong`: ONE config-3 interval list (the 9 alyrata scaffolds, 196 Mb, cut at synthetic mask
gaps) LPT-sharded over the ranks (tehmm_amd.dist.lpt_shard) instead of 100 Mb per rank.
`--mode estep` times BASELINE config 4 instead (Baum-Welch iterations: fused E-step per rank, ONE
all-reduce of the packed statistics over RCCL, device M-step).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the steps and prints the line.  `--full` adds, after the timing, what
else the benchmark measures and checks: two intervals of the workload (the shortest and one of >= 1 Mb)
compared with the CPU oracle (`"verified": true` means paths and Viterbi scores bit-exact, posteriors and
log-likelihood within 1e-6; `--mode estep`: four chunks of statistics), the other BASELINE shapes
(`extra`), the CPU baseline, and on several ranks the gather of the per-interval scores; `--no-verify`,
`--no-extra` and `--no-cpu-baseline` drop parts of it.
`--dump-outputs DIR` writes what the last timed step computed, as float64 .npy files (see dump_eval /
em_iterations); the inputs depend on the arguments only, so two builds can be compared output for output.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_STATES = 35
HBM_PEAK_GBPS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
F64_VALU_PEAK_TFLOPS = 78.6


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", choices=("eval", "estep"), default="eval")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak: --mb per GPU; strong: one 196 Mb whole-genome interval list sharded over the GPUs")
    ap.add_argument("--full", action="store_true",
                    help="after the timing also run the oracle checks, the extra measurements and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy")
    ap.add_argument("--no-verify", action="store_true", help="with --full: skip the oracle check of two bench intervals")
    ap.add_argument("--mb", type=float, default=None, help="Mb of genome per GPU (eval: 100, estep: 200)")
    ap.add_argument("--min-kb", type=int, default=200, help="shortest interval (kb)")
    ap.add_argument("--max-kb", type=int, default=2000, help="longest interval (kb)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true",
                    help="with --full: skip the untimed extra measurements (other BASELINE configs, model variants, PCIe)")
    ap.add_argument("--cpu-sample-kb", type=int, default=250,
                    help="positions per CPU-baseline interval (kb); 4 intervals per thread")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def launch_ranks(args):
    """`--gpus N` without a launcher around us: start the N ranks as children of THIS process, which has
    not touched the GPU (never re-exec a process that has), and exit with their code."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def init_dist(dist, device):
    """RCCL prints a version banner on STDOUT when its first communicator comes up; stdout is kept for the one
    JSON line, so the banner goes to stderr."""
    sys.stdout.flush()
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        dist.init_process_group("nccl", device_id=device)
        dist.barrier()
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)


def gen_obs_torch(model, lens, seed, device):
    """Synthetic observations on the GPU (torch is plumbing here): state path made of geometric
    runs (sticky chain like the model's diagonal), symbols drawn from each state's per-track
    distribution by inverse-CDF.  Returns a uint8 [total, K] CUDA tensor."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    total = int(np.sum(lens))
    N, K = model.n_states, model.n_tracks
    stay = float(np.mean(np.diag(model.transmat)))
    n_runs = int(total * (1.0 - stay) * 1.3) + 1024
    u = torch.rand(n_runs, generator=g, device=device, dtype=torch.float64)
    run_len = (torch.log1p(-u) / np.log(stay)).floor().to(torch.int64) + 1
    run_state = torch.randint(0, N, (n_runs,), generator=g, device=device)
    states = torch.repeat_interleave(run_state, run_len)[:total]
    if states.numel() < total:
        states = torch.cat([states, states.new_zeros(total - states.numel())])
    del u, run_len, run_state
    obs = torch.empty((total, K), dtype=torch.uint8, device=device)
    for k, sk in enumerate(model.symbols_per_track):
        cdf = np.cumsum(model.probs[k, :, 1:1 + sk], axis=1)
        cdf[:, -1] = 1.0
        flat = torch.tensor((cdf + np.arange(N)[:, None]).ravel(), device=device, dtype=torch.float64)
        step = 1 << 24
        for a in range(0, total, step):
            st = states[a:a + step]
            uu = torch.rand(st.numel(), generator=g, device=device, dtype=torch.float64) * 0.999999
            idx = torch.searchsorted(flat, uu + st.to(torch.float64), right=True) - st * sk
            obs[a:a + step, k] = (idx.clamp_(0, sk - 1) + 1).to(torch.uint8)
    return obs


def cpu_baseline(model, n_threads, per_interval, n_iv, seed=123):
    """Times the CPU oracle (a port of the reference's Cython loops, oracle/tehmm_oracle.c) on a
    bounded sample of the same workload: the teHmmEval flow (score_samples + decode) per interval,
    one interval per worker thread at a time."""
    from oracle import oracle
    from tehmm_amd import synth
    lens = np.full(n_iv, per_interval, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    obs = synth.sample_obs(model, int(offs[-1]), seed=seed)
    t0 = time.perf_counter()
    oracle.eval_batch(obs, offs, model.log_probs, model.log_startprob, model.log_transmat,
                      1.0, None, want_post=True, n_threads=n_threads)
    dt = time.perf_counter() - t0
    return {"value": float(offs[-1]) / dt, "unit": "positions/s", "cores": int(n_threads),
            "kind": "port",
            "sample": "%d intervals x %d positions, Viterbi + posterior, %d thread(s), %.1f s"
                      % (n_iv, per_interval, n_threads, dt)}


# data/alyrata.bed of the reference: the 9 scaffolds of BASELINE configs[2] (sum 196 089 052)
ALYRATA_SCAFFOLDS = (33132539, 19320864, 24464547, 23328337, 21221946, 25113588, 24649197, 22951293, 1906741)


def genome_intervals(min_kb, max_kb, seed=1000):
    """every scaffold cut at synthetic mask gaps every U(min_kb, max_kb)."""
    from tehmm_amd import synth
    out = []
    for i, L in enumerate(ALYRATA_SCAFFOLDS):
        out.extend(int(x) for x in synth.interval_lengths(L, min_kb * 1000, max_kb * 1000, seed=seed + i))
    return np.asarray(out, dtype=np.int64)


def verify_intervals(model, hb, obs, offs, res, n_threads=2):
    """Oracle check of the bench workload itself: the shortest interval and the shortest one of >= 1 Mb (if
    any), results of the LAST timed step against oracle.eval_batch on the same observations."""
    from oracle import oracle
    lens = np.diff(offs)
    pick = [int(np.argmin(lens))]
    big = np.where(lens >= 1_000_000)[0]
    if len(big):
        pick.append(int(big[np.argmin(lens[big])]))
    pick = sorted(set(pick))
    sub_obs = np.concatenate([obs[int(offs[i]):int(offs[i + 1])].cpu().numpy() for i in pick], axis=0)
    sub_offs = np.concatenate([[0], np.cumsum(lens[pick])]).astype(np.int64)
    t0 = time.perf_counter()
    p_o, vlp_o, flp_o, post_o = oracle.eval_batch(sub_obs, sub_offs, model.log_probs, model.log_startprob,
                                                  model.log_transmat, 1.0, None, want_post=True,
                                                  n_threads=n_threads)
    ok, worst = True, 0.0
    for j, i in enumerate(pick):
        a, b = int(offs[i]), int(offs[i + 1])
        sl = slice(int(sub_offs[j]), int(sub_offs[j + 1]))
        ok &= bool(np.array_equal(hb.paths(a, b), p_o[sl]))
        ok &= bool(res["viterbi_logprob"][i] == vlp_o[j])
        ok &= bool(abs(res["forward_logprob"][i] - flp_o[j]) <= 1e-6 * abs(flp_o[j]))
        rel = float(np.max(np.abs(hb.posteriors(model.n_states, a, b) - post_o[sl]) / post_o[sl]))
        worst = max(worst, rel)
        ok &= rel <= 1e-6
    return {"verified": bool(ok), "verified_intervals": [int(lens[i]) for i in pick],
            "posterior_max_rel_err": worst, "verify_s": time.perf_counter() - t0}


def dump_eval(dirname, hb, res, n_states, n_blocks=64, block=1024, seed=2024):
    """--dump-outputs of the eval step: what tehmm_eval_batch hands its caller, as float64.  The per-interval Viterbi
    and forward log-likelihoods in full; the Viterbi path and the posterior rows (all of them would be 8 + 8 N bytes a
    position, GBs) at a fixed, seeded sample of n_blocks aligned blocks of `block` positions, ~19 MB at N = 35."""
    os.makedirs(dirname, exist_ok=True)
    total = hb.total
    block = min(block, total)
    n_grid = total // block
    starts = np.sort(np.random.default_rng(seed).choice(n_grid, size=min(n_blocks, n_grid), replace=False)) * block
    out = {"viterbi_logprob": res["viterbi_logprob"], "forward_logprob": res["forward_logprob"],
           "sample_positions": np.concatenate([np.arange(a, a + block) for a in starts]),
           "viterbi_path": np.concatenate([hb.paths(a, a + block) for a in starts]),
           "posteriors": np.concatenate([hb.posteriors(n_states, a, a + block) for a in starts])}
    for name, a in out.items():
        np.save(os.path.join(dirname, name + ".npy"), np.asarray(a, dtype=np.float64))


def cpu_baseline_estep(n_seq=4, per_seq=100_000):
    """The oracle's E-step (forward, backward, xi log-sum, emission statistics per sequence: basehmm.py:504-523 as
    restated in oracle/) on a bounded sample of the config-4 workload, one core (the reference is single-threaded)."""
    from oracle import oracle
    from tehmm_amd import synth
    m4 = synth.make_model(N_STATES, synth.CONFIG4_SYMBOLS, synth.CONFIG4_GAUSSIAN, seed=0)
    seqs = [synth.sample_obs(m4, per_seq, seed=300 + i) for i in range(n_seq)]
    t0 = time.perf_counter()
    oracle.estep(seqs, m4.log_probs, m4.log_startprob, m4.log_transmat, 1.0, None)
    dt = time.perf_counter() - t0
    return {"value": float(n_seq * per_seq) / dt, "unit": "positions/s per EM iteration", "cores": 1, "kind": "port",
            "sample": "%d sequences x %d positions, E-step statistics, 1 thread, %.1f s" % (n_seq, per_seq, dt)}


def time_eval(hm, hb, torch, steps=1, **kw):
    hm.eval(hb, **kw)                        # warm-up (allocates result buffers / workspaces)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(steps):
        time_eval.last = hm.eval(hb, **kw)
    return (time.perf_counter() - t1) / steps


def verify_one(model, hb, obs, offs, res, ratios=None, max_len=260_000, n_threads=2):
    """Oracle check of ONE interval of an `extra` workload (the shortest; skipped when longer than max_len): the results
    of the last evaluation against the oracle's decode / score_samples flow (decode: ratios on the transitions only,
    score_samples: none -- basehmm.py:327-329, 261-273).  Returns a dict for the extra's record."""
    from oracle import oracle
    lens = np.diff(offs)
    i = int(np.argmin(lens))
    if lens[i] > max_len:
        return {"verified": None, "note": "shortest interval %d > %d positions: not checked here" % (lens[i], max_len)}
    a, b = int(offs[i]), int(offs[i + 1])
    sub = obs[a:b].cpu().numpy()
    r = None if ratios is None else ratios[a:b].cpu().numpy()
    t0 = time.perf_counter()
    ok, worst = True, None
    if res.get("viterbi_logprob") is not None:
        vlp, path = oracle.decode(sub, model.log_probs, model.log_startprob, model.log_transmat, 1.0, r)
        ok &= bool(np.array_equal(hb.paths(a, b), path)) and bool(res["viterbi_logprob"][i] == vlp)
    if res.get("forward_logprob") is not None:
        flp, post = oracle.score_samples(sub, model.log_probs, model.log_startprob, model.log_transmat, 1.0)
        got = hb.posteriors(model.n_states, a, b)
        worst = float(np.max(np.abs(got - post) / post))
        ok &= worst <= 1e-6 and abs(res["forward_logprob"][i] - flp) <= 1e-6 * abs(flp)
    return {"verified": bool(ok), "verified_interval": int(lens[i]), "posterior_max_rel_err": worst,
            "verify_s": round(time.perf_counter() - t0, 2)}


def run_eval(args, rank, world, local_rank):
    import torch
    from tehmm_amd import _lib, synth
    from tehmm_amd.engine import HipBatch, HipModel

    torch.cuda.set_device(local_rank)
    _lib.check(_lib.load().tehmm_set_device(local_rank), "tehmm_set_device")
    device = torch.device("cuda", local_rank)
    use_dist = world > 1 or "RANK" in os.environ      # torchrun (even with one rank) -> RCCL path
    if use_dist:
        import torch.distributed as dist
        init_dist(dist, device)

    mb = 100.0 if args.mb is None else args.mb
    model = synth.make_model(N_STATES, synth.CONFIG2_SYMBOLS, synth.CONFIG2_GAUSSIAN, seed=0)
    strong = args.scaling == "strong"
    if strong:
        # ONE whole-genome interval list, identical on every rank; this rank evaluates its LPT shard
        from tehmm_amd import dist as tdist
        all_lens = genome_intervals(args.min_kb, args.max_kb)
        shard = tdist.lpt_shard(all_lens, world)[rank]
        lens = all_lens[shard]
        job_total = int(all_lens.sum())
    else:
        lens = synth.interval_lengths(int(mb * 1e6), args.min_kb * 1000, args.max_kb * 1000, seed=1000 + rank)
        job_total = int(mb * 1e6) * world
    total = int(lens.sum())
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    obs = gen_obs_torch(model, lens, seed=17 + rank, device=device)
    torch.cuda.synchronize()

    def mk_model(mdl):
        return HipModel(mdl.log_transmat, mdl.log_startprob, mdl.log_probs,
                        symbols_per_track=mdl.symbols_per_track)
    hm = mk_model(model)
    hb = HipBatch(obs.data_ptr(), offs, device_ptrs=True, K=model.n_tracks)

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        hm.eval(hb, viterbi=True, posterior=True)
    kt = {}
    res = None
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        hb.reset_cache()                          # every timed step is a first evaluation of its batch
        res = hm.eval(hb, viterbi=True, posterior=True)
        for name, ms in hb.timing().items():      # HIP events on the library's own streams
            if not name.startswith("count:"):
                kt.setdefault(name, []).append(ms)
    barrier()
    dt = time.perf_counter() - t0
    if use_dist:
        tt = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    if rank == 0 and args.dump_outputs:
        dump_eval(args.dump_outputs, hb, res, model.n_states)
    if use_dist and args.full:
        # the "trivial gather" of the per-interval scores (north_star): exercised once, outside the timing
        from tehmm_amd import dist as tdist
        if strong:
            tdist.gather_interval_scalars(shard, res["viterbi_logprob"], len(all_lens))
        else:
            rank_lens = [None] * world
            dist.all_gather_object(rank_lens, [int(x) for x in lens])
            flat = [x for r in rank_lens for x in r]
            first = sum(len(r) for r in rank_lens[:rank])
            tdist.gather_interval_scalars(np.arange(first, first + len(lens)), res["viterbi_logprob"], len(flat))
    verdict = None
    if rank == 0 and args.full and not args.no_verify:
        verdict = verify_intervals(model, hb, obs, offs, res)

    if rank == 0:
        K, N = model.n_tracks, model.n_states
        pos_per_step = float(job_total)
        value = pos_per_step * args.steps / dt
        step_s = dt / args.steps
        kavg = {k: float(np.mean(v)) for k, v in kt.items()}
        dom = max(kavg, key=kavg.get)
        # ALGORITHMIC bytes per position of Viterbi + full posterior = K (obs in) + 8 (int64
        # path out) + 8 N (posterior row out); roofline.achieved = that x the positions one step (one
        # tehmm_eval_batch launch sequence) processes / the step's duration.
        alg_pos = K + 8 + 8 * N
        achieved = alg_pos * float(total) / step_s / 1e9        # this rank's GPU: its positions / the step's duration
        # per-stage view (stage durations are HIP events on the streams the kernels ran on): algorithmic
        # bytes each stage is responsible for, fp64 operations, measured HBM traffic (rocprofv3 --pmc)
        alg = {"viterbi": 8, "viterbi_speculate": K, "traceback": 8, "emission_rows": K,
               "forward_backward_speculate": K, "forward_backward": K, "forward": K,
               "posterior_combine": 8 * N, "backward_posterior": K + 8 * N, "forward_pass": K,
               "backward_posterior_pass": K + 8 * N}
        flop = {"viterbi_speculate": 2 * 2 * N * N, "viterbi": 2 * N * N, "forward_backward_speculate": 2 * 2 * N * N,
                "forward_backward": 2 * 2 * N * N, "forward": 2 * N * N, "backward_posterior": 2 * N * N,
                "forward_pass": 2 * N * N, "backward_posterior_pass": 2 * N * N}
        traffic = None
        stage_hbm = None
        tpath = next((p for p in (os.path.join(ROOT, "profiles", "r04_traffic.json"),
                                  os.path.join(ROOT, "profiles", "r03_traffic.json"),
                                  os.path.join(ROOT, "profiles", "r02_traffic.json"),
                                  os.path.join(ROOT, "profiles", "r01_traffic.json")) if os.path.exists(p)), None)
        if tpath:     # HBM bytes per position measured with rocprofv3 --pmc (see file)
            tjson = json.load(open(tpath))
            tj = tjson.get("hbm_bytes_per_position", {})
            if "total" in tj:
                traffic = tj["total"] * float(total)
            stage_hbm = {k: tj[k] * float(total) / (kavg[k] * 1e-3) / 1e9 for k in kavg if k in tj}
        out = {
            "metric": "genome positions/sec (Viterbi+posterior), 35 states x 10 tracks",
            "value": value, "unit": "positions/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": step_s * 1e3,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": "teHmmEval Viterbi+posterior, 35 states, 10 tracks (8 multinomial "
                                   "+ 2 gaussian/250 bins), %s in intervals of %d-%d kb (config-3 geometry), "
                                   "obs resident in HBM, every step a first evaluation (index records rebuilt)"
                                   % ("ONE %.0f Mb whole-genome interval list (9 alyrata scaffolds, %d intervals) "
                                      "LPT-sharded over the GPUs" % (job_total / 1e6, len(all_lens)) if strong
                                      else "%.0f Mb per GPU in %d intervals" % (mb, len(lens)),
                                      args.min_kb, args.max_kb),
                       "arithmetic": "f64 arithmetic throughout; alpha' rows kept as f32 between the forward and "
                                     "backward passes (posteriors agree with the reference to ~1e-7, bar 1e-6)",
                       "positions_per_gpu": total, "intervals_per_gpu": int(len(lens)),
                       "parallelism": "intervals sharded over %d GPU(s), no collective" % world},
            "roofline": {"bound": "hbm", "kernel": "tehmm_eval_batch: Viterbi + posterior over the batch (SURVEY 8d)",
                         "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic,
                         "alg_bytes_per_position": alg_pos,
                         "traffic_source": os.path.basename(tpath) if tpath else None,
                         "dominant_stage": {"kernel": dom, "ms": kavg[dom],
                                            "alg_bytes_per_position": alg.get(dom),
                                            "achieved": alg.get(dom, 0) * float(total) / (kavg[dom] * 1e-3) / 1e9},
                         "stage_hbm_traffic_GBps": stage_hbm,
                         # what binds next to HBM: fp64 vector issue (78.6 TFLOP/s peak on MI355X)
                         "valu_f64": {"achieved": (2 * 3 * N * N) * float(total) / step_s / 1e12,
                                      "peak": F64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                                      "frac": (2 * 3 * N * N) * float(total) / step_s / 1e12 / F64_VALU_PEAK_TFLOPS,
                                      "stage": {k: flop[k] * float(total) / (kavg[k] * 1e-3) / 1e12
                                                for k in kavg if k in flop}}},
            "kernel_ms": kavg,
        }
        if verdict is not None:
            out.update(verdict)
        if world == 1 and args.full and not args.no_extra:
            out["extra"] = extras(args, model, hm, hb, obs, offs, lens, device, torch, mk_model)
        if world == 1 and args.full and not args.no_cpu_baseline:
            nthr = max(1, min(16, os.cpu_count() or 1))
            cb = cpu_baseline(model, nthr, args.cpu_sample_kb * 1000, 4 * nthr)
            cb["one_core"] = cpu_baseline(model, 1, args.cpu_sample_kb * 1000, 2)
            cb["gpu_over_cpu_all_cores"] = value / cb["value"]
            out["cpu_baseline"] = cb
        print(json.dumps(out))
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


def extras(args, model, hm, hb, obs, offs, lens, device, torch, mk_model):
    """Untimed measurements next to the headline: the same library on the other shapes BASELINE.json and
    SURVEY 8(d) name, so that the speculation's weak spots and the PCIe-inclusive rate are on the record."""
    from tehmm_amd import synth
    from tehmm_amd.engine import HipBatch
    ex = {}
    K = model.n_tracks
    total = int(offs[-1])

    def rate(n, s, **kw):
        d = dict(value=float(n) / s, unit="positions/s", ms=s * 1e3)
        d.update(kw)
        return d

    # (1) end to end over PCIe on a 20 Mb slice: H2D of the observations + evaluation + D2H of the paths and
    #     (a) the full posteriors, (b) the masked posterior sums teHmmEval actually writes
    n_e2e = min(total, 20_000_000)
    cut = int(np.searchsorted(offs, n_e2e, side="right")) - 1
    if cut >= 1:
        o2 = offs[:cut + 1]
        n2 = int(o2[-1])
        host_obs = obs[:n2].cpu().numpy()
        mask = (np.arange(model.n_states) % 3 == 0).astype(np.float64)
        for tag in ("full_posteriors_first_call", "full_posteriors", "masked_sum"):
            # (the host is shared: the steady-state figures are the best of three fresh batches, all three on the record)
            times, parts = [], []
            for _rep in range(1 if tag.endswith("first_call") else 3):
                t1 = time.perf_counter()
                hb2 = HipBatch(host_obs, o2)
                t2 = time.perf_counter()
                hm.eval(hb2, viterbi=True, posterior=True)
                t3 = time.perf_counter()
                p = hb2.paths()
                q = hb2.posteriors() if tag.startswith("full_posteriors") else hb2.posterior_masksum(mask)
                t4 = time.perf_counter()
                times.append(t4 - t1)
                parts.append([round((t2 - t1) * 1e3, 1), round((t3 - t2) * 1e3, 1), round((t4 - t3) * 1e3, 1)])
                nbytes = int(p.nbytes + q.nbytes)
                hb2.close()
                del p, q
            ex["end_to_end_pcie_" + tag] = rate(n2, min(times), positions=n2, bytes_d2h=nbytes,
                                                ms_all=[round(t * 1e3, 1) for t in times],
                                                ms_create_eval_fetch=parts[int(np.argmin(times))],
                                                ms_create_eval_fetch_all=parts,
                                                note="fresh batch: H2D of the observations, workspace allocation, "
                                                     "evaluation, D2H into pinned host memory from the library's pool"
                                                     + (" (first call: the pool is empty, pinning included)"
                                                        if tag.endswith("first_call") else "; best of three"))
        # the same job with the transfer hidden behind the evaluation (engine.eval_stream: interval groups, a worker
        # thread evaluates group g + 1 while group g's results cross PCIe)
        from tehmm_amd.engine import eval_stream
        times = []
        for _rep in range(3):
            t1 = time.perf_counter()
            ps, qs, _, _ = eval_stream(hm, host_obs, o2, group_rows=4_000_000)
            times.append(time.perf_counter() - t1)
            del ps, qs
        ex["end_to_end_pcie_full_posteriors_streamed"] = rate(
            n2, min(times), positions=n2, ms_all=[round(t * 1e3, 1) for t in times],
            note="as end_to_end_pcie_full_posteriors, in groups of ~4 Mb: H2D + evaluation of group g + 1 on a worker "
                 "thread while group g's paths and posterior rows are fetched; best of three")
        del host_obs
    hb.close()
    torch.cuda.empty_cache()

    # (2) BASELINE configs[1]: the same model on ONE 10 Mb interval -- a single dependent chain
    one = np.asarray([10_000_000], dtype=np.int64)
    obs1 = gen_obs_torch(model, one, seed=99, device=device)
    hb1 = HipBatch(obs1.data_ptr(), np.asarray([0, one[0]], dtype=np.int64), device_ptrs=True, K=K)
    d1 = time_eval(hm, hb1, torch, viterbi=True, posterior=True)
    ex["config2_single_10Mb_interval"] = rate(one[0], d1, kernel_ms=hb1.timing(),
                                              note="checked bit for bit against the oracle at this size by "
                                                   "tests/test_gpu_r2.py::test_config2_full_size_vs_oracle (100 s of CPU)")
    d1v = time_eval(hm, hb1, torch, viterbi=True, posterior=False)
    ex["config2_single_10Mb_interval_viterbi_only"] = rate(one[0], d1v)
    hb1.close()
    del obs1

    # (3) model variants on the bench geometry (30 Mb): sparse transitions (p = 0.5 zeros -> -1e100), sticky
    #     chain (self-transition 0.995, like trained TE models), decode with segment ratios (--segLen 100)
    sub = int(np.searchsorted(offs, 30_000_000, side="right")) - 1
    sub = max(sub, 1)
    o3 = offs[:sub + 1]
    n3 = int(o3[-1])
    for tag, mdl in (("sparse_p0.5", synth.make_model(N_STATES, synth.CONFIG2_SYMBOLS, synth.CONFIG2_GAUSSIAN,
                                                      seed=0, sparse=0.5)),
                     ("sticky_0.995", synth.make_model(N_STATES, synth.CONFIG2_SYMBOLS, synth.CONFIG2_GAUSSIAN,
                                                       seed=0, stay=0.995))):
        ob = gen_obs_torch(mdl, lens[:sub], seed=31, device=device)
        hmv = mk_model(mdl)
        hbv = HipBatch(ob.data_ptr(), o3, device_ptrs=True, K=K)
        d = time_eval(hmv, hbv, torch, viterbi=True, posterior=True)
        ex["model_" + tag] = rate(n3, d, positions=n3, kernel_ms=hbv.timing(),
                                  **({} if args.no_verify else verify_one(mdl, hbv, ob, o3, time_eval.last)))
        hbv.close()
        hmv.close()
        del ob
    # (3a) BASELINE configs[2] at the alyrata track-XML shape: K = 32 (15 multinomial + 14 gaussian / 250 bins + 3 binary)
    mdl = synth.make_model(N_STATES, synth.CONFIG3B_SYMBOLS, synth.CONFIG3B_GAUSSIAN, seed=0)
    ob = gen_obs_torch(mdl, lens[:sub], seed=34, device=device)
    hmv = mk_model(mdl)
    hbv = HipBatch(ob.data_ptr(), o3, device_ptrs=True, K=mdl.n_tracks)
    d = time_eval(hmv, hbv, torch, viterbi=True, posterior=True)
    ex["config3b_32_tracks"] = rate(n3, d, positions=n3, kernel_ms=hbv.timing())
    hbv.close()
    hmv.close()
    del ob
    # (3b) state counts between the 36 the VALU lane kernels were first built for and the 64-lane limit
    for ns in (50, 60):
        mdl = synth.make_model(ns, synth.CONFIG2_SYMBOLS, synth.CONFIG2_GAUSSIAN, seed=0)
        ob = gen_obs_torch(mdl, lens[:sub], seed=33, device=device)
        hmv = mk_model(mdl)
        hbv = HipBatch(ob.data_ptr(), o3, device_ptrs=True, K=K)
        d = time_eval(hmv, hbv, torch, viterbi=True, posterior=True)
        ex["states_%d" % ns] = rate(n3, d, positions=n3, kernel_ms=hbv.timing())
        hbv.close()
        hmv.close()
        del ob
    ob = gen_obs_torch(model, lens[:sub], seed=32, device=device)
    g = torch.Generator(device=device)
    g.manual_seed(5)
    seglen = torch.clamp(1 + torch.floor(torch.log1p(-torch.rand(n3, generator=g, device=device, dtype=torch.float64))
                                         / np.log(1 - 1 / 20.0)), max=100.0)
    ratios = (seglen / 100.0).contiguous()
    hbr = HipBatch(ob.data_ptr(), o3, ratios=ratios.data_ptr(), device_ptrs=True, K=K)
    d = time_eval(hm, hbr, torch, viterbi=True, posterior=True, use_ratios=True)
    ex["decode_with_segment_ratios"] = rate(n3, d, positions=n3, kernel_ms=hbr.timing(),
                                            **({} if args.no_verify else verify_one(model, hbr, ob, o3, time_eval.last, ratios)))
    hbr.close()
    del ob, ratios, seglen

    # (4) BASELINE configs[4] shape: 100 states, 10 tracks, segmented (ratios), 2 Mb in 20 intervals
    m5 = synth.make_model(100, synth.CONFIG2_SYMBOLS, synth.CONFIG2_GAUSSIAN, seed=0)
    l5 = np.full(20, 100_000, dtype=np.int64)
    o5 = np.concatenate([[0], np.cumsum(l5)]).astype(np.int64)
    ob = gen_obs_torch(m5, l5, seed=33, device=device)
    # segment ratios on both sides of 1 (lengths ~ 1 + Geometric(1 / 20) capped at 100, effective length 20)
    g5 = torch.Generator(device=device)
    g5.manual_seed(6)
    sl5 = torch.clamp(1 + torch.floor(torch.log1p(-torch.rand(int(o5[-1]), generator=g5, device=device, dtype=torch.float64))
                                      / np.log(1 - 1 / 20.0)), max=100.0)
    r5 = (sl5 / 20.0).contiguous()
    hm5 = mk_model(m5)
    hb5 = HipBatch(ob.data_ptr(), o5, ratios=r5.data_ptr(), device_ptrs=True, K=K)
    d = time_eval(hm5, hb5, torch, viterbi=True, posterior=True, use_ratios=True)
    ex["config5_100_states_segmented"] = rate(int(o5[-1]), d, positions=int(o5[-1]), kernel_ms=hb5.timing())
    if not args.no_verify:        # one 100 kb interval of this workload against the oracle (N = 100, ratios)
        v5 = verify_one(m5, hb5, ob, o5, time_eval.last, r5, n_threads=2)
        ex["config5_100_states_segmented"].update(v5)
        ex["config5_verified"] = v5["verified"]
    # the two halves: the posterior runs item-parallel on the matrix cores, the exact Viterbi with segment ratios
    # chunk-parallel with an exact chain that follows the quantised pass (tehmm_wide.hip.h)
    d = time_eval(hm5, hb5, torch, viterbi=False, posterior=True, use_ratios=True)
    ex["config5_100_states_posterior_only"] = rate(int(o5[-1]), d, positions=int(o5[-1]), kernel_ms=hb5.timing())
    d = time_eval(hm5, hb5, torch, viterbi=True, posterior=False, use_ratios=True)
    ex["config5_100_states_viterbi_only"] = rate(int(o5[-1]), d, positions=int(o5[-1]), kernel_ms=hb5.timing())
    hb5.close()
    hm5.close()
    del ob, r5

    # (5) BASELINE configs[3] shape on one GPU: Baum-Welch iterations, 35 states, 12 tracks, 100 kb chunks
    ex["config4_em_iteration"] = em_iterations(50.0, 2, device, torch, None, verify=not args.no_verify)
    # (5a) the E-step where the fused passes do not apply (review item 4): segment ratios at 35 states (5 Mb) and the
    #      100-state model of configs[4] with ratios (2 Mb), on the item-parallel passes of tehmm_wide_estep.hip.h
    ex["estep_with_segment_ratios_35_states"] = estep_other_routes("ratios", torch, device, verify=not args.no_verify)
    ex["estep_100_states_segmented"] = estep_other_routes("wide", torch, device, verify=not args.no_verify)
    return ex


def verify_estep(start, ob, o4, n_chunks=4):
    """The fused E-step of the FIRST n_chunks training chunks against the oracle's per-sequence E-step (hmm.py:545-574)
    from the same start model: statistics within 1e-6 (observed error on the record)."""
    from oracle import oracle
    from tehmm_amd.engine import HipBatch, HipModel
    n_chunks = min(n_chunks, len(o4) - 1)
    sub = ob[:int(o4[n_chunks])].cpu().numpy()
    so = np.asarray(o4[:n_chunks + 1], dtype=np.int64)
    K, N, S = start.log_probs.shape
    hm = HipModel(start.log_transmat, start.log_startprob, start.log_probs, symbols_per_track=start.symbols_per_track)
    hb = HipBatch(sub, so)
    st0, tr, ob_st = np.zeros(N), np.zeros((N, N)), np.zeros((K, N, S))
    lp = hm.estep(hb, False, st0, tr, ob_st)
    hb.close()
    hm.close()
    t0 = time.perf_counter()
    ref = oracle.estep([sub[int(so[i]):int(so[i + 1])] for i in range(n_chunks)], start.log_probs, start.log_startprob,
                       start.log_transmat, 1.0, None)

    def rel(a, b, floor):
        return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))
    worst = max(rel(st0, ref["start"], 1e-12), rel(tr, ref["trans"], 1e-6), rel(ob_st, ref["obs"], 1e-6))
    ok = worst <= 1e-6 and abs(lp - ref["logprob"]) <= 1e-9 * abs(ref["logprob"])
    return {"verified": bool(ok), "verified_chunks": int(n_chunks), "statistics_max_rel_err": worst,
            "verify_s": round(time.perf_counter() - t0, 2)}


def estep_other_routes(which, torch, device, verify=True):
    """One Baum-Welch E-step where the fused passes of tehmm_estep.hip.h do not apply -- segment ratios, 64..128 states --
    on the item-parallel passes (tehmm_wide_estep.hip.h), with the route of rounds 1-3 timed beside it
    (`before`: sequential chains for ratios below 64 states, BaseHMM._do_estep over the array-level entry points at
    100 states) and the first chunks checked against the oracle."""
    from tehmm_amd import synth
    from tehmm_amd.engine import HipBatch, HipModel
    if which == "ratios":
        mdl = synth.make_model(N_STATES, synth.CONFIG4_SYMBOLS, synth.CONFIG4_GAUSSIAN, seed=7)
        lens = np.full(50, 100_000, dtype=np.int64)
    else:
        mdl = synth.make_model(100, synth.CONFIG2_SYMBOLS, synth.CONFIG2_GAUSSIAN, seed=0)
        lens = np.full(20, 100_000, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(offs[-1])
    ob = gen_obs_torch(mdl, lens, seed=41, device=device)
    g = torch.Generator(device=device)
    g.manual_seed(8)
    sl = torch.clamp(1 + torch.floor(torch.log1p(-torch.rand(total, generator=g, device=device, dtype=torch.float64))
                                     / np.log(1 - 1 / 20.0)), max=100.0)
    r = (sl / 20.0).contiguous()
    K, N, S = mdl.log_probs.shape
    hm = HipModel(mdl.log_transmat, mdl.log_startprob, mdl.log_probs, symbols_per_track=mdl.symbols_per_track)

    def one(hb, use_r, reps=3):
        st0, tr, ost = np.zeros(N), np.zeros((N, N)), np.zeros((K, N, S))
        lp = hm.estep(hb, use_r, st0, tr, ost)
        best = None
        for _ in range(reps):
            st0[:], tr[:], ost[:] = 0.0, 0.0, 0.0
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            lp = hm.estep(hb, use_r, st0, tr, ost)
            d = time.perf_counter() - t1
            best = d if best is None else min(best, d)
        return best, lp, hb.timing(), (st0, tr, ost)

    hb = HipBatch(ob.data_ptr(), offs, ratios=r.data_ptr(), device_ptrs=True, K=K)
    d, lp, tm, got = one(hb, True)
    out = {"value": total / d, "unit": "positions/s per E-step", "ms": d * 1e3, "positions": total, "states": N,
           "segment_ratios": True, "logprob": lp, "kernel_ms": tm,
           "route": "item-parallel passes k_wide_fwd / k_wide_bwd<ESTEP> + k_wide_estep_xi / k_wide_estep_rows",
           "arithmetic": "f64 recurrences and sums; alpha', gamma, wz rows kept as f32"}
    if which == "ratios":
        os.environ["TEHMM_ESTEP_WIDE"] = "0"
        try:
            d0, lp0, _, _ = one(hb, True, reps=1)
        finally:
            del os.environ["TEHMM_ESTEP_WIDE"]
        out["before"] = {"ms": d0 * 1e3, "value": total / d0, "logprob": lp0,
                         "route": "sequential chains per interval (k_fb_coop<TRATIO>) + k_estep_accum"}
    else:
        d1, lp1, tm1, _ = one(hb, False)
        out["without_ratios"] = {"ms": d1 * 1e3, "value": total / d1, "logprob": lp1, "kernel_ms": tm1}
    hb.close()
    if verify:
        from oracle import oracle
        nv = 2 if which == "ratios" else 1
        nrow = 100_000 if which == "ratios" else 30_000          # (the oracle's xi pass is N^2 exponentials per position)
        sub = np.concatenate([ob[int(offs[i]):int(offs[i]) + nrow].cpu().numpy() for i in range(nv)])
        rsub = np.concatenate([r[int(offs[i]):int(offs[i]) + nrow].cpu().numpy() for i in range(nv)])
        so = np.arange(nv + 1, dtype=np.int64) * nrow
        hbv = HipBatch(sub, so, rsub)
        st0, tr, ost = np.zeros(N), np.zeros((N, N)), np.zeros((K, N, S))
        lpv = hm.estep(hbv, True, st0, tr, ost)
        ran = "estep_emission_rows" in hbv.timing()
        hbv.close()
        t0 = time.perf_counter()
        ref = oracle.estep([sub[int(so[i]):int(so[i + 1])] for i in range(nv)], mdl.log_probs, mdl.log_startprob,
                           mdl.log_transmat, 1.0, [rsub[int(so[i]):int(so[i + 1])] for i in range(nv)])

        def rel(a, b, floor):
            return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))
        worst = max(rel(st0, ref["start"], 1e-12), rel(tr, ref["trans"], 1e-6), rel(ost, ref["obs"], 1e-6))
        out.update({"verified": bool(ran and worst <= 1e-6 and abs(lpv - ref["logprob"]) <= 1e-9 * abs(ref["logprob"])),
                    "verified_positions": int(so[-1]), "statistics_max_rel_err": worst,
                    "verify_s": round(time.perf_counter() - t0, 2)})
    if which != "ratios":
        # what rounds 1-3 ran at this size: the reference's per-sequence loop over the array-level entry points
        from tehmm_amd.emission import IndependentMultinomialEmissionModel
        from tehmm_amd.hmm import MultitrackHmm
        em = IndependentMultinomialEmissionModel(N, list(mdl.symbols_per_track))
        em.logProbs = mdl.log_probs.copy()
        h = MultitrackHmm(em)
        h.transmat_ = np.exp(mdl.log_transmat)
        h.startprob_ = np.exp(mdl.log_startprob)
        seqs = [ob[int(offs[0]):int(offs[0]) + 20_000].cpu().numpy()]        # (one 20 kb sequence, one call: ~2 s)
        os.environ["TEHMM_ESTEP_WIDE"] = "0"
        try:
            t1 = time.perf_counter()
            h._do_estep(seqs, h._initialize_sufficient_statistics())
            d0 = time.perf_counter() - t1
        finally:
            del os.environ["TEHMM_ESTEP_WIDE"]
        out["before"] = {"ms": d0 * 1e3, "value": 20_000.0 / d0, "positions": 20_000, "segment_ratios": False,
                         "route": "BaseHMM._do_estep over the array-level entry points"}
    hm.close()
    del ob, r
    return out


def em_iterations(mb, n_iter, device, torch, dist, verify=False, warmup=1, dump_dir=None):
    """Baum-Welch iterations on the config-4 shape: per iteration one fused E-step over the rank's 100 kb
    chunks (statistics left on the device), ONE all-reduce of the flat statistics buffer, device M-step.
    dump_dir: --dump-outputs of the last iteration (float64): the statistics the M-step consumed and the model it
    made (log transition matrix, log start probabilities, log emission tables)."""
    from tehmm_amd import synth
    from tehmm_amd.engine import DeviceStats, HipBatch, HipModel
    m4 = synth.make_model(N_STATES, synth.CONFIG4_SYMBOLS, synth.CONFIG4_GAUSSIAN, seed=0)
    n_chunks = max(1, int(mb * 1e6) // 100_000)
    l4 = np.full(n_chunks, 100_000, dtype=np.int64)
    o4 = np.concatenate([[0], np.cumsum(l4)]).astype(np.int64)
    ob = gen_obs_torch(m4, l4, seed=41, device=device)
    # start EM from a perturbed model so that the iterations do real work
    start = synth.make_model(N_STATES, synth.CONFIG4_SYMBOLS, synth.CONFIG4_GAUSSIAN, seed=7)
    verdict = verify_estep(start, ob, o4) if verify else {}
    hm4 = HipModel(start.log_transmat, start.log_startprob, start.log_probs, symbols_per_track=start.symbols_per_track)
    hb4 = HipBatch(ob.data_ptr(), o4, device_ptrs=True, K=m4.n_tracks)
    st = DeviceStats(hm4)
    lps = []

    def one_iteration():
        st.zero()
        hm4.estep_device(hb4, False, st)
        if dist is not None:
            dist.all_reduce(st.tensor, op=dist.ReduceOp.SUM)
        lps.append(st.head()[0])
        hm4.mstep(st, False, True, True, 1.0, 1.0, 0.0, None)
    for _ in range(warmup):
        one_iteration()                     # warm-up (workspace allocation)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t1 = time.perf_counter()
    for _ in range(n_iter):
        one_iteration()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    d = (time.perf_counter() - t1) / n_iter
    n = int(o4[-1])
    stage_ms = {k: v for k, v in hb4.timing().items() if not k.startswith("count:")}
    if dump_dir:
        os.makedirs(dump_dir, exist_ok=True)
        lt, pi, lp = hm4.get_params(start.log_probs)
        for name, a in (("statistics", st.to_host()), ("log_transmat", lt), ("log_startprob", pi), ("log_probs", lp)):
            np.save(os.path.join(dump_dir, name + ".npy"), np.asarray(a, dtype=np.float64))
    hb4.close()
    st.close()
    hm4.close()
    del ob
    out = {"value": float(n) / d, "unit": "positions/s per EM iteration", "ms_per_iteration": d * 1e3,
           "positions": n, "chunks": int(n_chunks), "logprob_per_iteration": lps, "estep_stage_ms": stage_ms,
           "alg_bytes_per_position": m4.n_tracks, "hbm_GBps_algorithmic": m4.n_tracks * float(n) / d / 1e9}
    out.update(verdict)
    return out


def estep_traffic(positions):
    """Measured HBM bytes of one EM iteration (per-position figure of profiles/r04_estep_traffic.json x positions)."""
    p = os.path.join(ROOT, "profiles", "r04_estep_traffic.json")
    if not os.path.exists(p):
        return None
    tj = json.load(open(p)).get("hbm_bytes_per_position", {})
    return tj["total"] * float(positions) if "total" in tj else None


def run_estep(args, rank, world, local_rank):
    import torch
    from tehmm_amd import _lib
    torch.cuda.set_device(local_rank)
    _lib.check(_lib.load().tehmm_set_device(local_rank), "tehmm_set_device")
    device = torch.device("cuda", local_rank)
    import torch.distributed as dist
    use_dist = world > 1 or "RANK" in os.environ
    if use_dist:
        init_dist(dist, device)
    mb = 200.0 if args.mb is None else args.mb
    r = em_iterations(mb, args.steps, device, torch, dist if use_dist else None,
                      verify=(rank == 0 and args.full and not args.no_verify), warmup=args.warmup,
                      dump_dir=args.dump_outputs if rank == 0 else None)
    if rank == 0:
        d = r["ms_per_iteration"] * 1e-3
        value = r["positions"] * world / d
        out = {"metric": "genome positions/sec (Baum-Welch EM iteration), 35 states x 12 tracks",
               "value": value, "unit": "positions/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": d * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "f64", "data": "synthetic",
               "config": {"workload": "teHmmTrain E-step + all-reduce + M-step, 35 states, 12 tracks (10 multinomial "
                                      "+ 2 gaussian), %.0f Mb per GPU in 100 kb chunks (config-4 geometry)" % mb,
                          "arithmetic": "f64 arithmetic in the passes and all sums; the alpha', gamma and wz rows between "
                                        "the passes and the reductions are f32, the one-hot histogram products three "
                                        "exact bf16 pieces per f32 gamma (statistics agree with the reference to ~1e-7, "
                                        "bar 1e-6); sums reproducible run to run (per-writer partials, ordered fold)",
                          "positions_per_gpu": r["positions"], "intervals_per_gpu": r["chunks"],
                          "parallelism": "chunks sharded over %d GPU(s), one all-reduce of %s per iteration"
                                         % (world, "the packed statistics")},
               "roofline": {"bound": "hbm", "kernel": "tehmm_estep_batch_device (SURVEY 8d: K bytes / position)",
                            "achieved": r["alg_bytes_per_position"] * r["positions"] / d / 1e9,
                            "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                            "frac": r["alg_bytes_per_position"] * r["positions"] / d / 1e9 / HBM_PEAK_GBPS,
                            "traffic": estep_traffic(r["positions"]),
                            "traffic_source": "profiles/r04_estep_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE)"
                                              if estep_traffic(r["positions"]) is not None else None,
                            # what really binds: fp64 matrix + vector issue; forward + backward + xi = 3 x 2 N^2 flop
                            "f64": {"achieved": 6.0 * N_STATES * N_STATES * r["positions"] / d / 1e12,
                                    "peak": F64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s"}},
               "estep_stage_ms": r["estep_stage_ms"],
               "logprob_per_iteration": r["logprob_per_iteration"]}
        for k in ("verified", "verified_chunks", "statistics_max_rel_err", "verify_s"):
            if k in r:
                out[k] = r[k]
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_estep()
        print(json.dumps(out))
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


def main():
    args = parse_args()
    in_launcher = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    if args.gpus > 1 and not in_launcher:
        sys.exit(launch_ranks(args))         # before anything here has touched the GPU
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE is %d" % (args.gpus, world))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    if args.mode == "estep":
        run_estep(args, rank, world, local_rank)
    else:
        run_eval(args, rank, world, local_rank)


if __name__ == "__main__":
    main()
