#!/usr/bin/env python
"""Headline benchmark: PC-sampler throughput of NCSN++ cont. VE-SDE on CIFAR-10 (BASELINE configs[1]).

    python bench.py --gpus N --steps K --warmup W          (N > 1 without a launcher: re-executes itself under the line below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

Workload (per GPU): configs/ve/cifar10_ncsnpp_continuous, batch 256, reverse_diffusion predictor +
Langevin corrector, snr 0.16, N=1000 discretisation steps.  One "step" = ONE full PC iteration on
the batch = 2 U-Net evaluations + rocRAND noise + norms + Langevin update + predictor update, replayed
as one hipGraph.  All N iterations are identical work, so images/sec = n_gpus * batch / (1000 * t_step);
the timed region holds exactly K iterations with the state resident in HBM.  Sampling shards by
replication (one independent sampler per GPU, no collectives) -> "scaling": "weak".
Weights: deterministic random init of the full architecture (every tensor re-randomised);
data: synthetic prior noise.  fp32 end to end (dtype "f32"), as the reference.

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the JSON line.  With --full the line
also carries (the --no-* options take legs out of a full run)
  roofline     -- the dominant kernel class (the 3x3 convolution launches of one U-Net evaluation, HIP events on the
                  launch stream).  `frac` = EXECUTED matrix FLOP/s over the 157.3 TFLOP/s fp32 MFMA peak: a launch on
                  the Winograd F(2x2,3x3) kernel executes 1/2.25 of its direct-form FLOPs, one on the F(4x4,3x3) kernel
                  1/4, and they are counted at that
                  (this is the matrix-pipe utilisation SQ_VALU_MFMA_BUSY_CYCLES shows in profiles/);
                  `frac_algorithmic` = direct-form FLOP/s over the same peak (can exceed 1).  `by_class` adds the
                  fraction of every other kernel class against ITS roofline: 1x1 GEMMs and attention against the
                  MFMA peak, GroupNorm statistics / FIR resampling / PC-update kernels against 8 TB/s HBM with the
                  algorithmic bytes of the op list;
  cpu_baseline -- the CPU oracle (a torch-CPU port of the reference path, oracle/) timed on this host for a bounded
                  sample (rank 0, N=1 only): K PC iterations at the config batch, and a DSM training step;
  extra        -- compact results of the other BASELINE configs measured in the same run: `ffhq256` (configs[3]),
                  `subvp_ode` (configs[4]); `train` (configs[2]) is a top-level key;
  matrix_*     -- the sampler and the training step in the other matrix mode;
  telemetry    -- clock / power / temperature beside every timed leg.
Every run carries
  rccl_ranks   -- world size confirmed by an actual 1-element all-reduce over RCCL (N > 1).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 64 FLOP/clk/SIMD
PEAK_HBM_TBS = 8.0              # MI355X_MICROARCH.md: HBM3E spec (6.29 TB/s measured float4 copy)
WINOGRAD_FLOP_RATIO = 2.25      # F(2x2,3x3): 16 instead of 36 multiply-adds per 2x2 output tile and (ci, co)
WINOGRAD4_FLOP_RATIO = 4.0      # F(4x4,3x3): 36 instead of 144 per 4x4 output tile and (ci, co)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--sde-steps", type=int, default=1000)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="measure everything besides the headline: roofline and per-class kernel times, the CPU baseline, the DSM training "
                         "step with its exchange legs and replica check, the other matrix mode, the other BASELINE configs and telemetry "
                         "(the --no-* options below take legs out of it).  Without it a run times the headline workload alone")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--cpu-batch", type=int, default=256, help="batch of the CPU-oracle sampler sample (config batch)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="host threads for the CPU baseline (0: min(64, all))")
    ap.add_argument("--cpu-seconds", type=float, default=60.0,
                    help="CPU-work budget per baseline leg (60 s: K=1 PC iteration = 2 U-Net evaluations at batch 256, and 1 + 1 DSM steps at "
                         "batch 128 on this host; --cpu-seconds 200 gives BASELINE.md 3's K=5 and 1 + 3 steps)")
    ap.add_argument("--no-extras", action="store_true", help="skip the compact ffhq256 / subvp_ode measurements")
    ap.add_argument("--prewarm-s", type=float, default=3.0,
                    help="seconds of the same work run (untimed, outside --warmup) right before every timed sampler / training leg, so "
                         "that the timed region sees the clock and power state of sustained load; reported as prewarm_s")
    ap.add_argument("--no-exchange-probe", action="store_true",
                    help="skip the one-rank-RCCL-group leg of the training step (the data-parallel step form on a single GPU)")
    ap.add_argument("--no-telemetry", action="store_true", help="do not sample clocks / power / temperature beside the timed legs")
    ap.add_argument("--dump-ops", type=str, default="")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="after the timed steps, write what the last timed PC iteration computed -- the state x and its mean x_mean, "
                         "(batch, 3, R, R) float32 -- as DIR/<name>.npy (rank 0; at most 64 MB in all, a fixed seeded sample of a larger "
                         "output).  The timed steps start from the same seeded prior sample at the first iteration of the schedule in "
                         "every run, so two builds given the same arguments can be compared output for output.  Sampler workloads only")
    ap.add_argument("--no-train", action="store_true", help="skip the DSM training-step measurement")
    ap.add_argument("--train-only", action="store_true",
                    help="only the DSM training step (the leg that has a collective): what a multi-GPU scaling run needs per N")
    ap.add_argument("--matrix", default=os.environ.get("SSDE_MATRIX", "bf16x6"), choices=["bf16x6", "f32"],
                    help="matrix mode of the headline legs: bf16x6 = the 1x1 / NIN / Linear GEMMs as exact-fp32 products of a 3-way "
                         "bf16 split on the BF16 matrix pipe (fp32 accumulation; no further from fp64 than the fp32 MFMA, "
                         "tests/test_ops_gpu.py), f32 = the exact-fp32 MFMA kernels everywhere.  The other mode is measured beside it")
    ap.add_argument("--no-other-matrix", action="store_true", help="skip the legs in the other matrix mode")
    ap.add_argument("--workload", default="cifar10", choices=["cifar10", "ffhq256", "subvp_ode", "subvp_likelihood"],
                    help="cifar10 = BASELINE configs[1] (the headline line); ffhq256 = configs[3] (NCSN++ 256x256, N=2000, batch "
                         "16/GPU); subvp_ode = configs[4] (DDPM++ sub-VP, probability-flow ODE sampler with RK45; 1 step = 1 solve); "
                         "subvp_likelihood = configs[4]'s likelihood.py solve at rtol = atol = 1e-5")
    ap.add_argument("--likelihood-tol", type=float, default=1e-5,
                    help="rtol = atol of the likelihood solve inside a --full run (1e-5 = the config's own, likelihood.py:40; ~110 s)")
    ap.add_argument("--train-batch", type=int, default=128)
    ap.add_argument("--train-steps", type=int, default=100, help="timed training steps (SURVEY 8d: 100), a fresh batch each")
    ap.add_argument("--train-warmup", type=int, default=20, help="untimed training steps before them (SURVEY 8d: 20)")
    ap.add_argument("--dump-train-ops", type=str, default="")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend for --gpus N > 1: nccl (= RCCL over xGMI, one rank per GPU) or gloo (collectives "
                         "staged through the host; with --share-device it runs the N > 1 code paths on a single GPU)")
    ap.add_argument("--share-device", action="store_true",
                    help="rank r uses GPU r %% (visible GPUs): N ranks on fewer GPUs -- a functional run of the multi-rank branches "
                         "(self-launch, rank census; with --full the bucketed gradient exchange, exposed-exchange leg, parameter broadcast), NOT a "
                         "scaling measurement; needs --dist-backend gloo (RCCL refuses two ranks on one device)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and (args.train_only or args.workload not in ("cifar10", "ffhq256")):
        ap.error("--dump-outputs writes the outputs of the PC sampler: --workload cifar10 or ffhq256, without --train-only")
    if (args.dump_ops or args.dump_train_ops) and not args.full:
        ap.error("--dump-ops and --dump-train-ops write the per-kernel times of the roofline legs: they need --full")
    if not args.full:
        # a plain run: set-up, warm-up, the timed steps of the headline workload, --dump-outputs and the line
        args.no_roofline = args.no_cpu_baseline = args.no_train = args.no_other_matrix = args.no_extras = True
        args.no_exchange_probe = args.no_telemetry = True
    return args


def bench_train(args, cfg, dev, dist, world, rank, sync_all, leg="train"):
    """sec/train-step of the fused DSM step (BASELINE configs[2]): batch 128/GPU, dropout 0.1, Adam + clip + EMA,
    one all-reduce of the flat gradient per step when world > 1."""
    import _util
    from score_sde_pytorch_amd import sde_lib, losses, backward as B, engine as E
    from score_sde_pytorch_amd.models import utils as mutils, ema as ema_mod
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    _util.load_seeded(model, seed=1)
    model = model.to(dev).train()
    sde = sde_lib.VESDE(cfg.model.sigma_min, cfg.model.sigma_max, cfg.model.num_scales)
    opt = losses.get_optimizer(cfg, model.parameters())
    ema = ema_mod.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
    optimize_fn = losses.optimization_manager(cfg)
    step_fn = losses.get_step_fn(sde, train=True, optimize_fn=optimize_fn, reduce_mean=cfg.training.reduce_mean,
                                 continuous=True, likelihood_weighting=cfg.training.likelihood_weighting)
    state = dict(optimizer=opt, model=model, ema=ema, step=0)
    Bt, R = args.train_batch, cfg.data.image_size
    if dist is not None:
        # every replica starts from rank 0's parameters (the reference's DataParallel replicates device 0's module,
        # models/utils.py:93); one broadcast of the flat parameter buffer
        from score_sde_pytorch_amd import parallel
        parallel.broadcast_parameters(model)
    torch.manual_seed(100 + rank)
    pool = [torch.rand(Bt, 3, R, R, device=dev) for _ in range(8)]       # a fresh batch every step (this rank's shard)
    batch = pool[0]
    k = args.train_steps                               # 20 warm-up + 100 timed steps
    w = args.train_warmup
    graph_fallback = None
    try:
        loss = step_fn(state, pool[0])
        sync_all()
    except Exception as exc:                                    # noqa: BLE001
        # (N > 1 only ever ran under the builder's hands as a one-rank RCCL group: if the per-bucket graphs of the exchange step do not
        #  survive a real multi-device group, the same launches issued one by one are the step -- said in the line, not hidden)
        if world == 1 or os.environ.get("SSDE_TRAIN_GRAPH", "1") == "0":
            raise
        graph_fallback = repr(exc)[:300]
        os.environ["SSDE_TRAIN_GRAPH"] = "0"
        loss = step_fn(state, pool[0])
        sync_all()
    for i in range(1, w):
        loss = step_fn(state, pool[i % len(pool)])
    sync_all()

    def _chunk():
        for i in range(10):
            step_fn(state, pool[i % len(pool)])
    warm_s = prewarm(_chunk, sync_all, args.prewarm_s, dev, dist)
    with tele_leg(leg):
        t0 = time.perf_counter()
        for i in range(k):
            loss = step_fn(state, pool[(w + i) % len(pool)])
        sync_all()
        dt = time.perf_counter() - t0
    per_rank_ms = [dt / k * 1e3]
    if dist is not None:
        # every rank's own time goes into the line (a straggler or a fallback transport shows as a spread), the MAX is the step
        ts = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(ts, torch.tensor([dt], device=dev, dtype=torch.float64))
        per_rank_ms = [float(t.item()) / k * 1e3 for t in ts]
        dt = max(float(t.item()) for t in ts)
    sec = dt / k
    fs = step_fn.fused_for(state, batch)
    eng = fs.eng
    exposed_ms = None
    replicas_equal = None
    if dist is not None and args.full:
        # data parallel = same parameters everywhere after every step: compare a checksum and the extremes of the flat
        # parameter buffer across ranks (before the no-exchange leg below, which lets them diverge on purpose)
        flat = eng.flat.data
        sig = torch.stack([flat.double().sum(), flat.double().abs().sum(), flat.max().double(), flat.min().double()])
        lo, hi = sig.clone(), sig.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        replicas_equal = bool((lo == hi).all().item())
        # the same steps without the gradient exchange (replicas diverge -- timing only, the last thing this model does):
        # the difference is the part of the bucketed all-reduce that the backward program does not hide
        fs.skip_exchange = True
        for i in range(min(w, 3)):
            step_fn(state, pool[i % len(pool)])
        sync_all()
        t0 = time.perf_counter()
        for i in range(k):
            step_fn(state, pool[i % len(pool)])
        sync_all()
        dt0 = time.perf_counter() - t0
        t = torch.tensor([dt0], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        exposed_ms = (sec - float(t.item()) / k) * 1e3
        fs.skip_exchange = False
    one_rank = None
    if dist is None and not args.no_exchange_probe and torch.device(dev).type == "cuda":
        # The data-parallel form of the step on ONE GPU: a world-size-1 RCCL group with the gradient exchange forced on
        # (SSDE_FORCE_GRAD_EXCHANGE=1) -- one hipGraph per gradient bucket, an all-reduce behind each, the optimizer graph behind the
        # collectives (losses.FusedTrainStep._step_graph_segments).  A one-rank all-reduce moves nothing, so the ratio to the
        # single-graph step above is what the segmentation itself costs before any xGMI time.
        import socket
        import torch.distributed as tdist
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        # (under torch.distributed.run with one process TORCHELASTIC_USE_AGENT_STORE tells a tcp:// rendezvous that the AGENT hosts
        #  the store: rank 0 would then connect, as a client, to a port nobody listens on -- a 600 s timeout, seen in this round's
        #  call 35.  This group is private to the process: the variable is put aside while it is created, and the creation itself
        #  may take a minute at most)
        import datetime
        agent_store = os.environ.pop("TORCHELASTIC_USE_AGENT_STORE", None)
        try:
            try:
                tdist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=torch.device(dev),
                                         timeout=datetime.timedelta(seconds=60))
            finally:
                if agent_store is not None:
                    os.environ["TORCHELASTIC_USE_AGENT_STORE"] = agent_store
            os.environ["SSDE_FORCE_GRAD_EXCHANGE"] = "1"
            try:
                for i in range(5):
                    step_fn(state, pool[i % len(pool)])
                sync_all()
                prewarm(_chunk, sync_all, min(args.prewarm_s, 1.0))
                k2 = max(1, min(k, 50))
                with tele_leg((leg or "train") + "_exchange_one_rank"):
                    t0 = time.perf_counter()
                    for i in range(k2):
                        step_fn(state, pool[i % len(pool)])
                    sync_all()
                    sec2 = (time.perf_counter() - t0) / k2
                segs = getattr(fs, "_graph_seg", None)
                one_rank = {"value": sec2, "unit": "s/step", "steps": k2, "over_single_graph_step": sec2 / sec,
                            "graphs_per_step": len([1 for p_, _ in segs[1] if p_ is not None]) if segs else None,
                            "collectives_per_step": getattr(fs, "collectives_last_step", None),
                            "bucket_mb": float(os.environ.get("SSDE_GRAD_BUCKET_MB", "32")),
                            "note": "world-size-1 RCCL group, exchange forced on: the step as one hipGraph per gradient bucket + all-reduce "
                                    "per bucket + optimizer graph; a one-rank all-reduce moves no data"}
            finally:
                os.environ.pop("SSDE_FORCE_GRAD_EXCHANGE", None)
                tdist.destroy_process_group()
        except Exception as exc:                                   # noqa: BLE001  (diagnostic leg)
            one_rank = {"error": repr(exc)[:300]}
    fl = np.array(eng.program.flops)
    out = {"metric": "sec_per_train_step", "value": sec, "unit": "s/step", "higher_is_better": False,
           "exchange_one_rank": one_rank, "graph_fallback": graph_fallback,
           "batch_per_gpu": Bt, "global_batch": Bt * world, "images_per_sec": world * Bt / sec, "steps": k, "warmup": w,
           "prewarm_s": round(warm_s, 2),
           "loss": float(loss), "dropout": float(cfg.model.dropout), "path": "fused (losses.FusedTrainStep)",
           "algorithmic_tflops": float(fl.sum()) / sec / 1e12, "gflop_per_image": float(fl.sum()) / Bt / 1e9,
           "grad_allreduce_mb": eng.flat.numel * 4 / 1e6 if world > 1 else 0.0, "allreduce_exposed_ms": exposed_ms,
           "replicas_bit_identical_after_timed_steps": replicas_equal,
           "per_rank_ms_per_step": [round(v, 3) for v in per_rank_ms],
           "rank_spread_max_over_min": max(per_rank_ms) / min(per_rank_ms),
           "arena_gb": eng.b.arena_bytes / 1e9}
    if rank == 0 and not args.no_roofline:
        ms = np.array(eng.program.run_range_timed(0, eng.program.n))
        ms = np.array(eng.program.run_range_timed(0, eng.program.n))
        cls = np.array(eng.program.classes)
        idx = np.arange(eng.program.n)
        by = {}
        for name, c in [("conv3x3_fwd+dgrad", E.FC_CONV3), ("conv1x1_fwd+dgrad", E.FC_CONV1), ("wgrad", B.FC_WGRAD),
                        ("attention", E.FC_ATTN), ("groupnorm_stats", E.FC_GN), ("upfirdn", E.FC_FIR),
                        ("backward_elementwise", B.FC_BWD), ("other", E.FC_OTHER)]:
            m = cls == c
            by[name] = {"launches": int(m.sum()), "ms": float(ms[m].sum()), "gflop": float(fl[m].sum()) / 1e9}
            if name in ("backward_elementwise", "groupnorm_stats", "upfirdn") and by[name]["ms"] > 0:
                # HBM-bound classes: algorithmic bytes of the op list over the HIP-event time, against the 8 TB/s peak
                gb = float(sum(op_bytes(eng.program.ops[i]) for i in np.nonzero(m)[0])) / 1e9
                by[name].update(bound="hbm", gb=gb, achieved_tbs=gb / by[name]["ms"], frac=gb / by[name]["ms"] / PEAK_HBM_TBS)
        out["fwd_ms_events"] = float(ms[idx < eng.n_fwd].sum())
        out["bwd_ms_events"] = float(ms[idx >= eng.n_fwd].sum())
        out["by_class"] = by
        wg = cls == B.FC_WGRAD
        out["wgrad_tflops"] = float(fl[wg].sum()) / max(float(ms[wg].sum()), 1e-9) / 1e9
        if args.dump_train_ops:
            rows = []
            for i in range(eng.program.n):
                op = eng.program.ops[i]
                row = {"i": i, "kind": int(op.kind), "cls": int(cls[i]), "ms": float(ms[i]), "gflop": float(fl[i]) / 1e9,
                       "bwd": bool(i >= eng.n_fwd)}
                if op.kind == 1:
                    c = op.u.conv
                    row.update(h=c.h_out, w=c.w_out, cout=c.c_out, cin=c.main.c0 + c.main.c1, caux=c.aux.c0 + c.aux.c1, ks=c.ksize)
                elif op.kind == 15:
                    c = op.u.wgrad
                    row.update(h=c.h_out, w=c.w_out, cout=c.c_out, cin=c.src.c0 + c.src.c1, ks=c.ksize)
                rows.append(row)
            with open(args.dump_train_ops, "w") as f:
                json.dump(rows, f)
    return out


def bench_ode(args, dev, dist, world, rank):
    """BASELINE configs[4]: CIFAR-10 DDPM++ sub-VP, probability-flow ODE sampler (sampling.py:414-485: RK45, rtol = atol =
    1e-5, eps 1e-3) on the device-resident integrator.  One step = one full solve of a batch; the number of function
    evaluations is adaptive and is reported (random-init weights of the architecture: the NFE of a trained net differs)."""
    import _util
    from score_sde_pytorch_amd import sde_lib, sampling
    from score_sde_pytorch_amd.models import utils as mutils
    cfg = _util.cfgs.get_config("subvp/cifar10_ddpmpp_continuous")
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    _util.load_seeded(model, seed=1)
    model = model.to(dev).eval()
    B, R = args.batch, cfg.data.image_size
    sde = sde_lib.subVPSDE(beta_min=cfg.model.beta_min, beta_max=cfg.model.beta_max, N=cfg.model.num_scales)
    sampler = sampling.get_ode_sampler(sde, (B, 3, R, R), lambda v: v, denoise=cfg.sampling.noise_removal, rtol=1e-5, atol=1e-5,
                                       method="RK45", eps=1e-3, device=dev)
    torch.manual_seed(1234 + rank)
    steps, warm = max(1, min(args.steps, 3)), max(1, min(args.warmup, 1))

    def sync_all():
        torch.cuda.synchronize(dev)
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize(dev)
    for _ in range(warm):
        sampler(model, z=sde.prior_sampling((B, 3, R, R)).to(dev))
    sync_all()
    t0 = time.perf_counter()
    nfes = []
    for _ in range(steps):
        x, nfe = sampler(model, z=sde.prior_sampling((B, 3, R, R)).to(dev))
        nfes.append(int(nfe))
    sync_all()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    out = {"metric": "ode_sampler_images_per_sec", "value": world * B * steps / dt, "unit": "images/s", "n_gpus": world, "steps": steps,
           "warmup": warm, "ms_per_step": dt / steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32 (f64 integrator state)", "data": "synthetic",
           "config": {"workload": "configs/subvp/cifar10_ddpmpp_continuous probability-flow ODE sampler (RK45 rtol=atol=1e-5, eps=1e-3), "
                                  "batch %d/GPU, 32x32; 1 step = 1 solve" % B,
                      "batch_per_gpu": B, "nfe_per_solve": nfes, "state_finite": bool(torch.isfinite(x).all()),
                      "ms_per_nfe": dt / max(sum(nfes), 1) * 1e3, "parallelism": "replicas x%d (no collectives)" % world}}
    if rank == 0:
        _emit(out)
    if dist is not None:
        dist.destroy_process_group()


def _sync_factory(dev, dist):
    on_gpu = torch.device(dev).type == "cuda"           # (the CPU test of the rank logic passes a CPU device)

    def sync_all():
        if on_gpu:
            torch.cuda.synchronize(dev)
        if dist is not None:
            dist.barrier()
            if on_gpu:
                torch.cuda.synchronize(dev)
    return sync_all


def _max_over_ranks(dt, dev, dist, per_rank=None):
    """MAX over the ranks of a timed region (the job's time); per_rank (a list) receives every rank's own time."""
    if dist is not None:
        ts = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(dist.get_world_size())]
        dist.all_gather(ts, torch.tensor([dt], device=dev, dtype=torch.float64))
        if per_rank is not None:
            per_rank.extend(float(t.item()) for t in ts)
        dt = max(float(t.item()) for t in ts)
    elif per_rank is not None:
        per_rank.append(dt)
    return dt


import contextlib


@contextlib.contextmanager
def matrix_mode(mode):
    """SSDE_MATRIX for the programs lowered inside the block (the host maps it to SSDE_CONVF_BF16X6 when it builds launch
    arguments); the caller's own setting is restored afterwards."""
    prev = os.environ.get("SSDE_MATRIX")
    os.environ["SSDE_MATRIX"] = mode
    try:
        yield
    finally:
        if prev is None:
            os.environ.pop("SSDE_MATRIX", None)
        else:
            os.environ["SSDE_MATRIX"] = prev


class Telemetry:
    """Clock / power / temperature of THIS rank's GPU beside every timed leg (the line must explain its own
    clock).  Source: the amdsmi python binding in-process (amdsmi_get_gpu_metrics_info: one ~ms call returns gfx clock, memory
    clock, socket power, hotspot / memory temperature, throttle status), sampled by a background thread every 50 ms; falls back
    to `rocm-smi --json` (a subprocess, sampled every 0.5 s).  The hwmon files of this image read a constant (tools/energy_probe.py).
    A leg's record holds min / mean / max over the samples that fall inside it; `source` says where they came from."""

    def __init__(self, dev):
        import threading
        self.samples, self.legs, self._stop, self._lock = [], {}, threading.Event(), threading.Lock()
        self.source, self._handle, self.static = None, None, {}
        index = torch.device(dev).index or 0
        try:
            import amdsmi
            amdsmi.amdsmi_init()
            hs = amdsmi.amdsmi_get_processor_handles()
            # torch's device order follows HIP_VISIBLE_DEVICES; match by PCI bus id when torch exposes it
            want = None
            try:
                want = torch.cuda.get_device_properties(index).pci_bus_id
            except Exception:                                     # noqa: BLE001
                pass
            h = hs[index] if index < len(hs) else hs[0]
            if want is not None:
                for c in hs:
                    try:
                        bdf = amdsmi.amdsmi_get_gpu_device_bdf(c)
                        if int(bdf.split(":")[1], 16) == int(want):
                            h = c
                            break
                    except Exception:                             # noqa: BLE001
                        pass
            self._amdsmi, self._handle = amdsmi, h
            self._read_amdsmi()                                   # (raises if the call is not supported here)
            self.source = "amdsmi.amdsmi_get_gpu_metrics_info"
            try:
                cap = amdsmi.amdsmi_get_power_cap_info(h)
                self.static["power_cap_w"] = float(cap.get("power_cap", 0)) / (1e6 if float(cap.get("power_cap", 0)) > 1e5 else 1.0)
            except Exception:                                     # noqa: BLE001
                pass
        except Exception as exc:                                  # noqa: BLE001
            self._amdsmi = None
            self.static["amdsmi_error"] = repr(exc)[:200]
            try:
                self._read_rocm_smi()
                self.source = "rocm-smi --showclocks --showpower --showtemp --json"
            except Exception as exc2:                             # noqa: BLE001
                self.static["rocm_smi_error"] = repr(exc2)[:200]
        if self.source is not None:
            self._thread = threading.Thread(target=self._poll, daemon=True)
            self._thread.start()

    @staticmethod
    def _num(v):
        try:
            f = float(v)
            return f if f == f and abs(f) < 6.5e4 else None      # (0xFFFF / "N/A" = not reported)
        except (TypeError, ValueError):
            return None

    def _read_amdsmi(self):
        m = self._amdsmi.amdsmi_get_gpu_metrics_info(self._handle)
        gfx = m.get("current_gfxclks") or m.get("current_gfxclk")
        if isinstance(gfx, (list, tuple)):                        # one entry per XCD
            vals = [self._num(v) for v in gfx]
            vals = [v for v in vals if v]
            gfx_mean, gfx_min = (sum(vals) / len(vals), min(vals)) if vals else (None, None)
        else:
            gfx_mean = gfx_min = self._num(gfx)
        return {"sclk_mhz": gfx_mean, "sclk_min_xcd_mhz": gfx_min, "mclk_mhz": self._num(m.get("current_uclk")),
                "power_w": self._num(m.get("current_socket_power")) or self._num(m.get("average_socket_power")),
                "temp_hotspot_c": self._num(m.get("temperature_hotspot")), "temp_mem_c": self._num(m.get("temperature_mem")),
                "throttle_status": self._num(m.get("throttle_status")) or 0.0}

    def _read_rocm_smi(self):
        import subprocess
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--showtemp", "--json"], capture_output=True, text=True, timeout=10)
        d = json.loads(r.stdout[r.stdout.index("{"):])
        card = d[sorted(d)[0]]
        out = {"sclk_mhz": None, "sclk_min_xcd_mhz": None, "mclk_mhz": None, "power_w": None, "temp_hotspot_c": None, "temp_mem_c": None,
               "throttle_status": 0.0}
        import re
        for k, v in card.items():
            num = re.search(r"[-+]?\d+\.?\d*", str(v))
            val = float(num.group()) if num else None
            kl = k.lower()
            if "sclk" in kl and "level" in kl:
                out["sclk_mhz"] = out["sclk_min_xcd_mhz"] = val
            elif "mclk" in kl and "level" in kl:
                out["mclk_mhz"] = val
            elif "power" in kl and val is not None:
                out["power_w"] = val
            elif "junction" in kl:
                out["temp_hotspot_c"] = val
            elif "memory" in kl and "temp" in kl:
                out["temp_mem_c"] = val
        return out

    def _poll(self):
        read, period = (self._read_amdsmi, 0.05) if self._amdsmi is not None else (self._read_rocm_smi, 0.5)
        while not self._stop.is_set():
            try:
                rec = read()
                with self._lock:
                    self.samples.append((time.perf_counter(), rec))
            except Exception:                                     # noqa: BLE001
                pass
            self._stop.wait(period)

    @contextlib.contextmanager
    def leg(self, name):
        t0 = time.perf_counter()
        try:
            yield
        finally:
            self.legs[name] = self.summary(t0, time.perf_counter())

    def summary(self, t0, t1):
        with self._lock:
            recs = [r for t, r in self.samples if t0 <= t <= t1]
        out = {"samples": len(recs), "seconds": round(t1 - t0, 3)}
        for key in ("sclk_mhz", "sclk_min_xcd_mhz", "mclk_mhz", "power_w", "temp_hotspot_c", "temp_mem_c"):
            vals = [r[key] for r in recs if r.get(key) is not None]
            if vals:
                out[key] = {"min": round(min(vals), 1), "mean": round(sum(vals) / len(vals), 1), "max": round(max(vals), 1)}
        thr = [r["throttle_status"] for r in recs if r.get("throttle_status")]
        out["throttled_samples"] = len(thr)
        return out

    def report(self):
        self._stop.set()
        return {"source": self.source, **self.static, "legs": self.legs}


_TELE = None


def tele_leg(name):
    """context manager: telemetry of a timed leg (a no-op when no source is available / on ranks without telemetry)"""
    if _TELE is None or _TELE.source is None:
        return contextlib.nullcontext()
    return _TELE.leg(name)


def prewarm(run_chunk, sync, seconds, dev=None, dist=None):
    """Time-based pre-warm outside --warmup: the same work as the timed region for at least `seconds`, so that the device is in
    the clock / power state of sustained load when the timed region starts (a 1 s region after 3 warm-up iterations measures the
    boost clock of a cold device on one lease and a throttled one on the next).  Returns the seconds spent."""
    if seconds <= 0:
        return 0.0
    t0 = time.perf_counter()
    while True:
        run_chunk()
        sync()
        el = time.perf_counter() - t0
        if dist is not None:                  # every rank takes the same number of chunks (sync() holds a barrier)
            t = torch.tensor([el], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        if el >= seconds:
            return el


DTYPE = {"f32": "f32 (exact-fp32 MFMA kernels everywhere)",
         "bf16x6": "f32 via 3-way bf16 split, fp32 accumulate (the 1x1 / NIN / Linear GEMMs and the attention forward as exact-fp32 products "
                   "on the BF16 matrix pipe, fp32 softmax; 3x3 convolutions and the attention backward on the fp32-MFMA kernels)"}


def op_bytes(op):
    """Algorithmic (compulsory) HBM bytes of one HBM-bound op of the program, from its arguments (fp32):
    GroupNorm statistics = one read of the tensor; FIR = input + output (both outputs of a fused pair); randn = one write; squared norms = two reads;
    Langevin / predictor update = 3 reads (x, score, z) + 2 writes (x, x_mean)."""
    from score_sde_pytorch_amd import _lib as L
    k = int(op.kind)
    if k == L.OP_GN_STATS:
        a = op.u.gn
        return 4.0 * a.n * a.hw * (a.c0 + a.c1)
    if k == L.OP_UPFIRDN:
        a = op.u.fir
        # (a fused pair -- act(GroupNorm(x)) and x resampled by one launch, ssde_upfirdn_args.dst2 -- writes two outputs; its
        #  partner spec is not an op of its own.  An accumulating launch also reads its destination)
        outs = (2 if a.dst2 else 1) + (1 if a.accumulate else 0)
        return 4.0 * a.n * a.c * (a.h_in * a.w_in + outs * a.h_out * a.w_out)
    if k == L.OP_RANDN:
        return 4.0 * op.u.randn.numel
    if k == L.OP_SUMSQ:
        return 8.0 * op.u.sumsq.n * op.u.sumsq.per
    if k == L.OP_LANGEVIN:
        return 20.0 * op.u.langevin.n * op.u.langevin.per
    if k == L.OP_PREDICTOR:
        return 20.0 * op.u.predictor.numel
    if k == L.OP_GN_FINALIZE:                     # the producers' partial statistics: (mean, M2, count) per slice and channel quad
        a = op.u.gn_fin
        return 12.0 * a.n * (a.slices0 * (a.c0 // 4) + a.slices1 * (a.c1 // 4))
    # backward, element-wise class: GroupNorm / SiLU / dropout backward = read x, read d(act), write (or accumulate) dx;
    # its statistics pass = read x, read d(act); bias gradients = one read of the gradient; layout changes = read + write
    if k == L.OP_PROLOGUE_BWD:
        a = op.u.pro_bwd
        c = a.src.c0 + a.src.c1
        return 4.0 * a.n * a.hw * c * (3 + (1 if (a.acc0 or a.acc1) else 0))
    if k == L.OP_GN_BWD_REDUCE:
        a = op.u.gn_bwd
        c = a.src.c0 + a.src.c1
        if a.g0 or a.g1:                              # reduction AND apply in one call: read dp, read x, write (or accumulate) dx
            return 4.0 * a.n * a.hw * c * (3 + (1 if (a.acc0 or a.acc1) else 0))
        return 8.0 * a.n * a.hw * c
    if k == L.OP_COLSUM:
        return 4.0 * op.u.colsum.n * op.u.colsum.hw * op.u.colsum.c
    if k == L.OP_TO_NHWC:
        a = op.u.to_nhwc
        return 4.0 * a.n * a.h * a.w * (a.c + a.c_pad)
    if k == L.OP_TO_NCHW:
        a = op.u.to_nchw
        return 4.0 * a.n * a.h * a.w * (a.c + a.c_src)
    if k == L.OP_MEMSET:
        return float(op.u.memset.bytes)
    if k == L.OP_AXPY:
        return 12.0 * op.u.axpy.numel
    return 0.0


def conv_bytes(c):
    """Algorithmic bytes of a convolution launch: input(s) + output + packed weights (+ residual) in fp32."""
    px_in = c.n * (c.h_in * c.w_in if c.ksize else c.h_out * c.w_out)
    px_out = c.n * c.h_out * c.w_out
    cin3, cin1 = c.main.c0 + c.main.c1, c.aux.c0 + c.aux.c1
    b = 4.0 * (px_in * cin3 + px_out * cin1 + px_out * c.c_out)
    b += 4.0 * c.c_out * (9 * cin3 + cin1)
    if c.resid:
        b += 4.0 * px_out * c.c_out
    return b


def roofline_of(prog, E, L, reps=3):
    """Per-op HIP-event times of a program -> the roofline object of the bench line."""
    acc = np.zeros(prog.n)
    prog.run_timed()
    for _ in range(reps):
        acc += np.array(prog.run_timed())
    ms = acc / reps
    cls = np.array(prog.classes)
    fl = np.array(prog.flops)
    tiles = np.array([int(prog.ops[i].u.conv.tile) if int(prog.ops[i].kind) == L.OP_CONV else -1 for i in range(prog.n)])
    wino4 = np.isin(tiles, L.TILES_WINOGRAD4)     # F(4x4,3x3): fused, two kernels (LDS- or register-fed matrix kernel)
    wino4g = tiles == L.TILE_WINOGRAD4R                 # two-kernel form: transform pass + register-fed matrix kernel
    wino = (tiles == L.TILE_WINOGRAD) | wino4
    executed = np.where(wino4, fl / WINOGRAD4_FLOP_RATIO, np.where(wino, fl / WINOGRAD_FLOP_RATIO, fl))
    nbytes = np.array([op_bytes(prog.ops[i]) for i in range(prog.n)])
    conv3 = cls == E.FC_CONV3
    t3 = float(ms[conv3].sum()) * 1e-3
    achieved_exec = float(executed[conv3].sum()) / t3 / 1e12
    achieved_alg = float(fl[conv3].sum()) / t3 / 1e12
    by_class = {}
    for name, c, bound in [("conv3x3_fused", E.FC_CONV3, "mfma"), ("conv1x1_gemm", E.FC_CONV1, "mfma"), ("attention", E.FC_ATTN, "mfma"),
                           ("groupnorm_stats", E.FC_GN, "hbm"), ("upfirdn", E.FC_FIR, "hbm"), ("other", E.FC_OTHER, None)]:
        m = cls == c
        t = float(ms[m].sum()) * 1e-3
        row = {"launches": int(m.sum()), "ms": t * 1e3, "gflop": float(fl[m].sum()) / 1e9}
        if bound == "mfma" and t > 0:
            row.update(bound="mfma", executed_tflops=float(executed[m].sum()) / t / 1e12,
                       frac=float(executed[m].sum()) / t / 1e12 / PEAK_FP32_MFMA_TFLOPS)
        elif bound == "hbm" and t > 0:
            row.update(bound="hbm", algorithmic_gb=float(nbytes[m].sum()) / 1e9, achieved_tbs=float(nbytes[m].sum()) / t / 1e12,
                       frac=float(nbytes[m].sum()) / t / 1e12 / PEAK_HBM_TBS)
        if name == "groupnorm_stats" and row["launches"]:
            row["note"] = ("launch-bound, not bandwidth-bound: %d ssde_gn_finalize launches of %.1f us merging the producers' partial "
                           "statistics (the activations are not re-read); the fraction is kept for completeness"
                           % (row["launches"], row["ms"] * 1e3 / row["launches"]))
        if name == "groupnorm_stats":
            # ABI 10: the transform pass of a two-kernel F(4x4,3x3) convolution merges the partials of its source itself
            # (ssde_conv_args.gn_in_part0); its time is the pass's, in the 3x3 class
            row["merged_by_the_consuming_transform_pass"] = sum(
                1 for i in range(prog.n) if int(prog.ops[i].kind) == L.OP_CONV and prog.ops[i].u.conv.gn_in_part0)
        by_class[name] = row
    # PC-update kernels (rocRAND noise, norms, Langevin and predictor updates): HBM-bound, grouped by op kind
    upd = np.array([int(prog.ops[i].kind) in (L.OP_RANDN, L.OP_SUMSQ, L.OP_LANGEVIN, L.OP_PREDICTOR) for i in range(prog.n)])
    if upd.any():
        t = float(ms[upd].sum()) * 1e-3
        by_class["pc_update"] = {"launches": int(upd.sum()), "ms": t * 1e3, "bound": "hbm", "algorithmic_gb": float(nbytes[upd].sum()) / 1e9,
                                 "achieved_tbs": float(nbytes[upd].sum()) / t / 1e12,
                                 "frac": float(nbytes[upd].sum()) / t / 1e12 / PEAK_HBM_TBS}
    # the dominant kernel: the Winograd kernel that takes the larger share of the time
    dom4 = float(ms[wino4].sum()) >= float(ms[wino & ~wino4].sum())
    wl = [i for i in range(prog.n) if (wino4[i] if dom4 else (wino[i] and not wino4[i]))]
    alg_bytes_wino = float(np.mean([conv_bytes(prog.ops[i].u.conv) for i in wl])) if wl else None
    # (F(4x4,3x3) runs as transform pass + register-fed matrix kernel wherever the engine takes it: the pair is the dominant
    #  "kernel" then, and its HBM traffic is the sum of the two launches of a layer)
    dom4r = dom4 and float(ms[wino4g].sum()) >= float(ms[wino4 & ~wino4g].sum())
    return dict(ms=ms, cls=cls, fl=fl, wino=wino, wino4=wino4, wino4g=wino4g,
                dominant="conv_wino4r_kernel" if dom4r else "conv_wino4_kernel" if dom4 else "conv_wino_kernel",
                executed=executed, conv3=conv3, by_class=by_class,
                achieved_exec=achieved_exec, achieved_alg=achieved_alg, alg_bytes_wino=alg_bytes_wino)


class ScheduleRunner:
    """PC iterations of a sampler engine that keep its step index inside the N-iteration schedule (the kernels read the step
    tables at that index): a sampler run that has taken its last iteration starts over from the prior sample x0."""

    def __init__(self, eng, prog, x0, N, use_graph):
        self.eng, self.prog, self.x0, self.N, self.use_graph = eng, prog, x0, N, use_graph
        self.pos = 0                                  # the engine's step index (host copy; the engine was just reset to x0)

    def restart(self):
        self.eng.reset(self.x0)
        self.pos = 0

    def run(self, k):
        while k > 0:
            if self.pos == self.N:
                self.restart()
            n = min(k, self.N - self.pos)
            self.eng.run_steps(self.prog, n, self.use_graph)
            self.pos += n
            k -= n


DUMP_BYTES = 64 << 20


def dump_outputs(path, arrays, budget=DUMP_BYTES):
    """arrays {name: tensor or array} -> path/<name>.npy in float32 (float64 stays float64).  Above `budget` bytes in all, every
    array is cut to its share of the budget by a fixed seeded sample of its flattened elements (sorted indices, the same for a
    given size in every run).  Returns {name: shape written}."""
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    arrays = {k: v.astype(np.float64 if v.dtype == np.float64 else np.float32, copy=False) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    os.makedirs(path, exist_ok=True)
    shapes = {}
    for k, v in arrays.items():
        if total > budget:
            keep = max(1, int(budget * (v.nbytes / total)) // v.itemsize)
            if keep < v.size:
                idx = np.sort(np.random.default_rng(0).choice(v.size, keep, replace=False))
                v = v.reshape(-1)[idx]
        np.save(os.path.join(path, k + ".npy"), np.ascontiguousarray(v))
        shapes[k] = list(v.shape)
    return shapes


def bench_pc(args, cfg_name, B, N, dev, dist, world, rank, steps, warmup, detail, leg=None, keep_outputs=False):
    """PC sampler of a VE NCSN++ config: one hipGraph replay per iteration; returns (result dict, engine, model, sd, cfg).
    The timed steps are the first `steps` iterations of a sampler run from the seeded prior sample, whatever ran before them;
    keep_outputs: the result carries "_outputs", the state (x, x_mean) after the last timed step, on the host."""
    import _util
    from score_sde_pytorch_amd import sde_lib, sampling, engine as E, _lib as L
    from score_sde_pytorch_amd.models import utils as mutils
    cfg = _util.cfgs.get_config(cfg_name)
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    sd = _util.load_seeded(model, seed=1)
    model = model.to(dev).eval()
    R = cfg.data.image_size
    sde = sde_lib.VESDE(cfg.model.sigma_min, cfg.model.sigma_max, N=N)
    sampler = sampling.get_pc_sampler(sde, (B, 3, R, R), sampling.get_predictor(cfg.sampling.predictor),
                                      sampling.get_corrector(cfg.sampling.corrector), lambda v: v, snr=cfg.sampling.snr,
                                      n_steps=cfg.sampling.n_steps_each, probability_flow=False, continuous=True,
                                      denoise=True, eps=1e-5, device=dev)
    torch.manual_seed(1234 + rank)
    x_T = sde.prior_sampling((B, 3, R, R))
    sampler(model, x_init=x_T, max_steps=0)     # builds the engine, loads the state, draws this rank's Philox seed word
    eng = sampler.engine
    prog = eng.step_program(with_rng=True)
    use_graph = not args.no_graph
    sync_all = _sync_factory(dev, dist)
    runner = ScheduleRunner(eng, prog, x_T.to(dev), N, use_graph)
    runner.run(warmup)
    sync_all()
    warm_s = prewarm(lambda: runner.run(10), sync_all, args.prewarm_s, dev, dist)
    # (the time-based pre-warm takes a different number of iterations in every run: the timed ones start the schedule afresh)
    runner.restart()
    sync_all()
    with tele_leg(leg or ("sampler " + cfg_name)):
        t0 = time.perf_counter()
        runner.run(steps)
        sync_all()
        dt_own = time.perf_counter() - t0
    outputs = {"x": eng.x.view(eng.shape).cpu(), "x_mean": eng.x_mean.view(eng.shape).cpu()} if keep_outputs else None
    per_rank = []
    dt = _max_over_ranks(dt_own, dev, dist, per_rank)
    ms_per_step = dt / steps * 1e3
    res = {"value": world * B / (N * ms_per_step * 1e-3), "unit": "images/s", "ms_per_step": ms_per_step, "steps": steps, "warmup": warmup,
           "prewarm_s": round(warm_s, 2),
           "per_rank_ms_per_step": [round(t / steps * 1e3, 3) for t in per_rank], "rank_spread_max_over_min": max(per_rank) / min(per_rank),
           "workload": "configs/%s PC sampler (reverse_diffusion+langevin), batch %d/GPU, N=%d, %dx%d; 1 step = 1 PC iteration = "
                       "2 U-Net evaluations" % (cfg_name, B, N, R, R),
           "batch_per_gpu": B, "sde_steps": N, "nfe_per_step": eng.nfe_per_step(), "path": eng.last_path,
           "state_finite": bool(torch.isfinite(eng.x).all()), "unet_gflop_per_image": eng.unet.flops_per_forward() / B / 1e9,
           "end_to_end_tflops": eng.nfe_per_step() * eng.unet.flops_per_forward() / (ms_per_step * 1e-3) / 1e12,
           "direct_form_ceiling_images_per_sec": world * B / (N * eng.nfe_per_step() * eng.unet.flops_per_forward() / (PEAK_FP32_MFMA_TFLOPS * 1e12))}
    if detail and rank == 0 and not args.no_roofline:
        roof = roofline_of(eng.unet.program, E, L)                 # classes of ONE U-Net evaluation
        upd = roofline_of(prog, E, L, reps=2)["by_class"].get("pc_update")   # update kernels of one whole PC iteration
        if upd:
            roof["by_class"]["pc_update"] = upd
        res["_roof"] = roof
    if outputs is not None:
        res["_outputs"] = outputs
    return res, eng, model, sd, cfg


def bench_ode_compact(args, dev, dist, world, rank):
    """BASELINE configs[4] inside a --full run: ONE solve of a batch (RK45 rtol = atol = 1e-5, eps 1e-3) after a few warm-up
    evaluations of the right-hand side (engine lowering, graph of the integrator's stage kernels)."""
    import _util
    from score_sde_pytorch_amd import sde_lib, sampling
    from score_sde_pytorch_amd.models import utils as mutils
    cfg = _util.cfgs.get_config("subvp/cifar10_ddpmpp_continuous")
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    _util.load_seeded(model, seed=1)
    model = model.to(dev).eval()
    B, R = 256, cfg.data.image_size
    sde = sde_lib.subVPSDE(beta_min=cfg.model.beta_min, beta_max=cfg.model.beta_max, N=cfg.model.num_scales)
    sampler = sampling.get_ode_sampler(sde, (B, 3, R, R), lambda v: v, denoise=cfg.sampling.noise_removal, rtol=1e-5, atol=1e-5,
                                       method="RK45", eps=1e-3, device=dev)
    warm = sampling.get_ode_sampler(sde, (B, 3, R, R), lambda v: v, denoise=False, rtol=1e-1, atol=1e-1, method="RK45", eps=0.9,
                                    device=dev)
    torch.manual_seed(1234 + rank)
    warm(model, z=sde.prior_sampling((B, 3, R, R)).to(dev))
    sync_all = _sync_factory(dev, dist)
    sync_all()
    t0 = time.perf_counter()
    x, nfe = sampler(model, z=sde.prior_sampling((B, 3, R, R)).to(dev))
    sync_all()
    dt = _max_over_ranks(time.perf_counter() - t0, dev, dist)
    return {"metric": "ode_sampler_images_per_sec", "value": world * B / dt, "unit": "images/s", "solves": 1, "nfe": int(nfe),
            "ms_per_nfe": dt / max(int(nfe), 1) * 1e3, "seconds_per_solve": dt, "batch_per_gpu": B, "state_finite": bool(torch.isfinite(x).all()),
            "workload": "configs/subvp/cifar10_ddpmpp_continuous probability-flow ODE sampler (RK45 rtol=atol=1e-5, eps=1e-3), batch %d/GPU; "
                        "random-init weights (the NFE of a trained network differs)" % B}


def bench_likelihood(args, dev, dist, world, rank, tol=1e-5, batch=256):
    """BASELINE configs[4]'s other half (likelihood.py:69-111): bits/dim of a batch by the probability-flow ODE with the
    Hutchinson-Skilling divergence, RK45, the state [x | delta log p] resident on the device; every evaluation = one U-Net
    forward + one input-gradient (vector-Jacobian) pass as ONE captured program (ode.FusedLikelihoodRhs).  Synthetic data
    U[-1, 1) (the sub-VP configs centre their data), random-init weights: the NFE of a trained network differs."""
    import _util
    from score_sde_pytorch_amd import sde_lib, likelihood
    from score_sde_pytorch_amd.models import utils as mutils
    cfg = _util.cfgs.get_config("subvp/cifar10_ddpmpp_continuous")
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    _util.load_seeded(model, seed=1)
    model = model.to(dev).eval()
    B, R = batch, cfg.data.image_size
    sde = sde_lib.subVPSDE(beta_min=cfg.model.beta_min, beta_max=cfg.model.beta_max, N=cfg.model.num_scales)
    inv = lambda v: (v + 1.) / 2.                                    # noqa: E731  (datasets.get_data_inverse_scaler, centered data)
    lik = likelihood.get_likelihood_fn(sde, inv, rtol=tol, atol=tol, eps=1e-5)
    warm = likelihood.get_likelihood_fn(sde, inv, rtol=0.5, atol=0.5, eps=0.9)     # same SDE object: warms the cached program / graph
    torch.manual_seed(4321 + rank)
    data = torch.rand(B, 3, R, R, device=dev) * 2 - 1
    warm(model, data)
    sync_all = _sync_factory(dev, dist)
    sync_all()
    t0 = time.perf_counter()
    bpd, z, nfe = lik(model, data)
    sync_all()
    dt = _max_over_ranks(time.perf_counter() - t0, dev, dist)
    return {"metric": "likelihood_images_per_sec", "value": world * B / dt, "unit": "images/s", "nfe": int(nfe),
            "ms_per_nfe": dt / max(int(nfe), 1) * 1e3, "seconds_per_solve": dt, "batch_per_gpu": B, "bpd_mean": float(bpd.mean()),
            "bpd_finite": bool(torch.isfinite(bpd).all()), "path": lik.last_path, "rtol_atol": tol,
            "workload": "configs/subvp/cifar10_ddpmpp_continuous likelihood.get_likelihood_fn (RK45 rtol=atol=%g, eps=1e-5, Rademacher "
                        "probe), batch %d/GPU; 1 evaluation = U-Net forward + input-gradient pass" % (tol, B)}


def cpu_baseline(args, cfg, model, sd, R, N):
    """The CPU oracle (torch-CPU port of the reference path, the same ATen ops the reference runs on CPU) on this box's host
    cores: K whole PC iterations at the config batch (up to K=5, bounded by --cpu-seconds), extrapolated to N
    iterations; and DSM training steps (forward + autograd backward + clip + Adam + EMA) at the largest batch the budget allows."""
    from oracle import sampler_oracle, unet_oracle
    total = os.cpu_count() or 1
    full_sd = {k: v.detach().cpu() for k, v in sd.items()}
    full_sd["sigmas"] = model.sigmas.cpu()
    if args.cpu_threads:
        cores = max(1, min(args.cpu_threads, total))
    else:
        # oneDNN does not scale monotonically on this host (the same PC iteration ran 3x slower per image on 64 threads
        # than on 16): probe a few thread counts on one forward each and keep the fastest.  The probe batch is 32 (VERDICT r5
        # weak 8: a batch-4 forward says little about how oneDNN threads the batch-256 convolutions; 32 images give every
        # candidate thread count at least one image per two threads, ~2 s per probe)
        from oracle import unet_oracle as _uo
        xs = torch.randn(32, 3, R, R)
        sg = torch.ones(32)
        best, cores = None, 1
        for c in sorted({min(c, total) for c in (16, 32, 64)}):        # (all 256 threads: minutes per forward, measured)
            torch.set_num_threads(c)
            with torch.no_grad():
                _uo.ncsnpp_forward(cfg, full_sd, xs, sg)
                t0 = time.perf_counter()
                _uo.ncsnpp_forward(cfg, full_sd, xs, sg)
                dt = time.perf_counter() - t0
            if best is None or dt < best:
                best, cores = dt, c
    torch.set_num_threads(cores)
    g = torch.Generator().manual_seed(3)
    kw = dict(sigma_min=cfg.model.sigma_min, sigma_max=cfg.model.sigma_max, N=N)

    def cpu_iters(cb, steps):
        x0 = torch.randn(cb, 3, R, R, generator=g) * cfg.model.sigma_max
        nz = torch.randn(steps, 2, cb, 3, R, R, generator=g)
        t0 = time.perf_counter()
        sampler_oracle.pc_sample(cfg, full_sd, "vesde", kw, x0, nz, snr=cfg.sampling.snr, eps=1e-5, max_steps=steps)
        return time.perf_counter() - t0
    t_probe = cpu_iters(4, 1) / 4                              # warm-up + per-image cost of one iteration
    cb = int(max(4, min(args.cpu_batch, args.cpu_seconds / max(t_probe, 1e-4))))
    # K = 5 whole PC iterations at the config batch when the budget holds them (the default 200 s does on this
    # host: ~35 s per iteration at batch 256), fewer on a slower host -- ONE timed run
    # (the per-image cost of the batch-4 probe underestimates a batch-256 iteration: K is 1 below the 200 s budget)
    k = int(max(1, min(5, args.cpu_seconds // max(t_probe * cb, 1e-3)))) if args.cpu_seconds >= 200 else 1
    t_k = cpu_iters(cb, k)
    out = {"value": cb / (N / k * t_k), "unit": "images/s", "cores": cores, "host_cores_total": total, "kind": "port",
           "sample": "K=%d PC iteration(s) (%d U-Net evaluations) at batch %d with the torch-CPU oracle (oracle/sampler_oracle.py) "
                     "on %d of %d host threads: %.2f s; extrapolated img/s = B / ((N/K) * t_K) with N=%d"
                     % (k, 2 * k, cb, cores, total, t_k, N)}
    # ---- DSM training step on the CPU: oracle forward under autograd, reference optimizer sequence (losses.py:41-50)
    sd_req = {n: (v.clone().requires_grad_() if (v.dtype == torch.float32 and n != "sigmas") else v) for n, v in full_sd.items()}
    params = [v for v in sd_req.values() if torch.is_tensor(v) and v.requires_grad]
    opt = torch.optim.Adam(params, lr=2e-4, betas=(0.9, 0.999), eps=1e-8)
    ema = [p.detach().clone() for p in params]

    def train_step(tb):
        batch = torch.rand(tb, 3, R, R, generator=g)
        t = torch.rand(tb, generator=g) * (1 - 1e-5) + 1e-5
        z = torch.randn(tb, 3, R, R, generator=g)
        t0 = time.perf_counter()
        std = cfg.model.sigma_min * (cfg.model.sigma_max / cfg.model.sigma_min) ** t
        score = unet_oracle.ncsnpp_forward(cfg, sd_req, batch + std[:, None, None, None] * z, std)
        loss = torch.mean(0.5 * torch.sum((score * std[:, None, None, None] + z).reshape(tb, -1) ** 2, dim=-1))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        with torch.no_grad():
            for e, p in zip(ema, params):
                e.sub_(0.001 * (e - p))
        return time.perf_counter() - t0
    t_probe = train_step(4) / 4
    tb = int(max(4, min(128, (args.cpu_seconds / 4) / max(t_probe, 1e-4))))
    n_timed = 3 if (args.cpu_seconds >= 200 and t_probe * tb * 4 <= 2 * args.cpu_seconds) else 1   # 1 warm-up + 3 timed at the 200 s budget
    ts = [train_step(tb) for _ in range(1 + n_timed)][1:]
    out["train"] = {"value": float(np.mean(ts)) * 128.0 / tb, "unit": "s/step at batch 128 (linear in batch)", "measured_s_per_step": float(np.mean(ts)),
                    "measured_batch": tb, "cores": cores,
                    "sample": "1 warm-up + %d timed DSM steps (oracle forward, torch autograd backward, clip + Adam + EMA) at batch %d" % (n_timed, tb)}
    return out


def _launch_cmd(n, port, argv):
    """The driver's own command line for N ranks on one node (one rank per GPU, rendezvous on 127.0.0.1)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def _self_launch(n, share_device=False):
    import socket
    import subprocess
    have = torch.cuda.device_count()
    if have < (1 if share_device else n):
        print("bench.py: --gpus %d but only %d GPU(s) are visible%s" % (n, have, "" if share_device else " (--share-device --dist-backend gloo "
              "runs the N-rank code paths on fewer GPUs)"), file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC only on this driver (RCCL across processes)
    cmd = _launch_cmd(n, port, sys.argv[1:])
    print("[bench] self-launch: %s" % " ".join(cmd), file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env)


def rank_setup(args, env, n_devices, on_gpu=True):
    """(world, rank, device index) of this process and its process group (None at world 1): torchrun's RANK / LOCAL_RANK /
    WORLD_SIZE, one GPU per local rank -- or, with --share-device, GPU local_rank % n_devices.  Ends with an actual collective:
    every rank contributes 1 and the sum must be the world size."""
    world = int(env.get("WORLD_SIZE", "1"))
    rank = int(env.get("RANK", "0"))
    local_rank = int(env.get("LOCAL_RANK", "0"))
    assert args.gpus == world, "--gpus %d under a launcher with WORLD_SIZE=%d" % (args.gpus, world)
    assert not (args.share_device and args.dist_backend == "nccl" and world > n_devices), \
        "--share-device with more ranks than GPUs needs --dist-backend gloo (RCCL refuses two ranks on one device)"
    index = local_rank % max(n_devices, 1) if args.share_device else local_rank
    assert index < max(n_devices, 1), "local rank %d but %d visible GPU(s)" % (local_rank, n_devices)
    dev = torch.device("cuda", index) if on_gpu else torch.device("cpu")
    dist, ranks = None, 1
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        kw = {"device_id": dev} if args.dist_backend == "nccl" else {}
        dist.init_process_group(args.dist_backend, rank=rank, world_size=world, **kw)
        one = torch.ones(1, device=dev)
        dist.all_reduce(one)                          # an actual collective (RCCL / gloo): every rank contributes 1
        ranks = int(round(float(one.item())))
        assert ranks == dist.get_world_size() == world, (ranks, world)
    return world, rank, dev, dist, ranks


_T0 = time.perf_counter()
_REAL_STDOUT = None


def _own_stdout():
    """From here on file descriptor 1 is stderr for everybody in this process -- RCCL prints a version banner on stdout when a
    process group initialises, buffered by the C library and flushed at exit, i.e. AFTER the result line -- and the ONE JSON line
    of the contract is written to the real stdout by _emit."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)


def _emit(obj):
    line = (json.dumps(obj) + "\n").encode()
    if _REAL_STDOUT is None:
        sys.stdout.write(line.decode())
        sys.stdout.flush()
    else:
        os.write(_REAL_STDOUT, line)


def _phase(msg):
    print("[bench %7.1f s] %s" % (time.perf_counter() - _T0, msg), file=sys.stderr, flush=True)


def _rccl_version():
    """What NCCL_DEBUG=VERSION would print: the collective library torch.distributed's "nccl" backend is linked against."""
    try:
        return "RCCL %s (torch %s, HIP %s)" % (".".join(str(v) for v in torch.cuda.nccl.version()), torch.__version__, torch.version.hip)
    except Exception as e:                        # noqa: BLE001
        return "unavailable: %s" % e


def mfma_probe(dev, iters=20000, reps=5):
    """TFLOP/s of back-to-back fp32 MFMAs on every SIMD (the C ABI's diagnostic ssde_mfma_probe), best of `reps`."""
    import ctypes as C
    from score_sde_pytorch_amd import _lib as L
    lib = L.load()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    sink = torch.zeros(64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.ssde_mfma_probe.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.check(lib.ssde_mfma_probe(cus, 200, sink.data_ptr(), st), "ssde_mfma_probe")
    best = 0.0
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(lib.ssde_mfma_probe(cus, iters, sink.data_ptr(), st), "ssde_mfma_probe")
        e1.record()
        torch.cuda.synchronize()
        best = max(best, cus * 4 * iters * 8 * 4096.0 / (e0.elapsed_time(e1) * 1e-3) / 1e12)
    return best


def main():
    args = parse()
    assert torch.cuda.is_available(), "bench.py needs the MI355X (the HIP path has no CPU fallback)"
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: re-execute under torch.distributed.run, one rank per GPU over
        # RCCL (the same command line the driver uses); rank 0 of that job prints the JSON line on our stdout
        raise SystemExit(_self_launch(args.gpus, args.share_device))
    _own_stdout()
    n_dev = torch.cuda.device_count()
    lr = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(lr % max(n_dev, 1) if args.share_device else lr)
    world, rank, dev, dist, rccl_ranks = rank_setup(args, os.environ, n_dev)

    import _util
    from score_sde_pytorch_amd import engine as E, _lib as L

    global _TELE
    if rank == 0 and not args.no_telemetry:
        _TELE = Telemetry(dev)

    if args.workload == "subvp_ode":
        return bench_ode(args, dev, dist, world, rank)
    if args.workload == "subvp_likelihood":
        r = bench_likelihood(args, dev, dist, world, rank, tol=1e-5, batch=256 if args.batch == 256 else args.batch)
        r.update(n_gpus=world, higher_is_better=True, scaling="weak", vs_baseline=None, dtype="f32 (f64 integrator state)", data="synthetic",
                 steps=1, warmup=1, ms_per_step=r["seconds_per_solve"] * 1e3, config={"workload": r.pop("workload")})
        if rank == 0:
            _emit(r)
        if dist is not None:
            dist.destroy_process_group()
        return
    if args.workload == "ffhq256":
        cfg_name = "ve/ffhq_256_ncsnpp_continuous"
        if args.batch == 256:
            args.batch = 16
        if args.sde_steps == 1000:
            args.sde_steps = 2000
        args.no_train = args.no_cpu_baseline = args.no_extras = True
    else:
        cfg_name = "ve/cifar10_ncsnpp_continuous"
    sync_all = _sync_factory(dev, dist)
    other = "f32" if args.matrix == "bf16x6" else "bf16x6"
    if world > 1:
        # a multi-GPU run is a scaling point: the headline legs only (no CPU baseline, no other configs, no other matrix mode)
        args.no_extras = args.no_other_matrix = True
    if args.train_only:
        with matrix_mode(args.matrix):
            tr = bench_train(args, _util.cfgs.get_config("ve/cifar10_ncsnpp_continuous"), dev, dist, world, rank, sync_all)
        tr.update(n_gpus=world, scaling="weak", vs_baseline=None, dtype=DTYPE[args.matrix], data="synthetic", rccl_ranks=rccl_ranks,
                  ms_per_step=tr["value"] * 1e3, dist_backend=args.dist_backend if world > 1 else None,
                  rccl_version=_rccl_version(), config={"workload": "configs/ve/cifar10_ncsnpp_continuous DSM training step, batch %d/GPU" % args.train_batch,
                                                        "matrix_mode": args.matrix, "parallelism": "data parallel x%d" % world})
        if args.share_device and world > 1:
            tr["scaling"] = "none: %d ranks share %d GPU(s) over %s -- a functional run of the multi-rank code paths, not a scaling point" \
                % (world, n_dev, args.dist_backend)
        if _TELE is not None:
            tr["telemetry"] = _TELE.report()
        if rank == 0:
            _emit(tr)
        if dist is not None:
            dist.destroy_process_group()
        return
    with matrix_mode(args.matrix):
        res, eng, model, sd, cfg = bench_pc(args, cfg_name, args.batch, args.sde_steps, dev, dist, world, rank, args.steps, args.warmup, True,
                                            leg="sampler", keep_outputs=bool(args.dump_outputs) and rank == 0)
    B, R = args.batch, cfg.data.image_size
    roof = res.pop("_roof", None)
    outputs = res.pop("_outputs", None)
    dumped = dump_outputs(args.dump_outputs, outputs) if outputs is not None else None
    out = {
        "metric": "pc_sampler_images_per_sec", "value": res["value"], "unit": "images/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "prewarm_s": res["prewarm_s"], "ms_per_step": res["ms_per_step"],
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": DTYPE[args.matrix], "data": "synthetic",
        "rccl_ranks": rccl_ranks, "dist_backend": args.dist_backend if world > 1 else None, "rccl_version": _rccl_version(),
        "per_rank_ms_per_step": res["per_rank_ms_per_step"], "rank_spread_max_over_min": res["rank_spread_max_over_min"],
        "config": {"workload": res["workload"], "batch_per_gpu": B, "sde_steps": args.sde_steps, "nfe_per_step": res["nfe_per_step"],
                   "path": res["path"], "state_finite": res["state_finite"], "unet_gflop_per_image": res["unet_gflop_per_image"],
                   "end_to_end_tflops": res["end_to_end_tflops"],
                   "direct_form_ceiling_images_per_sec": res["direct_form_ceiling_images_per_sec"],
                   "matrix_mode": args.matrix, "parallelism": "replicas x%d (no collectives)" % world},
    }
    if dumped is not None:
        out["config"]["dumped_outputs"] = dumped

    if roof is not None:
        # HBM traffic of the dominant kernel: PMC counters cannot be read from inside this process; the figure is the
        # per-launch average of the committed rocprofv3 passes over THIS command with --no-train (tools/profile_gpu.sh ->
        # profiles/*_profile_summary.json: (2*FETCH_SIZE + WRITE_SIZE) * 1024, MI355X_MICROARCH.md HBM section), next to the
        # algorithmic bytes (inputs + output + weights + residual) of the same launches
        traffic = mfma_busy = traffic_parts = None
        try:
            import glob
            summ = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_profile_summary.json")))[-1]
            with open(summ) as f:
                prof = json.load(f)
            traffic = prof["hbm_traffic"][roof["dominant"]]["hbm_bytes_per_launch"]
            if roof["dominant"] == "conv_wino4r_kernel":      # + the transform pass of the same layer (one launch each)
                traffic_parts = {"conv_wino4r_kernel": traffic,
                                 "wino4_xform_vq_kernel": prof["hbm_traffic"]["wino4_xform_vq_kernel"]["hbm_bytes_per_launch"]}
                traffic = sum(traffic_parts.values())
            m = prof.get("mfma", {}).get(roof["dominant"], {})
            if m.get("SQ_VALU_MFMA_BUSY_CYCLES") and m.get("GRBM_GUI_ACTIVE"):
                # 1024 SIMDs; rocprofv3 reports GRBM_GUI_ACTIVE summed over the 8 XCDs
                mfma_busy = m["SQ_VALU_MFMA_BUSY_CYCLES"] / (1024.0 * m["GRBM_GUI_ACTIVE"] / 8.0)
            out["config"]["pmc_source"] = os.path.basename(summ)
            # the counters describe the kernels as they were when the profile was taken: flag them when a source changed since
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import summarize_profile
            out["config"]["pmc_stale"] = prof.get("csrc_sha256") != summarize_profile.csrc_sha()
        except Exception:
            pass
        n3 = int(roof["conv3"].sum())
        n3w = int((roof["conv3"] & roof["wino"]).sum())
        n3w4 = int((roof["conv3"] & roof["wino4"]).sum())
        n3w4g = int((roof["conv3"] & roof["wino4g"]).sum())
        out["roofline"] = {
            "bound": "mfma", "achieved": roof["achieved_exec"], "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
            "frac": roof["achieved_exec"] / PEAK_FP32_MFMA_TFLOPS,
            "achieved_algorithmic": roof["achieved_alg"], "frac_algorithmic": roof["achieved_alg"] / PEAK_FP32_MFMA_TFLOPS,
            "traffic": traffic, "traffic_parts": traffic_parts, "traffic_algorithmic": roof["alg_bytes_wino"], "mfma_busy_pmc": mfma_busy,
            "kernel": "the %d 3x3 convolution launches of one U-Net evaluation: %d as wino4_xform_vq_kernel + conv_wino4r_kernel (Winograd F(4x4,3x3) "
                      "in two kernels, fp32 MFMA, the matrix kernel fed from registers; on 8x8 maps with its reduction split over two workgroups per tile), "
                      "%d on conv_wino4_kernel (F(4x4,3x3) in one kernel), %d on conv_wino_kernel (F(2x2,3x3)), %d on conv_mfma_kernel (direct; "
                      "the 4x4 maps and the 3-channel input end), the image head on conv_small_cout_kernel (vector ALU)"
                      % (n3, n3w4g, n3w4 - n3w4g, n3w - n3w4, n3 - n3w),
            "note": "achieved = EXECUTED matrix FLOPs (F(4x4,3x3) launches at 1/4, F(2x2,3x3) launches at 1/2.25 of their direct-form "
                    "FLOPs) / HIP-event time of those launches; achieved_algorithmic = direct-form FLOPs / the same time; "
                    "traffic = HBM bytes per layer from the PMC passes (%s), traffic_algorithmic = input + output + weights + "
                    "residual of the same layers (op list): what a single fused kernel would have to move" % (
                        "transform pass + matrix kernel, traffic_parts" if roof["dominant"] == "conv_wino4r_kernel" else roof["dominant"]),
            "unet_eval_ms_eager_events": float(roof["ms"].sum()),
            "by_class": roof["by_class"]}
        # what the matrix pipe of THIS device sustains: every SIMD issuing back-to-back fp32 MFMAs on register operands
        # (ssde_mfma_probe), ~5 ms per timed launch.  `peak` above stays the data-sheet figure (2.4 GHz); under load the
        # device settles on a lower clock, and the fractions against the sustained rate are reported beside it.
        try:
            sustained = mfma_probe(dev)
            out["roofline"]["sustained_mfma_probe"] = {
                "tflops": sustained, "implied_clock_ghz": sustained / PEAK_FP32_MFMA_TFLOPS * 2.4,
                "frac_of_sustained": roof["achieved_exec"] / sustained,
                "note": "ssde_mfma_probe: 1 wave per SIMD, 8 independent v_mfma_f32_32x32x2_f32 chains, no LDS / memory traffic"}
        except Exception as exc:                                 # diagnostic only
            out["roofline"]["sustained_mfma_probe"] = {"error": repr(exc)}
        if args.dump_ops:
            up, ms, cls, fl = eng.unet.program, roof["ms"], roof["cls"], roof["fl"]
            rows = []
            for i in range(up.n):
                op = up.ops[i]
                row = {"i": i, "kind": int(op.kind), "cls": int(cls[i]), "ms": float(ms[i]), "gflop": float(fl[i]) / 1e9}
                if op.kind == 1:
                    c = op.u.conv
                    row.update(h=c.h_out, w=c.w_out, cout=c.c_out, cin=c.main.c0 + c.main.c1, caux=c.aux.c0 + c.aux.c1,
                               ks=c.ksize, stride=c.stride, pro=c.main.pro_mode, tile=c.tile)
                    row["tflops"] = row["gflop"] / max(row["ms"], 1e-9)
                rows.append(row)
            with open(args.dump_ops, "w") as f:
                json.dump(rows, f)

    if args.share_device and world > 1:
        out["scaling"] = "none: %d ranks share %d GPU(s) over %s -- a functional run of the multi-rank code paths, not a scaling point" \
            % (world, n_dev, args.dist_backend)
    _phase("sampler done" if roof is None else "sampler + roofline done")
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args, cfg, model, sd, R, args.sde_steps)
        _phase("cpu baseline done")

    del eng, model
    torch.cuda.empty_cache()
    if not args.no_train:
        # second headline quantity of BASELINE.json's metric ("... + sec/train-step"): reported inside the same JSON line
        with matrix_mode(args.matrix):
            tr = bench_train(args, _util.cfgs.get_config("ve/cifar10_ncsnpp_continuous"), dev, dist, world, rank, sync_all)
        out["train"] = tr
        torch.cuda.empty_cache()
        _phase("train step done")
    if not args.no_other_matrix and args.workload == "cifar10":
        # the other matrix mode beside the headline, in the same run: the sampler of the headline mode once more (minutes into
        # the run the device is warmer than it was for the headline), then the other mode, then its training step
        with matrix_mode(args.matrix):
            ra, ea, ma, _, _ = bench_pc(args, "ve/cifar10_ncsnpp_continuous", args.batch, args.sde_steps, dev, dist, world, rank,
                                        args.steps, args.warmup, False, leg="sampler_%s_again" % args.matrix)
        del ea, ma
        torch.cuda.empty_cache()
        with matrix_mode(other):
            rb, eb, mb, _, _ = bench_pc(args, "ve/cifar10_ncsnpp_continuous", args.batch, args.sde_steps, dev, dist, world, rank,
                                        args.steps, args.warmup, False, leg="sampler_" + other)
            by_other = None
            if rank == 0 and not args.no_roofline:         # per-class HIP-event ms of one U-Net evaluation in THIS mode, same process
                by_other = {k: {kk: v[kk] for kk in ("launches", "ms", "frac") if kk in v}
                            for k, v in roofline_of(eb.unet.program, E, L)["by_class"].items()}
            del eb, mb
            torch.cuda.empty_cache()
            mx = {"dtype": DTYPE[other], "matrix_mode": other, "by_class": by_other,
                  "sampler": {k: rb[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup", "state_finite")},
                  "sampler_%s_measured_just_before" % args.matrix: {k: ra[k] for k in ("value", "unit", "ms_per_step")},
                  "headline_mode_over_this_mode": ra["value"] / rb["value"]}
            if not args.no_train:
                a2 = argparse.Namespace(**vars(args))
                a2.no_roofline = a2.no_exchange_probe = True
                a2.train_steps, a2.train_warmup = min(args.train_steps, 30), min(args.train_warmup, 5)
                tb = bench_train(a2, _util.cfgs.get_config("ve/cifar10_ncsnpp_continuous"), dev, dist, world, rank, sync_all,
                                 leg="train_" + other)
                mx["train"] = {k: tb[k] for k in ("value", "unit", "steps", "warmup", "prewarm_s", "loss")}
                torch.cuda.empty_cache()
        out["matrix_" + other] = mx
        _phase("other matrix mode (%s) done" % other)
    if not args.no_extras:
        # the other BASELINE configs, compact, so that a --full run witnesses them
        extra = {}
        with matrix_mode(args.matrix):                # (the other configs run in the headline's matrix mode)
            r3, e3, m3, _, _ = bench_pc(args, "ve/ffhq_256_ncsnpp_continuous", 16, 2000, dev, dist, world, rank, min(args.steps, 5), 2, False,
                                        leg="ffhq256")
            extra["ffhq256"] = r3
            _phase("ffhq256 done")
            del e3, m3
            torch.cuda.empty_cache()
            with tele_leg("subvp_ode"):
                extra["subvp_ode"] = bench_ode_compact(args, dev, dist, world, rank)
            _phase("subvp_ode done")
            torch.cuda.empty_cache()
            # the likelihood of the same config at the config's own tolerance (rtol = atol = 1e-5, likelihood.py:40: ~1600
            # evaluations of forward + input gradient, ~110 s); --likelihood-tol loosens it for quick runs
            with tele_leg("subvp_likelihood"):
                extra["subvp_likelihood"] = bench_likelihood(args, dev, dist, world, rank, tol=args.likelihood_tol)
            _phase("subvp_likelihood done")
        out["extra"] = extra

    if _TELE is not None:
        out["telemetry"] = _TELE.report()
    if rank == 0:
        _emit(out)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
