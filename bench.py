"""Benchmark of the hot path: AV Efficient Conformer training step (forward + 6 CTC losses + backward + gradient all-reduce + Adam)
on synthetic LRS2-shaped batches: B=32 per GPU, audio 63 840 samples (400 mel frames), video 100x88x88, 20 labels.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
                                                             (N>1: one rank per GPU over RCCL -- started by torch.distributed.run, or by bench.py itself
                                                              when it is run as plain `python bench.py --gpus N`)

Prints ONE JSON line (rank 0): whole-job utterances/s and `ms_per_step`, the time of one of the K timed steps.  A plain run sets up, warms up, times the K steps
and prints that line, nothing else.  `--full` adds what takes runs of its own: `roofline` (one row per kernel instance of the MFMA product / convolution families:
what a launch computes comes from an eager, event-bracketed leg run AFTER the timed region -- events cannot be recorded inside the timed hipGraph --, how long it
takes inside the replayed step from the committed rocprofv3 summary of this command, `roofline.timing_source`), the eager step times and `cpu_baseline` (the CPU
oracle on the host cores, bounded sample).

`--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy (see dump_outputs).  The last two timed steps start from the initial weights
and optimizer state, restored outside the timed region: the kernels sum with fp32 atomics in an order that differs from run to run, and in bf16 that rounding
grows with every training step, while two steps from a fixed state differ only by it.  The inputs, the initial weights and the dropout seeds are fixed, so two
builds run with the same arguments can be compared output for output."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

GFLOP_PER_UTT = 214.16          # fwd+bwd, conv/linear/bmm only
PEAK_BF16_TFLOPS = 2500.0       # dense MFMA peak, MI355X_MICROARCH.md
PEAK_F32_TFLOPS = 157.3


def synthetic_batch(B, device, seed):
    g = torch.Generator().manual_seed(seed)
    video = torch.randn(B, 100, 88, 88, 1, generator=g)
    audio = 0.1 * torch.randn(B, 63840, generator=g)
    labels = torch.randint(1, 256, (B, 20), generator=g)
    vlen, alen, llen = torch.full((B,), 100), torch.full((B,), 63840), torch.full((B,), 20)
    return [t.to(device) for t in (video, vlen, audio, alen)], (labels.to(device), llen.to(device))


def cpu_baseline(budget_s=28.0, B=8, thread_counts=(8, 16, 32, 64)):
    """CPU oracle (oracle/avec_oracle.py, a restatement pinned to the reference: tests/golden/check_oracle_fullsize.py) fwd+bwd on the host cores:
    B utterances per pass, a sweep over torch thread counts (small batches oversubscribe a 256-core host: more threads is not faster), best reported
    with the thread count that produced it.  Bounded: one warm-up pass, then one timed pass per thread count while the budget lasts."""
    import nnet
    from oracle import avec_oracle as O
    torch.manual_seed(0)
    model = nnet.AudioVisualEfficientConformerInterCTC()
    sd = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in model.state_dict().items()}
    del model
    g = torch.Generator().manual_seed(0)
    video, audio = torch.randn(B, 100, 88, 88, 1, generator=g), 0.1 * torch.randn(B, 63840, generator=g)
    vlen, alen = torch.full((B,), 100), torch.full((B,), 63840)
    labels, llen = torch.randint(1, 256, (B, 20), generator=g), torch.full((B,), 20)

    def one_pass():
        for v in sd.values():
            v.grad = None
        t0 = time.time()
        out = O.av_forward(sd, video, vlen, audio, alen, train=True, stats_out={})
        O.total_loss(out, labels, llen, O.AV_LOSS_WEIGHTS)["loss"].backward()
        return time.time() - t0

    ncpu = os.cpu_count() or 1
    counts = [t for t in thread_counts if t <= ncpu] or [ncpu]
    before = torch.get_num_threads()
    results, t_start = {}, time.time()
    try:
        torch.set_num_threads(counts[0])
        one_pass()                                       # warm-up (allocator, oneDNN primitive caches)
        for t in counts:
            if results and time.time() - t_start > budget_s:
                break
            torch.set_num_threads(t)
            results[t] = one_pass()
    finally:
        torch.set_num_threads(before)
    best_t = min(results, key=results.get)
    sweep = ", ".join("%d thr: %.2f utt/s" % (t, B / results[t]) for t in sorted(results))
    return {"value": round(B / results[best_t], 3), "unit": "utt/s", "cores": best_t, "kind": "port",
            "sample": "oracle fwd+bwd fp32, one pass of B=%d per thread count after a warm-up pass (%s), %d host cores visible; "
                      "the reference itself measured 1.79 utt/s on 8 Xeon cores at B=2 (BASELINE.md section 3, build container)" % (B, sweep, ncpu)}


def pmc_summary_path():
    """newest committed profiles/rNN_pmc_traffic.json (one per round), or None"""
    import glob
    found = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_traffic.json")))
    return found[-1] if found else None


def pmc_traffic(family):
    """HBM bytes per launch of the dominant GEMM family from the committed rocprofv3 --pmc summary (newest profiles/rNN_pmc_traffic.json, made by
    tools/pmc_traffic.py from separate FETCH_SIZE / WRITE_SIZE passes of this same command; FETCH_SIZE doubled as MI355X_MICROARCH.md
    prescribes for gfx950).  None when the summary is absent or has no kernel of that family."""
    import re
    path = pmc_summary_path()
    if not family or path is None:
        return None
    if family.startswith("conv3x3"):
        ks = [v for k, v in json.load(open(path))["kernels"].items() if "conv3x3_c64_kernel" in k or k.startswith("conv3x3_c64_res_kernel") or k.startswith("wgrad3x3_c64")]
        n = sum(v["launches"] for v in ks)
        return round(sum(v["launches"] * (v["fetch_bytes_per_launch"] + (v["write_bytes_per_launch"] or 0.0)) for v in ks) / n) if n else None
    want_tn = family.startswith("gemm_tn")
    want_mode = {"plain": 0, "conv_fwd": 1, "conv_bwd_data": 2, "conv_wgrad": 1}.get(family[family.find("<") + 1:-1]) if "<" in family else "all"
    if want_mode is None:
        return None
    tot, n = 0.0, 0
    for name, v in json.load(open(path))["kernels"].items():
        m = re.match(r"void (gemm_nt_glds_kernel|gemm_nt_kernel|gemm_tn_kernel|gemm_tn_tr_kernel)<(.*)>\(", name)
        if not m or m.group(1).startswith("gemm_tn") != want_tn:
            continue
        args = [a.strip() for a in m.group(2).split(",")]
        mode = int(args[2] if m.group(1) == "gemm_tn_tr_kernel" else args[3])
        if want_mode != "all" and mode != want_mode:
            continue
        tot += v["launches"] * (v["fetch_bytes_per_launch"] + (v["write_bytes_per_launch"] or 0.0))
        n += v["launches"]
    return round(tot / n) if n else None


def pmc_traffic_kernel(kernel):
    """HBM bytes per launch (fetch + write) of ONE kernel instance from the newest committed rocprofv3 --pmc summary; None when absent"""
    path = pmc_summary_path()
    if not kernel or path is None:
        return None
    norm = lambda s_: s_.replace(" ", "").replace("void", "").replace("false", "0").replace("true", "1").replace(",tr>", ",1>").replace("__hip_bfloat16", "bf16").replace("(anonymousnamespace)::", "")
    want = norm(kernel)
    for name, v in json.load(open(path))["kernels"].items():
        if norm(name).split("(")[0] == want:
            return round(v["fetch_bytes_per_launch"] + (v["write_bytes_per_launch"] or 0.0))
    return None


def graph_kernel_stats():
    """{normalised kernel name: average duration in us} from the newest committed rocprofv3 --kernel-trace --stats summary of THIS command's graph-replayed step
    (profiles/rNN_kernel_stats_final.csv), and the file name; ({}, None) when there is none"""
    import csv
    import glob
    found = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_kernel_stats_final.csv")))
    if not found:
        return {}, None
    norm = lambda s_: s_.replace(" ", "").replace("void", "").replace("false", "0").replace("true", "1").replace(",tr>", ",1>").replace("__hip_bfloat16", "bf16").replace("(anonymousnamespace)::", "").split("(")[0]
    out = {}
    for r in csv.DictReader(open(found[-1])):
        out[norm(r["Name"])] = float(r["AverageNs"]) / 1e3
    return out, os.path.basename(found[-1])


def rows_from_graph_trace(roof, peak):
    """The step that is TIMED is one hipGraph; HIP events cannot be recorded inside it, so the eager leg supplies what a launch computes (kernel instance, algorithmic
    FLOPs and bytes, launches per step) and the committed rocprofv3 summary of the graph replays supplies how long it takes there (the eager, single-stream leg runs
    on a cool chip: its durations are 5-35 % off the replayed ones).  Rows whose kernel is not in the summary keep the live event timing and say so."""
    stats, fname = graph_kernel_stats()
    norm = lambda s_: s_.replace(" ", "").replace("void", "").replace("false", "0").replace("true", "1").replace(",tr>", ",1>").replace("__hip_bfloat16", "bf16").replace("(anonymousnamespace)::", "").split("(")[0]
    if not stats:
        roof["timing_source"] = "live HIP events, eager single-stream leg (no profiles/rNN_kernel_stats_final.csv committed)"
        return roof
    for r in roof["rows"]:
        us = stats.get(norm(r["kernel"]))
        r["avg_us_eager_events"] = r["avg_us"]
        if us is None:
            r["timing"] = "eager events (kernel not in %s)" % fname
            continue
        r["timing"] = fname
        r["avg_us"] = round(us, 2)
        r["ms_per_step"] = round(r["launches_per_step"] * us / 1e3, 3)
        r["tflops"] = round(r["alg_gflop_per_launch"] / us * 1e3, 1)            # GFLOP / us = PFLOP/s
        r["frac"] = round(r["alg_gflop_per_launch"] / us * 1e3 / peak, 4)
    top = max(roof["rows"], key=lambda r: r["ms_per_step"])
    roof.update({"kernel": top["kernel"], "achieved": top["tflops"], "frac": round(top["tflops"] / peak, 5), "launches": top["launches_per_step"],
                 "avg_launch_ms": round(top["avg_us"] / 1e3, 5), "alg_gflop_per_launch": top["alg_gflop_per_launch"], "alg_bytes_per_launch": top["alg_bytes_per_launch"]})
    roof["timing_source"] = ("rows[*].avg_us: average kernel duration inside the graph-replayed step, rocprofv3 --kernel-trace --stats of this command (profiles/%s); "
                             "kernel instance, FLOPs, bytes and launch counts from the eager event-bracketed leg (avg_us_eager_events keeps its timing)" % fname)
    return roof


def initial_state(model):
    """copies of what a training step changes (master weights, BatchNorm buffers), taken before the first step"""
    return model.arena.master.clone(), [b.detach().clone() for b in model.buffers()]


def restore_state(model, state):
    """back to the initial weights, BatchNorm buffers and (zero) Adam moments, in place: the captured graph keeps its addresses"""
    master, bufs = state
    model.arena.master.copy_(master)
    for b, v in zip(model.buffers(), bufs):
        b.copy_(v)
    model.optimizer._flat["exp_avg"].zero_()
    model.optimizer._flat["exp_avg_sq"].zero_()
    model.arena.mark_dirty()
    torch.cuda.synchronize()


def dump_outputs(out_dir, model, losses):
    """What the last timed step handed back: its losses (float64 scalars; they follow the forward pass of the weights that the step before updated, so they
    depend on one whole backward pass and Adam update as well) and the BatchNorm running statistics.  The gradients are not handed back (the Adam kernel clears
    them), and the updated weights are not written: Adam's first update is lr x sign(gradient), so wherever the gradient is rounding noise around zero (biases in
    front of a BatchNorm or a softmax, which do not change the output) a rounding difference flips a whole update."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for k, v in losses.items():
        np.save(os.path.join(out_dir, k + ".npy"), np.array(float(v.detach()), dtype=np.float64))          # loss, loss_<output>
    sd = model.state_dict()
    bn = [sd[k].detach().float().flatten() for k in sd if k.endswith(("running_mean", "running_var"))]
    np.save(os.path.join(out_dir, "bn_running_stats.npy"), torch.cat(bn).cpu().numpy())


def spawn_ranks(n):
    """Re-run this command under torch.distributed.run with `n` ranks on this node (free rendezvous port on 127.0.0.1); rank 0 prints the JSON line."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC only on this driver (RCCL / cross-process device memory)
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--fp8", action="store_true", help="e4m3 operands for the eligible forward Linear products on top of bf16 (BASELINE config 5's arithmetic; DESIGN.md section 15)")
    ap.add_argument("--full", action="store_true", help="also the roofline / eager-step leg and the CPU baseline after the timed steps (runs of their own)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-kernel-timing", action="store_true", help="with --full: skip the roofline / eager-step leg")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed as DIR/<name>.npy")
    ap.add_argument("--eager", action="store_true", help="do not capture the step into a hipGraph")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for single-GPU multi-process debugging)")
    ap.add_argument("--share-gpu", action="store_true", help="debug: every rank uses cuda:0 (with --backend gloo)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    kernel_timing = args.full and not args.no_kernel_timing
    cpu_leg = args.full and not args.no_cpu_baseline
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # (before the HIP runtime starts) dmabuf IPC: RCCL and the peer exchange buffers need it on this driver

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))          # plain `python bench.py --gpus N`: start one rank per GPU ourselves (the reference self-spawns too, main.py:179-190)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, "WORLD_SIZE=%d but --gpus %d: launch one rank per GPU (torch.distributed.run --nproc-per-node %d, or plain python bench.py --gpus %d)" % (world, args.gpus, args.gpus, args.gpus)
    if args.share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    single_dist = world == 1 and os.environ.get("AVEC_DIST_SINGLE", "0") == "1"       # a one-rank RCCL group through every data-parallel code path (tests / tools/gpu/r4_rccl.sh)
    if world > 1 or single_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29561")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", init_method="env://", device_id=device)
        else:
            dist.init_process_group(backend=args.backend, init_method="env://")

    import avec_amd
    import nnet
    from avec_amd import ops
    avec_amd.set_compute_dtype(args.dtype)
    if args.fp8:
        from avec_amd import fp8
        fp8.enable(True)
    avec_amd.manual_seed(1234 + rank)
    torch.manual_seed(0)
    model = nnet.AudioVisualEfficientConformerInterCTC(vocab_size=256, v_interctc_blocks=[3, 6], a_interctc_blocks=[8, 11], f_interctc_blocks=[2])
    model.compile(losses=nnet.CTCLoss(zero_infinity=True, assert_shorter=False))
    model = model.to(device).train()
    if world > 1 or single_dist:
        model.distribute_strategy(local_rank)
        world_dist = True
    else:
        world_dist = False
    inputs, targets = synthetic_batch(args.batch, device, seed=rank)
    state0 = initial_state(model) if args.dump_outputs else None
    precision = torch.bfloat16 if args.dtype == "bf16" else torch.float32

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    # The step is captured into a hipGraph (same launches, one submission).  Data parallel: forward + backward are captured when the SyncBatchNorm statistics
    # travel by peer-write kernels (avec_amd/peer.py; verified at start-up on this node), the RCCL gradient all-reduce and the Adam launch follow each replay;
    # without the peer exchange (refused IPC, gloo debugging on CPU tensors, ...) the step runs eagerly.
    from avec_amd import peer
    use_graph = not args.eager and (not world_dist or peer.active() is not None or args.backend == "nccl")      # (RCCL collectives are capturable: SyncBatchNorm falls back to them inside the graph)
    graphed = None
    if use_graph:
        try:
            graphed = model.make_graphed_train_step(inputs, targets, precision=precision, warmup=min(max(args.warmup, 1), 3))
        except Exception as e:                                   # (multi-GPU: all ranks must take the same path, see the agreement below)
            if world == 1:
                raise
            print("[bench] rank %d: graph capture of the data-parallel step failed (%s: %s); falling back to eager steps" % (rank, type(e).__name__, e), file=sys.stderr, flush=True)
            graphed = None
        if world > 1:
            ok = torch.tensor([int(graphed is not None)], dtype=torch.int32, device=device if args.backend == "nccl" else "cpu")
            torch.distributed.all_reduce(ok, op=torch.distributed.ReduceOp.MIN)
            if int(ok.item()) == 0:
                graphed = None
        use_graph = graphed is not None
    # which path the timed steps take (a fallback shows here instead of as a silently slower number)
    if use_graph:
        if not world_dist:
            step_path, fallback = "one hipGraph: shadow refresh + forward + losses + backward + Adam", None
        elif getattr(graphed, "collectives_in_graph", False):
            step_path, fallback = "one hipGraph incl. SyncBatchNorm exchanges, range-wise RCCL gradient all-reduce and Adam", (None if peer.active() is not None else "SyncBatchNorm statistics over RCCL (peer exchange unavailable)")
        else:
            step_path, fallback = "hipGraph forward + backward; RCCL gradient all-reduce + Adam after each replay", "collectives outside the graph"
    else:
        step_path, fallback = "eager launches", (None if args.eager else "graph capture unavailable: eager steps")
    if use_graph:
        run_step = lambda: graphed()
    else:
        run_step = lambda: model.train_step(inputs, targets, precision=precision)[0]
    last = None
    for _ in range(args.warmup):
        last = run_step()
    barrier()

    def timed(n):
        t0 = time.perf_counter()
        out = None
        for _ in range(n):
            out = run_step()
        barrier()
        return time.perf_counter() - t0, out

    if args.dump_outputs:
        # the last two timed steps start from the initial state (module docstring); the restore itself is not timed
        tail = min(args.steps, 2)
        elapsed, last = timed(args.steps - tail)
        restore_state(model, state0)
        barrier()
        t_tail, last = timed(tail)
        elapsed += t_tail
        if rank == 0:
            dump_outputs(args.dump_outputs, model, last)
    else:
        elapsed, last = timed(args.steps)
    if kernel_timing:
        # roofline leg: the same step, eagerly, with HIP events around every GEMM-family launch (events cannot be recorded inside a graph).
        # Every rank runs it (the step contains collectives); only rank 0 records events.
        # The audio branch's second stream is switched off for this leg, so that an event pair brackets exactly one kernel.
        from avec_amd import runtime as rt
        rt.set_branch_streams(False)
        ops.KERNEL_TIMER.reset(enabled=(rank == 0))
        timed_steps = min(args.steps, 3)
        te0 = time.perf_counter()
        for _ in range(timed_steps):
            model.train_step(inputs, targets, precision=precision)
        barrier()
        eager_ms = 1000 * (time.perf_counter() - te0) / timed_steps      # eager, single-stream, event-instrumented step: an upper bound of the eager fallback's cost
        ops.KERNEL_TIMER.enabled = False
        rt.set_branch_streams(os.environ.get("AVEC_BRANCH_STREAMS", "1") != "0")
        # what a capture fallback would cost: the same step as plain launches, two streams, no instrumentation (the data-parallel path drops to this on every rank when
        # one rank cannot capture)
        for _ in range(2):
            model.train_step(inputs, targets, precision=precision)
        barrier()
        te1 = time.perf_counter()
        for _ in range(timed_steps):
            model.train_step(inputs, targets, precision=precision)
        barrier()
        eager2_ms = 1000 * (time.perf_counter() - te1) / timed_steps
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t)
    loss = float(last["loss"].detach())
    if world > 1 and peer.active() is not None:
        peer.active().check()                # a rank that never arrived at a SyncBatchNorm exchange: say so (its sums were NaN)
    assert loss == loss and abs(loss) < 1e6, "training step produced a non-finite loss"

    if rank == 0:
        utt = world * args.batch * args.steps
        value = utt / elapsed
        peak = PEAK_BF16_TFLOPS if args.dtype == "bf16" else PEAK_F32_TFLOPS
        roof = ops.KERNEL_TIMER.summary(peak, steps=timed_steps) if kernel_timing else None
        if roof is not None and args.dtype == "bf16" and args.batch == 32 and use_graph and world == 1:
            roof = rows_from_graph_trace(roof, peak)
        if roof is not None and args.dtype == "bf16" and args.batch == 32:
            roof["traffic"] = pmc_traffic_kernel(roof["kernel"])
            for r in roof["rows"]:                   # per row: measured HBM bytes (PMC summary) next to the algorithmic bytes -> the wasted-traffic ratio is explicit
                r["traffic"] = pmc_traffic_kernel(r["kernel"])
                r["traffic_over_alg"] = round(r["traffic"] / r["alg_bytes_per_launch"], 2) if (r["traffic"] and r["alg_bytes_per_launch"]) else None
            roof["traffic_unit"] = "bytes per launch (rocprofv3 PMC, profiles/%s)" % os.path.basename(pmc_summary_path() or "none")
        out = {
            "metric": "AV utterances/sec fwd+bwd (audio T=400, video 100x88x88)", "value": round(value, 2), "unit": "utt/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1000 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype + ("+fp8(e4m3) forward Linear operands" if args.fp8 else ""), "data": "synthetic",
            "config": {"workload": "AV EffConfInterCTC (LRS23/AV) training step: fwd + 6 CTC losses + bwd + grad all-reduce + Adam; "
                                   "batch %d/GPU, audio 63840 samples (400 mel frames), video 100x88x88, 20 labels; dropout 0.1 + SpecAugment on" % args.batch,
                       "global_batch": world * args.batch, "parallelism": "dp%d" % world, "hipgraph": bool(use_graph), "step_path": step_path, "fallback": fallback, "syncbn_exchange": ("peer-write kernels over xGMI" if (world > 1 and peer.active() is not None) else ("torch.distributed" if world > 1 else None)), "params": 61738836, "loss": round(loss, 4),
                       "model_mfma_util": round(value * GFLOP_PER_UTT / 1e3 / peak, 5),
                       "eager_instrumented_ms_per_step": (round(eager_ms, 2) if kernel_timing else None),
                       "eager_two_stream_ms_per_step": (round(eager2_ms, 2) if kernel_timing else None),
                       "notes": "parity: every module against fixtures generated from the reference (tests/golden); the mel front-end is pinned to a restatement of "
                                "torchaudio's documented MelSpectrogram defaults only (torchaudio is not part of /root/reference: tests/golden/ref_shims.py). "
                                "bf16 gradient parity (tests/test_gpu_round2.py, test_gpu_round4.py: every gradient tensor of the timed B=32 graph against the oracle) is enforced as "
                                "|err| <= 1.5 x (error of torch CPU autocast on the same tensor) + 0.02 relative, capped at 0.15 (front-end tensors exempt from the cap); north_star's 1e-3 "
                                "is met in fp32 mode (B=2, test_full_model_grads_match_oracle).  roofline: see timing_source; grouped weight-gradient launches are cut by queue length in "
                                "the eager leg (7 launches) and by stream in the graph (8)"},
            "roofline": roof,
        }
        if world == 1 and cpu_leg:
            out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out))
    if world > 1 or single_dist:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
