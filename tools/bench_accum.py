"""Time one OPTIMIZER step with gradient accumulation on one MI355X, three ways, in one process:

    python tools/bench_accum.py [--rounds R] [--iters N] [--batch 16] [--k 4] [--out FILE]

  eager     k eager Model.train_step micro-steps (accumulated_steps = k): what Model.fit runs without use_graphs
  micro     k Model.graphed_micro_step micro-steps: forward + backward replayed from a hipGraph, shadow refresh / optimizer / EMA launches eager behind the last replay
  single    k replays of the existing captured single step (Model.make_graphed_train_step): k optimizer steps on micro-batches -- not the same training, a floor for
            k forward + backward passes from a graph that still pays k Adam launches and k shadow refreshes

on the shipped shape: AV model, bf16, B = 16 clips of 100 frames per micro-batch (the synthetic batch of bench.py), k = 4, dropout and SpecAugment on.  The legs
alternate, each is warmed up, each timing is a host clock around --iters optimizer steps that ends in a device synchronise; minimum and maximum over --rounds rounds
are printed (the spread on a shared box).  `--clip` adds gradient clipping (the norm launches) to eager and micro ONLY: the whole-step
graph of `single` ignores grad_max_norm, so that leg stays an unclipped step (the result row says so: "single_clipped": false).

It also times avec_grad_norm alone on an arena of 61.7 M elements (HIP events around back-to-back launches) against its HBM floor: 4 n bytes over the 8.0 TB/s peak
(6.29 TB/s measured for a float4 copy)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBPS, HBM_COPY_TBPS = 8.0, 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--clip", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_accum.py measures on the GPU"
    import avec_amd
    import bench
    import nnet
    from avec_amd import ops
    dev = torch.device("cuda")
    res = []

    # ---- the norm launch alone
    n = 61_700_000
    g = torch.randn(n, device=dev)
    ws, stats, flag = ops.grad_norm_workspace(n, dev), torch.zeros(2, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    for _ in range(3):
        ops.grad_norm(g, ws, stats, flag, 1.0, 1.0)
    ref = float(g.double().norm())
    times = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            ops.grad_norm(g, ws, stats, flag, 1.0, 1.0)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 20 * 1e3)
    us = min(times)
    row = {"group": "grad_norm", "n": n, "MB": round(4 * n / 1e6, 1), "us": round(us, 1), "max_us": round(max(times), 1), "TBps": round(4 * n / us / 1e6, 2),
           "floor_us_at_peak": round(4 * n / HBM_PEAK_TBPS / 1e6, 1), "floor_us_at_measured_copy_rate": round(4 * n / HBM_COPY_TBPS / 1e6, 1),
           "rel_err_vs_fp64": abs(float(stats[0]) - ref) / ref}
    print(json.dumps(row))
    res.append(row)
    del g

    # ---- one optimizer step, three ways
    k, B = args.k, args.batch
    avec_amd.set_compute_dtype("bf16")
    avec_amd.manual_seed(1234)
    torch.manual_seed(0)
    model = nnet.AudioVisualEfficientConformerInterCTC(vocab_size=256, v_interctc_blocks=[3, 6], a_interctc_blocks=[8, 11], f_interctc_blocks=[2])
    model.compile(losses=nnet.CTCLoss(zero_infinity=True, assert_shorter=False))
    model = model.to(dev).train()
    model.grad_max_norm = args.clip
    batches = [bench.synthetic_batch(B, dev, seed=s) for s in range(k)]
    single = model.make_graphed_train_step(*batches[0], precision=torch.bfloat16, warmup=1)

    def eager():
        acc = 0
        for inp, tgt in batches:
            _, _, acc = model.train_step(inp, tgt, torch.bfloat16, None, k, acc)

    def micro():
        acc = 0
        for inp, tgt in batches:
            _, acc = model.graphed_micro_step(inp, tgt, torch.bfloat16, k, acc)

    def single_k():
        for inp, tgt in batches:
            single(inp, tgt)

    legs = {"eager": eager, "micro": micro, "single": single_k}
    times = {name: [] for name in legs}
    for name, fn in legs.items():                       # warm-up of every leg (micro: the first pass captures)
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.iters * 1e3)
    row = {"group": "optimizer_step", "B": B, "frames": 100, "k": k, "dtype": "bf16", "clip": args.clip, "single_clipped": False, "graphs_cached": model.captured_steps.count("micro")}
    for name, v in times.items():
        row[name + "_ms"], row[name + "_max_ms"] = round(min(v), 2), round(max(v), 2)
    print(json.dumps(row))
    res.append(row)
    avec_amd.set_compute_dtype("f32")
    if args.out:
        with open(args.out, "w") as f:
            for row in res:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
