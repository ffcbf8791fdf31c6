"""Time the Transformer-LM rescoring pass at the evaluation shape: GPT-Small (12 x 768, 12 heads of 64, V = 1025), B = 32 utterances x beam 16 = 512 hypotheses,
L in {16, 32, 64} tokens, fp32 and bf16.

    python tools/bench_rescore.py [--iters N] [--out FILE]

Legs per (dtype, L), HIP events around --iters calls after warm-up (seeded weights, random ids, all hypotheses of full length):
  fused     model.score: embedding -> block stack -> head + log-softmax + gather in one kernel (avec_lm_head_nll), logits never written
  unfused   the same scoring through the materialised logits: model.forward -> log_softmax -> gather -> masked sum on the device (torch)
  stack     embedding + block stack + final LayerNorm alone (what both paths share)
and ops.ctc_beam_search alone (B = 32, T = 100, V = 256, beam 16, no LM) for scale.  FLOP counts are computed from the shapes:
2 * (parameters of the block stack and head) * rows for the products plus 4 * L * D per row for attention, halved by causality; `mfma_tflops` is that count over the
fused time (an end-to-end rate of the pass, not a kernel's share of peak)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def time_device(fn, iters):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import avec_amd
    import nnet
    import ctc_beam_oracle as CO
    import make_synthetic_lm_assets as A
    from avec_amd import ops
    assert torch.cuda.is_available(), "bench_rescore.py measures on the GPU"
    N, V, D, NB = 512, 1025, 768, 12
    model = A.draw_weights(nnet.GPT(vocab_size=V, padding_idx=0, model="GPT-Small", pos_embedding=nnet.SinPosEmbedding), seed=0)
    model = model.eval().requires_grad_(False).cuda()
    stack_params = NB * (4 * D * D + 8 * D * D)
    res = {"N": N, "V": V, "rows": []}
    g = torch.Generator().manual_seed(0)
    for dtype in ("f32", "bf16"):
        avec_amd.set_compute_dtype(dtype)
        for L in (16, 32, 64):
            ids = torch.randint(1, V - 1, (N, L), generator=g).cuda()
            lens = torch.full((N,), L, dtype=torch.int64).cuda()

            def unfused():
                lp = model(ids).log_softmax(-1)
                return -lp[:, :-1].gather(2, ids[:, 1:, None])[:, :, 0].sum(1)
            with torch.no_grad():
                a, b = model.score(ids, lens), unfused()
                agree = float(((a - b).abs() / b.abs()).max())
                fused_ms = time_device(lambda: model.score(ids, lens), args.iters)
                unfused_ms = time_device(unfused, args.iters)
                stack_ms = time_device(lambda: model._rows(ids, lens), args.iters)
            R = N * L
            flop = 2.0 * (stack_params + D * V) * R + NB * 4.0 * D * L * R / 2
            row = {"dtype": dtype, "L": L, "fused_ms": fused_ms, "unfused_ms": unfused_ms, "stack_ms": stack_ms, "fused_over_unfused": fused_ms / unfused_ms,
                   "head_fused_ms": fused_ms - stack_ms, "head_unfused_ms": unfused_ms - stack_ms, "gflop": flop / 1e9, "mfma_tflops": flop / fused_ms / 1e9,
                   "logits_bytes_not_written": R * V * 4, "fused_vs_unfused_max_rel_diff": agree}
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
    avec_amd.set_compute_dtype("f32")
    logits = torch.from_numpy(CO.ctc_like_logits(32, 100, 256, seed=0)).cuda()
    blens = torch.full((32,), 100, dtype=torch.int64).cuda()
    res["ctc_beam_search_ms"] = time_device(lambda: ops.ctc_beam_search(logits, blens, 16), args.iters)
    print(json.dumps({"ctc_beam_search_ms": res["ctc_beam_search_ms"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
