"""Time one push of the look-ahead streaming encoder (ConformerInterCTC.stream(lookahead=True), nnet.ConformerLookaheadStreamSession) beside one push of the plain
session on the same stack dimensions.

    python tools/bench_encoder_lookahead.py [--rounds N] [--iters N] [--out FILE]

Shape: the audio back-end's real dims ([180, 256, 360], blocks [5, 6, 5], H = 4, K = 15, InterCTC after blocks 3, 6, 10, 13, vocabulary 256) built with plain
RelPos1dMultiHeadAttention and causal depthwise padding; B = 32 utterance slots, Tc = 16 input frames per push.  Two masks: Mask(64, 0), the plain session (16 frames
per push), and Mask(64, 2), the look-ahead session (LAe = 24, a window of W = 40 frames per push).  Legs: one eager push and one push of a captured session
(session.capture(): a graph replay), for each mask, in bf16 and in fp32.  Both masks run in the same process in alternating rounds (plain, look-ahead, plain, ...),
so that clock and thermal drift hit both alike; per leg the min / median / max over the rounds of the mean of --iters back-to-back pushes between HIP events, after
warm-up.  The eager legs include the host's launch chain (that IS their cost per chunk).  One JSON line; no threshold."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_encoder_stream import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import avec_amd
    import nnet
    assert torch.cuda.is_available(), "bench_encoder_lookahead.py measures on the GPU"
    B, Tc, L = 32, 16, 64
    att = {"class": "RelPos1dMultiHeadAttention", "params": dict(num_heads=4, attn_drop_rate=0.0, num_pos_embeddings=10000, weight_init="default", bias_init="default")}
    res = {"tool": "bench_encoder_lookahead", "B": B, "chunk_frames": Tc, "left_context": L, "rounds": args.rounds, "iters": args.iters,
           "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0)}
    x = torch.randn(B, Tc, 180, device="cuda")
    for dtype in ("bf16", "f32"):
        avec_amd.set_compute_dtype(dtype)
        legs = {}
        for name, R in (("plain", 0), ("lookahead", 2)):
            torch.manual_seed(0)
            net = nnet.ConformerInterCTC(dim_model=[180, 256, 360], num_blocks=[5, 6, 5], interctc_blocks=[3, 6, 10, 13], vocab_size=256, att_params=att,
                                         conv_params={"class": "Conv1d", "params": {"padding": "causal", "kernel_size": 15}}, ff_ratio=4, drop_rate=0.1,
                                         mask=nnet.Mask(left_context=L, right_context=R), conv_stride=2).to("cuda").eval()
            eager, graph = net.stream(B, Tc, lookahead=True), net.stream(B, Tc, lookahead=True).capture()
            if R:
                res["lookahead"], res["window"] = eager.lookahead, eager.window
            legs[name + "_eager"], legs[name + "_captured"] = (lambda s=eager: s.push(x)), (lambda s=graph: s.push(x))
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():                                     # plain eager, plain captured, look-ahead eager, look-ahead captured: alternating
                times[k].append(timed(fn, args.iters))
        res[dtype] = {k: {"min_ms": round(min(v), 4), "median_ms": round(statistics.median(v), 4), "max_ms": round(max(v), 4)} for k, v in times.items()}
    avec_amd.set_compute_dtype("f32")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
