"""Time one push of the streaming encoder (ConformerInterCTC.stream(), nnet.ConformerStreamSession) beside what a caller had to do without it: re-run the offline
forward over every frame heard so far.

    python tools/bench_encoder_stream.py [--iters N] [--dtype bf16|f32] [--out FILE]

Shape: the audio back-end's real dims ([180, 256, 360], blocks [5, 6, 5], H = 4, K = 15, InterCTC after blocks 3, 6, 10, 13, vocabulary 256) built with plain
RelPos1dMultiHeadAttention, causal depthwise padding and Mask(left_context=64, right_context=0); B = 32 utterance slots, Tc = 16 input frames per push (total stride 4:
4 output frames).  Legs: one eager push, one push of a captured session (session.capture(): a graph replay), and the offline eval forward at T = 64, 128, 256, 512
frames -- the cost of the same new chunk for a caller who has heard T frames.  Times are HIP events around --iters back-to-back calls after warm-up, so the eager legs
include the host's launch chain (that IS their cost per chunk).  One JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warm=5):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import avec_amd
    import nnet
    assert torch.cuda.is_available(), "bench_encoder_stream.py measures on the GPU"
    avec_amd.set_compute_dtype(args.dtype)
    torch.manual_seed(0)
    B, Tc, L = 32, 16, 64
    att = {"class": "RelPos1dMultiHeadAttention", "params": dict(num_heads=4, attn_drop_rate=0.0, num_pos_embeddings=10000, weight_init="default", bias_init="default")}
    net = nnet.ConformerInterCTC(dim_model=[180, 256, 360], num_blocks=[5, 6, 5], interctc_blocks=[3, 6, 10, 13], vocab_size=256, att_params=att,
                                 conv_params={"class": "Conv1d", "params": {"padding": "causal", "kernel_size": 15}}, ff_ratio=4, drop_rate=0.1,
                                 mask=nnet.Mask(left_context=L, right_context=0), conv_stride=2).to("cuda").eval()
    x = torch.randn(B, Tc, 180, device="cuda")
    res = {"tool": "bench_encoder_stream", "dtype": args.dtype, "B": B, "chunk_frames": Tc, "left_context": L, "iters": args.iters,
           "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0)}
    eager = net.stream(B, Tc)
    res["push_eager_ms"] = round(timed(lambda: eager.push(x), args.iters), 4)
    graph = net.stream(B, Tc).capture()
    res["push_captured_ms"] = round(timed(lambda: graph.push(x), args.iters), 4)
    with torch.no_grad():
        for T in (64, 128, 256, 512):
            xt = torch.randn(B, T, 180, device="cuda")
            lens = torch.full((B,), T, dtype=torch.int64, device="cuda")
            res["offline_T%d_ms" % T] = round(timed(lambda: net(xt, lens), max(args.iters // 3, 5), warm=2), 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
