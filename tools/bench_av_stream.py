"""Time one push of the audio-visual session (AudioVisualEfficientConformerEncoder.stream(), nnet.AudioVisualStreamSession) beside its parts and beside what a caller
had to do without it: re-run the offline forward over everything heard so far.

    python tools/bench_av_stream.py [--iters N] [--rounds R] [--dtype bf16|f32] [--out FILE]

Shape: the shipped audio-visual encoder's dimensions made causal (video back-end dims [256, 360], blocks [6, 1], InterCTC after 3 and 6; audio back-end dims
[180, 256, 360], blocks [5, 6, 1], InterCTC after 8 and 11; fusion 360 | 360 -> 1440 -> 360; fusion stack 5 blocks of 360, InterCTC after 2; H = 4, K = 15 causal, plain
attention, Mask(left_context=64, right_context=0); vocabulary 256) behind the shipped front-ends on 88x88 frames; B = 32 utterance slots; Tv = 4 video frames per push
(160 ms: 2560 samples, R = 2 rows).  Legs: one combined push eager and captured; the separate audio (.audio_encoder.stream(B, 8)) and visual (.video_encoder.stream(B, 4))
session pushes at the same settings, eager and captured (their sum is reported); the fuse launch alone (ops.av_fuse_stream, R rows in, R pairs out); and the offline
forward over the 16 / 32 / 64 frames heard so far.  All legs run in one process, alternating, --rounds times; each figure is HIP events around --iters back-to-back
calls after warm-up (the eager legs include the host's launch chain: that IS their cost per chunk), reported as [min, median, max] over the rounds.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import avec_amd
    import nnet
    from avec_amd import ops
    assert torch.cuda.is_available(), "bench_av_stream.py measures on the GPU"
    avec_amd.set_compute_dtype(args.dtype)
    torch.manual_seed(0)
    B, L, Tv, HW, V = 32, 64, 4, 88, 256
    att = {"class": "RelPos1dMultiHeadAttention", "params": dict(num_heads=4, attn_drop_rate=0.0, num_pos_embeddings=10000, weight_init="default", bias_init="default")}
    kw = dict(vocab_size=V, att_params=att, conv_params={"class": "Conv1d", "params": {"padding": "causal", "kernel_size": 15}}, ff_ratio=4, drop_rate=0.1, conv_stride=2)
    mask = lambda: nnet.Mask(left_context=L, right_context=0)
    enc = nnet.AudioVisualEfficientConformerEncoder(vocab_size=V)
    enc.video_encoder.back_end = nnet.ConformerInterCTC(dim_model=[256, 360], num_blocks=[6, 1], interctc_blocks=[3, 6], loss_prefix="v_ctc", mask=mask(), **kw)
    enc.audio_encoder.back_end = nnet.ConformerInterCTC(dim_model=[180, 256, 360], num_blocks=[5, 6, 1], interctc_blocks=[8, 11], loss_prefix="a_ctc", mask=mask(), **kw)
    enc.audio_visual_encoder = nnet.ConformerInterCTC(dim_model=360, num_blocks=5, interctc_blocks=[2], loss_prefix="f_ctc", mask=mask(), **kw)
    enc = enc.to("cuda").eval()

    legs = {}
    for mode in ("eager", "captured"):
        ses = enc.stream(B, Tv)
        va, au = enc.video_encoder.stream(B, Tv), enc.audio_encoder.stream(B, 2 * Tv)
        if mode == "captured":
            ses.capture(frame=(HW, HW)), va.capture(frame=(HW, HW)), au.capture()
        v = 0.5 * torch.randn(B, ses.first_frames, HW, HW, device="cuda")
        w = 0.1 * torch.randn(B, ses.first_samples, device="cuda")
        legs["av_push_%s_ms" % mode] = (lambda s=ses, v=v, w=w: s.push(v, w))
        legs["video_push_%s_ms" % mode] = (lambda s=va, v=v: s.push(v))
        legs["audio_push_%s_ms" % mode] = (lambda s=au, w=w: s.push(w))
    R = Tv // 2
    state = ops.av_fuse_stream_state(B, 360, 360, R + 2, "cuda")
    a, b = torch.randn(B, R, 360, device="cuda"), torch.randn(B, R, 360, device="cuda")
    n = torch.full((B,), R, dtype=torch.int64, device="cuda")
    out = ops.av_fuse_stream(a, n, b, n, state, torch.ones(B, dtype=torch.uint8, device="cuda"), R)
    legs["fuse_launch_ms"] = lambda: ops.av_fuse_stream(a, n, b, n, state, None, R, out=out)
    for T in (16, 32, 64):
        x, xl = 0.5 * torch.randn(B, 1, T, HW, HW, device="cuda"), torch.full((B,), T, dtype=torch.int64, device="cuda")
        y, yl = 0.1 * torch.randn(B, 640 * T - 160, device="cuda"), torch.full((B,), 640 * T - 160, dtype=torch.int64, device="cuda")

        def offline(x=x, xl=xl, y=y, yl=yl):
            with torch.no_grad():
                return enc(x, xl, y, yl)
        legs["offline_forward_T%d_ms" % T] = offline
    for fn in legs.values():                       # warm up every shape the timed windows use
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, args.iters if not k.startswith("offline") else max(2, args.iters // 5)))
    for mode in ("eager", "captured"):
        times["audio_plus_video_push_%s_ms" % mode] = [x + y for x, y in zip(times["audio_push_%s_ms" % mode], times["video_push_%s_ms" % mode])]
    res = {"tool": "bench_av_stream", "dtype": args.dtype, "B": B, "Tv": Tv, "R": R, "frame": HW, "left_context": L, "iters": args.iters, "rounds": args.rounds,
           "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "figures": "[min, median, max] ms over the rounds"}
    for k, v_ in times.items():
        res[k] = [round(min(v_), 4), round(statistics.median(v_), 4), round(max(v_), 4)]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
