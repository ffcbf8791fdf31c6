"""Time one push of the streamed visual front-end (VisualEfficientConformerEncoder.stream_front(), nnet.VisualFrontStreamSession) and of the combined session
(.stream(): front + causal stack + head) beside what a caller had to do without them: re-run the offline front-end over every frame heard so far.

    python tools/bench_video_stream.py [--iters N] [--rounds R] [--dtype bf16|f32] [--out FILE]

Shape: the shipped visual front-end (Conv3d stem + BatchNorm3d + ReLU + max pool, ResNet-18, Linear 512 -> 256) on 88x88 frames in front of the visual back-end's
dimensions made causal (dims [256, 360], blocks [6, 6], H = 4, K = 15 causal, plain attention, Mask(left_context=64, right_context=0), InterCTC after blocks 3, 6, 9,
vocabulary 256); B = 32 utterance slots; Tc = 4 frames per push (160 ms of video).  Legs: one front push eager and captured, the stem launch alone
(ops.video_stem_stream on the session's state, Tmax = Tc + 2), the ResNet + Linear alone on the B * Tc frames of a push, one combined push eager and captured; and the
offline front-end (forward_front) over the 16 / 32 / 64 / 128 frames heard so far.  All legs run in one process, alternating, --rounds times; each figure is HIP
events around --iters back-to-back calls after warm-up (the eager legs include the host's launch chain: that IS their cost per chunk), reported as
[min, median, max] over the rounds.  One JSON line."""
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
    assert torch.cuda.is_available(), "bench_video_stream.py measures on the GPU"
    avec_amd.set_compute_dtype(args.dtype)
    torch.manual_seed(0)
    B, L, Tc, HW = 32, 64, 4, 88
    att = {"class": "RelPos1dMultiHeadAttention", "params": dict(num_heads=4, attn_drop_rate=0.0, num_pos_embeddings=10000, weight_init="default", bias_init="default")}
    enc = nnet.VisualEfficientConformerEncoder(vocab_size=256, num_blocks=[1, 1], interctc_blocks=[])
    enc.back_end = nnet.ConformerInterCTC(dim_model=[256, 360], num_blocks=[6, 6], interctc_blocks=[3, 6, 9], vocab_size=256, att_params=att,
                                          conv_params={"class": "Conv1d", "params": {"padding": "causal", "kernel_size": 15}}, ff_ratio=4, drop_rate=0.1,
                                          mask=nnet.Mask(left_context=L, right_context=0), conv_stride=2)
    enc.head = nnet.Linear(360, 256)
    enc = enc.to("cuda").eval()

    legs = {}
    for name, make in (("front", enc.stream_front), ("combined", enc.stream)):
        for mode in ("eager", "captured"):
            ses = make(B, Tc)
            if mode == "captured":
                ses.capture(frame=(HW, HW))
            v = 0.5 * torch.randn(B, ses.first_frames, HW, HW, device="cuda")
            legs["%s_push_%s_ms" % (name, mode)] = (lambda s=ses, v=v: s.push(v))
    probe = enc.stream_front(B, Tc)
    v = 0.5 * torch.randn(B, probe.first_frames, HW, HW, device="cuda")
    probe.push(v)
    probe.push(v)                                  # (every slot past its start: the stem launch below reads the ring and yields Tc frames per slot)
    conv = enc.front_end[0].layers[0][0]
    legs["stem_launch_ms"] = lambda: ops.video_stem_stream(v, probe.state["ring"], probe.w8, conv.bias, probe.ss, probe.nframes, probe.reset_flags, probe.last_flags, Tmax=Tc + 2)
    frames = probe._frames[:Tc].reshape(Tc * B, *probe._frames.shape[2:]).clone()

    def resnet():
        with torch.no_grad():
            return enc.front_end[3].forward_nhwc(frames)
    legs["resnet_linear_BTc_ms"] = resnet
    for T in (16, 32, 64, 128):
        x = 0.5 * torch.randn(B, 1, T, HW, HW, device="cuda")

        def offline(x=x):
            with torch.no_grad():
                return enc.forward_front(x)
        legs["offline_front_T%d_ms" % T] = offline
    for fn in legs.values():                       # warm up every shape the timed windows use
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, args.iters if not k.startswith("offline") else max(2, args.iters // 5)))
    res = {"tool": "bench_video_stream", "dtype": args.dtype, "B": B, "Tc": Tc, "frame": HW, "left_context": L, "iters": args.iters, "rounds": args.rounds,
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
