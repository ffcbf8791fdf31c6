"""Time one push of the streamed audio front-end (AudioEfficientConformerEncoder.stream_front(), nnet.AudioFrontStreamSession) and of the combined session
(.stream(): front + causal stack + head) beside what a caller had to do without them: re-run the offline front-end over every sample heard so far.

    python tools/bench_audio_stream.py [--iters N] [--rounds R] [--dtype bf16|f32] [--out FILE]

Shape: the shipped audio front-end (80 mel bins, Conv2d 1 -> 180 + BatchNorm2d + Swish, Linear 7200 -> 180) in front of the back-end of tools/bench_encoder_stream.py
(dims [180, 256, 360], blocks [5, 6, 5], H = 4, K = 15 causal, plain attention, Mask(left_context=64, right_context=0), InterCTC after blocks 3, 6, 10, 13, vocabulary
256); B = 32 utterance slots; Tc = 4 and 16 frames per push (1280 / 5120 samples).  Legs per Tc: one front push eager and captured, one combined push eager and
captured; and the offline front-end (AudioPreprocessing + stem + Linear) over the 64 / 128 / 256 / 512 frames (320 samples each) heard so far.  All legs run in one
process, alternating, --rounds times; each figure is HIP events around --iters back-to-back calls after warm-up (the eager legs include the host's launch chain: that
IS their cost per chunk), reported as [min, median, max] over the rounds.  One JSON line."""
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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import avec_amd
    import nnet
    from avec_amd import ops
    assert torch.cuda.is_available(), "bench_audio_stream.py measures on the GPU"
    avec_amd.set_compute_dtype(args.dtype)
    torch.manual_seed(0)
    B, L = 32, 64
    att = {"class": "RelPos1dMultiHeadAttention", "params": dict(num_heads=4, attn_drop_rate=0.0, num_pos_embeddings=10000, weight_init="default", bias_init="default")}
    enc = nnet.AudioEfficientConformerEncoder(vocab_size=256, num_blocks=[1, 1, 1], interctc_blocks=[], att_type="regular")
    enc.back_end = nnet.ConformerInterCTC(dim_model=[180, 256, 360], num_blocks=[5, 6, 5], interctc_blocks=[3, 6, 10, 13], vocab_size=256, att_params=att,
                                          conv_params={"class": "Conv1d", "params": {"padding": "causal", "kernel_size": 15}}, ff_ratio=4, drop_rate=0.1,
                                          mask=nnet.Mask(left_context=L, right_context=0), conv_stride=2)
    enc = enc.to("cuda").eval()
    stem = enc.subsampling_module.layers[0]

    def offline_front(x, lens):
        with torch.no_grad():
            mel, _ = enc.audio_preprocessing(x, lens)
            return ops.linear(ops.AudioStemFn.apply(mel, stem[0].weight, stem[0], stem[1], False), enc.linear.weight, enc.linear.bias)

    legs = {}
    for Tc in (4, 16):
        for name, make in (("front", enc.stream_front), ("combined", enc.stream)):
            for mode in ("eager", "captured"):
                ses = make(B, Tc)
                if mode == "captured":
                    ses.capture()
                w = 0.1 * torch.randn(B, ses.first_samples, device="cuda")
                legs["%s_push_Tc%d_%s_ms" % (name, Tc, mode)] = (lambda s=ses, w=w: s.push(w))
    for T in (64, 128, 256, 512):
        x = 0.1 * torch.randn(B, 320 * T, device="cuda")
        lens = torch.full((B,), 320 * T, dtype=torch.int64, device="cuda")
        legs["offline_front_T%d_ms" % T] = (lambda x=x, lens=lens: offline_front(x, lens))
    for fn in legs.values():                       # warm up every shape the timed windows use
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, args.iters))
    res = {"tool": "bench_audio_stream", "dtype": args.dtype, "B": B, "left_context": L, "iters": args.iters, "rounds": args.rounds,
           "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "figures": "[min, median, max] ms over the rounds"}
    for k, v in times.items():
        res[k] = [round(min(v), 4), round(statistics.median(v), 4), round(max(v), 4)]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
