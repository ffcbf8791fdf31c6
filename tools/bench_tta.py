"""Time the three pieces of test-time augmentation, each beside what it replaces, in one process:

    python tools/bench_tta.py [--rounds R] [--out FILE]

  forward  one augmented eval forward of VisualEfficientConformerInterCTC(test_augments=RandomHorizontalFlip(p=1.0)) (one encoder pass over 2 B clips) against two
           plain eval forwards of the same model, of the clips and of the mirrored clips (the reference's two passes, the flip included): B = 16, 100 frames, bf16
  clips    avec_video_tta_batch (n = 2, one flip) against torch.flip plus the interleaving copy, on the same (16, 100, 88, 88, 1) clips
  decode   CTCBeamSearchDecoder.decode_augmented (with and without timestamps) against beam_search: B = 16, n = 2, T = 50, V = 256, beam 16, no LM

forward and clips are device times (HIP events around back-to-back calls after warm-up); forward_enqueue is the host time to enqueue the same calls without
waiting for them (a leg whose two figures agree is bound by the host's launch rate); decode ends in a device-to-host copy, so it is a host clock around whole calls.
The legs of a group alternate and the whole thing is repeated --rounds times: the minimum and the maximum over the rounds are printed (the spread on a shared box).  Before anything is timed the augmented logits are compared with the two plain forwards."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    return e0.elapsed_time(e1) / iters * 1e3          # microseconds


def time_host(fn, iters):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()                                           # (every leg ends in a device-to-host copy)
    return (time.perf_counter() - t0) / iters * 1e6


def time_enqueue(fn, iters):
    """host time to ENQUEUE one call (no synchronise inside the window): where it equals the device-event time of the same leg, that leg is bound by the host's
    launch rate, not by the device"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    dt = (time.perf_counter() - t0) / iters * 1e6
    torch.cuda.synchronize()
    return dt


def run_group(name, shape, fns, timer, iters, rounds):
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timer(fn, iters))
    row = dict({"group": name}, **shape)
    for k, v in times.items():
        row[k + "_us"], row[k + "_max_us"] = round(min(v), 1), round(max(v), 1)
    print(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "bench_tta.py measures on the GPU"
    import avec_amd
    import ctc_beam_oracle as CO
    import nnet
    from avec_amd import ops
    from avec_amd.compat import torchvision_fallback as tv
    res = []
    B, F = args.batch, args.frames

    # ---- forward
    torch.manual_seed(0)
    flip = tv.RandomHorizontalFlip(p=1.0)
    model = nnet.VisualEfficientConformerInterCTC(test_augments=flip)
    model.compile(losses=None)
    model = model.to(torch.device("cuda")).eval()
    torch.manual_seed(1)
    video, vlen = torch.randn(B, F, 88, 88, 1).cuda(), torch.full((B,), F, dtype=torch.int64).cuda()
    avec_amd.set_compute_dtype("bf16")

    def augmented():
        model.test_augments = [flip]
        with torch.no_grad():
            return model([video, vlen])["outputs"][0]

    def two_plain():
        model.test_augments = None
        with torch.no_grad():
            return model([video, vlen])["outputs"][0], model([video.flip(3), vlen])["outputs"][0]

    a, (p0, p1) = augmented().float(), two_plain()
    err = [float((a[:, k] - p.float()).abs().max() / p.float().abs().max()) for k, p in enumerate((p0, p1))]
    print(json.dumps({"group": "forward_check", "dtype": "bf16", "rel_err_unaugmented": err[0], "rel_err_mirrored": err[1]}))
    fwd = {"augmented_one_pass": augmented, "two_plain_passes": two_plain}
    res.append(run_group("forward", {"B": B, "frames": F, "dtype": "bf16"}, fwd, time_device, 10, args.rounds))
    res.append(run_group("forward_enqueue", {"B": B, "frames": F, "dtype": "bf16"}, fwd, time_enqueue, 10, args.rounds))
    avec_amd.set_compute_dtype("f32")

    # ---- clips
    def torch_clips():
        return torch.stack([video, video.flip(3)], dim=1).flatten(0, 1)
    assert torch.equal(ops.video_tta_batch(video, 2, 0b10), torch_clips())
    mb = video.numel() * 4 * 3 / 1e6                  # read once, written twice
    row = run_group("clips", {"B": B, "frames": F, "algorithmic_MB": round(mb, 1)}, {"video_tta_batch": lambda: ops.video_tta_batch(video, 2, 0b10), "torch_flip_stack": torch_clips},
                    time_device, 50, args.rounds)
    row["video_tta_batch_GBps"] = round(mb / 1e3 / (row["video_tta_batch_us"] * 1e-6), 1)
    res.append(row)
    del model, video

    # ---- decode
    c = dict(B=16, n=2, T=50, V=256, W=16)
    logits = torch.from_numpy(np.stack([CO.ctc_like_logits(c["B"], c["T"], c["V"], seed=7 + k) for k in range(c["n"])], 1)).cuda()
    lens = torch.full((c["B"], c["n"]), c["T"], dtype=torch.int64).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dec = nnet.CTCBeamSearchDecoder(beam_size=c["W"], test_time_aug=True)
    assert dec.decode_augmented((logits, lens))[0] == dec.beam_search(logits, lens)
    res.append(run_group("decode", c, {"beam_search": lambda: dec.beam_search(logits, lens), "decode_augmented": lambda: dec.decode_augmented((logits, lens)),
                                       "decode_augmented_timestamps": lambda: dec.decode_augmented((logits, lens), timestamps=True)}, time_host, 20, args.rounds))
    if args.out:
        with open(args.out, "w") as f:
            for row in res:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
