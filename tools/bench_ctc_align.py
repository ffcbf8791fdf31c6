"""Time one launch of the CTC forced alignment (avec_ctc_align) beside one launch of avec_ctc_loss (forward + gradient) at the same shape:

    python tools/bench_ctc_align.py [--iters N] [--rounds R] [--out FILE]

Shapes: the evaluation batch B = 32, T = 100, V = 256, Lmax = 40 (all-LDS tier and workspace tier) and the 15 s clips B = 8, T = 376, V = 256, Lmax = 130
(workspace tier only).  Logits carry +6 along a random monotone alignment of each target (tests/ctc_align_oracle.py), full lengths.  Every leg is called through the
C ABI on preallocated buffers, so a figure is the device time of one launch: HIP events around --iters back-to-back launches after warm-up, the legs of a shape
alternated and the whole thing repeated --rounds times (the minimum and the maximum over the rounds are printed: the spread on a shared box)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def time_device(fn, iters):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # microseconds


def legs(B, T, V, Lmax, seed):
    import numpy as np
    import torch
    import ctc_align_oracle as O
    from avec_amd.lib import lib
    tg_np, tl_np = O.random_targets(B, Lmax, V, seed, lens=np.full(B, Lmax))
    il_np = np.full(B, T, dtype=np.int64)
    x = torch.from_numpy(O.aligned_logits(T, V, tg_np, tl_np, il_np, seed + 1)).cuda()
    il, tl = torch.from_numpy(il_np).cuda(), torch.from_numpy(tl_np).cuda()
    tg = torch.from_numpy(np.where((tg_np < 0) | (tg_np >= V), 1, tg_np)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(lib.raw("avec_ctc_align_workspace_bytes")(B, T, Lmax), dtype=torch.uint8, device="cuda")
    path = torch.empty(B, T, dtype=torch.int32, device="cuda")
    spans = torch.empty(B, Lmax, 2, dtype=torch.int32, device="cuda")
    score, tlp = torch.empty(B, device="cuda"), torch.empty(B, Lmax, device="cuda")
    nll, mean, grad = torch.empty(B, device="cuda"), torch.zeros((), device="cuda"), torch.empty(B, T, V, device="cuda")
    lws = torch.empty(lib.raw("avec_ctc_workspace_floats")(B, T, Lmax), device="cuda")

    def align(tier):
        return lambda: lib.ctc_align(x.data_ptr(), il.data_ptr(), tg.data_ptr(), tl.data_ptr(), B, T, V, Lmax, 0, tier, ws.data_ptr(), ws.numel(),
                                     path.data_ptr(), spans.data_ptr(), score.data_ptr(), tlp.data_ptr(), st)
    out = {}
    if lib.raw("avec_ctc_align_fits_lds")(T, Lmax):
        out["align_lds_us"] = align(1)
    out["align_workspace_us"] = align(2)
    out["ctc_loss_fwd_bwd_us"] = lambda: lib.ctc_loss(x.data_ptr(), il.data_ptr(), tg.data_ptr(), tl.data_ptr(), nll.data_ptr(), mean.data_ptr(), grad.data_ptr(),
                                                      lws.data_ptr(), B, T, V, Lmax, 0, 1, st)
    out["ctc_loss_fwd_us"] = lambda: lib.ctc_loss(x.data_ptr(), il.data_ptr(), tg.data_ptr(), tl.data_ptr(), nll.data_ptr(), mean.data_ptr(), None,
                                                  lws.data_ptr(), B, T, V, Lmax, 0, 1, st)
    return out, (score, nll)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_ctc_align.py measures on the GPU"
    res = []
    for B, T, V, Lmax in ((32, 100, 256, 40), (8, 376, 256, 130)):
        fns, (score, nll) = legs(B, T, V, Lmax, seed=B)
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                times[k].append(time_device(fn, args.iters))
        row = {"B": B, "T": T, "V": V, "Lmax": Lmax}
        for k, v in times.items():
            row[k] = round(min(v), 1)
            row[k.replace("_us", "_max_us")] = round(max(v), 1)
        assert bool((score > float("-inf")).all()) and bool((score <= -nll + 1e-3 * nll.abs()).all())          # the timed launches aligned something
        res.append(row)
        print(json.dumps(row))
    if args.out:
        with open(args.out, "w") as f:
            for row in res:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
