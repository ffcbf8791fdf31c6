"""Time the CTC prefix beam search (avec_amd.ops.ctc_beam_search) at the evaluation shape: B = 32 utterances, T = 100 frames, V = 256, beam 16.

    python tools/bench_beam.py [--iters N] [--ngrams N] [--out FILE]

Legs: no LM; a synthetic order-6 ARPA of about --ngrams n-grams generated from a seed (random, not normalised: the search's cost does not depend on
it); the fp64 oracle of tests/ctc_beam_oracle.py on the CPU, once, for context.  Device times are HIP events around --iters launches after warm-up.
Also reports the host time to write, parse and build the LM tables."""
import argparse
import json
import os
import sys
import tempfile
import time

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
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ngrams", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ctc_beam_oracle as O
    from avec_amd import ngram, ops
    assert torch.cuda.is_available(), "bench_beam.py measures on the GPU"
    B, T, V, W, order = 32, 100, 256, 16, 6
    logits_np = O.ctc_like_logits(B, T, V, seed=0)
    lens_np = np.full(B, T, dtype=np.int64)
    logits, lens = torch.from_numpy(logits_np).cuda(), torch.from_numpy(lens_np).cuda()
    res = {"B": B, "T": T, "V": V, "W": W}
    res["no_lm_ms"] = time_device(lambda: ops.ctc_beam_search(logits, lens, W), args.iters)
    path = os.path.join(tempfile.mkdtemp(), "synthetic6.arpa")
    t0 = time.time()
    entries, _ = O.write_random_arpa(path, V=V, order=order, n_per_order=args.ngrams // (order - 1), seed=6, extras=False)
    res["arpa_write_s"] = time.time() - t0
    t0 = time.time()
    lm = ngram.NGramLM(path, V)
    res["arpa_parse_build_s"] = time.time() - t0
    res["ngrams"], res["contexts"], res["order"] = len(entries), lm.n_contexts, lm.order
    res["lm6_ms"] = time_device(lambda: ops.ctc_beam_search(logits, lens, W, 1.0, lm, 0.6, 1.0), args.iters)
    t0 = time.time()
    for b in range(B):
        O.beam_search(O.log_softmax64(logits_np[b]), T, W)
    res["oracle_cpu_no_lm_s"] = time.time() - t0
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
