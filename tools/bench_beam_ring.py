"""Time one push of the endless streaming CTC beam search (avec_amd.ops.ctc_beam_stream_ring, window = 64) beside the same push of the bounded one
(ops.ctc_beam_stream, max_frames = 400), in one process: B = 32 utterances, V = 256, beam 16, Tc = 4 frames per chunk.

    python tools/bench_beam_ring.py [--iters N] [--rounds N] [--ngrams N] [--out FILE]

Legs: without an LM and with the synthetic order-6 ARPA of tools/bench_beam.py; emit on (traceback + stable prefix) and off; the push that takes an utterance from
96 to 100 frames and the one from 396 to 400.  With window = 64 the ring commits before frames 64, 96, 128, ...: its push at 96 contains a commit step, its push at
396 does not (the result says so), so "ring_period" is also timed: the eight silent pushes from 96 to 128, one commit among them, as the amortised cost of a silent push.
Every timed push starts from the same state: what the push changes (the state; for the ring also its backpointer rows, because a commit rewrites one) is restored
from a snapshot before it, and the same number of restores alone is subtracted.  Times are HIP events around --iters back-to-back (restore, push) pairs; the legs
are run in --rounds alternating rounds (every leg once per round, ring and bounded next to each other) and reported as [min, median, max] ms over the rounds."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ngrams", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import ctc_beam_oracle as O
    from bench_beam import time_device
    from avec_amd import ngram, ops
    assert torch.cuda.is_available(), "bench_beam_ring.py measures on the GPU"
    B, T, V, W, Tc, order, window = 32, 400, 256, 16, 4, 6, 64
    logits = torch.from_numpy(O.ctc_like_logits(B, T + 32, V, seed=0)).cuda()
    path = os.path.join(tempfile.mkdtemp(), "synthetic6.arpa")
    entries, _ = O.write_random_arpa(path, V=V, order=order, n_per_order=args.ngrams // (order - 1), seed=6, extras=False)
    lm6 = ngram.NGramLM(path, V)
    res = {"B": B, "V": V, "W": W, "Tc": Tc, "window": window, "max_frames": T, "ngrams": len(entries), "iters": args.iters, "rounds": args.rounds}
    legs = {}

    def add_leg(name, mode, lm, t0, emit, pushes=1):
        if mode == "ring":
            st = ops.CTCBeamRingState(B, W, window, 4 * window)
            push = ops.ctc_beam_stream_ring
            saved = [(st.state, None), (st.backptr, None)]
        else:
            st = ops.CTCBeamStreamState(B, W, T)
            push = ops.ctc_beam_stream
            saved = [(st.state, None)]
        ones = st.reset_flags.fill_(1)
        for off in range(0, t0, Tc):                        # bring the session to t0 frames
            push(st, logits[:, off:off + Tc].contiguous(), None, ones if off == 0 else None, 1.0, lm, emit=False)
        saved = [(buf, buf.clone()) for buf, _ in saved]
        chunks = [logits[:, t0 + k * Tc:t0 + (k + 1) * Tc].contiguous() for k in range(pushes)]
        if mode == "ring":
            commits = int(st.header()[0, 7])
            for c in chunks:
                push(st, c, None, None, 1.0, lm, emit=False)
            res["%s_commits_in_leg" % name] = int(st.header()[0, 7]) - commits

        def restore():
            for buf, snap in saved:
                buf.copy_(snap)

        def one():
            restore()
            for c in chunks:
                push(st, c, None, None, 1.0, lm, emit=emit)
        legs[name] = (one, restore, pushes)

    for lname, lm in (("no_lm", None), ("lm6", lm6)):
        for t0 in (96, T - Tc):
            for emit in (False, True):
                for mode in ("ring", "bounded"):
                    add_leg("%s_%s_t%d_%s" % (mode, lname, t0, "emit" if emit else "silent"), mode, lm, t0, emit)
        add_leg("ring_period_%s_silent" % lname, "ring", lm, 96, False, pushes=window // 2 // Tc)
    times = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, (one, restore, pushes) in legs.items():
            times[name].append((time_device(one, args.iters) - time_device(restore, args.iters)) / pushes)
    for name, v in times.items():
        res[name + "_ms"] = [round(min(v), 4), round(statistics.median(v), 4), round(max(v), 4)]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
