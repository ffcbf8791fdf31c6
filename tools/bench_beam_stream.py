"""Time one push of the streaming CTC beam search (avec_amd.ops.ctc_beam_stream) at B = 32 utterances, V = 256, beam 16, Tc = 4 frames per chunk (160 ms of
audio at 0.04 s per frame), beside one offline ops.ctc_beam_search at T = 100 in the same process.

    python tools/bench_beam_stream.py [--iters N] [--ngrams N] [--out FILE]

Legs: without an LM and with the synthetic order-6 ARPA of tools/bench_beam.py; emit on (traceback + stable prefix) and off; the push that starts an utterance
(t0 = 0: one live beam at the first frame) and the push that takes it from 96 to 100 frames (t0 = 96: a full beam, a traceback over 100 frames).  Every timed
push starts from the same state: the state buffer is restored from a snapshot before it, so the figure is that of one push, not of a session.  Times are HIP
events around --iters back-to-back (restore, push) pairs after warm-up, minus the same number of restores alone (a 35 KB device copy, reported as state_restore_ms); a single launch between two events would count the host's
own time to issue it."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--ngrams", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import ctc_beam_oracle as O
    from bench_beam import time_device
    from avec_amd import ngram, ops
    assert torch.cuda.is_available(), "bench_beam_stream.py measures on the GPU"
    B, T, V, W, Tc, order = 32, 100, 256, 16, 4, 6
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=0)).cuda()
    lens = torch.from_numpy(np.full(B, T, dtype=np.int64)).cuda()
    path = os.path.join(tempfile.mkdtemp(), "synthetic6.arpa")
    entries, _ = O.write_random_arpa(path, V=V, order=order, n_per_order=args.ngrams // (order - 1), seed=6, extras=False)
    lm6 = ngram.NGramLM(path, V)
    res = {"B": B, "V": V, "W": W, "Tc": Tc, "T_offline": T, "ngrams": len(entries), "iters": args.iters}

    def push_ms(lm, t0, emit):
        st = ops.CTCBeamStreamState(B, W, T)
        ones = st.reset_flags.fill_(1)
        for off in range(0, t0, Tc):                        # bring the session to t0 frames
            ops.ctc_beam_stream(st, logits[:, off:off + Tc].contiguous(), None, ones if off == 0 else None, 1.0, lm, emit=False)
        snap, chunk = st.state.clone(), logits[:, t0:t0 + Tc].contiguous()
        reset = ones if t0 == 0 else None
        def one():
            st.state.copy_(snap)
            ops.ctc_beam_stream(st, chunk, None, reset, 1.0, lm, emit=emit)
        both = time_device(one, args.iters)
        restore = time_device(lambda: st.state.copy_(snap), args.iters)
        if emit:                                            # the timed push is the real one: it must agree with the offline search on the same frames
            ref = ops.ctc_beam_search(logits[:, :t0 + Tc].contiguous(), lens.clamp(max=t0 + Tc), W, 1.0, lm)
            assert torch.equal(st.tokens[..., :t0 + Tc], ref[0]) and torch.equal(st.score, ref[2])
        res["state_restore_ms"] = restore
        return both - restore

    for name, lm in (("no_lm", None), ("lm6", lm6)):
        for t0 in (0, T - Tc):
            for emit in (True, False):
                res["push_%s_t%d_%s_ms" % (name, t0, "emit" if emit else "silent")] = push_ms(lm, t0, emit)
        res["offline_%s_ms" % name] = time_device(lambda: ops.ctc_beam_search(logits, lens, W, 1.0, lm), 20)
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
