"""Captured steps: the capture procedure (CapturedStep) and the shape-keyed cache of captured training steps (StepCache).  Host sequencing only: what a captured
body launches is its caller's business (nnet/model.py: the whole training step and the micro-step; nnet/streaming.py: one push of a streaming session)."""
import gc
import time
import warnings

import torch

from .. import ops


class CapturedStep:
    """One hipGraph over static copies of a batch.  warm_up() runs eager passes on a side stream, capture() records `body`, load() copies a new batch into the
    static buffers, replay() submits the graph and returns the body's outputs (static too: every replay refills them)."""

    def __init__(self, inputs=(), targets=()):
        self.inputs = [t.clone() for t in inputs]
        self.targets = tuple(t.clone() for t in targets)
        self.graph, self.outputs = None, None

    def warm_up(self, fn, passes=1):
        """`passes` eager calls of `fn` on a side stream, as torch.cuda.graph's own warm-up advice: lazily created constants (DFT matrix, sinusoid tables, loss
        weights), kernel attributes and the allocator's blocks exist before the capture.  Returns the last call's result."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        out = None
        with torch.cuda.stream(side):
            for _ in range(passes):
                out = fn()
        torch.cuda.current_stream().wait_stream(side)
        return out

    def capture(self, body, drain=False, before=None):
        """synchronise, `before()` (eager work that must directly precede the graph), record body() -> self.graph, self.outputs.
        drain (data parallel over the nccl backend): the process group's watchdog thread polls the events of collectives it still tracks (hipEventQuery, every
        ~100 ms); under a "global"-mode capture such a poll is a capture violation and aborts the process, and in "thread_local" mode HIP reports the backward
        pass's collectives (issued from the autograd thread) as not capturing, so they ARE tracked and their captured events get polled.  So: global mode, and the
        watchdog's list drained before the capture starts (everything issued so far has completed -- the synchronize -- and is reaped within one watchdog period)."""
        torch.cuda.synchronize()
        # a captured graph that died in a reference cycle (a discarded model and its cached steps hold each other) waits for Python's cyclic collector, and
        # destroying a CUDAGraph synchronises the device on this stack: a collection that starts in the middle of the capture below would be a capture violation
        # that aborts the process.  torch.cuda.graph no longer collects on entry, so collect here
        gc.collect()
        if drain:
            time.sleep(0.6)
        if before is not None:
            before()
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph):
                outputs = body()
        except Exception:
            ops.reset_backward_state()          # an aborted capture leaves a half-run backward pass behind: queued weight gradients, hand-over tags, group counters
            raise
        self.graph, self.outputs = graph, outputs

    def load(self, inputs, targets):
        for d, s in zip(self.inputs, inputs):
            d.copy_(s, non_blocking=True)
        for d, s in zip(self.targets, targets):
            d.copy_(s, non_blocking=True)

    def replay(self):
        self.graph.replay()
        return self.outputs


class StepCache:
    """The captured steps of one model, least recently used first.  A key is (kind, ...): kind "step" (the whole training step) or "micro" (forward + backward of
    one micro-step), then whatever the capture depends on (shapes and dtypes of the batch, precision, the accumulation count of a micro-step).  `cache_size`
    bounds the cache as a whole, not per kind; within one training run only one kind occurs.  Each entry holds its own activation pool.  A deep copy of the
    cache is an empty one: a copy of the model (Model.set_ema) must not hold steps captured on the original's buffers."""

    def __init__(self):
        self.entries = {}                       # dict order = recency
        self.evictions = 0

    def __deepcopy__(self, memo):
        return StepCache()

    def count(self, kind=None):
        return sum(1 for key in self.entries if kind is None or key[0] == kind)

    def clear(self, kind=None):
        for key in [key for key in self.entries if kind is None or key[0] == kind]:
            del self.entries[key]

    def get_or_make(self, key, make, cache_size, who):
        """-> (entry, made): the entry of `key`, now the most recent; made: make() built it just now, after the least recent entries left to make room"""
        entry = self.entries.pop(key, None)
        made = entry is None
        if made:
            while self.entries and len(self.entries) >= cache_size:
                self.entries.pop(next(iter(self.entries)))
                self.evictions += 1
                if self.evictions == 2 * cache_size:         # every new shape costs an eager warm-up step, a capture and a private activation pool
                    warnings.warn("%s: %d captured steps evicted from a cache of %d -- the batch shapes do not repeat; bucket the batches "
                                  "(graph_bucket_frames / a length-bucketed sampler, nnet/samplers.py) or raise graph_cache_size" % (who, self.evictions, cache_size))
            entry = make()
        self.entries[key] = entry
        return entry, made
