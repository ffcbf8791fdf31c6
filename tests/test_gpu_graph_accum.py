"""GPU (-m gpu): the captured micro-step (Model.graphed_micro_step: forward + backward replayed from a hipGraph, the optimizer tail eager), gradient clipping and
the non-finite guard on the device, Model.fit(use_graphs=True) with accumulation -- on the full AV model, 1 s clips at B = 2, fp32, dropout off, SpecAugment in
eval mode.

The quantity compared is the ACCUMULATED GRADIENT as the optimizer saw it: an optimizer step that starts with Adam's moments at zero leaves
exp_avg = (1 - beta1) (g + wd p0), so g = exp_avg / (1 - beta1) - wd p0 (the device of tests/test_gpu_round4.py), taken on the flat arena and compared per tensor.
Every measured step starts from the initial weights (put back with load_state_dict), so eager and replayed passes see the same parameters and differ only by the
arrival order of float atomics.

What that order does to a gradient (measured on an MI355X, eight eager runs of ONE micro-batch from a zeroed arena).  Most tensors repeat
to 1e-5 (the last two ResNet blocks: 6e-6 .. 1e-5).  On top of that sit two independent two-way decisions per run -- read from the pattern as two activations of the visual
front-end's ResNet on a ReLU's threshold within the forward pass's own rounding noise (an inference, not traced to the activations).  One decision moves the gradient of
front_end.3.blocks.5.layers.4.bias (256 values, norm 0.107) by 5.1e-4 in element 88 and nothing else beyond 3e-7, the other by 8.3e-4 in element 176; the 3 x 3
weights and BatchNorm parameters upstream of them follow.  The distance between two runs of that tensor is therefore one of FOUR values: ~1e-5, 4.76e-3, 7.72e-3 or
9.07e-3 = sqrt(4.76^2 + 7.72^2), the same digits in every session, for eager runs and replays alike (eager against eager over eight runs: 4.762e-3, 4.760e-3,
9.069e-3, 4.761e-3, 7.720e-3, 9.071e-3, 4.761e-3; five replays of one graph among themselves: 3.3e-3 .. 9.065e-3; replay against eager 9.068e-3).  A step that
accumulates k micro-batches dilutes one batch's decisions by about 1 / k: 2.5e-3 .. 3.6e-3 for k = 3 over the two shapes.

So the bound is not guessed, and it is taken on the sequence it is applied to: `floor(seq)` runs the same eager accumulated step several times with the same seed
(five times for k = 3 and k = 2, eight times for the single micro-batch: a pair of runs that happens to agree on every such decision would measure 1e-5) and takes
the worst tensor's relative L2 distance over all pairs; a replayed step may differ from an eager one by 4 x that, and never less than 1e-6.  Tensors whose gradient
is structurally zero (a per-query constant cancels in the softmax, a bias in front of a training-mode BatchNorm cancels in the mean) hold rounding noise only: they
are checked to be that small in the reference and compared in absolute terms against the largest live gradient element.

Where no second run is needed none is used: the gradient the clipped optimizer launch saw is compared with the arena as it stood before that very launch (fp32
rounding only, bound 1e-6), and infos["grad_norm"] with the fp64 norm of that arena (2 fp32 ulp)."""
import contextlib
import itertools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCT_ZERO = ("key_layer.bias", "pos_layer.bias", "conv_module.layers.3.bias", "layers.0.0.bias")
SECS = [(0.9, 0.7), (1.0, 0.8)]                  # two batch shapes (23 and 26 video frames)
SEQ3, SEQ2, SEQ1 = (1, 0, 1), (0, 1), (0,)       # the micro-batches of one optimizer step: the second step of two_steps (k = 3), the data-parallel tool's, one batch
N_EAGER = {SEQ3: 5, SEQ2: 5, SEQ1: 8}            # eager runs behind each floor


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _small_av_batch(B, secs, seed):
    g = torch.Generator().manual_seed(seed)
    alen = torch.tensor([int(16000 * s) for s in secs])
    vlen = alen // 640 + 1
    Ta, Tv = int(alen.max()), int(vlen.max())
    audio, video = torch.zeros(B, Ta), torch.zeros(B, Tv, 88, 88, 1)
    for b in range(B):
        audio[b, :alen[b]] = 0.1 * torch.randn(int(alen[b]), generator=g)
        video[b, :vlen[b]] = torch.randn(int(vlen[b]), 88, 88, 1, generator=g)
    labels = torch.randint(1, 256, (B, 3), generator=g)
    return [video.to(dev()), vlen.to(dev()), audio.to(dev()), alen.to(dev())], (labels.to(dev()), torch.full((B,), 3).to(dev()))


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


class Ctx:
    """ONE model for the whole module (building it and capturing its graphs is most of the cost): every run starts with reset(), which puts back the initial weights
    and buffers, clears Adam's moments, the gradient arena, the step counter, the guard's counter and the infos; captured graphs survive a reset.  Gradients are
    flat fp32 tensors on the device, laid out like the parameter arena; `segs` names their tensors."""

    def __init__(self):
        import avec_amd
        import nnet
        avec_amd.set_compute_dtype("f32")
        avec_amd.manual_seed(7)
        torch.manual_seed(0)
        model = nnet.AudioVisualEfficientConformerInterCTC()
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
            if hasattr(m, "drop_rate"):
                m.drop_rate = 0.0
        model.compile(losses=nnet.CTCLoss(zero_infinity=True, assert_shorter=False))
        self.model = model.to(dev()).train()
        model.encoder.audio_encoder.spec_augment.eval()
        self.sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        self.master0 = model.arena.master.detach().clone()
        self.batches = [_small_av_batch(2, s, i + 1) for i, s in enumerate(SECS)]
        names = {id(p): k for k, p in model.named_parameters()}
        self.segs = [(names[id(p)], int(o), p.numel()) for p, o in zip(model.arena.params, model.arena.offsets)]
        assert len(self.segs) == len(names) > 800
        self.live = [not k.endswith(STRUCT_ZERO) for k, _, _ in self.segs]
        self.live_t = torch.tensor(self.live, device=dev())
        self.cache = {}

    def reset(self, zero_step=True):
        import avec_amd
        m = self.model
        avec_amd.set_compute_dtype("f32")
        avec_amd.manual_seed(7)
        m.train()                                          # (Model.fit switches every module to training mode, SpecAugment included)
        m.encoder.audio_encoder.spec_augment.eval()
        m.load_state_dict(self.sd0)
        m.optimizer._flat["exp_avg"].zero_()
        m.optimizer._flat["exp_avg_sq"].zero_()
        m.optimizer._flat["clip_flag"].zero_()
        m.arena.grad.zero_()
        if zero_step:
            m.model_step.fill_(0)
        m.grad_max_norm, m.skip_nonfinite_steps = None, False
        m.reset_infos()

    def grads(self):
        """the gradient the last optimizer step saw (it started from the initial weights with zero moments), flat"""
        m = self.model
        grp = m.optimizer.param_groups[0]
        beta1, wd = grp["betas"][0], grp["weight_decay"]
        return m.optimizer._flat["exp_avg"].detach().float() / (1.0 - beta1) - wd * self.master0

    def views(self, flat, live=None):
        return [flat[o:o + n] for (_, o, n), lv in zip(self.segs, self.live) if live is None or lv == live]

    def micro(self, mode, inp, tgt, k, acc):
        m = self.model
        if mode == "eager":
            l, _, acc = m.train_step(inp, tgt, torch.float32, None, k, acc)
        else:
            l, acc = m.graphed_micro_step(inp, tgt, torch.float32, k, acc)
        return l, acc

    def one_step(self, mode, seq):
        """one optimizer step over the micro-batches `seq` from the initial state -> its gradient"""
        self.reset()
        acc = 0
        for b in seq:
            _, acc = self.micro(mode, *self.batches[b], len(seq), acc)
        assert acc == 0
        return self.grads()

    def two_steps(self, mode, k=3, **attrs):
        """six micro-steps over the two shapes = two optimizer steps; the second starts again from the initial weights with zero moments, and in graph mode all of
        its micro-steps are replays.  -> (gradient of the second step, the six losses, model_step, parameters after the second step)"""
        m = self.model
        self.reset()
        losses, acc = [], 0
        for i in range(2 * k):
            if i == k:
                self.reset(zero_step=False)
            for a, v in attrs.items():
                setattr(m, a, v)
            inp, tgt = self.batches[i % 2]
            l, acc = self.micro(mode, inp, tgt, k, acc)
            losses.append(l["loss"].detach().clone())
        assert acc == 0 and tuple(i % 2 for i in range(k, 2 * k)) == SEQ3
        g = self.grads()
        return g, [float(x) for x in losses], int(m.model_step), m.arena.master.detach().clone()

    @contextlib.contextmanager
    def watching_tail(self):
        """-> dict that receives the gradient arena as it stands when the optimizer tail begins (behind the last micro-step's backward pass)"""
        m, seen = self.model, {}
        tail = m._finish_optimizer_step

        def watched():
            seen["grad"] = m.arena.grad.detach().clone()
            tail()
        m._finish_optimizer_step = watched
        try:
            yield seen
        finally:
            del m._finish_optimizer_step

    def get(self, name, fn):
        if name not in self.cache:
            self.cache[name] = fn()
        return self.cache[name]

    # shared, computed once, never modified
    def eager_a(self):
        return self.get("eager_a", lambda: self.two_steps("eager"))

    def eager_b(self):
        return self.get("eager_b", lambda: self.two_steps("eager"))

    def graph(self):
        return self.get("graph", lambda: self.two_steps("graph"))

    def eager_runs(self, seq):
        def f():
            first = [self.eager_a()[0], self.eager_b()[0]] if seq == SEQ3 else []
            return first + [self.one_step("eager", seq) for _ in range(N_EAGER[seq] - len(first))]
        return self.get(("eager_runs", seq), f)

    def tensor_errs(self, got, ref, scale=1.0):
        """-> (per tensor: relative L2 distance of got * scale to ref, the difference)"""
        r = ref.double()
        d = got.double() * scale - r
        num, den = torch.stack(torch._foreach_norm(self.views(d))), torch.stack(torch._foreach_norm(self.views(r)))
        return num / den.clamp_min(1e-30), d

    def floor(self, seq):
        """over all pairs of the eager runs of `seq`: (worst live tensor's relative L2 distance, relative L2 distance over the whole arena); and the largest
        live gradient element"""
        def f():
            runs = self.eager_runs(seq)
            worst, whole = torch.zeros((), dtype=torch.float64, device=dev()), torch.zeros((), dtype=torch.float64, device=dev())
            for i, j in itertools.combinations(range(len(runs)), 2):
                e, d = self.tensor_errs(runs[j], runs[i])
                worst = torch.maximum(worst, e[self.live_t].max())
                whole = torch.maximum(whole, d.norm() / runs[i].double().norm())
            gmax = max(float(v.abs().max()) for v in self.views(runs[0], live=True))
            print("eager floor of %s over %d runs: worst tensor %.3e, whole arena %.3e, largest live element %.3e" % (seq, len(runs), float(worst), float(whole), gmax))
            return float(worst), float(whole), gmax
        return self.get(("floor", seq), f)

    def param_floor(self):
        """relative L2 over the whole parameter arena after the second step of two_steps, between two eager runs"""
        return rel_l2(self.eager_b()[3], self.eager_a()[3])

    def bound(self, seq):
        return max(4.0 * self.floor(seq)[0], 1e-6)

    def assert_same_gradient(self, tag, got, ref, seq, scale=1.0, bound=None):
        floor, _, gmax = self.floor(seq)
        bound = self.bound(seq) if bound is None else bound
        e, d = self.tensor_errs(got, ref, scale)
        e = e.cpu().tolist()
        errs = sorted(((x, k) for x, (k, _, _), lv in zip(e, self.segs, self.live) if lv), reverse=True)
        print("%s: worst tensors %s; eager-vs-eager floor %.3e, bound %.3e" % (tag, [(k, "%.3e" % x) for x, k in errs[:3]], floor, bound))
        assert len(errs) > 800
        for x, k in errs:
            assert x <= bound, (tag, k, x, bound)
        # structurally zero gradients: rounding noise around zero in the reference (a live tensor that merely carries such a name would show here) and in the difference
        zd = max(float(v.abs().max()) for v in self.views(d, live=False))
        zr = max(float(v.abs().max()) for v in self.views(ref, live=False))
        assert zr <= 1e-3 * gmax and zd <= 1e-3 * gmax, (tag, zr, zd, gmax)


@pytest.fixture(scope="module")
def ctx():
    import avec_amd
    c = Ctx()
    yield c
    avec_amd.set_compute_dtype("f32")


def test_accumulated_gradient_replayed_against_eager(ctx):
    """k = 3 micro-batches of two shapes, two optimizer steps: train_step(accumulated_steps=3) against graphed_micro_step, gradient of the second step per tensor.
    Measured on an MI355X (fp32), worst tensor: eager against eager 2.5e-3 .. 3.6e-3, replayed against eager 1.3e-3 .. 3.8e-3."""
    ge, le, se, _ = ctx.eager_a()
    gg, lg, sg, _ = ctx.graph()
    print("parameters after the step, eager against eager: %.3e" % ctx.param_floor())
    ctx.assert_same_gradient("graph vs eager", gg, ge, SEQ3)
    assert se == sg == 2, (se, sg)
    for a, b in zip(le, lg):
        assert abs(a - b) < 2e-2 * abs(a), (le, lg)
    assert ctx.model.captured_steps.count("micro") == 2, "six micro-steps over two shapes: exactly two captured graphs"
    assert ctx.model.captured_steps.count("step") == 0


def test_same_batch_accumulated_four_times_is_the_gradient_of_one_captured_step(ctx):
    """BatchNorm normalises with batch statistics in training, so the gradient does not depend on the running ones: k = 4 micro-steps on ONE batch, each scaled by
    1 / 4, add up to the gradient of the existing captured single step on that batch.  The floor is that batch's (SEQ1).  Measured: 6.2e-4 .. 5.3e-3."""
    m = ctx.model
    inp, tgt = ctx.batches[0]
    for rnd in range(2):                                  # round 0 captures (its first micro-step is eager), round 1 is four replays
        ctx.reset()
        acc = 0
        for _ in range(4):
            _, acc = m.graphed_micro_step(inp, tgt, torch.float32, 4, acc)
        assert acc == 0
    g4 = ctx.grads()
    assert int(m.model_step) == 1
    ctx.reset()
    step = m.make_graphed_train_step(inp, tgt, precision=torch.float32, warmup=1)
    ctx.reset()
    step()
    g1 = ctx.grads()
    ctx.assert_same_gradient("4 x (g / 4) vs one captured step", g4, g1, SEQ1)


def _fit_batches(ctx, n):
    return [{"inputs": [t.cpu() for t in ctx.batches[i % 2][0]], "targets": tuple(t.cpu() for t in ctx.batches[i % 2][1])} for i in range(n)]


def test_fit_with_graphs_takes_the_captured_micro_step_when_accumulating(ctx):
    m = ctx.model
    ctx.reset()
    m.captured_steps.clear("micro")
    m.fit(_fit_batches(ctx, 4), epochs=1, precision=torch.float32, accumulated_steps=2, use_graphs=True)
    torch.cuda.synchronize()
    assert m.captured_steps.count("micro") == 2, "fit(use_graphs=True, accumulated_steps=2) did not go through graphed_micro_step"
    assert int(m.model_step) == 2
    assert bool(torch.isfinite(m.arena.master).all()) and not bool(m.arena.grad.any()), "the optimizer launch cleared the gradient arena"
    m.captured_steps.clear("micro")           # (captured with every module in training mode, SpecAugment included: not for the other tests)


def test_fit_with_graphs_and_clipping_takes_the_captured_micro_step(ctx):
    m = ctx.model
    ctx.reset()
    m.captured_steps.clear("micro")
    m.grad_max_norm = 1.0
    m.fit(_fit_batches(ctx, 4), epochs=1, precision=torch.float32, accumulated_steps=1, use_graphs=True)
    torch.cuda.synchronize()
    assert m.captured_steps.count("micro") == 2 and m.captured_steps.count("step") == 0
    assert int(m.model_step) == 4
    norm = float(m.infos["grad_norm"])
    assert norm == norm and norm > 0
    # graphed_train_step itself no longer falls back to eager launches with clipping set
    m.captured_steps.clear("micro")           # (fit's graphs were captured with every module in training mode, SpecAugment included)
    ctx.reset()
    m.grad_max_norm = 1.0
    before = m.captured_steps.count("micro")
    m.graphed_train_step(*ctx.batches[0], precision=torch.float32)
    assert m.captured_steps.count("micro") == before + 1 and int(m.model_step) == 1 and m.captured_steps.count("step") == 0
    m.captured_steps.clear("micro")


def test_fit_says_once_when_it_cannot_replay(ctx, capsys):
    """compiled metrics with eval_training (fit's default) need the host on every step: the micro-steps run eagerly, and fit says so instead of leaving the user
    to believe in the replay path"""
    m = ctx.model
    metrics, m.compiled_metrics = m.compiled_metrics, {"outputs": None}
    try:
        assert m._micro_fallback_reason(eval_training=False) is None and "eval_training" in m._micro_fallback_reason(eval_training=True)
    finally:
        m.compiled_metrics = metrics
    assert m._micro_fallback_reason(eval_training=True) is None, "without compiled metrics there is nothing for the host to compute"
    ctx.reset()
    m.captured_steps.clear("micro")
    m.eager_fallback, m._eager_fallback_said = None, False
    m._micro_fallback_reason = lambda eval_training=False: "for the sake of this test"
    try:
        m.fit(_fit_batches(ctx, 4), epochs=1, precision=torch.float32, accumulated_steps=2, use_graphs=True)
    finally:
        del m._micro_fallback_reason
    torch.cuda.synchronize()
    said = [line for line in capsys.readouterr().out.splitlines() if line.startswith("use_graphs: training with eager launches")]
    assert len(said) == 1 and said[0].endswith("for the sake of this test"), said
    assert m.captured_steps.count("micro") == 0 and int(m.model_step) == 2
    m.eager_fallback, m._eager_fallback_said = None, False


def test_clipping_scales_the_gradient_the_optimizer_sees(ctx):
    """grad_max_norm at half the norm.  Against the arena of the SAME step (taken when the tail begins; no second run, so fp32 rounding only): the gradient in Adam's
    state is coef times it within 1e-6 per tensor -- one rounding each of grad_scale * coef, its product with g, the decay term, (1 - beta1) *, and of the three
    steps back (division, subtraction, 1 / coef) are 7 x 2^-24 = 4.2e-7, and beta1 = 0.9 as fp32 puts 2.4e-7 on 1 - beta1; measured 3.5e-7 -- and
    infos["grad_norm"] is its fp64 norm within 2 fp32 ulp (the kernel test's bound).  Against separate runs, as the arrival order of atomics allows (the floor of
    this batch, SEQ1): the unclipped replay against an eager pass, the clipped replay / coef against the unclipped one (measured 4.8e-3 .. 9.07e-3: the two
    threshold decisions of the module docstring), and the norm against torch's of the eager pass -- two norms differ by no more than the distance of their
    vectors, so by 4 x the whole-arena distance of two eager runs."""
    m = ctx.model
    inp, tgt = ctx.batches[0]
    # a separate eager run: the unclipped gradient and its norm, with torch
    ctx.reset()
    m.train_step(inp, tgt, torch.float32, None, 2, 0)                 # (a micro-step that does not reach the optimizer: the arena holds g / 2)
    norm = float(m.arena.grad.double().norm()) * 2.0
    g_ref = m.arena.grad.detach().clone() * 2.0
    for (k, o, n), p in zip(ctx.segs, m.arena.params):
        assert p.grad.data_ptr() == m.arena.grad.data_ptr() + 4 * o, k       # the gradient arena is laid out like the parameter arena
    # unclipped and clipped, both replayed (round 0 captures this (shape, k = 1) eagerly): max_norm at half the norm
    for rnd in range(2):
        ctx.reset()
        _, acc = m.graphed_micro_step(inp, tgt, torch.float32, 1, 0)
        assert acc == 0 and "grad_norm" not in m.infos
    g_plain = ctx.grads()
    ctx.assert_same_gradient("unclipped replay vs eager", g_plain, g_ref, SEQ1)
    ctx.reset()
    m.grad_max_norm = 0.5 * norm
    with ctx.watching_tail() as seen:
        _, acc = m.graphed_micro_step(inp, tgt, torch.float32, 1, 0)
    assert acc == 0
    g_clip = ctx.grads()
    stats = m.optimizer.grad_norm_stats.cpu()
    got_norm, coef = float(m.infos["grad_norm"]), float(stats[1])
    own_norm = float(seen["grad"].double().norm())
    whole = max(4.0 * ctx.floor(SEQ1)[1], 1e-6)
    print("norm %.9g (torch, separate eager run) %.9g (torch fp64, this step's arena) %.9g (infos); coef %.9g; whole-arena bound %.3e" % (norm, own_norm, got_norm, coef, whole))
    assert abs(got_norm - own_norm) <= 2 * 2.0 ** -23 * own_norm, (got_norm, own_norm)
    assert abs(got_norm - norm) <= whole * norm, (got_norm, norm, whole)
    assert abs(coef - 0.5 * norm / (got_norm + 1e-6)) <= 4 * 2.0 ** -24 and coef < 0.51
    ctx.assert_same_gradient("clipped / coef vs the arena of the same step", g_clip, seen["grad"], SEQ1, scale=1.0 / coef, bound=1e-6)
    ctx.assert_same_gradient("clipped / coef vs unclipped (both replayed)", g_clip, g_plain, SEQ1, scale=1.0 / coef)


def test_a_clip_threshold_far_above_the_norm_changes_nothing(ctx):
    """grad_max_norm = 1e9: coef = 1 exactly, the clipped launch scales by fp32(grad_scale * 1) = grad_scale, so given the same gradient the update is the same bit
    for bit; the gradients of two runs differ by the arrival order of atomics.  The parameters after the step equal the unclipped run's: relative L2 over the whole
    parameter arena, bound 4 x the same quantity between two eager runs and never less than 1e-6 (per tensor the quantity is not meaningful: the first Adam step
    moves an element by lr sign(g), and where the gradient is rounding noise so is the sign).  Measured on an MI355X: two eager runs 6.6e-8 .. 7.0e-8, graph
    against eager 4.2e-8 .. 6.7e-8, clipped at 1e9 against unclipped 4.0e-8.  The gradient the clipped optimizer launch saw is compared per tensor as everywhere else."""
    m = ctx.model
    _, _, _, p_plain = ctx.graph()
    g, _, s, p_clip = ctx.two_steps("graph", grad_max_norm=1e9)
    assert s == 2 and float(m.optimizer.grad_norm_stats[1]) == 1.0
    bound = max(4.0 * ctx.param_floor(), 1e-6)
    e = rel_l2(p_clip, p_plain)
    print("parameters, whole arena: clipped at 1e9 vs unclipped %.3e (bound %.3e); graph vs eager %.3e; eager vs eager %.3e"
          % (e, bound, rel_l2(p_plain, ctx.eager_a()[3]), ctx.param_floor()))
    assert not torch.equal(p_clip, ctx.master0), "the step moved the parameters"
    assert e <= bound, (e, bound)
    ctx.assert_same_gradient("clip 1e9 vs eager", g, ctx.eager_a()[0], SEQ3)


def test_nonfinite_guard_skips_the_step_and_the_next_one_trains(ctx):
    m = ctx.model
    ctx.reset()
    m.skip_nonfinite_steps = True
    (i0, t0), (i1, t1) = ctx.batches
    _, acc = m.graphed_micro_step(i0, t0, torch.float32, 2, 0)
    assert acc == 1
    m.optimizer._flat["exp_avg"].normal_()                            # moments that would show any write
    m.optimizer._flat["exp_avg_sq"].uniform_()
    torch.cuda.synchronize()
    before = [t.clone() for t in (m.arena.master, m.optimizer._flat["exp_avg"], m.optimizer._flat["exp_avg_sq"])]
    m.arena.grad[12345] = float("nan")                                # one NaN in the arena before the tail
    _, acc = m.graphed_micro_step(i1, t1, torch.float32, 2, acc)
    torch.cuda.synchronize()
    assert acc == 0
    after = (m.arena.master, m.optimizer._flat["exp_avg"], m.optimizer._flat["exp_avg_sq"])
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(after, before)), "a skipped step leaves parameters and moments bit-identical"
    assert not bool(m.arena.grad.any()) and not bool(torch.isnan(m.arena.grad).any()), "... and clears the gradient arena"
    assert int(m.infos["skipped_steps"]) == 1 and not (float(m.infos["grad_norm"]) == float(m.infos["grad_norm"]))
    m.optimizer._flat["exp_avg"].zero_()
    m.optimizer._flat["exp_avg_sq"].zero_()
    acc = 0
    for inp, tgt in ctx.batches:                                       # the next step trains
        _, acc = m.graphed_micro_step(inp, tgt, torch.float32, 2, acc)
    torch.cuda.synchronize()
    assert acc == 0 and int(m.infos["skipped_steps"]) == 1
    assert not torch.equal(m.arena.master, before[0]) and bool(torch.isfinite(m.arena.master).all())
    n = float(m.infos["grad_norm"])
    assert n == n and n > 0 and float(m.optimizer.grad_norm_stats[1]) == 1.0, "the guard alone does not clip"


def test_one_rank_data_parallel_micro_step_graph_against_eager(ctx, tmp_path):
    """a one-rank nccl group takes every data-parallel path (SyncBatchNorm exchanges inside the captured micro-step, gradient all-reduce behind the last replay):
    k = 2, two optimizer steps, eager against graph in one child process each; the floor is that of the same two micro-batches (SEQ2) in this process.  Measured:
    3.2e-3 .. 5.9e-3.  No retry: a child that fails or times out is a finding to read."""
    tool = os.path.join(ROOT, "tools", "graph_accum_equiv.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29571", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0", AVEC_DIST_SINGLE="1",
               AVEC_PEER_SYNCBN="1")
    outs = {}
    for mode in ("eager", "graph"):
        outs[mode] = str(tmp_path / (mode + ".pt"))
        r = subprocess.run([sys.executable, tool, "--out", outs[mode], "--mode", mode], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    e, g = torch.load(outs["eager"]), torch.load(outs["graph"])
    assert e["world"] == g["world"] == 1 and e["step"] == g["step"] == 2
    assert g["cached"] == 2 and e["cached"] == 0
    assert e["layout"] == g["layout"] == [list(s) for s in ctx.segs], "the child's arena is laid out like this process's"
    ctx.assert_same_gradient("data parallel, graph vs eager", g["grads"].to(dev()), e["grads"].to(dev()), SEQ2)
    for a, b in zip(e["losses"], g["losses"]):
        assert abs(a - b) < 2e-2 * abs(a), (e["losses"], g["losses"])
