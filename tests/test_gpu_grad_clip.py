"""GPU (-m gpu): avec_grad_norm and avec_adam_step_clipped (csrc/loss_optim.hip) through the C ABI, against the fp64 references of tests/grad_clip_ref.py and
tests/loss_optim_ref.py (pinned on the host by tests/test_grad_clip_ref.py and tests/test_loss_optim_ref.py).

Every buffer a kernel writes is carved out of a larger device buffer pre-filled with a sentinel (Carve, the pattern of tests/test_gpu_loss_optim.py): a write outside
the views shows, and so does an output that was never written.

Bounds.  norm: |norm - ref| <= 2 ulp(fp32) of ref -- the fp64 sum of up to 6e7 squares errs by < 1e-8 relative (an fp32 ulp is 6e-8 .. 1.2e-7), the rest is one
rounding each of the product with grad_scale (fp64), the conversion to fp32 and the square root.  coef: within 2 ulp of the fp32 formula evaluated on the kernel's own
norm (one addition, one division).  The clipped Adam launch meets the bound tests/test_gpu_loss_optim.py states for the unclipped one (4 x the float32 host
evaluation's own error, never below 2^-22 in units of the summed terms), against adam_ref at the effective scale fp32(grad_scale * coef)."""
import math

import numpy as np
import pytest
import torch

from avec_amd.lib import lib
from tests import grad_clip_ref as C
from tests import loss_optim_ref as R

pytestmark = pytest.mark.gpu
GAP = 64
NAN = float("nan")
BLOCKS = lib.raw("avec_grad_norm_blocks")
N_PASS = 4 * 256 * BLOCKS(1 << 40)          # the largest n whose 16-byte loads one pass of the capped grid covers
SIZES = [4, 1020, 1024, 1028, N_PASS, N_PASS + 1200, 4 * N_PASS + 1200]      # ... the stride loop runs; ... and past its unrolled round (four loads per lane and round)
ADAM_CAP = 4 * 256 * 8192                    # one pass of the Adam launch's capped grid (tests/test_gpu_loss_optim.py)


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


class Carve:
    """one device buffer filled with a sentinel; `sizes` regions carved out of it, each followed (and the first preceded) by at least GAP untouched elements"""

    def __init__(self, sizes, dtype=torch.float32, fill=NAN):
        assert torch.cuda.is_available(), "these tests need the MI355X"
        offs, o = [], GAP
        for n in sizes:
            offs.append(o)
            o += (n + GAP - 1) // GAP * GAP + GAP
        self.fill, self.spans = fill, list(zip(offs, sizes))
        self.buf = torch.full((o,), fill, dtype=dtype, device="cuda")
        self.views = [self.buf[a:a + n] for a, n in self.spans]

    def untouched(self, t):
        return bool(torch.isnan(t).all()) if isinstance(self.fill, float) and math.isnan(self.fill) else bool((t == self.fill).all())

    def intact(self):
        end = 0
        for a, n in self.spans:
            if not self.untouched(self.buf[end:a]):
                return False
            end = a + n
        return self.untouched(self.buf[end:])


class NormRun:
    """device buffers of one series of avec_grad_norm launches on one gradient: g and stats (fp32, NaN sentinel), the fp64 workspace (NaN), flag (int32, sentinel
    -77 around it, {0, 0} inside)"""

    def __init__(self, g):
        self.n = g.numel()
        self.nb = BLOCKS(self.n)
        self.f = Carve([self.n, 2])
        self.w = Carve([self.nb], dtype=torch.float64)
        self.i = Carve([2, 1], dtype=torch.int32, fill=-77)
        self.g, self.stats = self.f.views
        self.flag, self.skip_in = self.i.views
        self.g.copy_(g)
        self.flag.zero_()
        self.skip_in.zero_()

    def launch(self, grad_scale=1.0, max_norm=0.0, skip_nonfinite=0, skip_in=None):
        if skip_in is not None:
            self.skip_in.fill_(skip_in)
        lib.grad_norm(self.g.data_ptr(), self.n, grad_scale, max_norm, skip_nonfinite, None if skip_in is None else self.skip_in.data_ptr(),
                      self.w.views[0].data_ptr(), 8 * self.nb, self.stats.data_ptr(), self.flag.data_ptr(), st())
        torch.cuda.synchronize()
        assert self.f.intact() and self.w.intact() and self.i.intact(), "a write outside the outputs"
        assert not bool(torch.isnan(self.w.views[0]).any()) or bool(torch.isnan(self.g).any()), "every workgroup of the first pass stores its partial"
        s, f = self.stats.cpu().numpy().copy(), self.flag.cpu().tolist()
        return np.float32(s[0]), np.float32(s[1]), f


@pytest.mark.parametrize("n", SIZES)
def test_norm_and_coef_against_fp64_and_bit_reproducible(n):
    g = R.adam_inputs(n, 80 + n % 97)[1]                 # magnitudes from 1e-20 to 1e4, and exact zeros
    run = NormRun(g)
    assert torch.equal(run.g.cpu(), g), "the gradient is read, never written"
    for gs in (1.0, 0.25):
        ref = C.norm_ref(g, gs)
        max_norm = 0.37 * ref
        norm, coef, flag = run.launch(gs, max_norm, 1)
        e = abs(float(norm) - ref) / C.ulp32(ref)
        want = C.coef_f32(norm, max_norm)
        ec = abs(float(coef) - float(want)) / C.ulp32(want)
        print("n %d grad_scale %g: norm %.9g ref %.17g err %.2f ulp; coef %.9g err %.2f ulp" % (n, gs, norm, ref, e, coef, ec))
        assert e <= 2.0, (n, gs, float(norm), ref, e)
        assert ec <= 2.0 and coef < 1.0, (n, gs, float(coef), float(want), ec)
        assert flag[0] == 0 and flag[1] == 0
        again = run.launch(gs, max_norm, 1)
        assert bits(torch.tensor([norm, coef])).tolist() == bits(torch.tensor([again[0], again[1]])).tolist(), "two launches on the same input give the same bits"
    assert torch.equal(run.g.cpu(), g)


def test_max_norm_below_equal_above_and_off():
    n = 1028
    g = R.adam_inputs(n, 81)[1]
    run = NormRun(g)
    norm0 = float(run.launch(1.0, 0.0)[0])
    norm, coef, _ = run.launch(1.0, 0.5 * norm0)
    assert float(norm) == norm0 and coef < 1.0 and abs(float(coef) - 0.5) < 1e-6, (norm, coef)
    _, coef, _ = run.launch(1.0, norm0)                  # equal: max_norm / (norm + 1e-6), a hair below 1 or rounded to it
    assert coef <= 1.0 and 1.0 - float(coef) <= 1e-6 / norm0 + 2 * R.EPS32 * 2, coef
    for max_norm in (2.0 * norm0, 0.0, -3.0, math.inf, NAN):
        _, coef, _ = run.launch(1.0, max_norm)
        assert float(coef) == 1.0, (max_norm, coef)


def test_one_element_of_3e38_gives_a_finite_norm():
    """3e38 squared overflows fp32 (and so would any fp32 sum of squares); widened to fp64 first, the norm is the element itself"""
    n = 1028
    g = R.adam_inputs(n, 82)[1]
    g[n // 2 + 1] = 3e38
    run = NormRun(g)
    norm, coef, flag = run.launch(1.0, 1.0, 1)
    ref = C.norm_ref(g, 1.0)
    assert math.isfinite(float(norm)) and abs(float(norm) - ref) <= 2 * C.ulp32(ref), (norm, ref)
    want = C.coef_f32(norm, 1.0)
    assert abs(float(coef) - float(want)) <= 2 * C.ulp32(want) and flag == [0, 0]


@pytest.mark.parametrize("n", [1028, N_PASS + 1200])
def test_nonfinite_elements_raise_the_flag_iff_asked(n):
    base = R.adam_inputs(n, 83)[1]
    for pos in (0, n // 2 + 3, n - 1):
        for val in (NAN, math.inf, -math.inf):
            g = base.clone()
            g[pos] = val
            run = NormRun(g)
            for skip_nonfinite in (0, 1):
                norm, coef, flag = run.launch(1.0, 1.0, skip_nonfinite)
                assert not math.isfinite(float(norm)) and float(coef) == 1.0, (pos, val, norm, coef)
                assert flag[0] == skip_nonfinite, (pos, val, skip_nonfinite, flag)
            assert flag[1] == 1


def test_flag_counts_skipped_steps_and_passes_skip_in_on():
    n = 1028
    g = R.adam_inputs(n, 84)[1]
    bad = g.clone()
    bad[5] = NAN
    run = NormRun(g)
    seen = []
    for t in (bad, g, bad):                              # three launches with the guard on: skipped, taken, skipped
        run.g.copy_(t)
        seen.append(run.launch(1.0, 1.0, 1)[2])
    assert seen == [[1, 1], [0, 1], [1, 2]], seen
    run.g.copy_(g)
    assert run.launch(1.0, 1.0, 1, skip_in=0)[2] == [0, 2]
    norm, coef, flag = run.launch(1.0, 1.0, 0, skip_in=1)
    assert flag == [1, 3] and math.isfinite(float(norm)) and coef < 1.0, "skip_in raises the flag for a finite gradient; norm and coef are computed all the same"
    assert run.launch(1.0, 1.0, 0, skip_in=5)[2] == [1, 4]


# ==============================================================================================================================================
# avec_adam_step_clipped
# ==============================================================================================================================================
def _run_adam(inp, step, lr, b1, b2, eps, wd, gs, clip="guarded", flag="null"):
    """clip: "guarded" (avec_adam_step_guarded), "null" (avec_adam_step_clipped without the pair) or the (norm, coef) pair; flag: "null", or the value of flag[0]"""
    n = inp[0].numel()
    c = Carve([n, n, n, n, 2, 2])
    for v, t in zip(c.views, inp):
        v.copy_(t)
    p, g, m, v, state, pair = c.views
    state.copy_(torch.tensor([float(step), float(lr)]))
    ci = Carve([2], dtype=torch.int32, fill=-77)
    fl = None
    if flag != "null":
        fl = ci.views[0]
        fl.copy_(torch.tensor([flag, 9], dtype=torch.int32))
    if clip == "guarded":
        lib.adam_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), state.data_ptr(), b1, b2, eps, wd, gs, 1, n, None if fl is None else fl.data_ptr(), st())
    else:
        pp = None
        if clip != "null":
            pair.copy_(torch.tensor(clip, dtype=torch.float32))
            pp = pair.data_ptr()
        lib.adam_step_clipped(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), state.data_ptr(), b1, b2, eps, wd, gs, 1, n, None if fl is None else fl.data_ptr(), pp, st())
    torch.cuda.synchronize()
    assert c.intact() and ci.intact(), "a write outside the arenas"
    if fl is not None:
        assert fl.cpu().tolist() == [flag, 9], "the flag pair is read only"
    if clip not in ("guarded", "null"):
        assert same_bits(pair, torch.tensor(clip, dtype=torch.float32)), "the {norm, coef} pair is read only"
    return [t.cpu().clone() for t in (p, g, m, v)]


def _adam_assert(tag, out, inp, hp):
    """tests/test_gpu_loss_optim.py's bound: 4 x the float32 host evaluation's own error against adam_ref in fp64, never below 4 roundings (2^-22), every element in
    units of the terms it is summed from (loss_optim_ref.adam_scales)"""
    p0, g0, m0, v0 = inp
    r64, r32 = R.adam_ref(p0, g0, m0, v0, *hp), R.adam_ref(p0, g0, m0, v0, *hp, dtype=torch.float32)
    su, sm, sv = R.adam_scales(p0, g0, m0, v0, *hp)
    pd = p0.double()
    err = lambda got, ref, s: float(torch.nan_to_num((got.double() - ref).abs() / s, nan=math.inf).max())
    for k, e, e32 in (("update", err(out[0].double() - pd, r64[0] - pd, su), err(r32[0].double() - pd, r64[0] - pd, su)),
                      ("m", err(out[2], r64[1], sm), err(r32[1], r64[1], sm)), ("v", err(out[3], r64[2], sv), err(r32[2], r64[2], sv))):
        bound = 4 * max(e32, R.EPS32)
        print("%s %-6s err %.2e float32 %.2e bound %.2e" % (tag, k, e, e32, bound))
        assert e <= bound, (tag, k, e, e32, bound)


HP = (1000, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.25)           # step, lr, beta1, beta2, eps, weight decay, grad_scale


@pytest.mark.parametrize("n", [4, 1028])
def test_clipped_adam_with_a_factor_of_one_is_the_guarded_launch_bit_for_bit(n):
    inp = R.adam_inputs(n, 90 + n)
    ref = _run_adam(inp, *HP, clip="guarded")
    for clip in ("null", (123.5, 1.0), (NAN, 1.0)):
        out = _run_adam(inp, *HP, clip=clip)
        assert all(same_bits(a, b) for a, b in zip(out, ref)), clip
    ref0, out0 = _run_adam(inp, *HP, clip="guarded", flag=0), _run_adam(inp, *HP, clip=(7.0, 1.0), flag=0)
    assert all(same_bits(a, b) for a, b in zip(out0, ref0)) and all(same_bits(a, b) for a, b in zip(ref0, ref))


@pytest.mark.parametrize("n", [1028, ADAM_CAP + 1200])
@pytest.mark.parametrize("coef", [0.5, 2.0 ** -20])
def test_clipped_adam_against_fp64_at_the_effective_scale(n, coef):
    inp = R.adam_inputs(n, 91)
    inp[0][1::2] = 0                                     # the update of half the elements is judged at its own magnitude, not at the rounding of p
    out = _run_adam(inp, *HP, clip=(3.25, coef), flag=0)
    hp = HP[:6] + (C.gscale_eff(HP[6], coef),)
    _adam_assert("n %d coef %g" % (n, coef), out, inp, hp)
    assert not bool(out[1].any()), "the gradient arena is cleared to its end"
    unclipped = _run_adam(inp, *HP, clip="guarded")
    assert not same_bits(out[2], unclipped[2]), "the factor was applied"


@pytest.mark.parametrize("n", [1028, ADAM_CAP + 1200])
def test_clipped_adam_with_a_raised_flag_only_clears_the_gradient(n):
    inp = R.adam_inputs(n, 92)
    out = _run_adam(inp, *HP, clip=(NAN, 1.0), flag=1)
    assert all(same_bits(out[i], inp[i]) for i in (0, 2, 3)), "a raised flag leaves parameters and moments untouched, bit for bit"
    assert same_bits(out[1], torch.zeros(n)), "... and clears the gradient"
