"""GPU (-m gpu): every kernel of avec_amd/csrc/loss_optim.hip, called through the C ABI, against the fp64 references of tests/loss_optim_ref.py (which
tests/test_loss_optim_ref.py pins to independent formulas on the host).

Output buffers are carved out of one larger device buffer that is pre-filled with NaN (Carve): an element the kernel had to write and did not stays NaN and fails the
comparison, and the NaN gaps before, between and after the outputs show that nothing was written past an end.

Tolerances.  CTC uses the bounds tests/test_gpu_parity.py states for it: loss 1e-4 relative; gradient 1e-4 (T < 100) or 1e-2 (beyond) in max-norm -- here per utterance,
not over the batch.  One row needs more at T < 100, the peaky one (logits x 20, |log-likelihood| ~ 2e3): its bound is 4 x the error of aten's float32 CPU CTC on the
same row against the fp64 reference (the margin covers the kernel's fast exp / log).  Measured float32 errors of that row, and the bounds they give:
    (60, 12, 40) 5.0e-4 -> 2.0e-3    (80, 32, 32) 4.2e-4 -> 1.7e-3    (80, 32, 40) 2.9e-4 -> 1.2e-3    (10, 3, 2100) 3.8e-5 -> 1.5e-4 (the multi-head rows likewise)
(every other row of these shapes: float32 error <= 5.2e-5, inside 1e-4 with the same margin of 2; at T >= 100 the worst float32 error is 2.2e-3, the peaky row of
(160, 150, 40), inside 1e-2).  The bounds of softmax cross-entropy and Adam are taken the same way, from the float32 evaluation of the same formula on the host against
fp64, times 4; they are computed beside each assertion and documented there.  Argmax, gradient scaling and the shadow refresh are bit-exact."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from avec_amd import lib as L
from avec_amd.lib import lib
from tests import loss_optim_ref as R

pytestmark = pytest.mark.gpu
GAP = 64                                    # elements of sentinel before, between and after the carved regions (256 bytes of fp32: every region stays 256-byte aligned)
NAN = float("nan")


def st():
    return torch.cuda.current_stream().cuda_stream


def last_kernel():
    return lib.raw("avec_last_kernel")().decode()


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


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
        """every element outside the regions still holds the sentinel"""
        end = 0
        for a, n in self.spans:
            if not self.untouched(self.buf[end:a]):
                return False
            end = a + n
        return self.untouched(self.buf[end:])


def ptr(t):
    return None if t is None else t.data_ptr()


# ==============================================================================================================================================
# CTC
# ==============================================================================================================================================
def _grad_tol(T, peaky_err32):
    """per-row gradient bounds [9]: the module's bound, and for the peaky row 4 x aten's float32 error where that is more"""
    base = 1e-4 if T < 100 else 1e-2
    tol = torch.full((len(R.CTC_ROWS),), base, dtype=torch.float64)
    k = R.CTC_ROWS.index("peaky")
    tol[k] = max(base, 4 * peaky_err32)
    return tol


def _reference(x, il, tg, tl):
    """(nll fp64, grad fp64, per-row gradient bound): computed from the inputs and aten on the host alone"""
    nll, grad = R.ctc_ref(x, il, tg, tl, True)
    k = R.CTC_ROWS.index("peaky")
    _, g32 = R.ctc_ref(x[k:k + 1], il[k:k + 1], tg[k:k + 1], tl[k:k + 1], True, dtype=torch.float32)
    return nll, grad, _grad_tol(x.shape[1], float(R.row_rel(g32, grad[k:k + 1])[0]))


@functools.lru_cache(maxsize=None)
def _single_reference(T, Lmax, V):
    x, il, tg, tl, _ = R.ctc_case(T, Lmax, V)
    return _reference(x, il, tg, tl)


def _run_ctc(x, il, tg, tl, zero_inf, with_grad=True, with_mean=True):
    B, T, V = x.shape
    Lmax = tg.shape[1]
    c = Carve([B, 1, B * T * V, lib.raw("avec_ctc_workspace_floats")(B, T, max(Lmax, 1))])
    nll, mean, grad, ws = c.views
    mean.zero_()
    xd, ild, tgd, tld = x.cuda().contiguous(), il.cuda(), tg.cuda().contiguous(), tl.cuda()
    lib.ctc_loss(xd.data_ptr(), ild.data_ptr(), tgd.data_ptr(), tld.data_ptr(), nll.data_ptr(), ptr(mean if with_mean else None), ptr(grad if with_grad else None),
                 ws.data_ptr(), B, T, V, Lmax, 0, int(zero_inf), st())
    torch.cuda.synchronize()
    kern = last_kernel()
    assert c.intact(), "written outside the outputs"
    if not with_grad:
        assert bool(torch.isnan(grad).all()), "grad = NULL, yet the gradient buffer was written"
    if not with_mean:
        assert float(mean) == 0
    return nll.cpu(), float(mean), grad.cpu().view(B, T, V), kern


def _check_ctc_head(tag, nll, grad, il, feas, ref_nll, ref_grad, tol):
    """one head's per-utterance losses and gradient rows against the reference (zero_infinity = 1)"""
    rr = R.row_rel(grad, ref_grad) if grad is not None else None
    for b, name in enumerate(R.CTC_ROWS):
        a, r = float(nll[b]), float(ref_nll[b])
        print("%s %-9s in_len %3d nll %.6g ref %.6g rel %.2e%s" % (tag, name, int(il[b]), a, r, abs(a - r) / max(abs(r), 1e-30),
                                                                   "" if rr is None else "  grad rel %.2e (bound %.1e)" % (float(rr[b]), float(tol[b]))))
    for b, name in enumerate(R.CTC_ROWS):
        a, r = float(nll[b]), float(ref_nll[b])
        if feas[b]:
            assert abs(a - r) <= 1e-4 * abs(r), (tag, name, a, r)
        else:
            assert a == 0.0, (tag, name, a)
        if grad is None:
            continue
        assert float(rr[b]) <= float(tol[b]), (tag, name, float(rr[b]), float(tol[b]))
        n = int(il[b])
        assert bool((grad[b, n:] == 0).all()), (tag, name, "frames beyond the length must be written as exact zeros")
        if not feas[b]:
            assert bool((grad[b] == 0).all()), (tag, name, "an infeasible utterance has an all-zero gradient")


def _check_mean(tag, mean, nll):
    """the batch mean is an atomic fp32 sum of nll_b / B: one rounding per quotient and one per addition"""
    B = nll.numel()
    want = float(nll.double().sum()) / B
    assert abs(mean - want) <= (B + 1) * R.EPS32 * float(nll.double().abs().sum()) / B, (tag, mean, want)


@pytest.mark.parametrize("shape,route", R.CTC_SHAPES, ids=["T%d-L%d-V%d" % s for s, _ in R.CTC_SHAPES])
def test_ctc_single_head_edges_on_every_route(shape, route):
    """the nine rows of loss_optim_ref.CTC_ROWS (none dropped at any shape) on each kernel and wave count avec_ctc_loss can choose"""
    T, Lmax, V = shape
    x, il, tg, tl, feas = R.ctc_case(T, Lmax, V)
    ref_nll, ref_grad, tol = _single_reference(T, Lmax, V)
    nll, mean, grad, kern = _run_ctc(x, il, tg, tl, 1)
    print("shape", shape, "kernel", kern)
    assert kern == route
    _check_ctc_head(str(shape), nll, grad, il, feas, ref_nll, ref_grad, tol)
    _check_mean(str(shape), mean, nll)
    # no gradient wanted: the same losses, bit for bit
    nll_ng, mean_ng, _, kern_ng = _run_ctc(x, il, tg, tl, 1, with_grad=False)
    assert kern_ng == route and same_bits(nll_ng, nll)
    _check_mean(str(shape), mean_ng, nll_ng)
    # zero_infinity = 0: the infeasible utterances report inf, everything else is unchanged.  aten's gradient of an infeasible utterance is NaN there; the kernel
    # writes zeros (the loss is inf either way, and a zero gradient keeps the other utterances' step usable), so only the feasible rows are compared with aten
    nll0, _, grad0, kern0 = _run_ctc(x, il, tg, tl, 0, with_mean=False)
    ref0, _ = R.ctc_ref(x, il, tg, tl, False)
    assert kern0 == route
    assert bool(torch.isinf(ref0[~feas]).all()) and bool((nll0[~feas] == math.inf).all())
    assert same_bits(nll0[feas], nll[feas])
    rr0 = R.row_rel(grad0, ref_grad)
    assert bool((rr0[feas] <= tol[feas]).all()), (rr0, tol)
    assert bool((grad0[~feas] == 0).all())
    for b in range(len(R.CTC_ROWS)):
        assert bool((grad0[b, int(il[b]):] == 0).all())


def _run_multi(n, tg, tl, heads, null_head, weights, with_total=True):
    B, Lmax, V = tg.shape[0], tg.shape[1], heads[0][0].shape[2]
    sizes = [B] * n + [1] * n + [1] + [h[0].numel() for h in heads]
    c = Carve(sizes)
    nll, means, total, grads = c.views[:n], c.views[n:2 * n], c.views[2 * n], c.views[2 * n + 1:]
    for m in means:
        m.zero_()
    total.zero_()
    xs, ils = [h[0].cuda().contiguous() for h in heads], [h[1].cuda() for h in heads]
    tgd, tld = tg.cuda().contiguous(), tl.cuda()
    arr = lambda ps: (ctypes.c_void_p * n)(*ps)
    lib.ctc_loss_multi(n, arr([t.data_ptr() for t in xs]), arr([t.data_ptr() for t in ils]), (ctypes.c_int * n)(*[h[0].shape[1] for h in heads]),
                       arr([t.data_ptr() for t in nll]), arr([t.data_ptr() for t in means]), arr([None if i == null_head else grads[i].data_ptr() for i in range(n)]),
                       tgd.data_ptr(), tld.data_ptr(), (ctypes.c_float * n)(*weights), ptr(total if with_total else None), B, V, Lmax, 0, 1, st())
    torch.cuda.synchronize()
    return c, [t.cpu() for t in nll], [float(m) for m in means], float(total), [g.cpu().view(h[0].shape) for g, h in zip(grads, heads)], last_kernel()


@pytest.mark.parametrize("n_heads", [1, 3, 8])
def test_ctc_multi_head_every_head_against_the_reference(n_heads):
    """distinct frame counts, lengths and weights per head: a head that read another head's T, in_lens, weight or output slot cannot pass"""
    tg, tl, heads = R.ctc_multi_case(n_heads)
    assert all(R.ctc_multi_fits(h[0].shape[1], R.MH_V, R.MH_LMAX) for h in heads) and len({h[0].shape[1] for h in heads}) == n_heads
    w = R.MH_W[:n_heads]
    null_head = 1 if n_heads > 1 else None
    c, nll, means, total, grads, kern = _run_multi(n_heads, tg, tl, heads, null_head, w)
    assert kern == "ctc_lds_multi_kernel w16"
    assert c.intact()
    want_total = 0.0
    for h, (x, il, feas) in enumerate(heads):
        ref_nll, ref_grad, tol = _reference(x, il, tg, tl)
        if h == null_head:
            assert bool(torch.isnan(grads[h]).all()), "grad = NULL for this head, yet its buffer was written"
        _check_ctc_head("head %d T %d" % (h, x.shape[1]), nll[h], None if h == null_head else grads[h], il, feas, ref_nll, ref_grad, tol)
        _check_mean("head %d" % h, means[h], nll[h])
        ref_mean = float(ref_nll.sum()) / ref_nll.numel()
        assert abs(means[h] - ref_mean) <= 1e-4 * abs(ref_mean), (h, means[h], ref_mean)
        want_total += R.f32(w[h]) * ref_mean
    print("total", total, "fp64", want_total)
    assert abs(total - want_total) <= 1e-4 * abs(want_total), (total, want_total)


def test_ctc_multi_head_rejections_come_before_any_launch():
    tg, tl, heads = R.ctc_multi_case(1)
    B = tg.shape[0]
    nine = [heads[0]] * 9
    with pytest.raises(RuntimeError, match="9 heads"):
        _run_multi(9, tg, tl, nine, None, [1.0] * 9)
    T_big = 420
    assert not R.ctc_multi_fits(T_big, R.MH_V, R.MH_LMAX) and not lib.raw("avec_ctc_loss_multi_fits")(T_big, R.MH_V, R.MH_LMAX)
    assert lib.raw("avec_ctc_loss_multi_fits")(100, R.MH_V, R.MH_LMAX) == 1
    big = (torch.zeros(B, T_big, R.MH_V), torch.full((B,), T_big), heads[0][2])
    with pytest.raises(RuntimeError, match="does not fit"):
        _run_multi(2, tg, tl, [heads[0], big], None, [1.0, 1.0])
    with pytest.raises(RuntimeError, match="weights"):
        c = Carve([1])
        lib.ctc_loss_multi(1, None, None, None, None, None, None, None, None, None, c.views[0].data_ptr(), B, R.MH_V, R.MH_LMAX, 0, 1, st())


# ==============================================================================================================================================
# softmax cross-entropy
# ==============================================================================================================================================
def _run_ce(x, y, with_grad=True, with_mean=True):
    M, V = x.shape
    c = Carve([M, 1, M * V])
    loss, mean, grad = c.views
    mean.zero_()
    xd, yd = x.cuda().contiguous(), y.cuda()
    lib.softmax_ce(xd.data_ptr(), yd.data_ptr(), -100, loss.data_ptr(), ptr(mean if with_mean else None), ptr(grad if with_grad else None), M, V, st())
    torch.cuda.synchronize()
    assert c.intact()
    if not with_grad:
        assert bool(torch.isnan(grad).all())
    return loss.cpu(), float(mean), grad.cpu().view(M, V)


def _ce_float32(x, y):
    """torch's float32 CPU cross-entropy and its gradient on the rows it accepts (the others are zero by definition)"""
    M, V = x.shape
    ok = (y >= 0) & (y < V)
    loss, grad = torch.zeros(M), torch.zeros(M, V)
    if bool(ok.any()):
        xx = x[ok].clone().requires_grad_(True)
        t = torch.nn.functional.cross_entropy(xx, y[ok], reduction="none")
        t.sum().backward()
        loss[ok], grad[ok] = t.detach(), xx.grad
    return loss, grad


@pytest.mark.parametrize("M,V", R.CE_SHAPES)
def test_softmax_ce_against_fp64(M, V):
    """Bound per row: 4 x the worst error of torch's float32 CPU cross-entropy (over the rows of the row's class: the peaky row 0, or the
    others) + 2^-23 max|x_row| -- lse - x[y] cancels when the prediction is confident, leaving the rounding of the two terms, each of magnitude <= max|x|; a
    probability exp(x - lse) inherits that absolute error of its argument as a relative one, and is <= 1.  torch's float32 cross-entropy, measured on these cases: loss error <= 6.8e-7
    (peaky row: <= 1.3e-6, its floor 6.9e-6 .. 1.2e-5), gradient error <= 4.3e-8."""
    x, _ = R.ce_case(M, V)
    for y in R.ce_case_ys(M, V):
        r_loss, r_grad, r_mean = R.softmax_ce_ref(x, y)
        h_loss, h_grad = _ce_float32(x, y)
        loss, mean, grad = _run_ce(x, y)
        floor = 2.0 ** -23 * x.double().abs().amax(1)
        cls = torch.zeros(M, dtype=torch.bool)
        cls[0] = True
        tol_l, tol_g = torch.zeros(M, dtype=torch.float64), torch.zeros(M, dtype=torch.float64)
        for sel in (cls, ~cls):
            if bool(sel.any()):
                tol_l[sel] = 4 * float((h_loss.double() - r_loss)[sel].abs().max()) + floor[sel]
                tol_g[sel] = 4 * float((h_grad.double() - r_grad)[sel].abs().max()) + floor[sel]
        e_l, e_g = (loss.double() - r_loss).abs(), (grad.double() - r_grad).abs().amax(1)
        e_l, e_g = torch.where(torch.isnan(e_l), torch.full_like(e_l, math.inf), e_l), torch.where(torch.isnan(e_g), torch.full_like(e_g, math.inf), e_g)
        print("M %d V %d targets %s: loss err %.2e (bound %.2e), grad err %.2e (bound %.2e)" % (M, V, sorted(set(y.tolist()) - set(range(V))), float(e_l.max()), float(tol_l.min()),
                                                                                              float(e_g.max()), float(tol_g.min())))
        assert bool((e_l <= tol_l).all()), (e_l, tol_l)
        assert bool((e_g <= tol_g).all()), (e_g, tol_g)
        bad = (y < 0) | (y >= V)
        assert bool((loss[bad] == 0).all()) and bool((grad[bad] == 0).all()), "ignored and out-of-range targets: loss 0 and a zero gradient row, exactly"
        # mean over ALL M rows (ignored ones included): the atomic fp32 sum of loss_m / M
        want = float(loss.double().sum()) / M
        assert abs(mean - want) <= (M + 1) * R.EPS32 * float(loss.double().abs().sum()) / M, (mean, want)
        assert abs(mean - float(r_mean)) <= float(tol_l.sum()) / M + (M + 1) * R.EPS32 * float(r_loss.abs().sum()) / M, (mean, float(r_mean))
        # grad = NULL and mean_out = NULL are accepted and change nothing else
        loss2, mean2, _ = _run_ce(x, y, with_grad=False, with_mean=False)
        assert same_bits(loss2, loss) and mean2 == 0


# ==============================================================================================================================================
# argmax
# ==============================================================================================================================================
def _argmax_rows(kind, M, V, g):
    x = torch.randn(M, V, generator=g)
    for r in range(M):
        a = (r * 37) % V
        dup = sorted({a, (a + 1) % V, (a + 64) % V, (a + 65) % V, (a + 1024) % V})          # the next lane, the same lane one stride on, both, 16 strides on
        if kind == "dup":
            x[r, dup] = 7.0
        elif kind == "neginf":
            x[r] = -math.inf
        elif kind == "one_nan":
            x[r, dup] = 7.0
            x[r, (a + 3) % V] = NAN
        elif kind == "two_nan_and_inf":
            x[r, dup] = math.inf
            x[r, [(a + 70) % V, (a + 5) % V]] = NAN
        elif kind == "all_nan":
            x[r] = NAN
        elif kind == "neginf_but_last":
            x[r] = -math.inf
            x[r, V - 1] = -3.0e38
    return x


@pytest.mark.parametrize("V", [1, 5, 64, 65, 256, 2100])
@pytest.mark.parametrize("M", [1, 6, 133])
def test_argmax_rows_equals_torch_argmax(M, V):
    """first maximal index; a NaN counts as maximal and the first NaN wins (torch.argmax); every index written lies in [0, V)"""
    g = torch.Generator().manual_seed(M * 10000 + V)
    for kind in ["random", "dup", "neginf", "one_nan", "two_nan_and_inf", "all_nan", "neginf_but_last"]:
        x = _argmax_rows(kind, M, V, g)
        c = Carve([M], dtype=torch.int64, fill=-7777)
        xd = x.cuda().contiguous()
        lib.argmax_rows(xd.data_ptr(), c.views[0].data_ptr(), M, V, st())
        torch.cuda.synchronize()
        got = c.views[0].cpu()
        assert c.intact()
        assert int(got.min()) >= 0 and int(got.max()) < V, (kind, got)
        assert torch.equal(got, x.argmax(-1)), (kind, got, x.argmax(-1))


# ==============================================================================================================================================
# Adam
# ==============================================================================================================================================
def _run_adam(inp, step, lr, b1, b2, eps, wd, gs, zero_grad, flag="null"):
    """flag: "null" (no pointer), 0 or 1 (a device int)"""
    n = inp[0].numel()
    c = Carve([n, n, n, n, 2])
    for v, t in zip(c.views, inp):
        v.copy_(t)
    c.views[4].copy_(torch.tensor([float(step), float(lr)]))
    fl = None if flag == "null" else torch.tensor([flag], dtype=torch.int32, device="cuda")
    p, g, m, v, state = c.views
    lib.adam_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), state.data_ptr(), b1, b2, eps, wd, gs, int(zero_grad), n, ptr(fl), st())
    torch.cuda.synchronize()
    assert c.intact()
    return [t.cpu().clone() for t in (p, g, m, v)]


def _adam_errors(out, inp, hp):
    """{quantity: (error of the kernel, error of the float32 host evaluation)} against adam_ref in fp64, every element in units of the terms it is summed from
    (loss_optim_ref.adam_scales): one fp32 rounding is 2^-24 = 6e-8 there.  The update is p_new - p_old; half the elements have p_old = 0, so that it is judged
    at its own magnitude and not at the rounding of p."""
    p0, g0, m0, v0 = inp
    r64, r32 = R.adam_ref(p0, g0, m0, v0, *hp), R.adam_ref(p0, g0, m0, v0, *hp, dtype=torch.float32)
    su, sm, sv = R.adam_scales(p0, g0, m0, v0, *hp)
    pd = p0.double()
    err = lambda got, ref, s: float(torch.nan_to_num((got.double() - ref).abs() / s, nan=math.inf).max())
    return {"update": (err(out[0].double() - pd, r64[0] - pd, su), err(r32[0].double() - pd, r64[0] - pd, su)),
            "m": (err(out[2], r64[1], sm), err(r32[1], r64[1], sm)), "v": (err(out[3], r64[2], sv), err(r32[2], r64[2], sv))}


def _adam_assert(tag, out, inp, hp):
    """bound: 4 x the float32 host evaluation's own error, and never below 4 roundings (2^-22) -- at n = 4 the host evaluation can be exact by chance.
    Float32 host errors measured over the cases below, in those units: update <= 2.4e-7, m <= 6.1e-8, v <= 2.8e-7."""
    for k, (e, e32) in _adam_errors(out, inp, hp).items():
        bound = 4 * max(e32, R.EPS32)
        print("%s %-6s err %.2e float32 %.2e bound %.2e" % (tag, k, e, e32, bound))
        assert e <= bound, (tag, k, e, e32, bound)


ADAM_HP = [(0.9, 0.98, 1e-9), (0.9, 0.999, 1e-8)]


@pytest.mark.parametrize("n", [4, 1028])
def test_adam_step_against_fp64_over_the_hyperparameters(n):
    """the whole grid of betas / eps, weight decay, gradient scale and step count, at the two small sizes only: the size above the block cap
    (test_adam_step_above_the_block_cap) runs one setting, since the grid changes scalars and the size changes only the indexing.  zero_grad = 0 is used at step 2."""
    inp = R.adam_inputs(n, 40 + n)
    inp[0][1::2] = 0                                                      # (see _adam_errors)
    for (b1, b2, eps) in ADAM_HP:
        for wd in (0.0, 1e-6, 0.1):
            for gs in (1.0, 0.25):
                for step in (1, 2, 1000, 100000):
                    zg = step != 2                                        # zero_grad = 0 at one of the steps
                    out = _run_adam(inp, step, 1e-3, b1, b2, eps, wd, gs, zg)
                    _adam_assert("n %d betas (%g, %g) wd %g gs %g step %d" % (n, b1, b2, wd, gs, step), out, inp, (step, 1e-3, b1, b2, eps, wd, gs))
                    if zg:
                        assert same_bits(out[1], torch.zeros(n)), "zero_grad = 1 clears the gradient (to +0)"
                    else:
                        assert same_bits(out[1], inp[1]), "zero_grad = 0 leaves the gradient as it was, bit for bit"


def test_adam_step_above_the_block_cap():
    """n / 4 elements per thread-quad, 256 threads, 8192 blocks at most: 1200 elements more than one pass of the grid covers, so the stride loop runs (and its
    second pass is partial)"""
    n = 4 * 256 * 8192 + 1200
    inp = R.adam_inputs(n, 41)
    inp[0][1::2] = 0
    hp = (1000, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.25)
    out = _run_adam(inp, *hp, True)
    _adam_assert("n %d" % n, out, inp, hp)
    assert not bool(out[1].any()), "the gradient arena is cleared to its end"
    skipped = _run_adam(inp, *hp, True, flag=1)
    assert all(same_bits(skipped[i], inp[i]) for i in (0, 2, 3)) and not bool(skipped[1].any())


@pytest.mark.parametrize("zero_grad", [0, 1])
def test_adam_skip_flag(zero_grad):
    n = 1028
    inp = R.adam_inputs(n, 42)
    hp = (7, 1e-3, 0.9, 0.98, 1e-9, 1e-6, 0.25)
    plain, flag0, flag1 = (_run_adam(inp, *hp, zero_grad, flag=f) for f in ("null", 0, 1))
    assert all(same_bits(a, b) for a, b in zip(plain, flag0)), "a NULL flag and a flag of 0 behave alike"
    assert not same_bits(plain[0], inp[0]) and not same_bits(plain[2], inp[2]) and not same_bits(plain[3], inp[3])
    assert all(same_bits(flag1[i], inp[i]) for i in (0, 2, 3)), "a raised flag leaves parameters and moments untouched, bit for bit"
    assert same_bits(flag1[1], torch.zeros(n) if zero_grad else inp[1]), "... and clears the gradient iff zero_grad"
    assert same_bits(plain[1], torch.zeros(n) if zero_grad else inp[1])


def test_adam_rejects_a_length_that_is_no_multiple_of_4():
    c = Carve([8, 8, 8, 8, 2])
    p, g, m, v, state = c.views
    with pytest.raises(RuntimeError, match="multiple of 4"):
        lib.adam_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), state.data_ptr(), 0.9, 0.98, 1e-9, 0.0, 1.0, 1, 6, None, st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(c.buf).all()), "rejected before any launch"


def test_adam_trajectory_of_50_steps_against_float64_optimizer():
    """the Noam schedule and hyperparameters of test_adam_steps_golden; torch.optim.Adam in float64 (hyperparameters and lr rounded to fp32, as the kernel receives
    them; coupled weight decay added to the gradient by hand).  Bound: 4 x the drift of the same optimizer run in float32 on the host -- measured 9.9e-10 on
    parameters of the order of 1e-3 (a few roundings of p, 1.2e-10 each, over 50 steps), while the parameters move by 6.1e-5."""
    n, b1, b2, eps, wd = 1028, 0.9, 0.98, 1e-9, 1e-6
    p0 = 0.01 * R.adam_inputs(n, 43)[0]               # of the order of 1e-3: the 50 warm-up updates (1e-7 .. 5e-6 each) are then far above the rounding of p
    grads = [torch.randn(n, generator=torch.Generator().manual_seed(500 + s)) for s in range(50)]

    def host(dtype):
        p = torch.nn.Parameter(p0.to(dtype).clone())
        opt = torch.optim.Adam([p], lr=0.0, betas=(R.f32(b1), R.f32(b2)), eps=R.f32(eps), weight_decay=0.0)
        for s, g in enumerate(grads, 1):
            opt.param_groups[0]["lr"] = R.f32(R.noam_lr(s))
            p.grad = g.to(dtype) + torch.tensor(R.f32(wd), dtype=dtype) * p.detach()
            opt.step()
        return p.detach().double()

    p64, p32 = host(torch.float64), host(torch.float32)
    c = Carve([n, n, n, n, 2])
    p, g, m, v, state = c.views
    p.copy_(p0)
    m.zero_()
    v.zero_()
    for s, gr in enumerate(grads, 1):
        g.copy_(gr)
        state.copy_(torch.tensor([float(s), R.noam_lr(s)]))
        lib.adam_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), state.data_ptr(), b1, b2, eps, wd, 1.0, 1, n, None, st())
    torch.cuda.synchronize()
    assert c.intact() and not bool(g.any())
    drift32, drift = float((p32 - p64).abs().max()), float((p.cpu().double() - p64).abs().max())
    moved = float((p64 - p0.double()).abs().max())
    print("moved %.3e, float32 host drift %.3e, kernel drift %.3e" % (moved, drift32, drift))
    assert moved > 1000 * drift32, "the trajectory is long enough to tell a wrong update from rounding"
    assert drift <= 4 * drift32, (drift, drift32)


# ==============================================================================================================================================
# gradient scaling
# ==============================================================================================================================================
def _factor(scalar, mul):
    return float(np.float32(1.0 if scalar is None else scalar) * np.float32(mul))


@pytest.mark.parametrize("scalar", [None, 0.37])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2 * 4096 * 256 + 3])
def test_scale_by_scalar_bit_exact(n, scalar):
    """out = g * (fl32(s) * fl32(mul)), both products rounded to fp32; the last n is three elements more than two passes of the capped grid"""
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    mul = 1.0 / 7.0
    c = Carve([n, n])
    gin, out = c.views
    gin.copy_(x)
    s = None if scalar is None else torch.tensor([scalar], dtype=torch.float32, device="cuda")
    lib.scale_by_scalar(gin.data_ptr(), ptr(s), mul, out.data_ptr(), n, st())
    torch.cuda.synchronize()
    assert c.intact() and same_bits(gin, x)
    assert same_bits(out, x * _factor(scalar, mul))


MULTI_N = [1, 70000, 2 * 1024 * 256 + 5, 255, 257, 1025, 33, 4097]
MULTI_MUL = [0.5, -1.25, 1.0 / 3.0, 3.0, 0.1, 7.0, 1e-3, 11.0]


def _run_scale_multi(k, scalar):
    sizes = MULTI_N[:k]
    xs = [torch.randn(n, generator=torch.Generator().manual_seed(900 + i)) for i, n in enumerate(sizes)]
    c = Carve(sizes + sizes)
    gin, out = c.views[:k], c.views[k:]
    for a, b in zip(gin, xs):
        a.copy_(b)
    s = None if scalar is None else torch.tensor([scalar], dtype=torch.float32, device="cuda")
    lib.scale_by_scalar_multi(k, (ctypes.c_void_p * k)(*[t.data_ptr() for t in gin]), (ctypes.c_void_p * k)(*[t.data_ptr() for t in out]),
                              (ctypes.c_longlong * k)(*sizes), (ctypes.c_float * k)(*MULTI_MUL[:k]), ptr(s), st())
    torch.cuda.synchronize()
    return c, xs, gin, out


@pytest.mark.parametrize("scalar", [None, 0.37])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_scale_by_scalar_multi_bit_exact_and_in_bounds(k, scalar):
    """tensors of 1 .. 524 293 elements in one launch whose grid is sized by the largest: each gets its own factor, and the sentinels after every short tensor hold"""
    c, xs, gin, out = _run_scale_multi(k, scalar)
    assert c.intact(), "written past the end of a tensor"
    for i in range(k):
        assert same_bits(gin[i], xs[i])
        assert same_bits(out[i], xs[i] * _factor(scalar, MULTI_MUL[i])), i


def test_scale_by_scalar_multi_rejects_nine_tensors():
    c = Carve([4] * 18)
    v = c.views
    with pytest.raises(RuntimeError, match="9 tensors"):
        lib.scale_by_scalar_multi(9, (ctypes.c_void_p * 9)(*[t.data_ptr() for t in v[:9]]), (ctypes.c_void_p * 9)(*[t.data_ptr() for t in v[9:]]),
                                  (ctypes.c_longlong * 9)(*[4] * 9), (ctypes.c_float * 9)(*[1.0] * 9), None, st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(c.buf).all())


# ==============================================================================================================================================
# shadow refresh
# ==============================================================================================================================================
SHADOW_DT = {"f32": (L.F32, torch.float32), "bf16": (L.BF16, torch.bfloat16)}


def _shadow_expect(master, table, n, dtype, entries):
    """the shadow buffer after a refresh of `entries`: the sentinel everywhere, the images of those table rows on top"""
    want = torch.full((n,), NAN, dtype=dtype)
    for i in entries:
        fp, fv, bp, bv = R.shadow_ref(master, table[i], dtype)
        want[fp] = fv
        want[bp] = bv
    return want


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_shadow_refresh_images_bit_exact_and_nothing_else_written(mode):
    """hand-built table (loss_optim_ref.shadow_case): vector and element-wise paths of the load and of both stores, the padded forward layout (its pad columns stay
    as allocated: the kernel must not write them), taps, the fused backward pitch.  The shadow is pre-filled with NaN; afterwards it equals, bit for bit, NaN with
    the images of shadow_ref on top."""
    code, dtype = SHADOW_DT[mode]
    master, entries, n = R.shadow_case()
    table, total = R.shadow_table(entries)
    md, td = master.cuda(), table.cuda().contiguous()
    sh = torch.full((n,), NAN, dtype=dtype, device="cuda")
    lib.shadow_refresh(code, md.data_ptr(), sh.data_ptr(), td.data_ptr(), len(entries), total, st())
    torch.cuda.synchronize()
    want = _shadow_expect(master, table, n, dtype, range(len(entries)))
    got = sh.cpu()
    assert int(torch.isnan(want).sum()) >= 64 * 3, "gaps and pad columns exist"
    for i in range(len(entries)):
        fp, fv, bp, bv = R.shadow_ref(master, table[i], dtype)
        assert same_bits(got[fp], fv), ("forward image of entry", i, entries[i])
        assert same_bits(got[bp], bv), ("backward image of entry", i, entries[i])
    assert same_bits(got, want), "an element outside every image was written"
    assert same_bits(md, master)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("first", [1, 4, 7, 11])
def test_shadow_refresh_range_writes_only_its_entries(mode, first):
    code, dtype = SHADOW_DT[mode]
    master, entries, n = R.shadow_case()
    table, total = R.shadow_table(entries)
    md, td = master.cuda(), table.cuda().contiguous()
    sh = torch.full((n,), NAN, dtype=dtype, device="cuda")
    fb = int(table[first, 6])
    lib.shadow_refresh_range(code, md.data_ptr(), sh.data_ptr(), td.data_ptr(), len(entries), fb, total - fb, st())
    torch.cuda.synchronize()
    assert same_bits(sh.cpu(), _shadow_expect(master, table, n, dtype, range(first, len(entries))))
