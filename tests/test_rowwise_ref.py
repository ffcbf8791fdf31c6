"""Host-only tests of tests/rowwise_ref.py: every reference formula against an independent implementation (torch.nn.functional in fp64 with autograd, explicit
loops for the patch pool), the numpy dropout hash against hand-computed vectors and its statistics, the exactness precondition of every exact case of
tests/test_gpu_rowwise.py, and the recorded host fp32 error of every formula that the tolerances are 8 x of."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import rowwise_ref as R

D64 = torch.float64


def close(a, b, tol=1e-11):
    return a.shape == b.shape and bool(((a - b).abs() <= tol * (1 + b.abs())).all())


def test_tolerance_is_8x_host_fp32():
    """R.TOL is 8 x the recorded worst per-element error of the plain fp32 host evaluation.  Re-measured here: torch's fp32 sums depend on the CPU's vector width and
    thread count, so the re-measurement may move by a small factor -- it must stay within 2 x of the record (then the tolerance is still >= 4 x a host evaluation)"""
    m = R.measure_host_fp32()
    assert sorted(m) == sorted(R.TOL)
    for k, v in sorted(m.items()):
        print("%-16s worst per-element ratio %.3g (recorded %.3g)   tolerance %.3g" % (k, v, R.HOST_FP32_WORST[k], R.TOL[k]))
        assert R.TOL[k] == 8 * R.HOST_FP32_WORST[k] and v <= 2 * R.HOST_FP32_WORST[k], (k, v, R.HOST_FP32_WORST[k])
    assert max(R.TOL.values()) < 2.0 ** -18, "a per-element tolerance of more than 64 fp32 roundings of the element's own terms is no fp32 tolerance"


def test_ratio_judges_every_element_on_its_own():
    """a wrong coefficient on one small-magnitude channel passes the max-norm metric of tests/helpers.py and fails this one; NaN never passes; a bf16 output may
    miss by half its spacing and no more; a flushed subnormal passes"""
    from tests.helpers import rel_err
    x, g, b = R.gauss((9, 16), 1), R.coef(16, 1), R.coef(16, 2)
    g[5], b[5] = 1e-4, 1e-5
    r = R.layernorm_fwd(x, g, b, 1e-6)["y"]
    got = r[0].clone()
    got[:, 5] = (r[0][:, 5] - b[5]) * 1.5 + b[5]                       # gamma of channel 5 off by 50 %
    assert rel_err(got, r[0]) < 1e-4
    q = R.ratio(got, r[0], r[1]).view(9, 16)
    assert float(q[:, 5].max()) > 0.05 and float(q[:, [0, 4, 6, 13]].max()) == 0
    got = r[0].clone(); got[8, 15] = float("nan")
    assert math.isinf(R.worst(got, *r))
    one = torch.tensor([1.003, 1.99, 255.0], dtype=D64)
    assert R.worst(one.to(torch.bfloat16), one, one * 1e-9, "bf16") == 0, "round-to-nearest of a bf16 output is within the bf16 term"
    assert R.worst(one.to(torch.bfloat16) + torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0]), one, one * 1e-9, "bf16") > 1e5, "the next bf16 number is not"
    assert R.half_ulp_bf16(torch.tensor([1.0, 1.5, 2.0, 0.0])).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 0.0]
    z = torch.zeros(3, dtype=D64)
    assert R.worst(z, z - 3.7e-42, z + 3.7e-42) == 0 and math.isinf(R.worst(z + 1e-30, z, z))


# ---- dropout ---------------------------------------------------------------------------------------------------------------------------------------
def _mix32_int(x):
    """the same five steps on a Python integer"""
    x ^= x >> 16; x = x * 0x7FEB352D & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846CA68B & 0xFFFFFFFF; x ^= x >> 16
    return x


def test_dropout_hash_hand_vectors():
    """mix32(0) = 0 (every step maps 0 to 0) and mix32(1), mix32(0xffffffff) worked by hand below; a key and four masks from first principles"""
    assert int(R.mix32(0)[0]) == 0
    # mix32(1): 1 ^ 0 = 1; * 0x7feb352d = 0x7feb352d; ^ (>> 15 = 0xffd6) = 0x7febcafb; * 0x846ca68b mod 2^32; ^ >> 16
    x = 0x7FEB352D ^ (0x7FEB352D >> 15)
    assert x == 0x7FEBCAFB
    y = (x * 0x846CA68B) & 0xFFFFFFFF
    assert int(R.mix32(1)[0]) == y ^ (y >> 16) == _mix32_int(1)
    # mix32(0xffffffff): ^ >> 16 = 0xffff0000; * 0x7feb352d mod 2^32 = 0xcad30000 ...
    assert (0xFFFF0000 * 0x7FEB352D) & 0xFFFFFFFF == 0xCAD30000
    assert int(R.mix32(0xFFFFFFFF)[0]) == _mix32_int(0xFFFFFFFF)
    assert R.mix32(np.arange(1000)).tolist() == [_mix32_int(i) for i in range(1000)]
    # the key: seed' = seed + golden * step (mod 2^64); k0 = mix32(low + stream * 0x9e3779b9) ^ mix32(high ^ 0x85ebca6b)
    seed, step, stream = 3, 2, 5
    s = (seed + 0x9E3779B97F4A7C15 * step) & R.U64
    assert s == 0x3C6EF372FE94F82D
    k0, thr, scale = R.drop_key((seed, step), stream, 0.5)
    assert k0 == _mix32_int((0xFE94F82D + 5 * 0x9E3779B9) & R.U32) ^ _mix32_int(0x3C6EF372 ^ 0x85EBCA6B) and thr == 32768 and scale == 2.0
    # elements 2k and 2k + 1 take the low and the high half of ONE hash
    h = _mix32_int(7 ^ k0)
    keep = R.drop_keep((k0, thr, scale), np.array([14, 15]))
    assert keep.tolist() == [(h & 0xFFFF) >= thr, (h >> 16) >= thr]
    # beyond 2^33 elements the high word of the pair index enters
    big = (1 << 33) + 6
    hb = _mix32_int((3 ^ k0) ^ ((1 * 0x9E3779B1) & R.U32))
    assert bool(R.drop_keep((k0, thr, scale), np.array([big], dtype=np.uint64))[0]) == ((hb & 0xFFFF) >= thr)
    # negative int64 seeds are the same bits
    assert R.drop_key((-1, 0), 0, 0.5) == R.drop_key((R.U64, 0), 0, 0.5)


def test_dropout_threshold_scale_and_rate():
    assert R.drop_key(R.RNG, 1, 0.1)[1:] == (6554, 65536.0 / (65536 - 6554))            # 0.1 * 65536 + 0.5 = 6554.1
    assert R.drop_key(R.RNG, 1, 0.25)[1:] == (16384, 65536.0 / 49152)
    assert R.drop_key(R.RNG, 1, 1.0)[1:] == (65536, 0.0) and R.drop_key(R.RNG, 1, 1.5)[1:] == (65536, 0.0)
    assert R.drop_key(R.RNG, 1, 0.0) == (0, 0, 1.0) and R.drop_key(R.RNG, 1, -0.5) == (0, 0, 1.0)
    n = 1 << 20
    for p in (0.1, 0.5, 0.9):
        k0, thr, scale = R.drop_key(R.RNG, R.RNG_STREAM, p)
        m = R.drop_mask(R.RNG, R.RNG_STREAM, p, (n,))
        q = 1 - thr / 65536
        kept = int((m > 0).sum())
        assert abs(kept - n * q) <= 5 * math.sqrt(n * q * (1 - q)), (p, kept, n * q)
        assert set(m.unique().tolist()) == {0.0, scale}
        assert abs(float(m.mean()) - 1) < 5 * math.sqrt((1 - q) / (q * n)), "E[mask] = 1 with the scale of the quantised probability"
    assert bool((R.drop_mask(R.RNG, 3, 1.0, (4, 100)) == 0).all()), "p >= 1 drops everything with scale 0"
    assert bool((R.drop_mask(R.RNG, 3, 0.0, (4, 100)) == 1).all()) and bool((R.drop_mask(R.RNG, 3, -1.0, (7,)) == 1).all()), "p <= 0 is the identity"
    a, b = R.drop_mask(R.RNG, 1, 0.5, (4096,)), R.drop_mask(R.RNG, 2, 0.5, (4096,))
    assert not torch.equal(a, b), "the stream enters the key"
    idx = torch.arange(4096).view(64, 64)[:, 10:30]
    assert torch.equal(R.drop_mask(R.RNG, 1, 0.5, idx.shape, index=idx), a.view(64, 64)[:, 10:30])


# ---- references against torch -------------------------------------------------------------------------------------------------------------------------
def test_layernorm_references_agree_with_torch_autograd():
    M, D = 5, 12
    x, g, b = (R.gauss((M, D), 1) * 2 + 3).requires_grad_(True), (R.coef(D, 1)).requires_grad_(True), R.coef(D, 2).requires_grad_(True)
    y = F.layer_norm(x, (D,), g, b, 1e-3)
    r = R.layernorm_fwd(x.detach(), g.detach(), b.detach(), 1e-3)
    assert close(r["y"][0], y.detach()) and close(r["mean"][0], x.detach().mean(-1)) and close(r["rstd"][0], 1 / torch.sqrt(x.detach().var(-1, unbiased=False) + 1e-3))
    assert bool((r["y"][1] >= r["y"][0].abs() - 1e-12).all())
    dy, dres = R.gauss((M, D), 2), R.gauss((M, D), 3)
    y.backward(dy)
    mask = R.drop_mask(R.RNG, 1, 0.5, (M, D))
    q = R.layernorm_bwd(dy, x.detach(), r["mean"][0], r["rstd"][0], g.detach(), dres, mask, 0.5)
    assert close(q["dx"][0], x.grad + dres) and close(q["prep"][0], 0.5 * mask * (x.grad + dres))
    assert close(R.layernorm_bwd(dy, x.detach(), r["mean"][0], r["rstd"][0], g.detach())["dx"][0], x.grad)
    # a constant row: variance 0, rstd = 1 / sqrt(eps), y = beta
    c = R.layernorm_fwd(torch.full((1, 8), 2.5, dtype=D64), R.coef(8, 1), R.coef(8, 2), 1e-6)
    assert close(c["rstd"][0], torch.tensor([1000.0], dtype=D64)) and close(c["y"][0], R.coef(8, 2)[None])
    # two norms composed, and the gradient of the composition with a residual branch on the first norm's output
    x1 = (R.gauss((M, D), 4) + 1).requires_grad_(True)
    g1, b1, g2, b2 = R.coef(D, 4), R.coef(D, 5), R.coef(D, 6), R.coef(D, 7)
    y1 = F.layer_norm(x1, (D,), g1, b1, 1e-6)
    h2 = F.layer_norm(y1, (D,), g2, b2, 1e-2)
    f = R.layernorm_fwd2(x1.detach(), g1, b1, 1e-6, g2, b2, 1e-2)
    assert close(f["y1"][0], y1.detach()) and close(f["h2"][0], h2.detach())
    y1.retain_grad()
    (h2 * dy).sum().add((y1 * dres).sum()).backward()
    b = R.layernorm_bwd2(dy, f["y1"][0], f["mean2"][0], f["rstd2"][0], g2, dres, x1.detach(), f["mean1"][0], f["rstd1"][0], g1, mask, 0.5)
    assert close(b["dx2"][0], y1.grad) and close(b["dx1"][0], x1.grad, 1e-9) and close(b["prep"][0], 0.5 * mask * x1.grad, 1e-9)
    assert close(R.grad_prep(dy, mask, 0.5)["dacc"][0], 0.5 * mask * dy)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("with_res", [False, True])
def test_bn_apply_references_agree_with_batch_norm_autograd(act, with_res):
    """forward and backward against a training-mode F.batch_norm in fp64: ss, dstats and count are those of the batch itself"""
    M, Cn, eps = 40, 6, 1e-5
    x = (R.gauss((M, Cn), 5) * 2 + 1).requires_grad_(True)
    g, b = R.coef(Cn, 1).requires_grad_(True), R.coef(Cn, 2).requires_grad_(True)
    res = R.gauss((M, Cn), 6).requires_grad_(True) if with_res else None
    z = F.batch_norm(x, None, None, g, b, True, 0.1, eps)
    pre = z + res if with_res else z
    out = [pre, F.silu(pre), F.relu(pre)][act]
    dout = R.gauss((M, Cn), 7)
    out.backward(dout)
    xd = x.detach()
    mean, rs = xd.mean(0), 1 / torch.sqrt(xd.var(0, unbiased=False) + eps)
    ss = torch.stack([g.detach() * rs, b.detach() - mean * g.detach() * rs, mean, rs])
    f = R.bn_apply_fwd(xd, ss, act, res.detach() if with_res else None)
    assert close(f["out"][0], out.detach())
    dact = [torch.ones_like(xd), None, (out.detach() > 0).double()][act]
    if act == 1:
        p = pre.detach().clone().requires_grad_(True)
        F.silu(p).sum().backward()
        dact = p.grad
        assert close(R.dswish_(pre.detach()), dact)
    d = dout * dact
    dstats = torch.cat([d.sum(0), (d * (xd - mean) * rs).sum(0)])
    assert close(dstats[:Cn], b.grad) and close(dstats[Cn:], g.grad)
    # Swish recomputes y scale + shift; with a residual in front of the activation the kernel is given the saved output (ReLU) -- Swish + residual has no entry
    if act == 1 and with_res:
        return
    q = R.bn_bwd_apply(dout, xd, ss, g.detach(), dstats, float(M), act, out=out.detach() if act == 2 else None)
    assert close(q["dy"][0], x.grad, 1e-9) and close(q["dres"][0], d)
    if with_res:
        assert close(q["dres"][0], res.grad)
    if act == 2:
        m = R.bn_bwd_apply(dout, xd, ss, g.detach(), dstats, float(M), 2, mask=out.detach() > 0)
        assert close(m["dy"][0], x.grad, 1e-9)
        if not with_res:
            assert close(R.bn_bwd_apply(dout, xd, ss, g.detach(), dstats, float(M), 2)["dy"][0], x.grad, 1e-9), "out = NULL: by the recomputed pre-activation"
    # the projection shortcut: relu(y sc + sh + r rsc + rsh)
    rss = torch.stack([R.coef(Cn, 8), R.coef(Cn, 9)])
    r2 = R.gauss((M, Cn), 8)
    assert close(R.bn_apply_fwd(xd, ss, 2, r2, rss)["out"][0], F.relu(z.detach() + r2 * rss[0] + rss[1]))


def test_softmax_and_activation_references_agree_with_torch():
    x = R.softmax_rows(5, 65).requires_grad_(True)
    p = F.softmax(x, -1)
    assert close(R.softmax_fwd(x.detach())["p"][0], p.detach())
    dp, dadd = R.gauss((5, 65), 1), R.gauss((5, 65), 2)
    fin = torch.isfinite(x.detach())
    xs = x.detach().clone().masked_fill(~fin, -1e300).requires_grad_(True)            # autograd through -inf gives NaN; -1e300 has the same probabilities
    F.softmax(xs, -1).backward(dp)
    assert close(R.softmax_bwd(dp, x.detach(), dadd)["dx"][0], xs.grad + dadd) and close(R.softmax_bwd(dp, x.detach())["dx"][0], xs.grad)
    s = x.detach()[2:3]
    assert close(R.softmax_fwd(s)["p"][0], R.softmax_fwd(s - s.mean())["p"][0], 1e-9), "shift invariance"
    assert bool((R.softmax_fwd(R.softmax_rows(5, 1))["p"][0] == 1).all())
    for act, fn in ((1, F.silu), (2, F.relu), (3, lambda t: F.glu(t, -1))):
        x, dy = R.act_inputs(3, 5, act)
        x = x.clamp(-50, 50).requires_grad_(True)
        y = fn(x)
        y.backward(dy)
        assert close(R.act_fwd(act, x.detach())["out"][0], y.detach()) and close(R.act_bwd(act, x.detach(), dy)["out"][0], x.grad)
    # the fp32 model of the fast exponential: exp2 of the ROUNDED product
    v = torch.tensor([-30.0, 0.5, 30.0])
    assert R.exp_(v).dtype == torch.float32 and R.exp_(v.double()).dtype == D64
    assert float((R.exp_(v).double() / torch.exp(v.double()) - 1).abs().max()) < 30 * 2.0 ** -22
    big = torch.tensor([100.0, -100.0])
    assert torch.isfinite(R.swish_(big)).all() and torch.isfinite(R.dswish_(big)).all(), "the fp32 model at +-100: exp overflows to inf, 1 / inf = 0, no NaN"


def test_pool_references_agree_with_loops_and_torch():
    """patch pool / un-pool against the conventions of the oracle's patch attention, written as loops: zero padding, divisor P, nearest up-sampling sliced to T"""
    for B, T, P in R.PATCH:
        D = 4
        Tp = (T + P - 1) // P
        x, o, res = R.gauss((B, T, D), 1), R.gauss((B, Tp, D), 2), R.gauss((B, T, D), 3)
        mask = R.drop_mask(R.RNG, 2, 0.5, (B, T, D))
        y, dx, out, dob = torch.zeros(B, Tp, D, dtype=D64), torch.zeros(B, T, D, dtype=D64), torch.zeros(B, T, D, dtype=D64), torch.zeros(B, Tp, D, dtype=D64)
        for b in range(B):
            for t in range(T):
                y[b, t // P] += x[b, t] / P
                dx[b, t] = o[b, t // P] / P
                out[b, t] = res[b, t] + o[b, t // P] * mask[b, t]
                dob[b, t // P] += res[b, t] * mask[b, t]
        assert close(R.patch_pool_fwd(x, P)["y"][0], y) and close(R.patch_pool_bwd(o, T, P)["dx"][0], dx)
        assert close(R.patch_unpool_add(o, res, mask, P)["out"][0], out) and close(R.patch_unpool_bwd(res, mask, P)["dob"][0], dob)
        pad = Tp * P - T
        assert close(R.patch_pool_fwd(x, P)["y"][0], F.pad(x, (0, 0, 0, pad)).view(B, Tp, P, D).mean(2)), "the oracle's patch_attention pooling"
        assert close(o.repeat_interleave(P, dim=1)[:, :T], R.patch_unpool_add(o, torch.zeros_like(res), torch.ones_like(res), P)["out"][0])
        # pool backward is the adjoint of pool forward, un-pool backward of un-pool
        assert abs(float((R.patch_pool_fwd(x, P)["y"][0] * o).sum() - (x * dx).sum())) < 1e-10
    for N, HW, Cn in R.AVGPOOL:
        x = R.gauss((N, HW, Cn), 4).requires_grad_(True)
        y = F.adaptive_avg_pool1d(x.transpose(1, 2), 1)[:, :, 0]
        dy = R.gauss((N, Cn), 5)
        y.backward(dy)
        assert close(R.avgpool_fwd(x.detach())["y"][0], y.detach()) and close(R.avgpool_bwd(dy, HW)["dx"][0], x.grad)
    for B, T, To, step in R.STRIDED:
        dx, src = R.int_tensor((B, T, 4), -3, 3, 6), R.int_tensor((B, To, 4), -3, 3, 7)
        want = dx.clone()
        for to in range(To):
            want[:, to * step] += src[:, to]
        assert torch.equal(R.strided_rows_add(dx, src, step), want) and (To - 1) * step < T


# ---- the exact cases ------------------------------------------------------------------------------------------------------------------------------------
def _is_dtype_number(t, dtype):
    return torch.equal(R.rd(t, dtype), t.double())


def test_exact_cases_satisfy_their_preconditions():
    """every input, intermediate and result of an exact case is a number of the storage dtype, and every sum stays below 2^24 units"""
    for dt in ("f32", "bf16"):
        for M, Cn in R.BN4 + R.BN8 + [(70, R.BN_CAP_C), (70, R.BN_CAP_CQ)]:
            for with_res, rss in ((False, False), (True, False), (True, True)):
                kw = R.bn_fwd_exact(M, Cn, with_res, 0, rss)
                r = R.bn_apply_fwd(**kw)
                pre, mag = r["pre"]
                assert _is_dtype_number(kw["y"], dt) and _is_dtype_number(r["out"][0], dt) and float(mag.max()) <= 24
                assert float(kw["ss"][0, 0]) == 1 and float(kw["ss"][1, 0]) == 0 and float(pre[0, 0]) == 0
                if not rss:
                    assert M < 3 or float(pre[2, 0]) == R.TINY32
                    assert M < 2 or (float(pre[1, 0]) == 0 and math.copysign(1, float(kw["y"][1, 0])) == -1)
                # no pre-activation within the tolerance of zero other than the exact zeros: the share of elements whose mask bit is undetermined is 0
                near = (pre != 0) & (pre.abs() <= R.TOL["bn_apply_fwd"] * mag)
                assert int(near.sum()) == 0
                assert int((pre == 0).sum()) >= 1 and int((pre > 0).sum()) >= 1
            kw = R.bn_bwd_exact(M, Cn)
            keep = R.bn_pre(kw["y"], kw["ss"])[0] > 0
            r = R.bn_bwd_apply(**kw, mask=keep)
            for k in ("dy", "dres"):
                assert _is_dtype_number(r[k][0], dt) and torch.equal(r[k][0] * 4, (r[k][0] * 4).round()) and float(r[k][1].max()) <= 12, (k, M, Cn)
            assert torch.equal(kw["dstats"], kw["dstats"].round()) and float(kw["dstats"].abs().max()) <= 4
    for N, HW, Cn in R.AVGPOOL:
        if HW & (HW - 1) == 0:
            R.exact_or_die(torch.tensor([3.0 * HW]), "avgpool", (N, HW, Cn))
            assert _is_dtype_number(torch.tensor([3.0 * HW / HW, 1.0 / HW]), "bf16")
    for B, T, P in R.PATCH:
        if P & (P - 1) == 0:
            R.exact_or_die(torch.tensor([3.0 * P]), "patch_pool", (B, T, P))
            assert _is_dtype_number(torch.arange(-3 * P, 3 * P + 1).double() / P, "bf16"), "sums of P integers in [-3, 3] over P = 2^k: bf16 numbers"
    assert R.drop_key(R.RNG, 0, 0.5)[2] == 2.0 and R.drop_key(R.RNG, 0, 0.75)[2] == 4.0, "dropout scales that are powers of two"
    assert float(R.TINY32) == float(torch.tensor(R.TINY32, dtype=torch.bfloat16)) > 0, "2^-126 is the smallest normal number of both dtypes"


def test_shape_tables_reach_the_launch_geometry_edges():
    """what norm.hip's bn8_blocks makes of the 8-wide shapes: one with the grid rounded down to a multiple of q (second in-flight chunk, tail), the conformer width with
    q = 45, the ResNet widths with q = 1, and the two shapes above the caps with a second loop trip"""
    assert R.bn8_blocks(343 * 24 // 8, 24, R.BN8_CAP_FWD) == (3, 3) and 343 * 24 // 8 == 1029 == 768 + 261
    assert R.bn8_blocks(31 * 360 // 8, 360, R.BN8_CAP_FWD) == (45, 45)
    assert R.bn8_blocks(33 * 64 // 8, 64, R.BN8_CAP_FWD)[1] == 1 and R.bn8_blocks(3 * 512 // 8, 512, R.BN8_CAP_BWD)[1] == 1
    for cases, cap in ((R.BN_CAP_FWD_CASES, R.BN8_CAP_FWD), (R.BN_CAP_BWD_CASES, R.BN8_CAP_BWD)):
        (M, Cn), (Mq, Cq) = cases
        nb, q = R.bn8_blocks(M * Cn // 8, Cn, cap)
        assert Cn == 64 and nb == cap and q == 1 and 2 * nb * 256 < M * Cn // 8 < 2 * nb * 256 + 512
        # q = 5: the cap itself is no multiple of q, the grid is rounded down, and only that keeps (grid stride) mod (C / 8) == 0
        nb, q = R.bn8_blocks(Mq * Cq // 8, Cq, cap)
        assert q == 5 and cap % q != 0 and nb == cap // q * q and (nb * 256) % (Cq // 8) == 0 and (cap * 256) % (Cq // 8) != 0
        assert 2 * cap * 256 < Mq * Cq // 8 < 2 * cap * 256 + 512
    # below the cap an unrounded grid never strides: the rounding of (343, 24) only folds the tail into the second in-flight chunk
    assert 5 * 256 >= 1029 > 2 * 3 * 256 - 3 * 256 and 3 * 256 < 1029 <= 2 * 3 * 256
    assert all(Cn % 8 == 4 for _, Cn in R.BN4) and all(Cn % 8 == 0 for _, Cn in R.BN8)
    assert {512, 516} <= set(R.LN_BWD_D) and max(R.LN_BWD_D) == 1536 and 1540 in R.LN_BWD_REJECT and 6 in R.LN_BWD_REJECT
    assert max(R.LN2_D) == 512 and R.LN2_REJECT == 516
    assert all((To - 1) * step < T for _, T, To, step in R.STRIDED)
