"""GPU (-m gpu): the row-wise and element-wise kernels of avec_amd/csrc/norm.hip -- LayerNorm forward and dx, the BatchNorm apply passes, the InterCTC softmax, the
patch-attention pool / un-pool, the stand-alone activations, the average pool, dropout and the strided casts -- called through the C ABI in f32 and bf16, against the
fp64 references of tests/rowwise_ref.py (which tests/test_rowwise_ref.py pins to torch.nn.functional, autograd and explicit loops on the host).

Harness.  Outputs are carved out of one device allocation pre-filled with the bit pattern 0x7FC0 (a NaN read as bf16 and as fp32), with gaps of at least 256 bytes
before, between and after them: after every launch the gaps must be intact and every element the kernel owes must no longer be NaN.  Accumulating destinations are
pre-filled with known values.  Per-channel coefficients differ in sign and magnitude from channel to channel (rowwise_ref.coef), so that an index off by 4 or 8
channels shows.  Dropout masks are computed on the host from the test's own {seed, step} tensor (rowwise_ref.drop_mask); avec_dropout_f32 pins that hash bit for bit.

Judgement, per element:  |got - ref| <= TOL * scale (+ half a bf16 ulp of ref for a bf16 output, + 2^-126 for a flushed subnormal), scale = the reference formula
with every term taken by its magnitude; TOL = 8 x the worst ratio of the plain fp32 host evaluation of the same formula over the same case table.  The exact cases
(integers and powers of two; preconditions in tests/test_rowwise_ref.py) are compared with torch.equal.

    formula            host fp32 worst   tolerance (x 8)   MI355X worst (2026-10-19, for the record; no tolerance is derived from it)
    layernorm_fwd          1.62e-7          1.3e-6            1.28e-7
    layernorm_fwd2         1.23e-7          9.8e-7            9.79e-8
    layernorm_bwd          1.86e-7          1.5e-6            1.80e-7
    layernorm_bwd2         1.07e-7          8.6e-7            1.28e-7
    grad_prep              8.38e-8          6.7e-7            8.38e-8
    bn_apply_fwd           1.32e-7          1.1e-6            1.18e-7
    bn_bwd_apply           1.99e-7          1.6e-6            1.84e-7
    softmax_fwd            9.49e-8          7.6e-7            9.49e-8
    softmax_bwd            5.75e-8          4.6e-7            7.07e-8
    act                    1.81e-7          1.4e-6            1.81e-7
    patch                  1.57e-7          1.3e-6            1.05e-7
    avgpool                1.32e-7          1.1e-6            7.35e-8
(worst over f32 and bf16.  grad_prep, softmax_fwd and act land exactly on the host figure: the host model of the fast exponential, exp2 of the rounded product, is what
the device computes.  The exact cases, the dropout hash and the mask bytes are bit-identical.)
"""
import itertools

import pytest
import torch

from tests import rowwise_ref as R

pytestmark = pytest.mark.gpu

DT = R.DT
DTYPES = ["f32", "bf16"]
TD = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}
PAT = 0x7FC0
GAPB = 256                       # bytes of sentinel before, between and after the carved regions
D64 = torch.float64


def _lib():
    from avec_amd.lib import lib
    return lib


def stream():
    """the engine's stream, with the project's reduction workspace registered as the runtime registers it"""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from avec_amd import runtime as rt
    return rt.stream()


class Carve:
    """one device allocation filled with the sentinel pattern; regions [(numel, "f32" | "bf16" | "u8")] carved out of it at 256-byte boundaries"""

    def __init__(self, specs):
        assert torch.cuda.is_available(), "these tests need the MI355X"
        self.spans, o = [], GAPB
        for n, dt in specs:
            nb = n * TD[dt].itemsize
            self.spans.append((o, nb, dt))
            o += (nb + GAPB - 1) // GAPB * GAPB + GAPB
        self.pat = torch.full((o // 2,), PAT, dtype=torch.int16, device="cuda").view(torch.uint8)
        self.raw = self.pat.clone()
        self.views = [self.raw[a:a + nb].view(TD[dt]) for a, nb, dt in self.spans]

    def intact(self):
        """every byte outside the regions still holds the sentinel"""
        chk = self.raw.clone()
        for a, nb, _ in self.spans:
            chk[a:a + nb] = self.pat[a:a + nb]
        return torch.equal(chk, self.pat)

    def untouched(self):
        return torch.equal(self.raw, self.pat)


def dev(t64, dt="f32"):
    return None if t64 is None else t64.to(TD[dt]).cuda().contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def rng_tensor():
    return torch.tensor([R.RNG[0], R.RNG[1]], dtype=torch.int64, device="cuda")


class Judge:
    """collects the worst ratio of a formula over a test's cases and every failure; report() prints the family line and fails the test if anything missed"""

    def __init__(self):
        self.worst, self.fails, self.n = {}, [], 0

    def __call__(self, fam, tag, got, ref, scale, out_dt="f32"):
        got = got.detach().cpu()
        assert not bool(torch.isnan(got.float()).any()) or bool(torch.isnan(ref).any()), (fam, tag, "an element the kernel owes is still NaN")
        r = R.ratio(got, ref, scale, out_dt)
        w = float(r.max())
        self.n += 1
        self.worst[fam] = max(self.worst.get(fam, 0.0), w)
        if not w <= R.TOL[fam]:
            i = int(r.argmax())
            self.fails.append((fam, tag, "ratio %.3g > %.3g at flat index %d: got %r ref %r scale %r" % (
                w, R.TOL[fam], i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(scale.reshape(-1)[i]))))

    def exact(self, tag, got, want):
        self.n += 1
        got, want = got.detach().cpu(), want.to(got.dtype)
        if not torch.equal(got, want):
            bad = (got != want) | torch.isnan(got.float())
            self.fails.append(("exact", tag, "%d of %d elements differ, first at flat index %d" % (int(bad.sum()), bad.numel(), int(bad.reshape(-1).float().argmax()))))

    def check(self, tag, cond, what):
        if not cond:
            self.fails.append(("check", tag, what))

    def report(self):
        for fam, w in sorted(self.worst.items()):
            print("%-16s worst ratio %.3g   tolerance %.3g   host fp32 %.3g" % (fam, w, R.TOL[fam], R.HOST_FP32_WORST[fam]))
        print("%d comparisons, %d failures" % (self.n, len(self.fails)))
        for f in self.fails[:40]:
            print("FAIL", f)
        assert not self.fails, self.fails[:10]


def launch(c, fn):
    """run, synchronise, and require the gaps intact"""
    try:
        fn()
        torch.cuda.synchronize()
    except Exception as e:              # a failed launch or a device fault: nothing more is started on this device in this session
        pytest.exit("GPU launch failed, session ended: %r" % (e,), returncode=3)
    assert c.intact(), "written outside the outputs"


def rejected(entry, name, c, *args):
    """the call fails before any launch: non-zero return, avec_last_error names the entry, nothing written"""
    lib = _lib()
    rc = lib.raw("avec_" + entry)(*args)
    torch.cuda.synchronize()
    msg = lib.raw("avec_last_error")().decode()
    assert rc != 0 and name in msg, (entry, rc, msg)
    assert c.untouched(), (entry, "a rejected call wrote to its outputs")


# ==============================================================================================================================================
# LayerNorm
# ==============================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_fwd(dtype):
    """y (fp32, and bf16 where the activation dtype is), mean, rstd at one row / a last block of one row / three blocks, D from one active lane to more than 8
    trips, both sides of 256 and 512; Gaussian, mean-1000, constant and 1e-3-scaled rows"""
    lib, st, J = _lib(), stream(), Judge()
    for (M, D, eps), kw in R.ln_fwd_cases():
        ref = R.layernorm_fwd(**kw)
        x, g, b = dev(kw["x"]), dev(kw["g"]), dev(kw["b"])
        for y_f32 in ((1,) if dtype == "f32" else (0, 1)):
            ydt = "f32" if (y_f32 or dtype == "f32") else "bf16"
            c = Carve([(M * D, ydt), (M, "f32"), (M, "f32")])
            y, mean, rstd = c.views
            launch(c, lambda: lib.layernorm_fwd(DT[dtype], x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), y_f32 if dtype != "f32" else 0, mean.data_ptr(), rstd.data_ptr(),
                                                M, D, eps, st))
            tag = (M, D, eps, ydt)
            J("layernorm_fwd", tag + ("y",), y.view(M, D), *ref["y"], ydt)
            J("layernorm_fwd", tag + ("mean",), mean, *ref["mean"])
            J("layernorm_fwd", tag + ("rstd",), rstd, *ref["rstd"])
    J.report()


def _prep_cfgs():
    return list(itertools.product(R.ALPHAS, R.DROP_P))


def _run_ln_bwd(lib, st, dtype, kw, M, D, prep=None, with_params=False):
    """one avec_layernorm_bwd / _bwd_prep launch -> (dx, prep or None) on the host"""
    gd = kw["_gd"]
    dy, x, mu, rs, g, dres = dev(kw["dy"], gd), dev(kw["x"]), dev(kw["mu"]), dev(kw["rs"]), dev(kw["g"]), dev(kw["dres"])
    dy_f32 = 1 if (gd == "f32" and dtype == "bf16") else 0
    specs = [(M * D, "f32")] + ([(M * D, dtype)] if prep else []) + ([(D, "f32"), (D, "f32")] if with_params else [])
    c = Carve(specs)
    dx = c.views[0]
    if with_params:
        c.views[-1].zero_(); c.views[-2].zero_()
        launch(c, lambda: lib.layernorm_bwd(DT[dtype], dy.data_ptr(), dy_f32, x.data_ptr(), mu.data_ptr(), rs.data_ptr(), g.data_ptr(), dx.data_ptr(), ptr(dres),
                                            c.views[-2].data_ptr(), c.views[-1].data_ptr(), M, D, st))
        assert bool(torch.isfinite(c.views[-1]).all()) and bool(torch.isfinite(c.views[-2]).all())
        return dx.cpu().view(M, D), None
    if prep is None:
        launch(c, lambda: lib.layernorm_bwd(DT[dtype], dy.data_ptr(), dy_f32, x.data_ptr(), mu.data_ptr(), rs.data_ptr(), g.data_ptr(), dx.data_ptr(), ptr(dres), None, None, M, D, st))
        return dx.cpu().view(M, D), None
    alpha, p = prep
    rng = rng_tensor()
    launch(c, lambda: lib.layernorm_bwd_prep(DT[dtype], dy.data_ptr(), dy_f32, x.data_ptr(), mu.data_ptr(), rs.data_ptr(), g.data_ptr(), dx.data_ptr(), ptr(dres),
                                             c.views[1].data_ptr(), alpha, p, rng.data_ptr(), R.RNG_STREAM, M, D, st))
    return dx.cpu().view(M, D), c.views[1].cpu().view(M, D)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_bwd_rows_and_prep(dtype):
    """the dx-only kernel (dgamma = NULL) and its second output: dy fp32 / bf16, with and without dres, D on both sides of the NG = 2 / NG = 6 switch (512 / 516) up to
    the limit 1536; prep = alpha * mask * dx in the activation dtype with the host's mask at element row * D + c; 1540 and 6 rejected before any launch"""
    lib, st, J = _lib(), stream(), Judge()
    for (M, D, gd, with_dres), kw in R.ln_bwd_cases():
        if dtype == "f32" and gd == "bf16":
            continue
        args = {k: v for k, v in kw.items()}
        ref = R.layernorm_bwd(**args)
        run = dict(kw, _gd=gd)
        dx, _ = _run_ln_bwd(lib, st, dtype, run, M, D)
        J("layernorm_bwd", (M, D, gd, with_dres, "dx"), dx, *ref["dx"])
        for alpha, p in _prep_cfgs():
            mask = R.drop_mask(R.RNG, R.RNG_STREAM, p, (M, D))
            refp = R.layernorm_bwd(**args, mask=mask, alpha=alpha)
            dx2, prep = _run_ln_bwd(lib, st, dtype, run, M, D, prep=(alpha, p))
            tag = (M, D, gd, with_dres, alpha, p)
            J.check(tag, torch.equal(dx2, dx), "dx differs between avec_layernorm_bwd and avec_layernorm_bwd_prep")
            J("layernorm_bwd", tag + ("prep",), prep, *refp["prep"], dtype)
            J.check(tag, bool((prep[mask == 0] == 0).all()), "a dropped element is not zero")
            if p == 0.5 and alpha == 0.5 and dtype == "f32":
                J.exact(tag + ("prep = dx where kept (scale 2 x alpha 1/2)",), prep, torch.where(mask > 0, dx, torch.zeros_like(dx)))
    for D in R.LN_BWD_REJECT:
        M = 2
        n = M * max(D, 8)
        ins = [torch.ones(n, device="cuda") for _ in range(5)]
        c = Carve([(n, "f32"), (n, dtype)])
        rng = rng_tensor()
        rejected("layernorm_bwd", "layernorm_bwd", c, DT[dtype], ins[0].data_ptr(), 1, ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), ins[4].data_ptr(),
                 c.views[0].data_ptr(), None, None, None, M, D, st)
        rejected("layernorm_bwd_prep", "layernorm_bwd", c, DT[dtype], ins[0].data_ptr(), 1, ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), ins[4].data_ptr(),
                 c.views[0].data_ptr(), None, c.views[1].data_ptr(), 1.0, 0.1, rng.data_ptr(), R.RNG_STREAM, M, D, st)
    J.report()


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_bwd_with_param_grads_dx(dtype):
    """dx of the kernel that also reduces dgamma / dbeta (those are covered by tests/test_gpu_colreduce.py), on the project's registered workspace: one row, two
    slots, and 4100 rows, where a wave walks several rows and hands the prefetched row over"""
    lib, st, J = _lib(), stream(), Judge()
    for (M, D, gd, with_dres), kw in R.ln_bwd_cases(R.LNP_M, R.LNP_D):
        if dtype == "f32" and gd == "bf16":
            continue
        ref = R.layernorm_bwd(**kw)
        dx, _ = _run_ln_bwd(lib, st, dtype, dict(kw, _gd=gd), M, D, with_params=True)
        J("layernorm_bwd", (M, D, gd, with_dres, "dx with dgamma"), dx, *ref["dx"])
    J.report()


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_fwd2_bwd2(dtype):
    """two LayerNorms per launch against the fp64 composition and its gradient (rowwise_ref.layernorm_fwd2 / _bwd2, pinned to autograd on the host); D <= 512, 516
    rejected"""
    lib, st, J = _lib(), stream(), Judge()
    rng = rng_tensor()
    for M in R.LN2_M:
        for D in R.LN2_D:
            for gd in (("f32",) if dtype == "f32" else ("bf16",)):
                for with_dres in (False, True):
                    f, b = R.ln2_inputs(M, D, gd, with_dres)
                    ref = R.layernorm_fwd2(**f)
                    c = Carve([(M * D, "f32"), (M, "f32"), (M, "f32"), (M * D, dtype), (M, "f32"), (M, "f32")])
                    y1, m1, r1, h2, m2, r2 = c.views
                    x, g1, b1, g2, b2 = (dev(f[k]) for k in ("x", "g1", "b1", "g2", "b2"))
                    launch(c, lambda: lib.layernorm_fwd2(DT[dtype], x.data_ptr(), g1.data_ptr(), b1.data_ptr(), f["eps1"], y1.data_ptr(), m1.data_ptr(), r1.data_ptr(),
                                                         g2.data_ptr(), b2.data_ptr(), f["eps2"], h2.data_ptr(), m2.data_ptr(), r2.data_ptr(), M, D, st))
                    for name, t, odt in (("y1", y1.view(M, D), "f32"), ("mean1", m1, "f32"), ("rstd1", r1, "f32"), ("h2", h2.view(M, D), dtype), ("mean2", m2, "f32"), ("rstd2", r2, "f32")):
                        J("layernorm_fwd2", (M, D, name), t, *ref[name], odt)
                    dy2, x2, mu2, rs2, dres2, x1, mu1, rs1 = (dev(b[k], gd if k == "dy2" else "f32") for k in ("dy2", "x2", "mu2", "rs2", "dres2", "x1", "mu1", "rs1"))
                    for alpha, p in [(None, 0.0)] + _prep_cfgs():
                        mask = None if alpha is None else R.drop_mask(R.RNG, R.RNG_STREAM, p, (M, D))
                        refb = R.layernorm_bwd2(**b, mask=mask, alpha=alpha or 1.0)
                        c = Carve([(M * D, "f32"), (M * D, "f32"), (M * D, dtype)])
                        dx2, dx1, prep = c.views
                        launch(c, lambda: lib.layernorm_bwd2(DT[dtype], dy2.data_ptr(), x2.data_ptr(), mu2.data_ptr(), rs2.data_ptr(), g2.data_ptr(), ptr(dres2), dx2.data_ptr(),
                                                             x1.data_ptr(), mu1.data_ptr(), rs1.data_ptr(), g1.data_ptr(), dx1.data_ptr(),
                                                             None if alpha is None else prep.data_ptr(), alpha or 1.0, p if alpha is not None else 0.0,
                                                             rng.data_ptr(), R.RNG_STREAM, M, D, st))
                        tag = (M, D, with_dres, alpha, p)
                        J("layernorm_bwd2", tag + ("dx2",), dx2.view(M, D), *refb["dx2"])
                        J("layernorm_bwd2", tag + ("dx1",), dx1.view(M, D), *refb["dx1"])
                        if alpha is None:
                            J.check(tag, bool(torch.isnan(prep.float()).all()), "prep = NULL, yet the prep buffer was written")
                        else:
                            J("layernorm_bwd2", tag + ("prep",), prep.view(M, D), *refb["prep"], dtype)
                            J.check(tag, bool((prep.cpu().view(M, D)[mask == 0] == 0).all()), "a dropped element is not zero")
    D, M = R.LN2_REJECT, 2
    ins = [torch.ones(M * D, device="cuda") for _ in range(10)]
    c = Carve([(M * D, "f32"), (M, "f32"), (M, "f32"), (M * D, dtype), (M, "f32"), (M, "f32")])
    v = c.views
    rejected("layernorm_fwd2", "layernorm_fwd2", c, DT[dtype], ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), 1e-6, v[0].data_ptr(), v[1].data_ptr(), v[2].data_ptr(),
             ins[3].data_ptr(), ins[4].data_ptr(), 1e-6, v[3].data_ptr(), v[4].data_ptr(), v[5].data_ptr(), M, D, st)
    c = Carve([(M * D, "f32"), (M * D, "f32"), (M * D, dtype)])
    v = c.views
    rejected("layernorm_bwd2", "layernorm_bwd2", c, DT[dtype], ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), ins[4].data_ptr(), None, v[0].data_ptr(),
             ins[5].data_ptr(), ins[6].data_ptr(), ins[7].data_ptr(), ins[8].data_ptr(), v[1].data_ptr(), v[2].data_ptr(), 1.0, 0.1, rng.data_ptr(), R.RNG_STREAM, M, D, st)
    J.report()


@pytest.mark.parametrize("dtype", DTYPES)
def test_grad_prep_flat_and_with_dbias(dtype):
    """dacc = alpha * mask * dout (fp32 -> activation dtype) from a source of pitch N and N + 8: the flat kernel (dbias = NULL) and the column-reducing one must give
    bit-identical dacc, with the mask at element row * N + col whatever the source pitch"""
    lib, st, J = _lib(), stream(), Judge()
    rng = rng_tensor()
    for M, N, pad in itertools.product(R.GP_M, R.GP_N, R.GP_PAD):
        ld = N + pad
        src = torch.full((M, ld), float("nan"), dtype=D64)
        dout = R.rd(R.gauss((M, N), 1400 + M + N), "f32")
        src[:, :N] = dout
        s = dev(src)
        for alpha, p in _prep_cfgs():
            mask = R.drop_mask(R.RNG, R.RNG_STREAM, p, (M, N))
            ref = R.grad_prep(dout, mask, alpha)["dacc"]
            got = []
            for with_dbias in (False, True):
                c = Carve([(M * N, dtype), (N, "f32")])
                dacc, dbias = c.views
                dbias.zero_()
                launch(c, lambda: lib.grad_prep(DT[dtype], s.data_ptr(), ld, dacc.data_ptr(), alpha, p, rng.data_ptr(), R.RNG_STREAM, dbias.data_ptr() if with_dbias else None, M, N, st))
                tag = (M, N, ld, alpha, p, with_dbias)
                J("grad_prep", tag, dacc.view(M, N), *ref, dtype)
                J.check(tag, with_dbias or bool((dbias == 0).all()), "dbias = NULL, yet written")
                got.append(dacc.cpu().view(M, N))
            J.check((M, N, ld, alpha, p), torch.equal(got[0].view(torch.int16 if dtype == "bf16" else torch.int32), got[1].view(torch.int16 if dtype == "bf16" else torch.int32)),
                    "the flat kernel and the dbias kernel differ in dacc")
            if p == 0.5 and alpha == 0.5 and dtype == "f32":
                J.exact((M, N, ld, "exact"), got[0], torch.where(mask > 0, dout, torch.zeros_like(dout)))
    J.report()


# ==============================================================================================================================================
# BatchNorm apply
# ==============================================================================================================================================
def _bn_fwd(lib, st, dtype, kw, M, Cn, mask=False):
    """-> (out on the host [M][C], mask bytes or None)"""
    y, ss, res = dev(kw["y"], dtype), dev(kw["ss"]), dev(kw.get("res"), dtype)
    rss = dev(kw.get("res_ss"))
    c = Carve([(M * Cn, dtype)] + ([(M * Cn // 8, "u8")] if mask else []))
    out = c.views[0]
    if mask:
        launch(c, lambda: lib.bn_apply_fwd_mask(DT[dtype], y.data_ptr(), ss.data_ptr(), ptr(res), ptr(rss), out.data_ptr(), c.views[1].data_ptr(), M, Cn, st))
        return out.cpu().view(M, Cn), c.views[1].cpu()
    launch(c, lambda: lib.bn_apply_fwd(DT[dtype], y.data_ptr(), ss.data_ptr(), ptr(res), kw["act"], out.data_ptr(), M, Cn, st))
    return out.cpu().view(M, Cn), None


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_apply_fwd(dtype):
    """act none / Swish / ReLU, with and without residual, on the 4-wide kernel (C % 8 == 4, the conformer width 180 among them) and the 8-wide one: one chunk; a grid
    rounded from 5 blocks to 3 with the second in-flight chunk and a tail; q = 45; the ResNet widths.  Swish with planted pre-activations +-30, +-100; ReLU with
    planted +0, -0 and 2^-126 on integers, exact"""
    lib, st, J = _lib(), stream(), Judge()
    for M, Cn in R.BN4 + R.BN8:
        for act in (0, 1, 2):
            for with_res in (False, True):
                kw = R.bn_fwd_inputs(M, Cn, dtype, act, with_res)
                ref = R.bn_apply_fwd(**kw)
                out, _ = _bn_fwd(lib, st, dtype, kw, M, Cn)
                J("bn_apply_fwd", (M, Cn, act, with_res), out, *ref["out"], dtype)
                if act == 1:
                    J.check((M, Cn), float(ref["pre"][0].abs().max()) > 90 or Cn < 4, "the planted extremes are missing")
        for with_res in (False, True):
            kw = R.bn_fwd_exact(M, Cn, with_res)
            out, _ = _bn_fwd(lib, st, dtype, kw, M, Cn)
            J.exact((M, Cn, "relu exact", with_res), out, R.bn_apply_fwd(**kw)["out"][0])
    J.report()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_apply_fwd_mask(dtype):
    """the ReLU pass that also writes one bit per element: residual none / plain / with its own BatchNorm coefficients (projection shortcut); integers, so that no
    pre-activation lies within the tolerance of zero (share 0, asserted in tests/test_rowwise_ref.py) and out and the mask bytes are exact"""
    lib, st, J = _lib(), stream(), Judge()
    for M, Cn in R.BN8:
        for with_res, rss in ((False, False), (True, False), (True, True)):
            kw = R.bn_fwd_exact(M, Cn, with_res, 0, rss)
            r = R.bn_apply_fwd(**kw)
            pre, mag = r["pre"]
            assert int(((pre != 0) & (pre.abs() <= R.TOL["bn_apply_fwd"] * mag)).sum()) == 0
            out, mask = _bn_fwd(lib, st, dtype, kw, M, Cn, mask=True)
            J.exact((M, Cn, with_res, rss, "out"), out, r["out"][0])
            J.exact((M, Cn, with_res, rss, "mask"), mask, R.pack_mask(r["out"][0] > 0))
            # random data as well: out within bound, and the bits equal out_ref > 0 wherever the pre-activation is clear of zero
            kw = R.bn_fwd_inputs(M, Cn, dtype, 2, with_res)
            if rss:
                kw["res_ss"] = R.rd(torch.stack([R.coef(Cn, 8), R.coef(Cn, 9)]), "f32")
            r = R.bn_apply_fwd(**kw)
            out, mask = _bn_fwd(lib, st, dtype, kw, M, Cn, mask=True)
            J("bn_apply_fwd", (M, Cn, with_res, rss, "random"), out, *r["out"], dtype)
            pre, mag = r["pre"]
            clear = pre.abs() > R.TOL["bn_apply_fwd"] * mag
            bits = ((mask.view(-1, 1).int() >> torch.arange(8, dtype=torch.int32)) & 1).bool().view(M, Cn)
            J.check((M, Cn, with_res, rss), float(clear.double().mean()) > 0.999 and torch.equal(bits[clear], (pre > 0)[clear]), "mask bits differ from pre > 0")
    J.report()


def _big_ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int8).float()


@pytest.mark.parametrize("M,Cn", R.BN_CAP_FWD_CASES, ids=["C%d" % c for _, c in R.BN_CAP_FWD_CASES])
def test_bn_apply_fwd_above_the_grid_cap(M, Cn):
    """bf16, more than 2 x 8192 x 256 chunks: every thread's second in-flight chunk, a second trip of its loop and that trip's tail; C = 64 (q = 1), and C = 40 (q = 5:
    the capped grid is rounded down to 8190 blocks -- an unrounded grid would hand a thread other channels on its second chunk).  Integers (fp32 host arithmetic on
    them is exact), with residual and ReLU, out and mask exact"""
    lib, st, J = _lib(), stream(), Judge()
    ss = R.bn_ss(Cn, 0, exact=True)
    y, res = _big_ints((M, Cn), -3, 3, 41), _big_ints((M, Cn), -3, 3, 42)
    want = (y * ss[0].float() + ss[1].float() + res).clamp_min(0)
    assert float(want.max()) <= 24
    yd, rd_, ssd = y.to(torch.bfloat16).cuda(), res.to(torch.bfloat16).cuda(), dev(ss)
    c = Carve([(M * Cn, "bf16"), (M * Cn // 8, "u8")])
    out, mask = c.views
    launch(c, lambda: lib.bn_apply_fwd_mask(DT["bf16"], yd.data_ptr(), ssd.data_ptr(), rd_.data_ptr(), None, out.data_ptr(), mask.data_ptr(), M, Cn, st))
    J.exact((M, Cn, "mask kernel out"), out.view(M, Cn), want)
    J.exact((M, Cn, "mask"), mask, R.pack_mask(want > 0))
    out.view(torch.int16).fill_(PAT)
    launch(c, lambda: lib.bn_apply_fwd(DT["bf16"], yd.data_ptr(), ssd.data_ptr(), rd_.data_ptr(), 2, out.data_ptr(), M, Cn, st))
    J.exact((M, Cn, "out"), out.view(M, Cn), want)
    J.report()


def _bn_bwd(lib, st, dtype, kw, M, Cn, out=None, mask=None, with_dres=True, count_ptr=None, count=None, init=None):
    """-> (dy, dres or None, dgamma, dbeta) on the host; dgamma / dbeta pre-filled with `init` [2][C]"""
    dout, y, ss, gamma, dstats = dev(kw["dout"], dtype), dev(kw["y"], dtype), dev(kw["ss"]), dev(kw["gamma"]), dev(kw["dstats"])
    o = dev(out, dtype)
    mk = None if mask is None else R.pack_mask(mask).cuda()
    c = Carve([(M * Cn, dtype), (M * Cn, dtype), (Cn, "f32"), (Cn, "f32")])
    dy, dres, dgamma, dbeta = c.views
    if init is not None:
        dgamma.copy_(init[0].float()); dbeta.copy_(init[1].float())
    cp = None if count_ptr is None else torch.tensor([count_ptr], dtype=torch.float32, device="cuda")
    cnt = kw["count"] if count is None else count
    pg, pb = (dgamma.data_ptr(), dbeta.data_ptr()) if init is not None else (None, None)
    if mask is not None:
        launch(c, lambda: lib.bn_bwd_apply_mask(DT[dtype], dout.data_ptr(), y.data_ptr(), mk.data_ptr(), ss.data_ptr(), gamma.data_ptr(), dstats.data_ptr(), ptr(cp), cnt,
                                                dy.data_ptr(), dres.data_ptr() if with_dres else None, pg, pb, M, Cn, st))
    else:
        launch(c, lambda: lib.bn_bwd_apply(DT[dtype], dout.data_ptr(), y.data_ptr(), ptr(o), ss.data_ptr(), gamma.data_ptr(), dstats.data_ptr(), ptr(cp), cnt, kw["act"],
                                           dy.data_ptr(), dres.data_ptr() if with_dres else None, pg, pb, M, Cn, st))
    if not with_dres:
        assert bool(torch.isnan(dres.float()).all()), "dres = NULL, yet written"
    if init is None:
        assert bool(torch.isnan(dgamma).all()) and bool(torch.isnan(dbeta).all()), "dgamma = NULL, yet written"
    return dy.cpu().view(M, Cn), dres.cpu().view(M, Cn), dgamma.cpu(), dbeta.cpu()


@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_bwd_apply(dtype):
    """dy and dres for act none / Swish / ReLU by the saved output / ReLU by the recomputed pre-activation / ReLU by the mask bits, on the 4-wide and 8-wide shapes;
    count by value and through count_ptr (holding the right value while the float argument is wrong: the pointer must win); dgamma += dstats[C + c] and
    dbeta += dstats[c] once per launch whatever the grid"""
    lib, st, J = _lib(), stream(), Judge()
    for M, Cn in R.BN4 + R.BN8:
        init = torch.stack([R.rd(R.coef(Cn, 11), "f32"), R.rd(R.coef(Cn, 12), "f32")])
        for act, how in ((0, None), (1, None), (2, "out"), (2, "recompute"), (2, "mask")):
            if how == "mask" and Cn % 8:
                continue
            kw = R.bn_bwd_inputs(M, Cn, dtype, act)
            pre, pmag = R.bn_pre(kw["y"], kw["ss"])
            out = keep = None
            if how == "out":                               # a residual was added before the ReLU: the saved output decides
                out = R.rd((pre + R.rd(R.gauss((M, Cn), 870 + M), dtype)).clamp_min(0), dtype)
            elif how is not None:
                keep = pre > 0
                assert int((pre.abs() <= R.TOL["bn_bwd_apply"] * pmag).sum()) == 0, "a pre-activation within the tolerance of zero: choose other data"
            ref = R.bn_bwd_apply(**kw, out=out, mask=keep if how == "mask" else None, keep=keep if how == "recompute" else None)
            for k, (with_dres, use_ptr) in enumerate(((True, False), (False, True))):
                dy, dres, dgamma, dbeta = _bn_bwd(lib, st, dtype, kw, M, Cn, out=out, mask=keep if how == "mask" else None, with_dres=with_dres,
                                                  count_ptr=kw["count"] if use_ptr else None, count=kw["count"] * 3 + 1 if use_ptr else None, init=init if k == 0 else None)
                tag = (M, Cn, act, how, with_dres, use_ptr)
                J("bn_bwd_apply", tag + ("dy",), dy, *ref["dy"], dtype)
                if with_dres:
                    J("bn_bwd_apply", tag + ("dres",), dres, *ref["dres"], dtype)
                if k == 0:                                 # one fp32 addition per channel: bit-exact
                    J.exact(tag + ("dgamma",), dgamma, init[0].float() + kw["dstats"][Cn:].float())
                    J.exact(tag + ("dbeta",), dbeta, init[1].float() + kw["dstats"][:Cn].float())
    J.report()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,Cn", [(4, R.BN_CAP_C), (70, R.BN_CAP_C)] + R.BN_CAP_BWD_CASES, ids=["one-block", "several-blocks", "above-the-cap", "above-the-cap-C40"])
def test_bn_bwd_apply_exact_and_once_per_launch(dtype, M, Cn):
    """integers and powers of two: dy, dres exact; dgamma / dbeta advance by dstats exactly once at one block, at several blocks, and above the backward grid cap
    (more than 2 x 3072 x 256 chunks: second in-flight chunk, second loop trip, tail; C = 64, and C = 40 where the capped grid is rounded down to a multiple of
    q = 5) -- by the mask bits and by the recomputed pre-activation"""
    lib, st, J = _lib(), stream(), Judge()
    kw = R.bn_bwd_exact(M, Cn, seed=M % 97)
    keep = R.bn_pre(kw["y"], kw["ss"])[0] > 0
    ref = R.bn_bwd_apply(**kw, mask=keep)
    init = torch.stack([R.icoef(Cn, 3), R.icoef(Cn, 4)])
    for how in ("mask", "recompute"):
        dy, dres, dgamma, dbeta = _bn_bwd(lib, st, dtype, kw, M, Cn, mask=keep if how == "mask" else None, count_ptr=4.0, count=7.0, init=init)
        J.exact((M, how, "dy"), dy, ref["dy"][0])
        J.exact((M, how, "dres"), dres, ref["dres"][0])
        J.exact((M, how, "dgamma"), dgamma, init[0] + kw["dstats"][Cn:])
        J.exact((M, how, "dbeta"), dbeta, init[1] + kw["dstats"][:Cn])
    J.report()


# ==============================================================================================================================================
# softmax, activations
# ==============================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_fwd_bwd(dtype):
    """V from 1 to 257 (one lane, both sides of one 64-lane trip, several trips): Gaussian rows, a dominant logit, rows shifted by +-1e4, equal logits, a -inf entry;
    backward with and without dadd, dprobs in the activation dtype"""
    lib, st, J = _lib(), stream(), Judge()
    for M in R.SM_M:
        for V in R.SM_V:
            x64 = R.softmax_rows(M, V)
            x = dev(x64)
            c = Carve([(M * V, dtype)])
            launch(c, lambda: lib.softmax_fwd(DT[dtype], x.data_ptr(), c.views[0].data_ptr(), M, V, st))
            p = c.views[0].cpu().view(M, V)
            J("softmax_fwd", (M, V), p, *R.softmax_fwd(x64)["p"], dtype)
            J.check((M, V), bool((p[torch.isinf(x64)] == 0).all()), "a -inf logit has probability 0")
            dp64, dadd64 = R.rd(R.gauss((M, V), 1050 + V), dtype), R.rd(R.gauss((M, V), 1060 + V), "f32")
            dp, dadd = dev(dp64, dtype), dev(dadd64)
            for with_dadd in (False, True):
                c = Carve([(M * V, "f32")])
                launch(c, lambda: lib.softmax_bwd(DT[dtype], dp.data_ptr(), x.data_ptr(), c.views[0].data_ptr(), dadd.data_ptr() if with_dadd else None, M, V, st))
                J("softmax_bwd", (M, V, with_dadd), c.views[0].view(M, V), *R.softmax_bwd(dp64, x64, dadd64 if with_dadd else None)["dx"])
    J.report()


def test_act_f32():
    """the stand-alone Swish / ReLU / GLU, forward and backward, with the planted +-30 and +-100 (no NaN, within bound) and ReLU at +0 and -0 (exact)"""
    lib, st, J = _lib(), stream(), Judge()
    for rows in R.ACT_ROWS:
        for Cn in R.ACT_C:
            for act in (1, 2, 3):
                x64, dy64 = R.act_inputs(rows, Cn, act)
                x, dy = dev(x64), dev(dy64)
                W = x64.shape[1]
                c = Carve([(rows * Cn, "f32"), (rows * W, "f32")])
                launch(c, lambda: lib.act_f32(act, x.data_ptr(), None, c.views[0].data_ptr(), rows, Cn, 0, st))
                launch(c, lambda: lib.act_f32(act, x.data_ptr(), dy.data_ptr(), c.views[1].data_ptr(), rows, Cn, 1, st))
                f, b = c.views[0].cpu().view(rows, Cn), c.views[1].cpu().view(rows, W)
                rf, rb = R.act_fwd(act, x64)["out"], R.act_bwd(act, x64, dy64)["out"]
                if act == 2:
                    J.exact((rows, Cn, "relu fwd"), f, rf[0])
                    J.exact((rows, Cn, "relu bwd"), b, rb[0])
                else:
                    J("act", (rows, Cn, act, "fwd"), f, *rf)
                    J("act", (rows, Cn, act, "bwd"), b, *rb)
    J.report()


# ==============================================================================================================================================
# dropout, casts
# ==============================================================================================================================================
@pytest.mark.parametrize("n", R.DROPOUT_N)
def test_dropout_f32_is_the_host_hash(n):
    """bit-exact: y = x * (0 | fl32(65536 / (65536 - thr))) with the host's mask -- this pins drop_one, and every other mask check of this file rests on it"""
    lib, st, J = _lib(), stream(), Judge()
    x64 = R.rd(R.gauss((n,), 1500 + n % 1000) + 3, "f32")            # no zeros: a dropped element is told from a kept one
    x, rng = dev(x64), rng_tensor()
    for p in (0.1, 0.5, 1.0):
        for strm in (R.RNG_STREAM, 0):
            mask = R.drop_mask(R.RNG, strm, p, (n,))
            c = Carve([(n, "f32")])
            launch(c, lambda: lib.dropout_f32(x.data_ptr(), c.views[0].data_ptr(), p, rng.data_ptr(), strm, n, st))
            J.exact((n, p, strm), c.views[0], x64.float() * mask.float())
    J.report()


@pytest.mark.parametrize("dtype", DTYPES)
def test_cast_rows_and_to_f32_rows(dtype):
    """source and destination pitches larger than N, the destination starting at a column offset inside a wider row (the fusion concatenation at Da = 180): columns
    outside [0, N) and the pitch padding keep their sentinel; bf16 round-to-nearest-even on planted ties; to_f32_rows with and without accumulation"""
    lib, st, J = _lib(), stream(), Judge()
    for N in R.CAST_N:
        for M in (1, 3, 67):
            lds, ldd, off = N + 4, 2 * N + 12, N + 8
            src64 = R.rd(R.gauss((M, lds), 1600 + N + M), "f32")
            ties = torch.tensor([1.00390625, 1.01171875, -1.00390625, 2.0 ** -126 * 1.00390625, 255.5, 3.0e38], dtype=D64)      # halfway cases: even below / even above
            src64.view(-1)[:min(N, 6)] = ties[:min(N, 6)]
            src = dev(src64)
            c = Carve([(M * ldd, dtype)])
            dst = c.views[0]
            launch(c, lambda: lib.cast_rows(DT[dtype], src.data_ptr(), lds, dst.data_ptr() + off * dst.element_size(), ldd, M, N, st))
            got = torch.cat([dst.cpu(), torch.full((ldd,), float("nan"), dtype=TD[dtype])]).double()[off:off + M * ldd].view(M, ldd)
            J.exact((M, N, "cast_rows"), got[:, :N].to(TD[dtype]), src64[:, :N].to(TD[dtype]))
            J.check((M, N, "cast_rows"), bool(torch.isnan(got[:, N:]).all()) and bool(torch.isnan(dst.cpu().float()[:off]).all()), "a column outside [0, N) lost its sentinel")
            # back to fp32: integers (and the bf16 image of the source), so that the accumulation is exact
            s64 = R.rd(R.int_tensor((M, lds), -100, 100, 1650 + N + M) * 0.5, dtype)
            s = dev(s64, dtype)
            pre64 = R.int_tensor((M, ldd), -50, 50, 1660 + N + M)
            for accum in (0, 1):
                c = Carve([(M * ldd + off, "f32")])
                full = c.views[0]
                if accum:
                    full[off:].copy_(pre64.view(-1).float())
                base = full.clone()
                launch(c, lambda: lib.to_f32_rows(DT[dtype], s.data_ptr(), lds, full.data_ptr() + off * 4, ldd, M, N, accum, st))
                want = base.cpu().clone()
                w = want[off:].view(M, ldd)
                w[:, :N] = (s64[:, :N] + (pre64[:, :N] if accum else 0)).float()
                gotf = full.cpu()
                same = torch.equal(gotf.view(torch.int32), want.view(torch.int32))
                J.check((M, N, "to_f32_rows", accum), same, "values, or columns outside [0, N), differ")
    J.report()


# ==============================================================================================================================================
# patch pool / un-pool, average pool, strided rows
# ==============================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
def test_patch_pool_unpool(dtype):
    """ragged last patch (divisor P all the same), T < P, P = 1; the un-pool passes use the mask at the UN-pooled element (b T + t) D + c; exact where P is a power of
    two and where the dropout scale is"""
    lib, st, J = _lib(), stream(), Judge()
    rng = rng_tensor()
    for B, T, P in R.PATCH:
        Tp = (T + P - 1) // P
        for D in R.PATCH_D:
            pow2 = P & (P - 1) == 0
            mk = (lambda s, k: R.rd(R.int_tensor(s, -3, 3, k), dtype)) if pow2 else (lambda s, k: R.rd(R.gauss(s, k), dtype))
            x64, o64 = mk((B, T, D), 1200 + T + D), mk((B, Tp, D), 1210 + T + D)
            res64 = R.rd(R.int_tensor((B, T, D), -3, 3, 1220 + T + D) if pow2 else R.gauss((B, T, D), 1220 + T + D), "f32")
            x, o, res = dev(x64, dtype), dev(o64, dtype), dev(res64)
            c = Carve([(B * Tp * D, dtype), (B * T * D, dtype)])
            launch(c, lambda: lib.patch_pool_fwd(DT[dtype], x.data_ptr(), c.views[0].data_ptr(), B, T, D, P, st))
            launch(c, lambda: lib.patch_pool_bwd(DT[dtype], o.data_ptr(), c.views[1].data_ptr(), B, T, D, P, st))
            rf, rb = R.patch_pool_fwd(x64, P)["y"], R.patch_pool_bwd(o64, T, P)["dx"]
            J("patch", (B, T, P, D, "pool fwd"), c.views[0].view(B, Tp, D), *rf, dtype)
            J("patch", (B, T, P, D, "pool bwd"), c.views[1].view(B, T, D), *rb, dtype)
            if pow2:
                J.exact((B, T, P, D, "pool fwd exact"), c.views[0].view(B, Tp, D), rf[0])
                J.exact((B, T, P, D, "pool bwd exact"), c.views[1].view(B, T, D), rb[0])
            for p in R.DROP_P:
                mask = R.drop_mask(R.RNG, R.RNG_STREAM, p, (B, T, D))
                c = Carve([(B * T * D, "f32"), (B * Tp * D, dtype)])
                launch(c, lambda: lib.patch_unpool_add(DT[dtype], o.data_ptr(), res.data_ptr(), c.views[0].data_ptr(), p, rng.data_ptr(), R.RNG_STREAM, B, T, D, P, st))
                launch(c, lambda: lib.patch_unpool_bwd(DT[dtype], res.data_ptr(), c.views[1].data_ptr(), p, rng.data_ptr(), R.RNG_STREAM, B, T, D, P, st))
                ra, rb = R.patch_unpool_add(o64, res64, mask, P)["out"], R.patch_unpool_bwd(res64, mask, P)["dob"]
                J("patch", (B, T, P, D, p, "unpool add"), c.views[0].view(B, T, D), *ra)
                J("patch", (B, T, P, D, p, "unpool bwd"), c.views[1].view(B, Tp, D), *rb, dtype)
                if pow2 and p in (0.0, 0.5, 1.0):
                    J.exact((B, T, P, D, p, "unpool add exact"), c.views[0].view(B, T, D), ra[0])
                    J.exact((B, T, P, D, p, "unpool bwd exact"), c.views[1].view(B, Tp, D), rb[0])
    J.report()


@pytest.mark.parametrize("dtype", DTYPES)
def test_avgpool(dtype):
    lib, st, J = _lib(), stream(), Judge()
    for N, HW, Cn in R.AVGPOOL:
        pow2 = HW & (HW - 1) == 0
        x64 = R.rd(R.int_tensor((N, HW, Cn), -3, 3, 1300 + HW) if pow2 else R.gauss((N, HW, Cn), 1300 + HW), dtype)
        dy64 = R.rd(R.int_tensor((N, Cn), -3, 3, 1310 + HW) if pow2 else R.gauss((N, Cn), 1310 + HW), dtype)
        x, dy = dev(x64, dtype), dev(dy64, dtype)
        c = Carve([(N * Cn, dtype), (N * HW * Cn, dtype)])
        launch(c, lambda: lib.avgpool_fwd(DT[dtype], x.data_ptr(), c.views[0].data_ptr(), N, HW, Cn, st))
        launch(c, lambda: lib.avgpool_bwd(DT[dtype], dy.data_ptr(), c.views[1].data_ptr(), N, HW, Cn, st))
        rf, rb = R.avgpool_fwd(x64)["y"], R.avgpool_bwd(dy64, HW)["dx"]
        J("avgpool", (N, HW, Cn, "fwd"), c.views[0].view(N, Cn), *rf, dtype)
        J("avgpool", (N, HW, Cn, "bwd"), c.views[1].view(N, HW, Cn), rb[0].contiguous(), rb[1].contiguous(), dtype)
        if pow2:
            J.exact((N, HW, Cn, "fwd exact"), c.views[0].view(N, Cn), rf[0])
            J.exact((N, HW, Cn, "bwd exact"), c.views[1].view(N, HW, Cn), rb[0].contiguous())
    J.report()


def test_strided_rows_add():
    """dx[b][to * step] += src[b][to] on integers: the addressed rows exact, every other row bit-identical; (To - 1) * step >= T rejected"""
    lib, st, J = _lib(), stream(), Judge()
    for B, T, To, step in R.STRIDED:
        for D in R.PATCH_D:
            dx64, src64 = R.int_tensor((B, T, D), -9, 9, 1700 + T + D), R.int_tensor((B, To, D), -9, 9, 1710 + T + D)
            dx64[0, T - 1, 0] = 0.1                                  # not an integer: a row that must not be touched keeps its bits (the last row is addressed only when (To - 1) * step == T - 1)
            src = dev(src64)
            c = Carve([(B * T * D, "f32")])
            c.views[0].copy_(dx64.view(-1).float())
            launch(c, lambda: lib.strided_rows_add(c.views[0].data_ptr(), src.data_ptr(), B, T, To, D, step, st))
            want = R.strided_rows_add(dx64.float(), src64.float(), step)
            J.check((B, T, To, step, D), torch.equal(c.views[0].cpu().view(B, T, D).view(torch.int32), want.view(torch.int32)), "rows differ")
    c = Carve([(2 * 7 * 4, "f32")])
    src = torch.ones(2 * 4 * 4, device="cuda")
    rejected("strided_rows_add", "strided_rows_add", c, c.views[0].data_ptr(), src.data_ptr(), 2, 7, 4, 4, 3, st)          # (4 - 1) * 3 = 9 >= 7
    rejected("strided_rows_add", "strided_rows_add", c, c.views[0].data_ptr(), src.data_ptr(), 2, 6, 4, 4, 2, st)          # (4 - 1) * 2 = 6 >= 6
    J.report()
