"""GPU (-m gpu): the fused convolution-module paths avec_glu_dwconv_fwd_bn (depthwise conv + BatchNorm finalize straight from the column-reduction partials,
bn_finalize_ws_kernel) and avec_dwconv_glu_bwd_bn (BatchNorm + Swish backward folded into the depthwise backward's staging pass) through the C ABI -- the paths
ops.CONVMOD_BN_FUSE = True runs in every conformer block -- together with the unfused chains the library still ships:
    avec_glu_dwconv_fwd(stats) + avec_bn_finalize          and          avec_bn_bwd_reduce + avec_bn_bwd_apply(act = Swish) + avec_dwconv_glu_bwd.

References, all fp64 on the host:
  (a) R.convmod_ref: glu -> pad -> conv1d(groups = C) -> batch_norm(training) -> swish, gradients by autograd from a random `da`, on the dtype-rounded inputs;
  (b) R.convmod_bwd_ref: the same backward formulas evaluated from what the backward kernels are given (the stored BatchNorm input c and the finalized ss), so that
      the column sums (dstats, dw, dbias) can be judged at fp32 level in bf16 mode as well (in bf16, c is stored rounded; (a) does not know that).
Both reduction set-ups of tests/test_gpu_colreduce.py (twopass: NaN-poisoned workspace of the test's own => bn_finalize_ws_kernel / col_finalize; atomics: no workspace
=> avec_bn_finalize on the atomically accumulated `stats`), fp32 and bf16, Gaussian inputs (the positive-valued set of section 3 puts mean / std of the
BatchNorm input near 10, where the 1e-5 bound on du is out of reach of ANY fp32 evaluation -- the host's own reaches 2e-5); every test ends with "both regimes were seen".

Tolerances
  out / du      per (frame, channel), normalised per channel (frames_check), the first and the last K frames of every sequence reported separately:
                1e-5 (fp32), 1e-2 / 2e-2 (bf16 out / du) -- the figures of the existing depthwise test.  A plain fp32 host evaluation of the whole chain reaches
                1.2e-6 on du and 4.8e-7 on out in this metric over the shape list (measured 2026-10-16), so 1e-5 is 8 x the formula's own fp32 error.
  column sums   dstats, dw, dbias and the mean row of ss: |got_c - ref_c| <= R.TOL[...] * scale_c (tests/colreduce_ref.py: 8 x the host fp32 evaluation,
                "convmod dstats" 4.1e-7, "convmod dw" 9.8e-7, "convmod dbias" 4.3e-7, "glu_dwconv stats" 2.0e-6).
  ss rows       derived from that tolerance on the two sums: |var - var_ref| <= TOL (E mag^2 + 2 |mean| E mag) (mag = the conv output with every factor by its
                magnitude), rstd relative 1/2 of that over (var + eps) plus 4 eps_fp32 for rsqrtf, scale / shift / running statistics by propagation (ss_tolerances).
  dgamma, dbeta one fp32 addition of the reduced sums onto the destination: bit-exact, whatever grid.y is.
  fused vs unfused (fp32): out is the same kernel: bit-identical.  du: within DU_FUSE_TOL = 8 x 7.0e-7 = 5.6e-6 of each other, per channel, where 7.0e-7 is the
                worst per-channel error of a plain fp32 host evaluation (torch autograd in fp32) of the backward formula over the shape list (measured 2026-10-16,
                tests/test_colreduce_ref.py::test_du_fused_tolerance_is_8x_host_fp32).  Measured on MI355X (ROCm 7.2, torch 2.10, 2026-10-16): 5.3e-7.
  Measured worst per-column ratios on the same machine: dstats 6.4e-8, dw 1.1e-7 (unfused 8.4e-8), dbias 4.8e-8 (unfused 4.2e-8); worst ss error 0.11 of its
  tolerance.  Wall time of this module and tests/test_gpu_colreduce.py together: 73 s for 182 cases (the parent's GPU suite: 554 s).
"""
import pytest
import torch

from tests import colreduce_ref as R
from tests.test_gpu_colreduce import DT, INIT, Ws, _lib, both_seen, check, dev, f32, put

pytestmark = pytest.mark.gpu

ACT_SWISH = 1
EPS, MOM = 1e-5, 0.1
CASES = pytest.mark.parametrize("setup,dtype,mode", [(s, d, "gauss") for s in ("twopass", "atomics") for d in ("f32", "bf16")])
OUT_TOL = {"f32": 1e-5, "bf16": 1e-2}
DU_TOL = {"f32": 1e-5, "bf16": 2e-2}
DU_FUSE_TOL = 8 * R.HOST_DU_FP32_WORST
AUTOGRAD_SUM_TOL = {"f32": 2e-5, "bf16": 2e-2}


def frames_check(name, case, got, ref, K, tol):
    """got, ref [B][T'][C]: per (frame, channel) error, normalised per channel by that channel's largest reference value, over all frames and -- reported on their own, so
    that a failure names the place -- over the first K and the last K frames of every sequence.  (Normalising an edge by the edge's own largest value was tried and is
    mis-designed for the fixed 1e-5: with B K = 3 samples a channel's edge maximum can be 10x below the channel's, and the fp32 HOST evaluation of the chain then reaches
    5.8e-6 itself, 8 x that is 4.6e-5; per channel over all frames the host reaches 1.2e-6, 8 x that is 9.4e-6.)"""
    got, ref = got.detach().cpu().double(), ref.double()
    assert bool(torch.isfinite(got).all()), (name, case, "not every element was written")
    den = ref.reshape(-1, ref.shape[-1]).abs().amax(0).clamp_min(1e-30)
    for part, sl in (("first K", slice(0, K)), ("last K", slice(-K, None)), ("all", slice(None))):
        r = (got[:, sl] - ref[:, sl]).abs().reshape(-1, ref.shape[-1]).amax(0) / den
        assert float(r.max()) <= tol, (name, case, part, "channel %d" % int(r.argmax()), float(r.max()), tol)
    return float(r.max())


def ss_tolerances(r, n, gamma, beta):
    """per-channel absolute tolerances of (scale, shift, mean, rstd, var) from the section-3 tolerance on the two column sums (see the module docstring)"""
    tol = R.TOL["glu_dwconv stats"]
    C = gamma.numel()
    mag = r["mag"].reshape(-1, C)
    e1, e2 = mag.sum(0) / n, (mag * mag).sum(0) / n
    mean, var, rs = r["mean"], r["var"], r["ss"][3]
    t_mean = tol * e1 + R.EPS32 * mean.abs()
    t_var = tol * (e2 + 2 * mean.abs() * e1)
    rel_rs = 0.5 * t_var / (var + EPS) + 4 * R.EPS_F32
    gr = (gamma * rs).abs()
    return dict(scale=gr * (rel_rs + R.EPS_F32), shift=gr * t_mean + (mean * gr).abs() * rel_rs + 2 * R.EPS_F32 * (beta.abs() + (mean * gr).abs()),
                mean=t_mean, rstd=rs * rel_rs, var=t_var)


def ss_check(name, case, ss, r, t):
    ss = ss.detach().cpu().double().view(4, -1)
    for k, row in enumerate(("scale", "shift", "mean", "rstd")):
        err = (ss[k] - r["ss"][k]).abs()
        assert bool(torch.isfinite(ss[k]).all()) and bool((err <= t[row]).all()), (name, case, row, "channel %d" % int((err / t[row]).argmax()), float((err / t[row]).max()))
    return max(float(((ss[k] - r["ss"][k]).abs() / t[row]).max()) for k, row in enumerate(("scale", "shift", "mean", "rstd")))


class Inputs:
    def __init__(self, shape, i, dtype, mode):
        self.shape = shape
        B, T, C, K, stride, causal = shape
        self.padl, self.To = (K - 1 if causal else K // 2), (T - 1) // stride + 1
        x = R.convmod_inputs(mode, shape, i)
        self.u, self.ub = put(x["u"], dtype)
        self.da, self.dab = put(x["da"], dtype)
        self.w, self.bias, self.gamma, self.beta, self.rm0, self.rv0 = [f32(x[k]) for k in ("w", "bias", "gamma", "beta", "rmean", "rvar")]
        self.wb, self.bb, self.gb, self.btb, self.rmb, self.rvb = [t.cpu().double() for t in (self.w, self.bias, self.gamma, self.beta, self.rm0, self.rv0)]
        self.dt, self.adt = DT[dtype], self.u.dtype


def fwd_fused(lib, ws, x, running=True):
    B, T, C, K, stride, _ = x.shape
    d = dev()
    out, stats, ss = torch.empty(B * x.To, C, dtype=x.adt, device=d), torch.zeros(2 * C, device=d), torch.full((4 * C,), float("nan"), device=d)
    rm, rv, nbt = x.rm0.clone(), x.rv0.clone(), torch.tensor([3], dtype=torch.int64, device=d)
    p = (lambda t: t.data_ptr()) if running else (lambda t: None)
    used = ws.run(lambda: lib.glu_dwconv_fwd_bn(x.dt, x.u.data_ptr(), x.w.data_ptr(), x.bias.data_ptr(), out.data_ptr(), stats.data_ptr(), B, T, C, K, stride, x.padl,
                                                x.gamma.data_ptr(), x.beta.data_ptr(), p(rm), p(rv), p(nbt), MOM, EPS, ss.data_ptr(), ws.stream))
    return out, ss, rm, rv, nbt, stats, used


def fwd_unfused(lib, ws, x):
    B, T, C, K, stride, _ = x.shape
    d = dev()
    out, stats, ss = torch.empty(B * x.To, C, dtype=x.adt, device=d), torch.zeros(2 * C, device=d), torch.full((4 * C,), float("nan"), device=d)
    rm, rv, nbt = x.rm0.clone(), x.rv0.clone(), torch.tensor([3], dtype=torch.int64, device=d)
    ws.run(lambda: lib.glu_dwconv_fwd(x.dt, x.u.data_ptr(), x.w.data_ptr(), x.bias.data_ptr(), out.data_ptr(), stats.data_ptr(), B, T, C, K, stride, x.padl, ws.stream))
    lib.bn_finalize(stats.data_ptr(), 1, None, float(B * x.To), x.gamma.data_ptr(), x.beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), MOM, EPS, ss.data_ptr(), C, 1,
                    ws.stream)
    torch.cuda.synchronize()
    return out, ss, rm, rv, nbt


@CASES
def test_glu_dwconv_fwd_bn(setup, dtype, mode):
    """conv output; ss rows scale / shift / mean / rstd per channel; running mean / unbiased running variance / num_batches_tracked, also with the running-statistics
    pointers NULL; count = B * To (stride 2 with odd T; a single row, n = 1); fused against unfused"""
    lib, seen, worst = _lib(), set(), 0.0
    with Ws(setup) as ws:
        for i, shape in enumerate(R.SHAPES_CONVMOD):
            B, T, C, K, stride, causal = shape
            case = shape + (dtype, setup, mode)
            x = Inputs(shape, i, dtype, mode)
            n = float(B * x.To)
            out, ss, rm, rv, nbt, stats, used = fwd_fused(lib, ws, x)
            seen.add("twopass" if used else "atomics")
            if setup == "atomics":
                assert not used
            if used:
                assert not bool(stats.any()), (case, "`stats` is documented as used only when the reduction runs on atomics")
            r = R.convmod_ref(x.ub, x.wb, x.bb, x.gb, x.btb, None, stride, x.padl, EPS)
            t = ss_tolerances(r, n, x.gb, x.btb)
            frames_check("glu_dwconv_fwd_bn out", case, out.view(B, x.To, C), r["c"], K, OUT_TOL[dtype])
            worst = max(worst, ss_check("glu_dwconv_fwd_bn ss", case, ss, r, t))
            # running statistics: (1 - m) old + m new, the variance with the unbiased factor n / max(n - 1, 1)
            fac = n / max(n - 1.0, 1.0)
            rm_ref, rv_ref = (1 - MOM) * x.rmb + MOM * r["mean"], (1 - MOM) * x.rvb + MOM * r["var"] * fac
            for nm, got, ref, tol in (("running_mean", rm, rm_ref, MOM * t["mean"] + 2 * R.EPS_F32 * (x.rmb.abs() + r["mean"].abs())),
                                      ("running_var", rv, rv_ref, MOM * fac * t["var"] + 2 * R.EPS_F32 * (x.rvb.abs() + r["var"] * fac))):
                err = (got.cpu().double() - ref).abs()
                assert bool((err <= tol).all()), ("glu_dwconv_fwd_bn", case, nm, float((err / tol).max()))
            assert int(nbt) == 4, (case, int(nbt))
            # NULL running statistics: the same ss, nothing else touched
            out_n, ss_n, rm_n, rv_n, nbt_n, _, used_n = fwd_fused(lib, ws, x, running=False)
            assert used_n == used and torch.equal(out_n, out) and torch.equal(rm_n, x.rm0) and int(nbt_n) == 3
            ss_check("glu_dwconv_fwd_bn ss (no running statistics)", case, ss_n, r, t)
            if used:
                assert torch.equal(ss_n, ss), (case, "the two-pass path is deterministic")
            # the unfused chain: same conv kernel (bit-identical out), ss to the same tolerances
            out_u, ss_u, rm_u, rv_u, nbt_u = fwd_unfused(lib, ws, x)
            assert torch.equal(out_u, out), (case, "fused and unfused conv outputs differ")
            ss_check("glu_dwconv_fwd + bn_finalize ss", case, ss_u, r, t)
            assert int(nbt_u) == 4 and bool(((rm_u.cpu().double() - rm_ref).abs() <= MOM * t["mean"] + 2 * R.EPS_F32 * (x.rmb.abs() + r["mean"].abs())).all())
        print("glu_dwconv_fwd_bn %s %s %s: worst ss error / tolerance %.3g" % (setup, dtype, mode, worst))
        both_seen(ws, seen, "avec_glu_dwconv_fwd_bn")


@CASES
def test_dwconv_glu_bwd_bn(setup, dtype, mode):
    """du (both halves), dw, dbias, dgamma, dbeta of the fused backward, each accumulated onto non-zero contents, and the unfused three-launch chain"""
    lib, seen, worst_fuse = _lib(), set(), 0.0
    d = dev()
    with Ws(setup) as ws:
        for i, shape in enumerate(R.SHAPES_CONVMOD):
            B, T, C, K, stride, causal = shape
            if stride != 1:
                continue                                      # the fused backward is stride 1 only: its signature has no stride
            case = shape + (dtype, setup, mode)
            x = Inputs(shape, i, dtype, mode)
            M = B * T
            c, ss = fwd_fused(lib, ws, x)[:2]
            dstats = torch.zeros(2 * C, device=d)
            ws.run(lambda: lib.bn_bwd_reduce(x.dt, x.da.data_ptr(), c.data_ptr(), None, ss.data_ptr(), ACT_SWISH, dstats.data_ptr(), M, C, ws.stream))
            fr = R.convmod_bwd_ref(x.ub, x.wb, c.cpu().double().view(B, T, C), ss.cpu().double().view(4, C), x.gb, x.dab, x.padl)
            check("convmod dstats", case, mode, dstats, fr["dstats"], 0.0)
            # ---- fused ----
            du = torch.full((M, 2 * C), float("nan"), dtype=x.adt, device=d)
            dw, dbias = torch.full((K, C), INIT[0], device=d), torch.full((C,), INIT[1], device=d)
            dgamma, dbeta = torch.full((C,), INIT[0], device=d), torch.full((C,), INIT[1], device=d)
            used = ws.run(lambda: lib.dwconv_glu_bwd_bn(x.dt, x.da.data_ptr(), c.data_ptr(), ss.data_ptr(), x.gamma.data_ptr(), dstats.data_ptr(), float(M), x.u.data_ptr(),
                                                        x.w.data_ptr(), du.data_ptr(), dw.data_ptr(), dbias.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), B, T, C, K, x.padl,
                                                        ws.stream))
            seen.add("twopass" if used else "atomics")
            if setup == "atomics":
                assert not used
            check("convmod dw", case, mode, dw, fr["dw"], INIT[0])
            check("convmod dbias", case, mode, dbias, fr["dbias"], INIT[1])
            assert torch.equal(dgamma.cpu(), INIT[0] + dstats.cpu()[C:]) and torch.equal(dbeta.cpu(), INIT[1] + dstats.cpu()[:C]), (case, "dgamma / dbeta += dstats, exactly once")
            frames_check("dwconv_glu_bwd_bn du", case, du.view(B, T, 2 * C), fr["du"], K, DU_TOL[dtype])
            # ---- the whole chain by autograd ----
            ar = R.convmod_ref(x.ub, x.wb, x.bb, x.gb, x.btb, x.dab, 1, x.padl, EPS)
            frames_check("dwconv_glu_bwd_bn du (autograd)", case, du.view(B, T, 2 * C), ar["du"], K, DU_TOL[dtype])
            # the sums once more against autograd: c and ss are the device's own (fp32- / bf16-rounded) here and exact there, so this is no rounding bound -- it is
            # the check that (b) is the right formula, at a tolerance a wrong term (O(1) of the scale) cannot meet
            for nm, got, init, ref, scale in (("dw", dw, INIT[0], ar["dw"], fr["dw"][1]), ("dbias", dbias, INIT[1], ar["dbias"], fr["dbias"][1]),
                                              ("dgamma", dgamma, INIT[0], ar["dgamma"], fr["dstats"][1][C:]), ("dbeta", dbeta, INIT[1], ar["dbeta"], fr["dstats"][1][:C])):
                e = R.worst(got.cpu().double().flatten() - init, ref.flatten(), scale.flatten() + abs(init))
                assert e <= AUTOGRAD_SUM_TOL[dtype], ("dwconv_glu_bwd_bn (autograd)", case, nm, e)
            # ---- unfused: bn_bwd_apply(act = Swish) + dwconv_glu_bwd, from the same dstats ----
            dc, du_u = torch.empty(M, C, dtype=x.adt, device=d), torch.full((M, 2 * C), float("nan"), dtype=x.adt, device=d)
            dw_u, dbias_u = torch.full((K, C), INIT[0], device=d), torch.full((C,), INIT[1], device=d)
            dgamma_u, dbeta_u = torch.full((C,), INIT[0], device=d), torch.full((C,), INIT[1], device=d)
            lib.bn_bwd_apply(x.dt, x.da.data_ptr(), c.data_ptr(), None, ss.data_ptr(), x.gamma.data_ptr(), dstats.data_ptr(), None, float(M), ACT_SWISH, dc.data_ptr(), None,
                             dgamma_u.data_ptr(), dbeta_u.data_ptr(), M, C, ws.stream)
            ws.run(lambda: lib.dwconv_glu_bwd(x.dt, dc.data_ptr(), x.u.data_ptr(), x.w.data_ptr(), du_u.data_ptr(), dw_u.data_ptr(), dbias_u.data_ptr(), B, T, C, K, 1, x.padl, ws.stream))
            assert torch.equal(dgamma_u, dgamma) and torch.equal(dbeta_u, dbeta), (case, "unfused dgamma / dbeta")
            frames_check("bn_bwd_apply + dwconv_glu_bwd du", case, du_u.view(B, T, 2 * C), fr["du"], K, DU_TOL[dtype])
            if dtype == "f32":                                # (in bf16 the unfused chain rounds dc to bf16 on its way through memory)
                check("convmod dw (unfused)", case, mode, dw_u, fr["dw"], INIT[0])
                check("convmod dbias (unfused)", case, mode, dbias_u, fr["dbias"], INIT[1])
                e = float(R.elem_ratio(du.cpu().view(M, 2 * C), du_u.cpu().view(M, 2 * C)).max())
                worst_fuse = max(worst_fuse, e)
                assert e <= DU_FUSE_TOL, ("du fused vs unfused", case, e, DU_FUSE_TOL)
        print("dwconv_glu_bwd_bn %s %s %s: worst fused-vs-unfused du difference %.3g (tolerance %.3g)" % (setup, dtype, mode, worst_fuse, DU_FUSE_TOL))
        both_seen(ws, seen, "avec_dwconv_glu_bwd_bn")


def test_dwconv_glu_bwd_bn_argument_errors():
    """what include/avec_hip.h and the argument checks forbid is refused, not launched: K > 16, C % 4 != 0, pad_left >= K, count <= 0, a NULL operand, and dgamma
    without dbeta (the kernel adds to both under one test; before the check this stored through NULL)"""
    from avec_amd import runtime as rt
    lib, d = _lib(), dev()
    B, T, C, K = 1, 8, 8, 3
    z = lambda *s: torch.zeros(*s, device=d)
    da, c, ss, g, ds, u, w, du, dw, db, dg, dbt = z(B * T, C), z(B * T, C), z(4 * C), z(C), z(2 * C), z(B * T, 2 * C), z(K, C), z(B * T, 2 * C), z(K, C), z(C), z(C), z(C)
    p = lambda t: t.data_ptr()

    def call(**kw):
        a = dict(da=p(da), c=p(c), count=float(B * T), dgamma=p(dg), dbeta=p(dbt), C=C, K=K, padl=1)
        a.update(kw)
        lib.dwconv_glu_bwd_bn(0, a["da"], a["c"], p(ss), p(g), p(ds), a["count"], p(u), p(w), p(du), p(dw), p(db), a["dgamma"], a["dbeta"], B, T, a["C"], a["K"], a["padl"], rt.stream())
    call()
    call(dgamma=None, dbeta=None)
    for kw in (dict(K=17), dict(C=6), dict(padl=3), dict(count=0.0), dict(c=None), dict(da=None)):
        with pytest.raises(RuntimeError, match="dwconv_glu_bwd_bn"):
            call(**kw)
    for kw in (dict(dbeta=None), dict(dgamma=None)):
        with pytest.raises(RuntimeError, match="dgamma and dbeta"):
            call(**kw)
    torch.cuda.synchronize()
    assert not bool(dg.any()) and not bool(dbt.any())


@pytest.mark.parametrize("setup", ["twopass", "atomics"])
def test_onepass_variance_envelope_fused(setup):
    """the envelope of tests/test_gpu_colreduce.py::test_onepass_variance_envelope through avec_glu_dwconv_fwd_bn: K = 1, unit tap, bias = the channel mean, gate half
    zero (sigmoid = 1/2), 32 x 200 = 6400 rows, per-channel mean / std in {0, 5, 50, 300}.  twopass (what the runtime runs at this size): KAPPA as it stands; measured
    2.2 / 2.2 / 3.5 / 2.8 on MI355X (ROCm 7.2, 2026-10-16).  atomics: KAPPA plus the recursive-summation term of 224 atomics, see below"""
    lib, d = _lib(), dev()
    B, T, C = 32, R.VAR_ROWS // 32, 128
    x64 = R.variance_case(B * T, C)
    mean64 = x64.mean(0)
    u = f32(torch.cat([2 * (x64 - mean64).view(B, T, C), torch.zeros(B, T, C, dtype=torch.float64)], -1))
    w, bias = torch.ones(1, C, device=d), f32(mean64)
    cb = bias.cpu().double() + 0.5 * u.cpu().double()[..., :C].reshape(-1, C)
    mean, var = cb.mean(0), cb.var(0, unbiased=False)
    with Ws(setup) as ws:
        out, stats, ss = torch.empty(B * T, C, device=d), torch.zeros(2 * C, device=d), torch.empty(4 * C, device=d)
        g, b = torch.ones(C, device=d), torch.zeros(C, device=d)
        used = ws.run(lambda: lib.glu_dwconv_fwd_bn(0, u.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), stats.data_ptr(), B, T, C, 1, 1, 0, g.data_ptr(), b.data_ptr(),
                                                    None, None, None, MOM, 0.0, ss.data_ptr(), ws.stream))
        assert used == (setup == "twopass")
    got = 1 / ss.cpu().double().view(4, C)[3] ** 2
    rel = (got - var).abs() / var
    const = rel / R.var_envelope(mean, var, 1.0)
    # Without a workspace the 224 partial sums of a channel reach the accumulator as 224 float atomics in whatever order the workgroups retire: recursive summation of n
    # numbers carries up to (n - 1) u sum|p| = (n - 1) / 2 eps_fp32 on top of the partials' own error (Higham, Accuracy and Stability, section 4.2), which kappa -- taken
    # from a pairwise host sum -- does not contain.  Measured on MI355X: 3.6 .. 4.1 / 7.6 .. 9.8 / 7.0 .. 11.7 / 7.6 .. 10.1 over three runs.
    kappa = R.KAPPA + ((R.dw_grid(B, T, C)[1] - 1) / 2 if setup == "atomics" else 0)
    for k, r in enumerate(R.VAR_RATIOS):
        print("glu_dwconv_fwd_bn %-8s mean/std %5g: relative variance error %.3g, constant %.3g (allowed %.3g)" % (setup, r, float(rel[k::4].max()), float(const[k::4].max()), kappa))
    assert bool((rel <= R.var_envelope(mean, var, kappa)).all()), (float(const.max()), kappa)


@pytest.mark.parametrize("fuse", [True, False])
def test_conformer_block_golden_with_and_without_bn_fusion(fuse):
    """ops.CONVMOD_BN_FUSE flipped in-process around the block_relpos golden (lengths mask): both settings meet the golden's existing tolerances, and the flag really
    selects the path (the fused forward entry point is called with it and not without)"""
    import nnet
    from avec_amd import ops
    from avec_amd.nnet.modules import LengthMask
    from tests.helpers import load_npz, rel_err
    from tests.test_gpu_parity import ATT, CONV, check_grads, nodrop
    import avec_amd
    avec_amd.set_compute_dtype("f32")
    avec_amd.manual_seed(1234)
    calls = []
    orig = ops.lib.glu_dwconv_fwd_bn
    old = ops.CONVMOD_BN_FUSE

    def counted(*a):
        calls.append(1)
        return orig(*a)
    try:
        ops.lib.__dict__["glu_dwconv_fwd_bn"] = counted
        ops.CONVMOD_BN_FUSE = fuse
        g = load_npz("block_relpos")
        D, De, T, stride, patch, H = [int(v) for v in g["meta"]]
        blk = nodrop(nnet.ConformerBlock(dim_model=D, dim_expand=De, ff_ratio=4, att_params=ATT("RelPos1dMultiHeadAttention"), drop_rate=0.1, conv_stride=stride, conv_params=CONV))
        blk.load_state_dict(g["sd"])
        blk = blk.to(dev()).train()
        x = g["x"].to(dev()).requires_grad_(True)
        y = blk(x, mask=LengthMask(g["lengths"].to(dev())))
        assert rel_err(y.detach().cpu(), g["y"]) < 1e-3
        (y * g["w"].to(dev())).sum().backward()
        assert rel_err(x.grad.cpu(), g["dx"]) < 2e-3
        check_grads(blk, g["grads"], 2e-3)
        sd = blk.state_dict()
        for k in ["conv_module.layers.4.running_mean", "conv_module.layers.4.running_var"]:
            assert torch.allclose(sd[k].cpu(), g["sd_after"][k], atol=1e-4), k
        assert int(sd["conv_module.layers.4.num_batches_tracked"]) == 1
        assert bool(calls) == fuse, "ops.CONVMOD_BN_FUSE = %s but the fused forward entry point was called %d times" % (fuse, len(calls))
    finally:
        ops.CONVMOD_BN_FUSE = old
        ops.lib.__dict__["glu_dwconv_fwd_bn"] = orig
        avec_amd.set_compute_dtype("f32")
