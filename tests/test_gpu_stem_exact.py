"""GPU (-m gpu): the visual stem kernels -- csrc/stem3p.hip (stem3p_fwd_kernel, stem3p_reduce_kernel, stem3p_dz_kernel, both instances of stem3p_wgrad_roles_kernel),
csrc/stem3d.hip (stem3_fwd_kernel, stem3_wgrad_kernel) and the stem tail of csrc/frontend.hip (stem_im2col_kernel, stem_pool_fwd_kernel, stem_pool_bwd_apply8_kernel /
stem_pool_bwd_apply_kernel) -- called through the C ABI, reproduce the integer references of tests/stem_exact_ref.py EXACTLY, at every element.

tests/stem_exact_ref.py holds the operands (video in {-2 .. 2}, weights in {-1, 0, 1} with eight one-hot channels, power-of-two BatchNorm constants, integer pooled
gradients) and asserts on the reference alone that a correct kernel has no choice (tests/test_stem_exact_ref.py runs those conditions on every operand set used here
without a GPU).  Every comparison is torch.equal through assert_exact: a failure names (frame, row, column, channel) or (channel, kd, kh, kw) with expected and got.
Outputs are NaN-filled (idx: 0xEE) with a guard row behind them; accumulated outputs start from non-zero dyadic values.

Every stem3p case asserts, through avec_stem3p_geom, the band layout its name promises: s3p_geom() serves W = 88 and W = 96 only, and a retuned geometry must not
silently turn a "two bands" case into something else -- move the case to a shape that reaches the layout again.  Every launch that notes its kernel is checked with
avec_last_kernel.

Regimes: every entry point that leaves through a ColPlan (the statistics of both forward kernels, stem3p_reduce, the three weight gradients) runs with the reduction
workspace owned by Ws("twopass") and by Ws("atomics") of tests/test_gpu_colreduce.py: exact in both, and the poisoned workspace shows which branch ran.

Not here: the fp8 products and the env-forced variants (AVEC_S3P_ABL, AVEC_S3W_ABL: read once per process).
"""
import ctypes

import pytest
import torch

from tests import stem_exact_ref as S
from tests.test_gpu_colreduce import Ws

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
NAN = float("nan")
BF, FP = torch.bfloat16, torch.float32
DT = {"f32": (F32, FP), "bf16": (BF16, BF)}
SETUPS = ("twopass", "atomics")


def dev():
    return torch.device("cuda:0")


def _lib():
    from avec_amd.lib import lib
    return lib


def up(t, dtype, off=0):
    """the float64 tensor on the device as `dtype` (exact: the reference checks have seen the values), `off` elements behind a 256-byte aligned address"""
    n = t.numel()
    buf = torch.zeros(n + off + 64, dtype=dtype, device=dev())
    buf[off:off + n].copy_(t.reshape(-1).to(dtype))
    return buf[off:off + n]


def nan_rows(rows, cols, dtype, init=None):
    """[rows + 1][cols]: NaN (or `init` in the first `rows` rows); the last row is the guard"""
    buf = torch.full((rows + 1, cols), NAN, dtype=dtype, device=dev())
    if init is not None:
        buf[:rows] = init if not torch.is_tensor(init) else init.to(dtype).to(dev())
    return buf


def idx_rows(rows, cols):
    return torch.full((rows + 1, cols), 0xEE, dtype=torch.uint8, device=dev())


def assert_guard(buf, what):
    if buf.dtype == torch.uint8:
        assert bool((buf[-1] == 0xEE).all()), "%s: the guard bytes behind idx were written" % what
    else:
        assert bool(torch.isnan(buf[-1]).all()), "%s: the guard row behind the output was written" % what


def last_kernel():
    return _lib().raw("avec_last_kernel")().decode()


def geom(shape):
    out = (ctypes.c_int * 10)()
    return tuple(out) if _lib().raw("avec_stem3p_geom")(*shape, out) else None


def stats_buf():
    b = nan_rows(2, 64, FP)
    b[0], b[1] = S.STAT_INIT
    return b


def check_stats(buf, ref, what):
    S.assert_exact(buf[:2].cpu().double() - torch.tensor(S.STAT_INIT, dtype=S.F64).unsqueeze(1), ref, (2, 64), S.STAT_NAMES, what)
    assert_guard(buf, what)


def affine_bufs():
    dg, db = nan_rows(1, 64, FP, S.DG_INIT), nan_rows(1, 64, FP, S.DB_INIT)
    return dg, db


def check_affine(dg, db, dstats, what):
    S.assert_exact(dg[0].cpu().double() - S.DG_INIT, dstats[1], (64,), ("channel",), what + ": dgamma += dstats[1]")
    S.assert_exact(db[0].cpu().double() - S.DB_INIT, dstats[0], (64,), ("channel",), what + ": dbeta += dstats[0]")
    assert_guard(dg, what), assert_guard(db, what)


def check_dw(dw, init, ref, what):
    S.assert_exact(dw[:64].cpu().double() - init, ref, (64, 5, 7, 7), S.TAP_NAMES, what)
    assert_guard(dw, what)


# ---- stem3p ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.S3P_CASES, ids=[c["id"] for c in S.S3P_CASES])
def test_stem3p_geometry_is_what_the_case_names(case):
    """avec_stem3p_geom (s3p_geom / s3w_geom themselves) reports the band layout of the case's name, and the two `supported` queries agree with it"""
    lib = _lib()
    got = geom(case["shape"])
    assert got == case["geom"], ("%s %s: avec_stem3p_geom reports (NB, pn, PH, PW, OH, OW, pitch, fused, CH, NCH) = %s, the case means %s -- s3p_geom / s3w_geom were "
                                 "retuned: move the case to a shape that reaches this layout again" % (case["id"], case["shape"], got, case["geom"]))
    assert lib.raw("avec_stem3p_supported")(*case["shape"]) == 1 and lib.raw("avec_stem3d_supported")(*case["shape"]) == 1
    assert lib.raw("avec_stem3p_wgrad_supported")(*case["shape"]) == case["geom"][7]


def test_stem3p_serves_two_widths():
    """the pooled path exists at W = 88 and W = 96 only (RING = 6 OW >= 3 OW + 128 and PW <= 24): the neighbouring multiples of 8 are declined"""
    for W, ok in [(64, False), (80, False), (88, True), (96, True), (104, False), (112, False)]:
        assert (geom((1, 2, 16, W)) is not None) == ok, W
    pitches = {c["geom"][6] for c in S.S3P_CASES if c["geom"][7]}
    assert pitches == set(S.S3P_ROLES_INSTANCE), "both instances of stem3p_wgrad_roles_kernel (pitch 208: <208>, any other: <0>) must be launched by some case"
    assert any(not c["geom"][7] for c in S.S3P_CASES), "some case must take the dz + stem3d_wgrad fallback"


@pytest.mark.parametrize("setup", SETUPS)
@pytest.mark.parametrize("case", S.S3P_CASES, ids=[c["id"] for c in S.S3P_CASES])
def test_stem3p_exact(case, setup):
    """forward (zp, idx, statistics; again without statistics), reduce (masked dpool, dstats), dz and the weight gradient (fused where s3w_geom accepts, else
    avec_stem3d_wgrad on dz), each with dstats = 0 (the routing alone) and with dstats != 0 (the whole formula), count by value and through count_ptr"""
    lib = _lib()
    cid, shape = case["id"], case["shape"]
    assert geom(shape) == case["geom"], (cid, geom(shape), "move the case to a shape that reaches the layout again")
    o = S.s3p_operands(cid)
    S.check_s3p(o)
    B, T, H, W = shape
    k, F, OH, OW, PH, PW, M = o["k"], o["F"], o["OH"], o["OW"], o["PH"], o["PW"], o["M"]
    P = F * PH * PW
    fused = bool(case["geom"][7])
    vb, vf = up(o["video"], BF), up(o["video"], FP)
    w8 = up(S.pack_w8(o["w"], True), BF)
    bias, gamma, ss = up(k["bias"], FP), up(k["gamma"], FP), up(S.ss_of(k), FP)
    count_dev = up(torch.tensor([S.COUNT]), FP)
    dw_init = S.s3p_dw_init(k).view(64, 245)
    with Ws(setup) as ws:
        st = ws.stream
        # forward, with and without statistics
        for want in (True, False):
            zp, idx, stats = nan_rows(P, 64, BF), idx_rows(P, 64), stats_buf()
            used = ws.run(lambda: lib.stem3p_fwd(vb.data_ptr(), w8.data_ptr(), bias.data_ptr(), gamma.data_ptr(), zp.data_ptr(), idx.data_ptr(),
                                                 stats.data_ptr() if want else None, B, T, H, W, st))
            assert last_kernel() == "stem3p_fwd_kernel"
            what = "%s fwd (%s, stats %s)" % (cid, setup, want)
            assert used == (want and setup == "twopass"), what
            S.assert_exact(zp[:P].cpu(), o["zp"], (F, PH, PW, 64), S.PIX_NAMES, what + ": zp")
            S.assert_exact(idx[:P].cpu(), o["idx"], (F, PH, PW, 64), S.PIX_NAMES, what + ": idx")
            assert_guard(zp, what), assert_guard(idx, what)
            check_stats(stats, o["stats"] if want else torch.zeros(2, 64, dtype=S.F64), what + ": statistics")
        # reduce: one pass at this size in either regime (fewer than 16 384 atomics); test_stem3p_reduce_regimes runs the other branch
        dpm, dstats = nan_rows(P, 64, BF, o["dp"].view(P, 64)), stats_buf()
        zpd = up(o["zp"], BF)
        used = ws.run(lambda: lib.stem3p_reduce(dpm.data_ptr(), zpd.data_ptr(), ss.data_ptr(), dstats.data_ptr(), F, PH, PW, st))
        assert not used
        S.assert_exact(dpm[:P].cpu(), o["d"], (F, PH, PW, 64), S.PIX_NAMES, cid + " reduce: masked dpool")
        assert_guard(dpm, cid + " reduce")
        check_stats(dstats, o["dstats"], cid + " reduce: dstats")
        # dz and the weight gradient, from the reference's masked gradients and window slots
        dm, ix = up(o["d"], BF), up(o["idx"], torch.uint8)
        zero = torch.zeros(2, 64, dtype=S.F64)
        for name, ds, by_ptr in (("route", zero, False), ("full", k["dstats"], True)):
            dsd = up(ds, FP)
            cnt = (count_dev.data_ptr(), 1.0) if by_ptr else (None, S.COUNT)          # (by pointer: the value argument is a decoy)
            common = (vb.data_ptr(), w8.data_ptr(), bias.data_ptr(), dm.data_ptr(), ix.data_ptr(), ss.data_ptr(), gamma.data_ptr(), dsd.data_ptr()) + cnt
            what = "%s %s (%s)" % (cid, name, setup)
            dz, (dg, db) = nan_rows(M, 64, BF), affine_bufs()
            used = ws.run(lambda: lib.stem3p_dz(*common, dz.data_ptr(), dg.data_ptr(), db.data_ptr(), B, T, H, W, st))
            assert last_kernel() == "stem3p_dz_kernel" and not used
            S.assert_exact(dz[:M].cpu(), o["dz_" + name], (F, OH, OW, 64), S.PIX_NAMES, what + ": dz")
            assert_guard(dz, what)
            check_affine(dg, db, ds, what + " dz")
            dw, (dg, db) = nan_rows(64, 245, FP, dw_init), affine_bufs()
            if fused:
                used = ws.run(lambda: lib.stem3p_wgrad(*common, dw.data_ptr(), dg.data_ptr(), db.data_ptr(), B, T, H, W, st))
                assert last_kernel() == "stem3p_wgrad_roles_kernel"
                check_affine(dg, db, ds, what + " fused wgrad")
            else:
                dzd = up(o["dz_" + name], BF)
                used = ws.run(lambda: lib.stem3d_wgrad(vf.data_ptr(), dzd.data_ptr(), dw.data_ptr(), B, T, H, W, st))
            assert used == (setup == "twopass"), what
            check_dw(dw, dw_init, o["dW_" + name], what + (": fused dW" if fused else ": dW of stem3d_wgrad on dz"))


def test_stem3p_reduce_regimes():
    """avec_stem3p_reduce at 4290 pooled pixels (135 blocks: more than 16 384 atomics): the two-pass branch with a workspace, atomics without, both exact"""
    lib, o = _lib(), S.reduce_big_operands()
    S.check_stem_exact(o["check"])
    F, PH, PW = S.REDUCE_BIG
    P = F * PH * PW
    ss, zp = up(S.ss_of(o["k"]), FP), up(o["zp"], BF)
    for setup in SETUPS:
        with Ws(setup) as ws:
            dpm, dstats = nan_rows(P, 64, BF, o["dp"].view(P, 64)), stats_buf()
            used = ws.run(lambda: lib.stem3p_reduce(dpm.data_ptr(), zp.data_ptr(), ss.data_ptr(), dstats.data_ptr(), F, PH, PW, ws.stream))
            assert used == (setup == "twopass"), setup
            S.assert_exact(dpm[:P].cpu(), o["d"], (F, PH, PW, 64), S.PIX_NAMES, "reduce (%s): masked dpool" % setup)
            assert_guard(dpm, setup)
            check_stats(dstats, o["dstats"], "reduce (%s): dstats" % setup)


# ---- stem3d ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", SETUPS)
@pytest.mark.parametrize("case", S.S3D_CASES, ids=[c[0] for c in S.S3D_CASES])
def test_stem3d_exact(case, setup):
    """avec_stem3d_fwd (y, statistics) and avec_stem3d_wgrad (dW from an integer bf16 dy), float4 and scalar staging"""
    lib = _lib()
    cid = case[0]
    o = S.s3d_operands(cid)
    S.check_stem_exact(o["check"])
    B, T, H, W = o["shape"]
    M = o["M"]
    assert lib.raw("avec_stem3d_supported")(B, T, H, W) == 1, cid
    vf = up(o["video"], FP, o["off"])
    assert vf.data_ptr() % 16 == (4 * o["off"]) % 16
    w8, bias, dy = up(S.pack_w8(o["w"], False), BF), up(o["k"]["bias"], FP), up(o["dy"], BF)
    with Ws(setup) as ws:
        for want in (True, False):
            y, stats = nan_rows(M, 64, BF), stats_buf()
            used = ws.run(lambda: lib.stem3d_fwd(vf.data_ptr(), w8.data_ptr(), 288, bias.data_ptr(), y.data_ptr(), stats.data_ptr() if want else None, B, T, H, W, ws.stream))
            what = "%s fwd (%s, stats %s)" % (cid, setup, want)
            assert used == (want and setup == "twopass"), what
            S.assert_exact(y[:M].cpu(), o["z"], (B * T, o["OH"], o["OW"], 64), S.PIX_NAMES, what + ": y")
            assert_guard(y, what)
            check_stats(stats, o["stats"] if want else torch.zeros(2, 64, dtype=S.F64), what + ": statistics")
        dw = nan_rows(64, 245, FP, S.DW_INIT)
        used = ws.run(lambda: lib.stem3d_wgrad(vf.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, T, H, W, ws.stream))
        assert used == (setup == "twopass"), cid
        check_dw(dw, S.DW_INIT, o["dW"], "%s wgrad (%s)" % (cid, setup))


# ---- stem tail ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldk", [248, 256])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", S.IM2COL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_im2col_exact(shape, dtype, ldk):
    lib = _lib()
    from avec_amd import runtime as rt
    video = S.im2col_operands(shape)
    ref = S.im2col(video, ldk)
    inside = torch.tensor([abs(k // 49 - 2) < shape[1] for k in range(245)])          # taps whose frame offset stays inside the clip for some frame
    assert float(ref[:, 245:].abs().sum()) == 0 and torch.equal((ref[:, :245] != 0).any(0), inside)
    M = ref.shape[0]
    A = nan_rows(M, ldk, DT[dtype][1])
    vf = up(video, FP)
    lib.stem_im2col(DT[dtype][0], vf.data_ptr(), A.data_ptr(), *shape, ldk, rt.stream())
    torch.cuda.synchronize()
    B, T, H, W = shape
    S.assert_exact(A[:M].cpu(), ref, (B * T, S.out_size(H), S.out_size(W), ldk), ("frame", "row", "column", "k"), "im2col %s %s ldk %d" % (shape, dtype, ldk))
    assert_guard(A, "im2col")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", S.POOL_CASES, ids=[c[0] for c in S.POOL_CASES])
def test_stem_pool_fwd_and_bwd_apply_exact(case, dtype):
    """avec_stem_pool_fwd (out, idx with its 255 case, ymax; once without ymax) and phase 1 of avec_stem_pool_bwd (dy, dgamma, dbeta): C = 64 through the 8-wide
    apply kernel, C = 12 and C = 4 through the generic one"""
    lib = _lib()
    from avec_amd import runtime as rt
    cid, F, H, W, C = case
    o = S.pool_operands(cid)
    S.check_stem_exact(o["check"])
    code, tdt = DT[dtype]
    k, PH, PW = o["k"], o["PH"], o["PW"]
    P, M = F * PH * PW, F * H * W
    y, ss = up(o["y"], tdt), up(S.ss_of(k), FP)
    for with_ymax in (True, False):
        out, idx, ymax = nan_rows(P, C, tdt), idx_rows(P, C), nan_rows(P, C, tdt)
        lib.stem_pool_fwd(code, y.data_ptr(), ss.data_ptr(), out.data_ptr(), idx.data_ptr(), ymax.data_ptr() if with_ymax else None, F, H, W, C, rt.stream())
        torch.cuda.synchronize()
        what = "%s pool_fwd %s" % (cid, dtype)
        S.assert_exact(out[:P].cpu(), o["out"], (F, PH, PW, C), S.PIX_NAMES, what + ": out")
        S.assert_exact(idx[:P].cpu(), o["idx"], (F, PH, PW, C), S.PIX_NAMES, what + ": idx")
        assert_guard(out, what), assert_guard(idx, what), assert_guard(ymax, what)
        if with_ymax:
            S.assert_exact(ymax[:P].cpu(), o["ymax"], (F, PH, PW, C), S.PIX_NAMES, what + ": ymax")
        else:
            assert bool(torch.isnan(ymax).all()), what
    dp, ix, gamma, ds = up(o["dp"], tdt), up(o["idx"], torch.uint8), up(k["gamma"], FP), up(k["dstats"], FP)
    count_dev = up(torch.tensor([S.COUNT]), FP)
    for by_ptr in (False, True):
        dy = nan_rows(M, C, tdt)
        dg, db = nan_rows(1, C, FP, S.DG_INIT), nan_rows(1, C, FP, S.DB_INIT)
        cnt = (count_dev.data_ptr(), 1.0) if by_ptr else (None, S.COUNT)
        lib.stem_pool_bwd(code, dp.data_ptr(), ix.data_ptr(), y.data_ptr(), ss.data_ptr(), gamma.data_ptr(), ds.data_ptr(), *cnt, 1, dy.data_ptr(), dg.data_ptr(), db.data_ptr(),
                          F, H, W, C, rt.stream())
        torch.cuda.synchronize()
        what = "%s pool_bwd phase 1 %s (count %s)" % (cid, dtype, "by pointer" if by_ptr else "by value")
        S.assert_exact(dy[:M].cpu(), o["dy_f32"] if dtype == "f32" else o["dy_bf16"], (F, H, W, C), S.PIX_NAMES, what + ": dy")
        assert_guard(dy, what)
        S.assert_exact(dg[0].cpu().double() - S.DG_INIT, k["dstats"][1], (C,), ("channel",), what + ": dgamma")
        S.assert_exact(db[0].cpu().double() - S.DB_INIT, k["dstats"][0], (C,), ("channel",), what + ": dbeta")
        assert_guard(dg, what), assert_guard(db, what)
