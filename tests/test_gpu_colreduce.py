"""GPU (-m gpu): the two-pass column reduction of avec_amd/csrc/vec.h (colreduce_atomic, colreduce8_atomic, as_commit, ws_slot, col_finalize, the workspace
registry of api.hip) through every entry point that leaves its kernel by it, called through the C ABI:

    avec_colsum, avec_grad_prep (dbias), avec_bn_stats, avec_bn_bwd_reduce, avec_bn_bwd_reduce_mask, avec_glu_dwconv_fwd (stats),
    avec_audio_stem_conv_fwd (y, stats), avec_audio_stem_bwd (phase 0 dstats; phase 1 dw, dbias, dgamma, dbeta)
    and the small finalizers avec_bn_finalize, avec_bn_collapse, avec_bn_affine_grads, avec_bn_bwd_finalize.

The harness (class Ws)
    The test owns the reduction workspace, in three set-ups:
      twopass  a 48 MB buffer of the test's own, filled with NaN before EVERY launch: a kernel or a finalize that reads a slot this launch did not write gives NaN.
               "Some word is no longer NaN after the launch" is the observation that the two-pass branch ran.
      atomics  no workspace registered.
      small    the 64 KB minimum registered inside a larger allocation whose remainder holds a sentinel that must be bit-identical afterwards.  avec_reduce_ws
               (api.hip) hands the buffer out when partial_floats * 4 <= bytes.  For every kernel behind ColPlan::grid / ColPlan::flat8 the partials are at least as many
               floats as the atomics they replace (gx * gy * NV * 128 >= gy * NV * C), so "more than 16 384 atomics" never fits 64 KB: they must run on atomics and
               leave the buffer alone.  The audio stem has no such threshold (nb * NV * C floats): 2048 blocks x 8 floats = exactly 64 KB must use the buffer, 2049
               blocks must not (STEM_EDGE).
    Destinations are pre-filled with known non-zero values (every kernel here accumulates).  Every test loops over its shape list and, in the twopass set-up,
    ends with the coverage condition "both regimes were seen": retuning col_ws_min_atomics() so that one branch is no longer reached fails the test.

Exact cases (mode "exact")
    Small-integer inputs: every product and every partial sum is an integer (or a multiple of 1/2) below 2^24, so any summation order gives the same fp32 result and
    the comparison with the fp64 reference is torch.equal.  The bound is asserted per case from the reference's own sum of magnitudes (exact_or_die).

Random cases (modes "gauss", "positive" = |N(0,1)| + 0.5), judged per column:  |got_c - ref_c| <= TOL * sum_i |t_ic|  (tests/colreduce_ref.py col_ratio; for the
    statistics of a convolution output the terms are taken with every factor by its magnitude, which is what the output's own rounding error scales with).
    R.TOL[formula] = 8 x the worst such ratio of a plain fp32 host evaluation of the same formula (torch fp32 sums) over the shape lists:

        measured 2026-10-16, torch 2 (CPU)     worst host fp32 ratio    tolerance (x 8)     worst on MI355X, ROCm 7.2 / torch 2.10 (2026-10-16)
        colsum, grad_prep dbias                2.03e-7                  1.6e-6              6.5e-7 (grad_prep 6.4e-7)
        bn_stats                               2.13e-7                  1.7e-6              7.4e-7
        bn_bwd_reduce (none, Swish, mask)      2.24e-7                  1.8e-6              1.1e-6
        glu_dwconv_fwd statistics              2.49e-7                  2.0e-6              9.3e-7
        audio stem statistics                  2.81e-7                  2.2e-6              9.3e-7
        audio stem dstats                      5.93e-8                  4.7e-7              2.4e-7
        audio stem dw                          2.80e-7                  2.2e-6              3.5e-7
        audio stem dbias                       7.29e-8                  5.8e-7              2.1e-7

    The device's worst cases are all in the atomics set-up with positive inputs (up to 256 float atomics per column, added in arrival order); with the workspace the
    worst is 6.4e-7 (audio stem statistics, B = 1).  The destination's old contents count as one more term of the scale (the sum's last rounding happens at that magnitude).
    (tests/colreduce_ref.py holds the constants; tests/test_colreduce_ref.py::test_tolerance_is_8x_host_fp32 re-measures the host column on every machine.)
    The largest tolerance, 2.2e-6, is 200 x below 1 / (2 * 2048) = 2.4e-4, the size of one lost partial at the largest slot count col_grid can produce.
    Random cases run in the twopass and atomics set-ups; exact cases in all three, fp32 and bf16.
"""
import pytest
import torch

from tests import colreduce_ref as R

pytestmark = pytest.mark.gpu

DT = {"f32": 0, "bf16": 1}
SETUPS = ["twopass", "atomics", "small"]
DTYPES = ["f32", "bf16"]
EXACT = [(s, d, "exact") for s in SETUPS for d in DTYPES]
RANDOM = [(s, d, m) for s in SETUPS[:2] for d in DTYPES for m in ("gauss", "positive")]
CASES = pytest.mark.parametrize("setup,dtype,mode", EXACT + RANDOM)
KEY = {"colsum": "colsum", "grad_prep": "colsum", "bn_stats": "bn_stats", "bn_bwd_reduce": "bn_bwd_reduce", "glu_dwconv_fwd": "glu_dwconv stats",
       "audio_stem_conv_fwd": "audio stem stats", "audio_stem_bwd/0": "audio stem dstats", "audio_stem_bwd/1 dw": "audio stem dw", "audio_stem_bwd/1 dbias": "audio stem dbias",
       "convmod dstats": "convmod dstats", "convmod dw": "convmod dw", "convmod dbias": "convmod dbias"}
INIT = (3.0, -2.0)              # pre-fill of the accumulated destinations (integers: the exact cases stay exact)


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _lib():
    from avec_amd.lib import lib
    return lib


class Ws:
    """the reduction workspace of the default stream, owned by the test for the duration of a `with` block"""
    BIG = 48 << 20
    TAIL = 1 << 20
    SENT = 0x7FC0BEEF                               # a quiet-NaN payload no kernel produces

    def __init__(self, setup):
        self.setup = setup

    def __enter__(self):
        from avec_amd import runtime as rt
        self.rt, self.lib, d = rt, _lib(), dev()
        self.stream = rt.stream()                   # registers the runtime's own workspace first, so that nothing re-registers behind the test's back
        self.dev = torch.cuda.current_device()
        if self.setup == "twopass":
            self.buf = torch.empty(self.BIG // 4, dtype=torch.float32, device=d)
            self.lib.set_reduce_workspace(self.buf.data_ptr(), self.BIG)
            self.head = self.buf
        elif self.setup == "small":
            self.buf = torch.empty((R.WS_MIN_BYTES + self.TAIL) // 4, dtype=torch.float32, device=d)
            assert self.buf.data_ptr() % 256 == 0
            self.head, self.tail = self.buf[:R.WS_MIN_BYTES // 4], self.buf[R.WS_MIN_BYTES // 4:].view(torch.int32)
            self.tail.fill_(self.SENT)
            self.lib.set_reduce_workspace(self.buf.data_ptr(), R.WS_MIN_BYTES)
        else:
            self.buf = self.head = None
            self.lib.set_reduce_workspace(None, 0)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.lib.set_reduce_workspace(self.rt._WORKSPACE[self.dev].data_ptr(), self.rt.WORKSPACE_BYTES)
        return False

    def run(self, fn):
        """poison, launch, synchronise; True when the launch wrote partial sums to the workspace"""
        if self.head is not None:
            self.head.fill_(float("nan"))
        fn()
        torch.cuda.synchronize()
        if self.setup == "small":
            assert bool((self.tail == self.SENT).all()), "a kernel wrote past the registered 64 KB of the reduction workspace"
        return self.head is not None and not bool(torch.isnan(self.head).all())


def put(x64, dtype):
    """fp64 host tensor -> (device tensor in the activation dtype, its values in fp64 on the host)"""
    t, back = R.as_dtype(x64, dtype)
    return t.to(dev()), back


def f32(x64):
    return x64.float().to(dev())


def check(name, case, mode, got, ref_scale, init, unit=1.0):
    """got: device fp32 destination, init: what it held before (counted as one more term); ref_scale: (fp64 reference, sum of the terms' magnitudes) per column"""
    ref, scale = ref_scale
    ref, scale = ref.flatten(), scale.flatten() + abs(init)      # the sum lands on the destination's old contents: its last rounding happens at that magnitude
    got = got.detach().cpu().double().flatten() - init
    if mode == "exact":
        R.exact_or_die(scale, name, case, unit)
        bad = got != ref
        assert not bool(bad.any()), (name, case, "exact case differs in %d of %d columns, first at %s" % (int(bad.sum()), bad.numel(), torch.nonzero(bad)[:4].flatten().tolist()),
                                     got[bad][:4].tolist(), ref[bad][:4].tolist())
    else:
        w, tol = R.worst(got, ref, scale), R.TOL[[v for k, v in KEY.items() if name.startswith(k)][-1]]
        print("%-24s %-48s %-8s per-column ratio %.3g (tolerance %.3g)" % (name, case, mode, w, tol))
        assert w <= tol, (name, case, mode, w, tol)


def expect_regime(ws, used, name, case, seen, never_fits=True):
    if ws.setup == "atomics":
        assert not used
    elif ws.setup == "small" and never_fits:
        assert not used, (name, case, "partials of more than 16 384 atomics cannot fit 64 KB, but the workspace was written")
    seen.add("twopass" if used else "atomics")


def both_seen(ws, seen, name):
    if ws.setup == "twopass":
        assert seen == {"twopass", "atomics"}, "%s: the shape list reached only %s with a workspace registered (col_ws_min_atomics retuned?)" % (name, sorted(seen))


data = R.data


def col_shapes(mode):
    return R.SHAPES_COL + (R.SHAPES_COL_CAP if mode == "exact" else [])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# col_grid kernels: colsum, grad_prep, bn_stats (4-wide mapping, slots = min(ceil(M / 64), 2048 / column blocks))
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@CASES
def test_colsum(setup, dtype, mode):
    """out[n] += sum_m x[m][n], also with a row pitch ld > N whose padding columns hold 1000 (an over-read is an integer discrepancy)"""
    lib, seen = _lib(), set()
    with Ws(setup) as ws:
        for i, (M, C) in enumerate(col_shapes(mode)):
            ld = C + (8 if i % 2 else 0)
            x64 = torch.full((M, ld), 1000.0, dtype=torch.float64)
            x64[:, :C] = data(mode, (M, C), 11 + i)
            x, xb = put(x64, dtype)
            out = torch.full((C,), INIT[0], device=dev())
            used = ws.run(lambda: lib.colsum(DT[dtype], x.data_ptr(), ld, out.data_ptr(), M, C, ws.stream))
            check("colsum", (M, C, ld, dtype, setup), mode, out, R.reduce([xb[:, :C]]), INIT[0])
            expect_regime(ws, used, "colsum", (M, C), seen)
        both_seen(ws, seen, "avec_colsum")


@CASES
def test_grad_prep_dbias(setup, dtype, mode):
    """dacc = alpha * dout (no dropout) in the activation dtype, dbias[n] += sum_m dacc (the fp32 value, before the cast)"""
    lib, seen = _lib(), set()
    with Ws(setup) as ws:
        for i, (M, C) in enumerate(col_shapes(mode)):
            ld = C + (4 if i % 2 else 0)
            d64 = torch.full((M, ld), 1000.0, dtype=torch.float64)
            d64[:, :C] = data(mode, (M, C), 41 + i, -3, 3)
            dout = f32(d64)
            dacc = torch.empty(M, C, dtype=torch.bfloat16 if dtype == "bf16" else torch.float32, device=dev())
            dbias = torch.full((C,), INIT[1], device=dev())
            used = ws.run(lambda: lib.grad_prep(DT[dtype], dout.data_ptr(), ld, dacc.data_ptr(), 2.0, 0.0, None, 0, dbias.data_ptr(), M, C, ws.stream))
            t = 2.0 * dout.cpu().double()[:, :C]
            check("grad_prep", (M, C, ld, dtype, setup), mode, dbias, R.reduce([t]), INIT[1])
            want = R.as_dtype(t, dtype)[0]
            assert torch.equal(dacc.cpu(), want), ("grad_prep dacc", M, C)
            expect_regime(ws, used, "grad_prep", (M, C), seen)
        both_seen(ws, seen, "avec_grad_prep")


@CASES
def test_bn_stats(setup, dtype, mode):
    lib, seen = _lib(), set()
    with Ws(setup) as ws:
        for i, (M, C) in enumerate(col_shapes(mode)):
            y, yb = put(data(mode, (M, C), 71 + i), dtype)
            stats = torch.full((2 * C,), INIT[0], device=dev())
            used = ws.run(lambda: lib.bn_stats(DT[dtype], y.data_ptr(), stats.data_ptr(), M, C, ws.stream))
            check("bn_stats", (M, C, dtype, setup), mode, stats, R.reduce(R.stats_terms(yb)), INIT[0])
            expect_regime(ws, used, "bn_stats", (M, C), seen)
        both_seen(ws, seen, "avec_bn_stats")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# bn_bwd_reduce / _mask: the flat 8-wide mapping (C % 8 == 0: slots = min(ceil(M / (256 / (C/8))), 1024), 256 without a workspace) and the 4-wide one
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _bwd_ss(C, mode):
    """ss = [scale | shift | mean | rstd]: scale a power of two (the sign of scale * y + shift is then the same in fp32 and fp64), mean an integer and rstd a power
    of two in the exact cases"""
    c = torch.arange(C, dtype=torch.float64)
    sc = torch.tensor([0.5, 1.0, 2.0, -1.0], dtype=torch.float64)[(c % 4).long()]
    if mode == "exact":
        return torch.stack([sc, torch.full((C,), -0.75, dtype=torch.float64) * sc.sign(), 1.0 + (c % 2), torch.tensor([0.5, 2.0, 1.0], dtype=torch.float64)[(c % 3).long()]])
    g = R.gauss((4, C), 5)
    return torch.stack([sc, 0.3 * g[1], 0.2 * g[2], 0.5 + g[3].abs()])


@pytest.mark.parametrize("setup,dtype,mode,variant", [c + (v,) for c in EXACT for v in ("none", "relu_out", "relu_pre", "mask")] +
                         [c + (v,) for c in RANDOM for v in ("none", "swish", "mask")])
def test_bn_bwd_reduce(setup, dtype, mode, variant):
    """dstats = (sum d, sum d * xhat), d = dout * act'(.) against the fp64 formula -- NOT against its own _mask twin.  ReLU by the saved output, by the recomputed
    pre-activation, by the bit mask; Swish (the conformer convolution module) in the random modes only: swish' has no exact form"""
    lib, seen = _lib(), set()
    act = {"none": 0, "swish": 1}.get(variant, 2)
    with Ws(setup) as ws:
        for i, (M, C) in enumerate(col_shapes(mode)):
            if variant == "mask" and C % 8:
                continue
            dout, db = put(data(mode, (M, C), 101 + i, -3, 3), dtype)
            y, yb = put(data(mode, (M, C), 201 + i), dtype)
            ss = _bwd_ss(C, mode)
            ssd = f32(ss.flatten())
            ssb = ssd.cpu().double().view(4, C)
            o = ob = mk = mask = None
            if variant == "relu_out":
                o, ob = put(data(mode, (M, C), 301 + i, -1, 1) if mode == "exact" else R.gauss((M, C), 301 + i), dtype)
            if variant == "mask":
                mk = R.gauss((M, C), 301 + i) > 0
                mask = R.pack_mask(mk).to(dev())
            dstats = torch.full((2 * C,), INIT[1], device=dev())
            if variant == "mask":
                used = ws.run(lambda: lib.bn_bwd_reduce_mask(DT[dtype], dout.data_ptr(), y.data_ptr(), mask.data_ptr(), ssd.data_ptr(), dstats.data_ptr(), M, C, ws.stream))
            else:
                used = ws.run(lambda: lib.bn_bwd_reduce(DT[dtype], dout.data_ptr(), y.data_ptr(), o.data_ptr() if o is not None else None, ssd.data_ptr(), act,
                                                        dstats.data_ptr(), M, C, ws.stream))
            check("bn_bwd_reduce/" + variant, (M, C, dtype, setup), mode, dstats, R.bn_bwd_reduce_ref(db, yb, ssb, act, ob, mk), INIT[1], 0.5)
            expect_regime(ws, used, "bn_bwd_reduce", (M, C), seen)
        both_seen(ws, seen, "avec_bn_bwd_reduce" + ("_mask" if variant == "mask" else ""))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# depthwise convolution statistics (slots = B * ceil(To / 32))
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def sigmoid0_exact():
    """True when the device's sigmoid(0) (rcp(1 + __expf(-0))) and swish'(0) are exactly 1/2 -- the proviso of the exact GLU / Swish cases; when it does not hold
    those cases are judged by TOL like the random ones"""
    lib, d = _lib(), dev()
    from avec_amd import runtime as rt
    x, dy, o1, o2 = torch.zeros(8, device=d), torch.ones(4, device=d), torch.empty(4, device=d), torch.empty(4, device=d)
    x[:4] = 6.0
    lib.act_f32(3, x.data_ptr(), None, o1.data_ptr(), 1, 4, 0, rt.stream())                 # GLU: 6 * sigmoid(0)
    lib.act_f32(1, x[4:].data_ptr(), dy.data_ptr(), o2.data_ptr(), 1, 4, 1, rt.stream())    # swish'(0)
    torch.cuda.synchronize()
    return bool((o1 == 3.0).all()) and bool((o2 == 0.5).all())


def test_sigmoid_of_zero_is_one_half():
    """rcp(1 + __expf(0)) = 0.5 exactly on gfx950: the exact GLU and Swish' cases of this module and of test_gpu_convmod_bn.py really are exact comparisons"""
    assert sigmoid0_exact()


@CASES
def test_glu_dwconv_fwd_stats(setup, dtype, mode):
    """the statistics output of avec_glu_dwconv_fwd (never requested by the existing depthwise test) and its conv output.  Exact: gate half zero (sigmoid = 1/2),
    value half even integers, integer taps and bias"""
    lib, seen = _lib(), set()
    md = mode if mode != "exact" or sigmoid0_exact() else "gauss"
    with Ws(setup) as ws:
        for i, shape in enumerate(R.SHAPES_DW):
            B, T, C, K, stride, causal = shape
            padl = K - 1 if causal else K // 2
            To = (T - 1) // stride + 1
            u64, w64, b64 = R.dw_inputs(mode, shape, i)
            u, ub = put(u64, dtype)
            w, bias = f32(w64), f32(b64)
            out = torch.empty(B * To, C, dtype=u.dtype, device=dev())
            stats = torch.full((2 * C,), INIT[0], device=dev())
            used = ws.run(lambda: lib.glu_dwconv_fwd(DT[dtype], u.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), stats.data_ptr(), B, T, C, K, stride, padl, ws.stream))
            c, ref, scale = R.dw_stats_ref(ub, w.cpu().double(), bias.cpu().double(), stride, padl)
            case = shape + (dtype, setup)
            check("glu_dwconv_fwd stats", case, md, stats, (ref, scale), INIT[0])
            if md == "exact":
                assert torch.equal(out.cpu().double().view(B, To, C), c), ("glu_dwconv_fwd out", case)
            expect_regime(ws, used, "glu_dwconv_fwd", case, seen)
        both_seen(ws, seen, "avec_glu_dwconv_fwd")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# audio stem: the three kernel families (8x, 8, generic); slots = ceil(B * To / 16) for the two 8-wide families, block-level atomics for the generic one
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _stem_case(ws, lib, seen, shape, dtype, mode, seed, sw0):
    B, NM, F, C = shape
    Fo, To = R.stem_dims(NM, F)
    fam, nb = R.stem_family(NM, C), R.stem_blocks(B, F)
    case = shape + (fam, dtype, ws.setup)
    i64 = R.stem_inputs(mode, shape, seed)
    mel, w, bias = f32(i64["mel"]), f32(i64["w"]), f32(i64["bias"])
    melb, wb, bb = mel.cpu().double(), w.cpu().double(), bias.cpu().double()
    M, J = B * To, C * Fo
    y = torch.empty(M, J, dtype=torch.bfloat16 if dtype == "bf16" else torch.float32, device=dev())
    stats = torch.full((2 * C,), INIT[0], device=dev())

    def regime(used, nv):
        """the 8-wide families take a registered workspace whenever nb * nv * C floats fit it (no atomics threshold), the generic family never"""
        if ws.setup == "twopass":
            assert used == (fam != "generic"), case
        elif ws.setup == "small":
            assert used == (fam != "generic" and nb * nv * C * 4 <= R.WS_MIN_BYTES), (case, nb * nv * C * 4, "avec_reduce_ws: partial_floats * 4 <= bytes")
        else:
            assert not used
        seen.add("twopass" if used else "atomics")

    used = ws.run(lambda: lib.audio_stem_conv_fwd(DT[dtype], mel.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), stats.data_ptr(), B, NM, F, C, ws.stream))
    regime(used, 2)
    yr, ref, scale = R.stem_fwd_ref(melb, wb, bb)
    check("audio_stem_conv_fwd", case, mode, stats, (ref, scale), INIT[0])
    yb = y.cpu().double().view(B, To, C, Fo)
    if mode == "exact":
        assert torch.equal(yb, yr), ("audio_stem_conv_fwd y", case)
    else:
        _, ymag = R.audio_stem_ref(melb, wb, bb)
        er = float(((yb - yr).abs() / ymag.clamp_min(1e-30)).max())
        assert er <= (2.0 ** -8 if dtype == "bf16" else 16 * R.EPS32), ("audio_stem_conv_fwd y", case, er)      # half an ulp of bf16 / ten fp32 FMAs
    # ---- backward on the y the device holds: phase 0 (dstats), phase 1 (dw, dbias, dgamma, dbeta) ----
    md = mode if mode != "exact" or sw0 else "gauss"
    da, dab = put(i64["da"].reshape(M, J), dtype)
    ssd, gam, ds_in, count = f32(i64["ss"].flatten()), f32(i64["gamma"]), f32(i64["dstats"]), i64["count"]
    refs = R.stem_bwd_ref(melb, yb, dab.view(B, To, C, Fo), ssd.cpu().double().view(4, C), gam.cpu().double(), ds_in.cpu().double(), count)
    dstats = torch.full((2 * C,), INIT[1], device=dev())
    used = ws.run(lambda: lib.audio_stem_bwd(DT[dtype], da.data_ptr(), y.data_ptr(), mel.data_ptr(), ssd.data_ptr(), gam.data_ptr(), dstats.data_ptr(), None, count, 0,
                                             None, None, None, None, B, NM, F, C, ws.stream))
    regime(used, 2)
    check("audio_stem_bwd/0 dstats", case, md, dstats, refs["dstats"], INIT[1], 0.5)
    dw = torch.full((C, 9), INIT[0], device=dev())
    dbias, dgamma, dbeta = torch.full((C,), INIT[1], device=dev()), torch.full((C,), INIT[0], device=dev()), torch.full((C,), INIT[1], device=dev())
    cnt = torch.tensor([count], device=dev())
    by_ptr = bool(seed % 20)                                                  # the count through count_ptr (the SyncBatchNorm path) or by value
    used = ws.run(lambda: lib.audio_stem_bwd(DT[dtype], da.data_ptr(), y.data_ptr(), mel.data_ptr(), ssd.data_ptr(), gam.data_ptr(), ds_in.data_ptr(),
                                             cnt.data_ptr() if by_ptr else None, -1.0 if by_ptr else count, 1,
                                             dw.data_ptr(), dbias.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), B, NM, F, C, ws.stream))
    regime(used, 10)
    check("audio_stem_bwd/1 dw", case, md, dw, refs["dw"], INIT[0], 0.25)
    check("audio_stem_bwd/1 dbias", case, md, dbias, refs["dbias"], INIT[1], 0.25)
    # dgamma / dbeta += the reduced sums, once, whatever the grid is: one fp32 addition each, so bit-exact in every mode
    assert torch.equal(dgamma.cpu(), INIT[0] + ds_in.cpu()[C:]) and torch.equal(dbeta.cpu(), INIT[1] + ds_in.cpu()[:C]), ("audio_stem_bwd dgamma / dbeta", case)


@CASES
def test_audio_stem(setup, dtype, mode):
    """y, BatchNorm statistics, dstats, dw / dbias / dgamma / dbeta of the audio stem in all three kernel families; B = 1 with a few dozen frames (the
    one-utterance-per-rank shape: fewer rows than AS_ROWS in the last block) and longer batches"""
    lib, seen = _lib(), set()
    sw0 = sigmoid0_exact()
    with Ws(setup) as ws:
        for i, shape in enumerate(R.SHAPES_STEM):
            _stem_case(ws, lib, seen, shape, dtype, mode, 700 + 10 * i, sw0)
        both_seen(ws, seen, "avec_audio_stem_conv_fwd / avec_audio_stem_bwd")


@pytest.mark.parametrize("setup,dtype", [("twopass", "f32"), ("atomics", "f32"), ("twopass", "bf16")])
def test_audio_stem_bench_shape(setup, dtype):
    """B = 32, 80 mels, 400 frames, 180 channels (400 slots of 16 rows), exact integers"""
    with Ws(setup) as ws:
        _stem_case(ws, _lib(), set(), R.STEM_BENCH, dtype, "exact", 990, sigmoid0_exact())


@pytest.mark.parametrize("F,fits", R.STEM_EDGE)
def test_small_workspace_edge(F, fits):
    """avec_reduce_ws hands a 64 KB workspace out for exactly 16 384 floats of partials (2048 blocks x 2 x C = 4) and not for one block more; nothing outside the
    registered 64 KB is written either way, and the statistics are exact both times"""
    lib = _lib()
    B, NM, C = 1, 16, 4
    assert (R.stem_blocks(B, F) * 2 * C * 4 <= R.WS_MIN_BYTES) == fits and R.stem_family(NM, C) == "8x"
    Fo, To = R.stem_dims(NM, F)
    with Ws("small") as ws:
        mel64, w64, b64 = R.int_tensor((B, NM, F), 0, 1, 5), R.int_tensor((C, 9), -1, 1, 6), R.int_tensor((C,), -1, 1, 7)
        mel, w, bias = f32(mel64), f32(w64), f32(b64)
        y = torch.empty(B * To, C * Fo, device=dev())
        stats = torch.full((2 * C,), INIT[0], device=dev())
        used = ws.run(lambda: lib.audio_stem_conv_fwd(0, mel.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), stats.data_ptr(), B, NM, F, C, ws.stream))
        assert used == fits
        yr, ref, scale = R.stem_fwd_ref(mel64, w64, b64)
        check("audio_stem_conv_fwd", ("edge", F), "exact", stats, (ref, scale), INIT[0])
        assert torch.equal(y.cpu().double().view(B, To, C, Fo), yr)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward parameter gradients: min(ceil(M / 16), 256) slots of [2][D], 128 without a workspace; no atomics threshold
# ---------------------------------------------------------------------------------------------------------------------------------------------------
LN_ROWS = [17, 16 * 128 + 5]          # two slots, the second with one row / 129 slots: more than the 128 blocks launched without a workspace


@pytest.mark.parametrize("setup", SETUPS)
@pytest.mark.parametrize("dy_dtype", DTYPES)
@pytest.mark.parametrize("D", [8, 180])
def test_layernorm_bwd_param_grads(setup, dy_dtype, D):
    """dgamma[c] += sum_m dy * (x - mean) * rstd, dbeta[c] += sum_m dy through avec_layernorm_bwd: integer dy, x and gamma, mean 0, rstd a power of two per row, so
    every term is a multiple of 1/2 and the comparison with fp64 is torch.equal.  A registered workspace is used whenever 2 * D floats per slot fit it."""
    lib = _lib()
    with Ws(setup) as ws:
        for i, M in enumerate(LN_ROWS):
            case = (M, D, dy_dtype, setup)
            dy, dyb = put(R.int_tensor((M, D), -3, 3, 1300 + i), dy_dtype)
            x64, g64 = R.int_tensor((M, D), 0, 3, 1310 + i), R.int_tensor((D,), -2, 2, 1320 + i)
            rs64 = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.arange(M) % 3]
            x, gamma, mean, rstd = f32(x64), f32(g64), torch.zeros(M, device=dev()), f32(rs64)
            dx = torch.empty(M, D, device=dev())
            dgamma, dbeta = torch.full((D,), INIT[0], device=dev()), torch.full((D,), INIT[1], device=dev())
            used = ws.run(lambda: lib.layernorm_bwd(DT[dy_dtype], dy.data_ptr(), 0, x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dx.data_ptr(), None,
                                                    dgamma.data_ptr(), dbeta.data_ptr(), M, D, ws.stream))
            nb = min((M + 15) // 16, 256)
            fits = {"twopass": True, "atomics": False, "small": nb * 2 * D * 4 <= R.WS_MIN_BYTES}[setup]
            assert used == fits, (case, nb, "slots of 2 * D floats")
            check("layernorm_bwd dgamma", case, "exact", dgamma, R.reduce([dyb * x64 * rs64[:, None]]), INIT[0], 0.5)
            check("layernorm_bwd dbeta", case, "exact", dbeta, R.reduce([dyb]), INIT[1])
            assert bool(torch.isfinite(dx).all()), case


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# video stem tail, BatchNorm-backward sums through the max pool: over the conv output (8-wide for C % 8 == 0, else 4-wide) and over the pooled tensors
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _pool_twopass_expected(M, C):
    """the regime tests/colreduce_ref.py's geometry asks for with a large workspace: more than 16 384 atomics in one pass"""
    if C % 8 == 0:
        return R.col8_blocks(M, C) * 2 * C > 16384
    return R.col_grid(M, C)[1] * 2 * C > 16384


# (C, H, W) of one frame, rows = H * W just below / just above the threshold, the last block or row slot partial:
#   C = 64 (8-wide, 32 rows per block): 128 blocks x 128 atomics = 16 384 up to 4096 rows; 63 x 65 = 4095 rows, 63 x 66 = 4158 rows (130 blocks)
#   C = 12 (4-wide, 64 rows per slot): 682 slots x 24 atomics = 16 368 up to 43 648 rows; 135 x 323 = 43 605 rows, 135 x 324 = 43 740 rows (684 slots)
POOL_SHAPES = {64: [(63, 65), (63, 66)], 12: [(135, 323), (135, 324)]}
IDENT_SS = lambda C: torch.cat([torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C)]).to(dev())      # scale 1, shift 0, mean 0, rstd 1


def _pool_regimes(name, C, rows, dtype, launch, ref_scale):
    """`launch(ws, dstats)` in the three set-ups: exact against fp64 in each, bit-equal between them, two-pass exactly where the geometry model says"""
    got = {}
    for setup in SETUPS:
        with Ws(setup) as ws:
            dstats = torch.full((2 * C,), INIT[1], device=dev())
            used = ws.run(lambda: launch(ws, dstats))
            case = (C, rows, dtype, setup)
            check(name, case, "exact", dstats, ref_scale, INIT[1])
            assert used == (setup == "twopass" and _pool_twopass_expected(rows, C)), (name, case, used)
            got[setup] = dstats.cpu()
    assert torch.equal(got["twopass"], got["atomics"]) and torch.equal(got["small"], got["atomics"]), (name, C, rows, dtype)
    return _pool_twopass_expected(rows, C)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [64, 12])
def test_stem_pool_bwd_reduce(C, dtype):
    """avec_stem_pool_bwd phase 0: dstats = (sum dr, sum dr * (y - mean) * rstd) over the conv output, dr the pooled gradient routed to each window's winner.  Integer
    y and dpool with ss = (1, 0, 0, 1): relu(y) = y where a winner exists, so the sums are (sum of dpool over windows with a winner, sum of dpool * pooled output)
    -- integers.  The window indices come from avec_stem_pool_fwd, whose output is compared with torch's max pool first."""
    lib, seen = _lib(), set()
    for k, (H, W) in enumerate(POOL_SHAPES[C]):
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y, yb = put(R.int_tensor((H * W, C), -2, 3, 1400 + k), dtype)
        dp, dpb = put(R.int_tensor((OH * OW, C), -3, 3, 1410 + k), dtype)
        ss, gamma = IDENT_SS(C), torch.ones(C, device=dev())
        out, idx = torch.empty(OH * OW, C, dtype=y.dtype, device=dev()), torch.empty(OH * OW, C, dtype=torch.uint8, device=dev())
        from avec_amd import runtime as rt
        lib.stem_pool_fwd(DT[dtype], y.data_ptr(), ss.data_ptr(), out.data_ptr(), idx.data_ptr(), None, 1, H, W, C, rt.stream())
        torch.cuda.synchronize()
        pooled = torch.nn.functional.max_pool2d(yb.view(1, H, W, C).permute(0, 3, 1, 2).clamp_min(0), 3, 2, 1).permute(0, 2, 3, 1).reshape(OH * OW, C)
        assert torch.equal(out.cpu().double(), pooled) and torch.equal(idx.cpu() != 255, pooled > 0), ("stem_pool_fwd", C, H, W)
        ref_scale = R.reduce([torch.cat([dpb * (pooled > 0), dpb * pooled], 1)])
        two = _pool_regimes("stem_pool_bwd/0", C, H * W, dtype,
                            lambda ws, dstats: lib.stem_pool_bwd(DT[dtype], dp.data_ptr(), idx.data_ptr(), y.data_ptr(), ss.data_ptr(), gamma.data_ptr(), dstats.data_ptr(),
                                                                 None, float(H * W), 0, None, None, None, 1, H, W, C, ws.stream), ref_scale)
        seen.add("twopass" if two else "atomics")
    assert seen == {"twopass", "atomics"}, "stem_pool_bwd C=%d: the shape list reached only %s (col_ws_min_atomics retuned?)" % (C, sorted(seen))


@pytest.mark.parametrize("dtype", DTYPES)
def test_stem_pool_bwd_reduce_pooled(dtype):
    """avec_stem_pool_bwd_reduce_pooled: dstats = (sum dpool, sum dpool * (ymax - mean) * rstd) over the pooled elements whose window has a winner (idx != 255).
    63 x 65 = 4095 / 63 x 66 = 4158 pooled rows of C = 64: 128 / 130 blocks of 32 rows around the 16 384-atomics threshold, the last block partial"""
    lib, seen, C = _lib(), set(), 64
    for k, (OH, OW) in enumerate(POOL_SHAPES[C]):
        H, W, P = 2 * OH - 1, 2 * OW - 1, OH * OW
        dp, dpb = put(R.int_tensor((P, C), -3, 3, 1500 + k), dtype)
        ym, ymb = put(R.int_tensor((P, C), -2, 3, 1510 + k), dtype)
        sel = R.int_tensor((P, C), 0, 11, 1520 + k)
        idx = torch.where(sel > 8, torch.full_like(sel, 255), sel).to(torch.uint8).to(dev())      # a quarter of the windows without a winner
        ss = IDENT_SS(C)
        has = (sel <= 8).double()
        ref_scale = R.reduce([torch.cat([dpb * has, dpb * has * ymb], 1)])
        two = _pool_regimes("stem_pool_bwd_reduce_pooled", C, P, dtype,
                            lambda ws, dstats: lib.stem_pool_bwd_reduce_pooled(DT[dtype], dp.data_ptr(), idx.data_ptr(), ym.data_ptr(), ss.data_ptr(), dstats.data_ptr(),
                                                                               1, H, W, C, ws.stream), ref_scale)
        seen.add("twopass" if two else "atomics")
    assert seen == {"twopass", "atomics"}, "stem_pool_bwd_reduce_pooled: the shape list reached only %s (col_ws_min_atomics retuned?)" % sorted(seen)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# visual stem (avec_stem3d_fwd / _wgrad, avec_stem3p_fwd / _reduce / _wgrad): the same clip with the workspace owned by the test, two-pass against atomics
# ---------------------------------------------------------------------------------------------------------------------------------------------------
LOST_PARTIAL = 1.0 / (2 * 2048)              # the size of one lost partial at the largest slot count (module header)
# worst twopass-versus-atomics rel_err (max |a - b| / max |b|) per tensor over the four modes (pooled, pooled_unfused, direct, im2col), measured on the parent
# commit, the one BEFORE the launch sites moved to ColPlan; the bound is 8 x that, the margin this module uses over a measured baseline.  A measured 0 is a bound
# of 0: the tensor is bit-equal in the two regimes.
STEM_REGIME_MEASURED = {
    (1, 3, 72, 40): {"stem output": 0.0, "conv weight gradient": 6.65e-6, "bn weight gradient": 1.7e-7, "running variance (batch statistics)": 6.47e-8, "bn bias gradient": 4.39e-8},
    (1, 5, 40, 64): {"stem output": 0.0, "conv weight gradient": 3.17e-6, "bn weight gradient": 3.02e-7, "running variance (batch statistics)": 6.43e-8, "bn bias gradient": 2.75e-8},
}
# (1, 5, 40, 64) stands in for (1, 5, 48, 64), the W % 8 == 0 shape of tests/test_gpu_parity.py: on the parent the weight gradient at (1, 5, 48, 64) differs by
# 1.29e-4 between the regimes in some runs (direct and "pooled" modes), and 8 x that is 1.0e-3, above LOST_PARTIAL; (1, 4, 56, 48) gave 2.04e-4.  (1, 5, 40, 64)
# and (1, 5, 56, 56) stayed at 3.2e-6 / 1.5e-6.
# At BOTH shapes below avec_stem3p_supported is 0 (s3p_geom serves W = 88 and W = 96 only), so the modes "pooled" and "pooled_unfused" fall through to stem3d.hip:
# three distinct paths run here (direct under three names, and im2col).  The two regimes of the stem3p kernels (forward statistics, stem3p_reduce, the fused
# weight gradient) are compared -- for equality -- in tests/test_gpu_stem_exact.py.
STEM_REGIME_SHAPES = [(1, 3, 72, 40), (1, 5, 40, 64)]


@pytest.mark.parametrize("shape", STEM_REGIME_SHAPES)
def test_visual_stem_twopass_matches_atomics(shape):
    """tests/test_gpu_parity.py's visual-stem comparison (its smallest shape and a T = 5, W % 8 == 0 shape) run twice, with the reduction workspace owned by Ws("twopass")
    and by Ws("atomics"): the path-against-path assertions of that test hold in each, the poisoned workspace shows that the two-pass branch ran, and every tensor
    of every path agrees between the regimes within 8 x STEM_REGIME_MEASURED[shape].  The paths are stem3d.hip (under the mode names "pooled", "pooled_unfused"
    and "direct": the pooled kernels decline both widths) and im2col; stem3p.hip's regimes are covered by tests/test_gpu_stem_exact.py.

                                                (1, 3, 72, 40)                   (1, 5, 40, 64)
                                                parent       bound (x 8)        parent       bound (x 8)
        stem output                             0            0 (bit-equal)      0            0 (bit-equal)
        conv weight gradient                    6.65e-6      5.3e-5             3.17e-6      2.5e-5
        bn weight gradient                      1.7e-7       1.4e-6             3.02e-7      2.4e-6
        running variance (batch statistics)     6.47e-8      5.2e-7             6.43e-8      5.1e-7
        bn bias gradient                        4.39e-8      3.5e-7             2.75e-8      2.2e-7

    Every bound is below 1 / (2 * 2048) = 2.4e-4: a lost or doubled partial row would not pass."""
    from tests.helpers import rel_err
    from tests.test_gpu_parity import STEM_TENSORS, assert_stem_paths_agree, visual_stem_modes
    res = {}
    for setup in ("twopass", "atomics"):
        with Ws(setup) as ws:
            used = ws.run(lambda: res.__setitem__(setup, visual_stem_modes(shape)))
            assert used == (setup == "twopass"), (shape, setup)
        assert_stem_paths_agree(res[setup], shape[3])
    measured = STEM_REGIME_MEASURED[shape]
    assert set(measured) == set(STEM_TENSORS) and all(8 * v < LOST_PARTIAL for v in measured.values()), measured
    worst = {}
    for path in res["twopass"]:
        for k, name in enumerate(STEM_TENSORS):
            e = rel_err(res["atomics"][path][k], res["twopass"][path][k])
            print("visual stem %s %-15s %-36s twopass vs atomics rel_err %.3g" % (shape, path, name, e))
            worst[name] = max(worst.get(name, 0.0), e)
    for name, e in worst.items():
        assert e <= 8 * measured[name], (shape, name, e, 8 * measured[name])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# two streams: the main stream's workspace and the branch stream's must never share partials
# ---------------------------------------------------------------------------------------------------------------------------------------------------
N_BACK_TO_BACK = 20          # each round is two ~10 us launches plus a synchronisation: well under a second in all


def test_two_streams_back_to_back():
    """the same exact-integer reductions (BatchNorm statistics, audio-stem statistics) on the main stream and on runtime.branch_stream(), back to back without a host
    synchronisation in between, both workspaces NaN-poisoned before every round: both results exact every time"""
    from avec_amd import runtime as rt
    lib, d = _lib(), dev()
    with Ws("twopass") as ws:
        side = rt.branch_stream()
        assert side is not None, "the branch stream is disabled"
        dv = torch.cuda.current_device()
        own = torch.empty(Ws.BIG // 4, dtype=torch.float32, device=d)
        lib.set_reduce_workspace_stream(own.data_ptr(), Ws.BIG, side.cuda_stream)
        try:
            M, C = 6400, 256
            B, NM, F, Cs = 1, 80, 61, 180                                      # one utterance, a few dozen frames: the shape of the open DDP finding
            Fo, To = R.stem_dims(NM, F)
            ins = []
            for s in (0, 1):
                yb = R.int_tensor((M, C), 0, 3, 900 + s)
                mel64, w64, b64 = R.int_tensor((B, NM, F), 0, 1, 910 + s), R.int_tensor((Cs, 9), -1, 1, 920 + s), R.int_tensor((Cs,), -1, 1, 930 + s)
                _, ref_s, sc_s = R.stem_fwd_ref(mel64, w64, b64)
                R.exact_or_die(sc_s, "two streams stem", s)
                ref_b, sc_b = R.reduce(R.stats_terms(yb))
                R.exact_or_die(sc_b, "two streams bn", s)
                ins.append(dict(y=f32(yb), mel=f32(mel64), w=f32(w64), b=f32(b64), ref_b=ref_b, ref_s=ref_s,
                                yo=torch.empty(B * To, Cs * Fo, device=d), st_b=torch.empty(2 * C, device=d), st_s=torch.empty(2 * Cs, device=d)))
            torch.cuda.synchronize()
            streams = [(ws.stream, torch.cuda.current_stream(), ws.buf), (side.cuda_stream, side, own)]
            for it in range(N_BACK_TO_BACK):
                for k, (h, ts, buf) in enumerate(streams):                     # no host synchronisation between the two streams' launches
                    a = ins[k]
                    with torch.cuda.stream(ts):
                        buf.fill_(float("nan")); a["st_b"].fill_(INIT[0]); a["st_s"].fill_(INIT[0])
                        lib.bn_stats(0, a["y"].data_ptr(), a["st_b"].data_ptr(), M, C, h)
                        lib.audio_stem_conv_fwd(0, a["mel"].data_ptr(), a["w"].data_ptr(), a["b"].data_ptr(), a["yo"].data_ptr(), a["st_s"].data_ptr(), B, NM, F, Cs, h)
                torch.cuda.synchronize()
                for k, (h, ts, buf) in enumerate(streams):
                    a = ins[k]
                    assert not bool(torch.isnan(buf).all()), ("stream %d did not use its own workspace" % k, it)
                    assert torch.equal(a["st_b"].cpu().double() - INIT[0], a["ref_b"]), ("bn_stats", "stream %d" % k, "round %d" % it)
                    assert torch.equal(a["st_s"].cpu().double() - INIT[0], a["ref_s"]), ("audio stem stats", "stream %d" % k, "round %d" % it)
        finally:
            torch.cuda.synchronize()
            lib.set_reduce_workspace_stream(rt._BRANCH["ws"][dv].data_ptr(), rt.WORKSPACE_BYTES, side.cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the small finalizers against closed forms / torch.nn.functional.batch_norm in fp64
# ---------------------------------------------------------------------------------------------------------------------------------------------------
FIN_TOL = 64 * R.EPS32        # a dozen fp32 operations and one rsqrtf per element on O(1) data, no long sum; a wrong replica or row is O(1)


def _close(got, ref, tol=FIN_TOL):
    got, ref = got.detach().cpu().double(), ref.double()
    return bool(((got - ref).abs() <= tol * (1 + ref.abs())).all())


@pytest.mark.parametrize("use_ptr", [False, True])
@pytest.mark.parametrize("nrep", [1, 17, 64])
@pytest.mark.parametrize("C", [4, 16, 180, 256, 2048])
def test_bn_finalize_training(C, nrep, use_ptr):
    """replica collapse, count vs count_ptr, momentum, running mean / unbiased running variance, num_batches_tracked, all four rows of ss -- built from data so that
    torch.nn.functional.batch_norm (fp64) is the reference"""
    from avec_amd import runtime as rt
    lib, d = _lib(), dev()
    n, mom, eps = 50, 0.3, 1e-5
    x = R.gauss((nrep, n, C), 3 * C + nrep) * (0.5 + torch.arange(C, dtype=torch.float64) % 3) + 0.7
    stats = f32(torch.cat([x.sum(1), (x * x).sum(1)], -1))                    # [nrep][2C]
    gamma, beta = R.gauss((C,), 1) + 1.5, R.gauss((C,), 2)
    rm0, rv0 = R.gauss((C,), 3), R.positive((C,), 4)
    rm, rv, nbt = f32(rm0), f32(rv0), torch.tensor([7], dtype=torch.int64, device=d)
    g, b, ss = f32(gamma), f32(beta), torch.full((4 * C,), 9.0, device=d)
    N = float(nrep * n)
    cnt = torch.tensor([N], device=d)
    lib.bn_finalize(stats.data_ptr(), nrep, cnt.data_ptr() if use_ptr else None, -1.0 if use_ptr else N, g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                    nbt.data_ptr(), mom, eps, ss.data_ptr(), C, 1, rt.stream())
    torch.cuda.synchronize()
    xs = x.reshape(-1, C)
    rmr, rvr = rm.cpu().double().clone(), rv.cpu().double().clone()
    rmr[:], rvr[:] = rm0.float().double(), rv0.float().double()
    z = torch.nn.functional.batch_norm(xs, rmr, rvr, g.cpu().double(), b.cpu().double(), training=True, momentum=mom, eps=eps)
    mean, var = xs.mean(0), xs.var(0, unbiased=False)
    rs = 1 / torch.sqrt(var + eps)
    ssg = ss.cpu().double().view(4, C)
    # the one-pass variance carries eps * (1 + mean^2 / var) relative error; mean / std <= 1.4 here
    assert _close(ssg[2], mean) and _close(ssg[3], rs, 256 * R.EPS32), (C, nrep)
    assert _close(xs * ssg[0] + ssg[1], z, 512 * R.EPS32), "scale / shift rows do not normalise the data as batch_norm does"
    assert _close(rm, rmr) and _close(rv, rvr, 256 * R.EPS32), "running statistics (unbiased n / (n - 1) variance)"
    assert int(nbt) == 8
    ref, _, _ = R.bn_finalize_ref(stats.cpu(), N, g.cpu(), b.cpu(), None, None, mom, eps)
    assert _close(ssg, ref, 256 * R.EPS32)


def test_bn_finalize_edges():
    """n = 1 (unbiased factor n / max(n - 1, 1) = 1), NaN sums leave the running statistics and the counter untouched, NULL running statistics, eval mode"""
    from avec_amd import runtime as rt
    lib, d = _lib(), dev()
    C, mom, eps = 20, 0.25, 1e-3
    g, b = f32(R.gauss((C,), 1) + 1.5), f32(R.gauss((C,), 2))
    x = R.gauss((1, C), 3)
    stats = f32(torch.cat([x, x * x], -1))
    rm0, rv0 = R.gauss((C,), 4).float(), R.positive((C,), 5).float()
    rm, rv, nbt, ss = rm0.to(d), rv0.to(d), torch.tensor([0], dtype=torch.int64, device=d), torch.empty(4 * C, device=d)
    lib.bn_finalize(stats.data_ptr(), 1, None, 1.0, g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), mom, eps, ss.data_ptr(), C, 1, rt.stream())
    torch.cuda.synchronize()
    ssg = ss.cpu().double().view(4, C)
    # one row: the variance is 0; the one-pass form leaves a rounding residue of up to 2 eps x^2 instead (s2 and mean^2 are rounded separately)
    res = 2 * R.EPS_F32 * x[0] ** 2
    rs0 = 1 / torch.sqrt(torch.tensor(eps, dtype=torch.float64))
    assert _close(ssg[2], x[0]) and int(nbt) == 1
    assert bool(((ssg[3] - rs0).abs() <= rs0 * (0.5 * res / eps + 8 * R.EPS_F32)).all()), "rstd of a single row"
    assert _close(rm, (1 - mom) * rm0.double() + mom * x[0])
    assert bool(((rv.cpu().double() - (1 - mom) * rv0.double()).abs() <= mom * res + 4 * R.EPS_F32 * rv0.double()).all()), "unbiased factor n / max(n - 1, 1) = 1 for n = 1"
    # NaN sums
    bad = stats.clone(); bad[0, 3] = float("nan")
    rm, rv, nbt = rm0.to(d), rv0.to(d), torch.tensor([5], dtype=torch.int64, device=d)
    lib.bn_finalize(bad.data_ptr(), 1, None, 1.0, g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), mom, eps, ss.data_ptr(), C, 1, rt.stream())
    torch.cuda.synchronize()
    assert torch.equal(rm.cpu()[3], rm0[3]) and torch.equal(rv.cpu()[3], rv0[3]), "a NaN statistic reached the running statistics"
    assert not torch.equal(rm.cpu()[4], rm0[4]), "finite channels still update"
    badall = torch.full_like(stats, float("nan"))
    rm, rv, nbt = rm0.to(d), rv0.to(d), torch.tensor([5], dtype=torch.int64, device=d)
    lib.bn_finalize(badall.data_ptr(), 1, None, 1.0, g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), mom, eps, ss.data_ptr(), C, 1, rt.stream())
    torch.cuda.synchronize()
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and int(nbt) == 5
    # NULL running statistics
    lib.bn_finalize(stats.data_ptr(), 1, None, 1.0, g.data_ptr(), b.data_ptr(), None, None, None, mom, eps, ss.data_ptr(), C, 1, rt.stream())
    torch.cuda.synchronize()
    assert _close(ss.view(4, C)[2], x[0])
    # eval: ss from the running statistics, which stay untouched
    rm, rv, nbt = rm0.to(d), rv0.to(d), torch.tensor([5], dtype=torch.int64, device=d)
    lib.bn_finalize(None, 0, None, 0.0, g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(), mom, eps, ss.data_ptr(), C, 0, rt.stream())
    torch.cuda.synchronize()
    ref, _, _ = R.bn_finalize_ref(None, 0, g.cpu(), b.cpu(), rm0, rv0, mom, eps, training=False)
    assert _close(ss.view(4, C), ref) and torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and int(nbt) == 5


@pytest.mark.parametrize("nrep", [1, 17, 64])
@pytest.mark.parametrize("C", [4, 130, 256, 2048])
def test_bn_collapse_affine_bwd_finalize(C, nrep):
    """integer data: the three helpers are exact"""
    from avec_amd import runtime as rt
    lib, d = _lib(), dev()
    st64 = R.int_tensor((nrep, 2 * C), -50, 50, C + nrep)
    stats, out = f32(st64), torch.full((2 * C + 1,), 9.0, device=d)
    lib.bn_collapse(stats.data_ptr(), nrep, 123.0, out.data_ptr(), C, rt.stream())
    c = torch.arange(C, dtype=torch.float64)
    ss64 = torch.stack([R.gauss((C,), 1), R.gauss((C,), 2), (c % 5) - 2, torch.tensor([0.5, 2.0, 1.0], dtype=torch.float64)[(c % 3).long()]])
    ss, dstats = f32(ss64.flatten()), torch.full((2 * C,), 9.0, device=d)
    lib.bn_bwd_finalize(stats.data_ptr(), nrep, ss.data_ptr(), dstats.data_ptr(), C, rt.stream())
    dg, db = torch.full((C,), INIT[0], device=d), torch.full((C,), INIT[1], device=d)
    lib.bn_affine_grads(dstats.data_ptr(), dg.data_ptr(), db.data_ptr(), C, rt.stream())
    torch.cuda.synchronize()
    s = st64.sum(0)
    assert torch.equal(out.cpu().double(), torch.cat([s, torch.tensor([123.0], dtype=torch.float64)]))
    want = torch.cat([s[:C], ss64[3] * (s[C:] - ss64[2] * s[:C])])
    assert torch.equal(dstats.cpu().double(), want)
    assert torch.equal(dg.cpu().double() - INIT[0], want[C:]) and torch.equal(db.cpu().double() - INIT[1], want[:C])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the one-pass variance (sum x, sum x^2 in fp32): characterised, not tuned away
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_onepass_variance_envelope():
    """|var - var_ref| / var_ref <= KAPPA * eps_fp32 * (1 + mean^2 / var) through avec_bn_stats + avec_bn_finalize, per-channel mean / std in {0, 5, 50, 300}.
    KAPPA = 4 x the worst constant of the host fp32 emulation of the same formula (tests/test_colreduce_ref.py::test_variance_kappa_is_4x_host_fp32).
    Measured on MI355X (ROCm 7.2, 2026-10-16): constants 1.6 / 3.0 / 3.7 / 3.0, relative variance errors 1.9e-7 / 9.2e-6 / 1.1e-3 / 3.1e-2 ("BatchNorm
    statistics: the one-pass envelope").  6400 x 128 runs two-pass on the runtime's own workspace, so the figures are deterministic."""
    from avec_amd import runtime as rt
    lib, d = _lib(), dev()
    M, C = R.VAR_ROWS, 4 * 32
    x64 = R.variance_case(M, C)
    x = f32(x64)
    xb = x.cpu().double()
    stats, ss = torch.zeros(2 * C, device=d), torch.empty(4 * C, device=d)
    g, b = torch.ones(C, device=d), torch.zeros(C, device=d)
    lib.bn_stats(0, x.data_ptr(), stats.data_ptr(), M, C, rt.stream())
    lib.bn_finalize(stats.data_ptr(), 1, None, float(M), g.data_ptr(), b.data_ptr(), None, None, None, 0.1, 0.0, ss.data_ptr(), C, 1, rt.stream())
    torch.cuda.synchronize()
    mean, var = xb.mean(0), xb.var(0, unbiased=False)
    got = 1 / ss.cpu().double().view(4, C)[3] ** 2
    rel = (got - var).abs() / var
    const = rel / R.var_envelope(mean, var, 1.0)
    for k, r in enumerate(R.VAR_RATIOS):
        print("bn_stats + bn_finalize   mean/std %5g: relative variance error %.3g, constant %.3g (KAPPA %.3g)" % (r, float(rel[k::4].max()), float(const[k::4].max()), R.KAPPA))
    assert bool((rel <= R.var_envelope(mean, var, R.KAPPA)).all()), (float(const.max()), R.KAPPA)
