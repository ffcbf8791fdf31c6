"""GPU (-m gpu): the PLAIN products of csrc/gemm.hip -- avec_gemm_nt in plain mode with every epilogue form, avec_gemm_nt_fp8 and the avec_gemm_tn family (plain, bias,
batched, batched-store, batched-multi, grouped) -- reproduce an integer reference EXACTLY, at every element.  The companion of tests/test_gpu_conv_exact.py, which holds
the convolution modes of the same entry points.

tests/gemm_exact_ref.py holds the operands (activations and gradients in {-2 .. 2}, weights in {-1, 0, 1}, bias / residual / initial values in integers or halves, alpha 1
or 0.5, dropout at p = 0.5 whose kept scale is exactly 2), the float64 references and the case tables; check_exact() asserts on the reference alone that every product,
every fp32 partial sum in any order (split-K atomics, the 64 statistics replicas, column sums) and every bf16 result is exactly representable.  Every comparison below is
therefore torch.equal; a failure names the differing elements as (row, column) / (i, j) / (batch, i, head, j) with expected and got values.  Operands lie `off` elements
behind an aligned address with 64 spare elements behind them -- NaN there and in the padding columns of rows with lda / ldw > K, so a kernel that reads past K or past the
last row into a product shows it (the zero padding that the header requires of avec_gemm_tn's Iq / Jq rows stays zero); outputs are NaN-filled with a guard row, and the
gap columns of ldo > N (ldpre, ldo > J) must still hold NaN afterwards.  Every case asserts the kernel instance it means to reach (avec_last_kernel): move a case whose
shape a retuned dispatch sends elsewhere.

Transcendental activations (Swish, GELU, dact = 1) cannot be bit-exact: out_pre and the set of written elements stay exact, the activated output is judged per element
(rowwise_ref.ratio) against the float64 function of the exact pre-activation with gemm_exact_ref.TOL (8 x the host fp32 evaluation's own worst ratio).

Instances reached (and asserted), beside the MODE 0 instances that launch_nt_mode / launch_nt_general can reach without an environment variable
(gemm_exact_ref.NT_REACHABLE, 22: none is missing):
  gemm_nt_plain_kernel<64,64,{2,4},{tr,false}>
  gemm_nt_glds_kernel<{bf16,float},{128,128 | 128,64},0,2,0,128>, <{bf16,float},64,64,0,4,0,128> (bf16: by the strided row source; without it the lean plain kernel
      takes every such product unless an operand exceeds 4 GiB)
  gemm_nt_kernel<bf16,{128,128 | 128,64 | 64,64},0,{0,0 | 1,0 | 1,1}> (K = 8n + 2; the fp32 source unaligned and aligned), <float,{128,128 | 128,64 | 64,64},0,0,0>
  gemm_nt_fp8_kernel<64,64,4>, <128,64,2>, <128,128,2>: the entry point notes no name; asserted are the return code and the shape rule of its dispatch (fp8_tile)
  gemm_tn_tr_kernel<{64,64 | 128,128 | 64,128},0,2,0,32>
  gemm_tn_kernel<bf16,64,64,0,{0,0 | 0,1 | 1,0 | 1,1}>, <bf16,128,128,0,0,0>, <float,64,64,0,{0,0 | 0,1}>, <float,128,128,0,0,1>
  gemm_tn_multi_kernel<1>, <2>, <3>;  gemm_tn_tr_grouped_kernel<64,2,64>, <128,2,64>
Not reached: gemm_tn_kernel<bf16,128,128,0,0,1> / <bf16,128,128,0,1,*> / <float,128,128,0,0,0> (the same code as the instances above at another tile or alignment flag;
left out to keep the file short), and everything behind an environment variable.

Not here, and why: the variants forced by AVEC_NT_RB, AVEC_NO_PLAIN_TR, AVEC_NO_EPI_TR, AVEC_TN_KT, AVEC_TN_WGS and AVEC_NO_LEAN_CONV are read once per process (the tests
that set them in child processes stay where they are); the convolution modes (tests/test_gpu_conv_exact.py); operands beyond 4 GiB (32-bit offsets of the lean kernel).

Wall time of the whole file on an MI355X: about 7 s for its 97 tests (the slowest, the 49 029-row cases, 0.3 s each: float64 reference and upload).  Measured per-element
ratios of the transcendental cases: Swish 0 beyond the half bf16 ulp, dswish 1.2e-7 (bound 1.45e-6), GELU 3.8e-8 (bound 3.1e-7).
"""
import ctypes

import pytest
import torch

from tests import gemm_exact_ref as R
from tests import rowwise_ref as RW

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
NAN = float("nan")
RC, IJ = ("row", "column"), ("i", "j")


def dev():
    return torch.device("cuda:0")


def _lib():
    from avec_amd import lib as L, runtime as rt
    return L, rt


def last_kernel():
    L, _ = _lib()
    return L.lib.raw("avec_last_kernel")().decode()


def up(t, dtype, ld=None, off=0, pad=NAN, spare=NAN):
    """the float64 matrix `t` on the device as `dtype` with row stride `ld` (padding columns hold `pad`), `off` elements behind an aligned address, 64 spare elements
    holding `spare` behind it (exact: check_exact has seen the values)"""
    rows, cols = t.shape
    ld = cols if ld is None else ld
    host = torch.full((rows, ld), pad, dtype=torch.float64)
    host[:, :cols] = t
    buf = torch.full((rows * ld + off + 64,), spare, dtype=dtype, device=dev())
    buf[off:off + rows * ld].copy_(host.reshape(-1).to(dtype))
    return buf[off:off + rows * ld]


def up_bytes(t, ld):
    """e4m3 bytes of an integer matrix, padding columns and spare bytes NaN (0x7f)"""
    rows, cols = t.shape
    host = torch.full((rows, ld), 0x7F, dtype=torch.uint8)
    host[:, :cols] = R.e4m3_bytes(t)
    buf = torch.full((rows * ld + 64,), 0x7F, dtype=torch.uint8, device=dev())
    buf[:rows * ld].copy_(host.reshape(-1))
    return buf[:rows * ld]


class Out:
    """[rows + 1][ld] on the device, `off` elements behind an aligned address: NaN everywhere (or `init` in the first `rows` rows and `cols` columns); the last row is the guard"""

    def __init__(self, rows, cols, ld, dtype, off=0, init=None):
        self.rows, self.cols, self.off = rows, cols, off
        self.flat = torch.full((off + (rows + 1) * ld,), NAN, dtype=dtype, device=dev())
        self.view = self.flat[off:].view(rows + 1, ld)
        if init is not None:
            self.view[:rows, :cols] = init if not torch.is_tensor(init) else init.to(dtype).to(dev())

    def ptr(self):
        return self.view.data_ptr()

    def got(self):
        return self.view[:self.rows, :self.cols].cpu()

    def check(self, ref, shape, names, what):
        R.assert_exact(self.got(), ref, shape, names, what)
        self.check_untouched(what)

    def check_untouched(self, what):
        assert bool(torch.isnan(self.view[:self.rows, self.cols:]).all()), "%s: the gap between the row width and the row stride was written" % what
        assert bool(torch.isnan(self.view[-1]).all()) and bool(torch.isnan(self.flat[:self.off]).all()), "%s: written outside the output" % what


def rng_state():
    return torch.tensor(list(R.RNG), dtype=torch.int64, device=dev())


# ---- avec_gemm_nt (plain mode) and avec_gemm_nt_fp8 -----------------------------------------------------------------------------------------------
def launch_nt(c, o, stream=R.RNG_STREAM):
    """one call on the operands `o` of case `c`: {name: Out}, the replicated statistics (or None), the kernel reached"""
    L, rt = _lib()
    fp8 = "tile" in c
    f32 = c["dtype"] == "f32"
    T = torch.float32 if f32 else torch.bfloat16
    M, N, K = c["M"], c["N"], c["K"]
    lda, ldw = c["lda"] or K, c["ldw"] or K
    ld = {k: c[k] or N for k in ("ldo", "ldpre", "ldres", "ldz")}
    rows = L.Rows()
    rows.ld = lda
    a = o["a"]
    if c["step"]:                     # strided row source: NaN in the rows that no output row reads
        idx, nsrc = R.step_rows(M, c["step"])
        src = torch.full((nsrc, K), NAN, dtype=torch.float64)
        src[idx] = a
        a = src
        rows.rows_out, rows.rows_in, rows.step = c["step"]
    if fp8:
        A, W = up_bytes(a, lda), up_bytes(o["w"], ldw)
        amax = torch.tensor([c["amax_a"], c["amax_w"]], dtype=torch.float32, device=dev())
    else:
        A, W = up(a, torch.float32 if c["a_f32"] else T, lda, c["off_a"]), up(o["w"], T, ldw, c["off_w"])
    keep = [A, W]
    odt = torch.float32 if (f32 or c["out_f32"]) else torch.bfloat16
    outs = {}
    ep = L.Epilogue()
    ep.alpha, ep.act, ep.out_f32 = c["alpha"], c["act"], int(c["out_f32"])
    if c["res"]:
        rdt = T if c["res"] == "bf16" else torch.float32
        if c["alias"]:                # `out` is the residual buffer itself
            assert rdt == odt and ld["ldo"] == ld["ldres"]
            outs["out"] = Out(M, N, ld["ldo"], odt, c["off_out"], init=o["res"])
            ep.res = outs["out"].ptr()
        else:
            keep.append(up(o["res"], rdt, ld["ldres"]))
            ep.res = keep[-1].data_ptr()
        ep.ldres, ep.res_act = ld["ldres"], int(c["res"] == "bf16")
    if "out" not in outs:
        outs["out"] = Out(M, N, ld["ldo"], odt, c["off_out"])
    ep.out, ep.ldo = outs["out"].ptr(), ld["ldo"]
    if c["out_pre"]:
        outs["pre"] = Out(M, N, ld["ldpre"], T)
        ep.out_pre, ep.ldpre = outs["pre"].ptr(), ld["ldpre"]
    if "bias" in o:
        keep.append(up(o["bias"].view(1, -1), torch.float32)); ep.bias = keep[-1].data_ptr()
    if c["drop"]:
        keep.append(rng_state()); ep.drop_p, ep.rng, ep.rng_stream = R.DROP_P, keep[-1].data_ptr(), stream
    if c["dact"]:
        keep.append(up(o["z"], T, ld["ldz"])); ep.dact_z, ep.ldz, ep.dact = keep[-1].data_ptr(), ld["ldz"], c["dact"]
    if c["colsum"]:
        outs["colsum"] = Out(1, N, N, torch.float32, init=0.5); ep.colsum = outs["colsum"].ptr()
    st = None
    if c["stats"]:
        st = Out(128, N, N, torch.float32, init=0.0); ep.stats = st.ptr()
    if fp8:
        L.lib.gemm_nt_fp8(A.data_ptr(), lda, W.data_ptr(), ldw, M, N, K, amax.data_ptr(), amax.data_ptr() + 4, ctypes.byref(ep), rt.stream())
        name = None
    else:
        L.lib.gemm_nt(F32 if f32 else BF16, A.data_ptr(), ctypes.byref(rows), 0, int(c["a_f32"]), W.data_ptr(), ldw, M, N, K, ctypes.byref(ep), rt.stream())
        name = last_kernel()
    torch.cuda.synchronize()
    return outs, st, name


def run_nt(c):
    o = R.nt_operands(c)
    R.check_exact(o["check"])
    M, N = c["M"], c["N"]
    outs, st, name = launch_nt(c, o)
    if "tile" in c:
        assert R.fp8_tile(M, N) == c["tile"], "%s: the dispatch rule sends this shape to %s" % (c["id"], R.fp8_tile(M, N))
    else:
        assert name == c["kernel"], "%s reached %s, not %s" % (c["id"], name, c["kernel"])
    if "pre" in outs:
        outs["pre"].check(o["pre"], (M, N), RC, c["id"] + ": out_pre")
    if o["transcendental"]:
        kind = o["transcendental"]
        odt = "f32" if (c["out_f32"] or c["dtype"] == "f32") else "bf16"
        worst = RW.worst(outs["out"].got(), o["out"], o["scale"], odt)
        print("%s: worst per-element ratio %.3g (tolerance %.3g)" % (c["id"], worst, R.TOL[kind]))
        assert worst <= R.TOL[kind], "%s: %s misses its per-element bound: %.3g > %.3g" % (c["id"], kind, worst, R.TOL[kind])
        outs["out"].check_untouched(c["id"])
        return
    outs["out"].check(o["out"], (M, N), RC, c["id"])
    if "colsum" in outs:
        outs["colsum"].check(o["colsum"], (N,), ("column",), c["id"] + ": column sums")
    if st is not None:               # the 64 replicas of [sum | second moment] summed in float64 (each replica is exact on its own)
        R.assert_exact(st.got().view(64, 2, N).double().sum(0), o["stats"], (2, N), ("sum | second moment", "column"), c["id"] + ": statistics")
        st.check_untouched(c["id"] + ": statistics")


@pytest.mark.parametrize("c", R.NT_CASES, ids=[c["id"] for c in R.NT_CASES])
def test_gemm_nt_plain_exact(c):
    """every MODE 0 instance of avec_gemm_nt with the epilogue forms it has (register-direct, 64-column four-row-group, staged 4-wide, staged scalar): bias, ReLU, out_pre,
    dropout, act'(z), column sums, statistics, alpha, bf16 / fp32 residual, fp32 output; ragged M and N, padded row strides, K tails, unaligned operands"""
    run_nt(c)


@pytest.mark.parametrize("c", R.FP8_CASES, ids=[c["id"] for c in R.FP8_CASES])
def test_gemm_nt_fp8_exact(c):
    """e4m3 operands holding the same small integers, amax 448 (scale exactly 1) or 224 (exactly 0.5), on the three tiles"""
    run_nt(c)


def _case(table, cid):
    return next(c for c in table if c["id"] == cid)


def test_one_altered_activation_in_the_k_tail_is_found_in_its_row():
    """negative control on the unmodified kernel: A[137][K - 1] (K = 180 = 8n + 4: the element lies in the in-LDS tail fix-up) raised by 1 on the device only.  The
    unaltered reference must differ in row 137 alone, exactly at the columns n with W[n][K - 1] != 0, and the result must equal the reference of the altered A"""
    c = _case(R.NT_CASES, "plain4_tr_ktail_180")
    o = R.nt_operands(c)
    a2 = o["a"].clone()
    a2[137, c["K"] - 1] += 1
    outs, _, name = launch_nt(c, dict(o, a=a2))
    assert name == c["kernel"]
    got = outs["out"].got().double()
    bad = (got != o["out"]).nonzero().tolist()
    want = [[137, n] for n in (o["w"][:, c["K"] - 1] != 0).nonzero().view(-1).tolist()]
    assert bad == want and len(want) > 20, (bad, want)
    assert torch.equal(got, R.nt_reference(c, a2, o["w"], o)["out"])


def test_the_mask_of_another_stream_does_not_match():
    """negative control: the dropout case launched with rng_stream + 1 differs from the reference of rng_stream and equals the one of rng_stream + 1"""
    c = _case(R.NT_CASES, "plain4_tr_dropout")
    o = R.nt_operands(c)
    outs, _, _ = launch_nt(c, o, stream=R.RNG_STREAM + 1)
    got = outs["out"].got().double()
    assert not torch.equal(got, o["out"]) and float((got != o["out"]).double().mean()) > 0.3
    other = dict(o, keep=R.drop_mask(R.RNG, R.RNG_STREAM + 1, R.DROP_P, (c["M"], c["N"])))
    assert torch.equal(got, R.nt_reference(c, o["a"], o["w"], other)["out"])


# ---- avec_gemm_tn / avec_gemm_tn_bias ---------------------------------------------------------------------------------------------------------------
def launch_tn(c, o):
    L, rt = _lib()
    f32 = c["dtype"] == "f32"
    T = torch.float32 if f32 else torch.bfloat16
    M, I, J = c["M"], c["I"], c["J"]
    ldp, ldq, ldo = c["ldp"] or I, c["ldq"] or J, c["ldo"] or J
    P = up(o["P"], T, ldp, c["off_p"], pad=0.0)                      # (padding columns zero as the header requires, NaN behind the last row)
    Q = up(o["Q"], torch.float32 if c["q_f32"] else T, ldq, c["off_q"], pad=0.0)
    O = Out(I, J, ldo, torch.float32, init=c["init"])
    cs = Out(1, I, I, torch.float32, init=0.5) if c["colsum"] else None
    rows = L.Rows()
    rows.ld = ldq
    dt = F32 if f32 else BF16
    if c["entry"] == "bias":
        L.lib.gemm_tn_bias(dt, P.data_ptr(), ldp, Q.data_ptr(), ctypes.byref(rows), 0, int(c["q_f32"]), O.ptr(), ldo, cs.ptr(), M, I, J, rt.stream())
    else:
        L.lib.gemm_tn(dt, P.data_ptr(), ldp, Q.data_ptr(), ctypes.byref(rows), 0, int(c["q_f32"]), O.ptr(), ldo, M, I, J, rt.stream())
    name = last_kernel()
    torch.cuda.synchronize()
    return O, cs, name


@pytest.mark.parametrize("c", R.TN_CASES, ids=[c["id"] for c in R.TN_CASES])
def test_gemm_tn_exact(c):
    """O += P^T Q on a non-zero O: split reductions with a short last slice and a partial last K tile, I / J padded to the vector width, ldo > J, the column sums of P
    fused and as the separate pass (on non-zero sums)"""
    o = R.tn_operands(c)
    R.check_exact(o["check"])
    O, cs, name = launch_tn(c, o)
    assert name == c["kernel"], "%s reached %s, not %s" % (c["id"], name, c["kernel"])
    O.check(o["out"], (c["I"], c["J"]), IJ, c["id"])
    if cs is not None:
        cs.check(o["colsum"], (c["I"],), ("i",), c["id"] + ": column sums")


def test_one_altered_gradient_in_the_last_k_tile_is_found_in_its_row():
    """negative control on the unmodified split-K kernel: P[1000][5] (M = 1003: the last, partial reduction tile of the last, short slice) raised by 1 on the device only.
    The unaltered reference must differ in row 5 of O alone, exactly at the columns j with Q[1000][j] != 0, and the result must equal the reference of the altered P"""
    c = R.TN_CASES[0]
    assert c["id"] == "tn_tr_64_m1003_j245"
    o, o2 = R.tn_operands(c), R.tn_operands(c, alter=(1000, 5))
    O, _, name = launch_tn(c, o2)
    assert name == c["kernel"]
    got = O.got().double()
    bad = (got != o["out"]).nonzero().tolist()
    want = [[5, j] for j in (o["Q"][1000] != 0).nonzero().view(-1).tolist()]
    assert bad == want and len(want) > 50, (bad, want)
    assert torch.equal(got, o2["out"])


# ---- batched forms ------------------------------------------------------------------------------------------------------------------------------------
BIHJ = ("batch", "i", "head", "j")


def batched_buffers(c, o):
    """P [B][H][M][I], Q [B][M][H * d + pad] (heads side by side: head h starts on element h * d), O [B][I][H * d + pad], the six batch strides"""
    B, H, M, I, d = c["B"], c["H"], c["M"], c["I"], c["d"]
    ldq = H * d + c["pad"]
    P = up(o["P"].reshape(B * H * M, I), torch.bfloat16, pad=0.0)
    Q = up(o["Q"].reshape(B * M, H * d), torch.bfloat16, ldq, pad=0.0)
    O = Out(B * I, H * d, ldq, torch.bfloat16 if c["store"] else torch.float32, init=None if c["store"] else c["init"])
    st6 = (ctypes.c_longlong * 6)(H * M * I, M * I, M * ldq, d, I * ldq, d)
    return P, Q, O, ldq, st6


def check_batched(c, o, O):
    O.check(o["out"].reshape(c["B"] * c["I"], c["H"] * c["d"]), (c["B"], c["I"], c["H"], c["d"]), BIHJ, c["id"])


@pytest.mark.parametrize("c", R.BATCHED_CASES, ids=[c["id"] for c in R.BATCHED_CASES])
def test_gemm_tn_batched_exact(c):
    """avec_gemm_tn_batched (fp32, accumulating) and _batched_store (bf16, every element of every head written once, the padding column untouched): 2 x 3 batches with
    different outer and inner strides, heads of width 45 (Q batches start on odd elements) and 90"""
    L, rt = _lib()
    o = R.batched_operands(c)
    R.check_exact(o["check"])
    P, Q, O, ldq, st6 = batched_buffers(c, o)
    fn = L.lib.gemm_tn_batched_store if c["store"] else L.lib.gemm_tn_batched
    fn(BF16, P.data_ptr(), c["I"], Q.data_ptr(), ldq, O.ptr(), ldq, c["M"], c["I"], c["d"], c["B"], c["H"], st6, rt.stream())
    name = last_kernel()
    torch.cuda.synchronize()
    assert name == c["kernel"], "%s reached %s, not %s" % (c["id"], name, c["kernel"])
    check_batched(c, o, O)


@pytest.mark.parametrize("kernel,problems", R.MULTI_CASES, ids=[k for k, _ in R.MULTI_CASES])
def test_gemm_tn_batched_multi_exact(kernel, problems):
    """up to three problems of different I, J and batch count in one launch, accumulating and storing ones mixed; a 128 x 128-tile problem runs alone before it"""
    L, rt = _lib()
    items, held = (L.TnBatched * len(problems))(), []
    for k, c in enumerate(problems):
        o = R.batched_operands(c)
        R.check_exact(o["check"])
        P, Q, O, ldq, st6 = batched_buffers(c, o)
        held.append((c, o, P, Q, O, st6))
        t = items[k]
        t.P, t.ldp, t.Q, t.ldq, t.ldo, t.M, t.I, t.J, t.nb_outer, t.nb_inner, t.strides6 = P.data_ptr(), c["I"], Q.data_ptr(), ldq, ldq, c["M"], c["I"], c["d"], c["B"], c["H"], st6
        if c["store"]:
            t.O_act = O.ptr()
        else:
            t.O = O.ptr()
    L.lib.gemm_tn_batched_multi(BF16, ctypes.byref(items), len(problems), rt.stream())
    name = last_kernel()
    torch.cuda.synchronize()
    assert name == kernel, name
    for c, o, _, _, O, _ in held:
        check_batched(c, o, O)


# ---- grouped weight gradients ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,group", R.GROUPED_CASES, ids=[g[0]["id"] for _, g in R.GROUPED_CASES])
def test_gemm_tn_grouped_exact(kernel, group):
    """avec_gemm_tn_grouped on both tile sizes: items of different M, I and J with ld == width (rows of I = 180 / 90 run into the next row), the step-2 row remap of Q
    with NaN in the skipped rows, column sums of P on some items only, 32 items, one item alone"""
    L, rt = _lib()
    items, held = (L.TnItem * len(group))(), []
    for k, t in enumerate(group):
        o = R.grouped_operands(t)
        R.check_exact(o["check"])
        q = o["Q"]
        it = items[k]
        if t["step"]:
            idx, nsrc = R.step_rows(t["M"], (R.G_ROWS_OUT, 2 * R.G_ROWS_OUT, 2))
            q = torch.full((nsrc, t["J"]), NAN, dtype=torch.float64)
            q[idx] = o["Q"]
            it.q_rows_out, it.q_rows_in, it.q_step = R.G_ROWS_OUT, 2 * R.G_ROWS_OUT, 2
        P, Q = up(o["P"], torch.bfloat16), up(q, torch.bfloat16)
        O = Out(t["I"], t["J"], t["J"], torch.float32, init=t["init"])
        cs = Out(1, t["I"], t["I"], torch.float32, init=0.5) if t["colsum"] else None
        held.append((t, o, P, Q, O, cs))
        it.P, it.Q, it.O, it.ldp, it.ldq, it.ldo, it.M, it.I, it.J = P.data_ptr(), Q.data_ptr(), O.ptr(), t["I"], t["J"], t["J"], t["M"], t["I"], t["J"]
        if cs is not None:
            it.p_colsum = cs.ptr()
        assert L.lib.raw("avec_gemm_tn_grouped_ok")(BF16, ctypes.byref(it)) == 1
    L.lib.gemm_tn_grouped(BF16, ctypes.byref(items), len(group), rt.stream())
    name = last_kernel()
    torch.cuda.synchronize()
    assert name == kernel, name
    for t, o, _, _, O, cs in held:
        O.check(o["out"], (t["I"], t["J"]), IJ, t["id"])
        if cs is not None:
            cs.check(o["colsum"], (t["I"],), ("i",), t["id"] + ": column sums")
