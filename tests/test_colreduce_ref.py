"""Host-only tests of tests/colreduce_ref.py: the reference formulas, the per-column metric, the input generators, the exactness bounds of every exact case of
tests/test_gpu_colreduce.py / tests/test_gpu_convmod_bn.py (worst-case sum < 2^24), and the two measured constants (TOL_SUM, KAPPA) against the host fp32
evaluation they are defined by."""
import math

import pytest
import torch

from tests import colreduce_ref as R


def test_col_ratio_judges_every_column_on_its_own():
    """one small-magnitude column that lost one of 16 partials passes the max-norm metric of tests/helpers.py and fails this one"""
    from tests.helpers import rel_err
    t = R.positive((1024, 8), 1)
    t[:, 3] *= 1e-4                                           # a column whose sum is 10^4 times smaller than its neighbours'
    ref, scale = R.reduce([t])
    got = ref.clone()
    got[3] -= t[:64, 3].sum()                                 # one slot of 64 rows dropped
    assert rel_err(got, ref) < 1e-5
    r = R.col_ratio(got, ref, scale)
    assert r[3] > 1 / 32 and float(r.max()) == float(r[3]) and bool((r[[0, 1, 2, 4, 5, 6, 7]] == 0).all())
    assert R.worst(got, ref, scale) > 1000 * R.TOL_SUM
    got = ref.clone(); got[5] = float("nan")
    assert math.isinf(R.worst(got, ref, scale)), "a NaN (stale workspace slot) must never pass"
    z = torch.zeros(4, dtype=torch.float64)
    assert R.worst(z, z, z) == 0 and math.isinf(R.worst(z + 1e-30, z, z)), "a column without terms must be exact"


def test_generators_are_reproducible_and_in_range():
    a, b = R.int_tensor((50, 7), -3, 3, 5), R.int_tensor((50, 7), -3, 3, 5)
    assert torch.equal(a, b) and a.min() == -3 and a.max() == 3 and torch.equal(a, a.round())
    assert torch.equal(a.to(torch.bfloat16).double(), a), "the exact inputs are bf16 numbers"
    p = R.positive((1000,), 2)
    assert p.min() >= 0.5 and not torch.equal(R.gauss((10,), 1), R.gauss((10,), 2))
    t, back = R.as_dtype(R.gauss((100,), 3), "bf16")
    assert t.dtype == torch.bfloat16 and torch.equal(t.double(), back)


def test_geometry_edges_are_in_the_shape_lists():
    """slot counts below / at / above 16 and 128 and not multiples of them; the col_grid cap; col8 with idle threads and with one row per block; all three audio-stem
    families; one utterance with fewer rows than a block"""
    gy = {R.col_grid(M, C)[1] for M, C in R.SHAPES_COL}
    assert {1, 2, 15, 16, 17, 20, 100, 127, 128, 129, 193} <= gy
    (M, C), = R.SHAPES_COL_CAP
    assert (M + 63) // 64 > R.col_grid(M, C)[1] == 2048 // R.col_grid(M, C)[0]
    cs = {C for _, C in R.SHAPES_COL}
    assert {4, 8, 64, 124, 128, 132, 144, 180, 256, 360, 2048} <= cs
    assert 256 % (144 // 8) != 0 and 256 // (2048 // 8) == 1 and 180 % 8 != 0
    ms = {M for M, _ in R.SHAPES_COL}
    assert {1, 7, 8, 9, 63, 64, 65, 1234, 6400} <= ms
    nb8 = {R.col8_blocks(M, C) for M, C in R.SHAPES_COL if C % 8 == 0}
    assert 1024 in nb8 and any(256 < n < 1024 for n in nb8), "col8: the cap, and a count the no-workspace path cuts to 256"
    slots = {R.dw_grid(B, T, C, s)[1] for B, T, C, K, s, _ in R.SHAPES_DW}
    assert {1, 3, 10, 16, 17, 36, 127, 128, 129, 384} <= slots
    assert {K for _, _, _, K, _, _ in R.SHAPES_DW} >= {3, 7, 15, 16} and any(T < K for _, T, _, K, _, _ in R.SHAPES_DW)
    fam = [R.stem_family(NM, C) for _, NM, _, C in R.SHAPES_STEM]
    assert set(fam) == {"8x", "8", "generic"} and R.stem_family(R.STEM_BENCH[1], R.STEM_BENCH[3]) == "8x"
    assert any(B == 1 and (R.stem_dims(NM, F)[1] % R.AS_ROWS) for B, NM, F, C in R.SHAPES_STEM)
    (F0, fit0), (F1, fit1) = R.STEM_EDGE
    assert R.stem_blocks(1, F0) * 2 * 4 * 4 == R.WS_MIN_BYTES and fit0 and R.stem_blocks(1, F1) == R.stem_blocks(1, F0) + 1 and not fit1


def test_partials_never_fit_64kb_when_the_threshold_asks_for_them():
    """the argument of the `small` set-up: a col_grid / col8 / depthwise launch that exceeds 16 384 atomics needs more than 16 384 floats of partials"""
    for M, C in R.SHAPES_COL + R.SHAPES_COL_CAP:
        gx, gy = R.col_grid(M, C)
        for NV in (1, 2):
            assert gx * gy * NV * 128 >= gy * NV * C
    for B, T, C, K, s, _ in R.SHAPES_DW + R.SHAPES_CONVMOD:
        gx, gy = R.dw_grid(B, T, C, s)
        for NV in (2, 17):
            assert gx * gy * NV * 128 >= gy * NV * C


def test_exact_cases_stay_below_2_pow_24():
    """every exact case: the sum of the magnitudes of its terms (which bounds every partial sum of every order), in units of the terms' granularity, is below 2^24"""
    for M, C in R.SHAPES_COL + R.SHAPES_COL_CAP:
        R.exact_or_die(torch.tensor([9.0 * M]), "colsum / bn_stats / grad_prep", (M, C))          # values 0..3, squares <= 9; 2 * |-3..3| = 6
        R.exact_or_die(torch.tensor([3.0 * (3 + 2) * 2 * M]), "bn_bwd_reduce", (M, C), 0.5)       # |d| <= 3, |y| + |mean| <= 5, rstd <= 2
    for i, shape in enumerate(R.SHAPES_DW):
        B, T, C, K, stride, causal = shape
        u, w, b = R.dw_inputs("exact", shape, i)
        _, ref, scale = R.dw_stats_ref(u, w, b, stride, K - 1 if causal else K // 2)
        R.exact_or_die(scale, "glu_dwconv_fwd stats", shape)
        assert torch.equal(ref, ref.round())
    for i, shape in enumerate(R.SHAPES_STEM):
        x = R.stem_inputs("exact", shape, 700 + 10 * i)
        y, ref, scale = R.stem_fwd_ref(x["mel"], x["w"], x["bias"])
        assert float(y.abs().max()) <= 10 and torch.equal(y, y.round())
        R.exact_or_die(scale, "audio stem stats", shape)
        refs = R.stem_bwd_ref(x["mel"], y, x["da"], x["ss"], x["gamma"], x["dstats"], x["count"])
        R.exact_or_die(refs["dstats"][1], "audio stem dstats", shape, 0.5)
        R.exact_or_die(refs["dw"][1], "audio stem dw", shape, 0.25)
        R.exact_or_die(refs["dbias"][1], "audio stem dbias", shape, 0.25)
        for k in refs:
            assert torch.equal(refs[k][0] * 4, (refs[k][0] * 4).round())
    with pytest.raises(AssertionError):
        R.exact_or_die(torch.tensor([2.0 ** 24]), "x", ())


def test_bench_shape_stem_statistics_bound():
    """the bench shape separately (its backward bounds are asserted by the GPU test itself, from the same reference)"""
    x = R.stem_inputs("exact", R.STEM_BENCH, 990)
    _, _, scale = R.stem_fwd_ref(x["mel"], x["w"], x["bias"])
    R.exact_or_die(scale, "audio stem stats", R.STEM_BENCH)


def test_reference_formulas_agree_with_torch():
    """glu -> conv1d -> batch_norm -> swish against torch modules; the audio stem against nn.Conv2d; bn_finalize_ref against batch_norm; the bit mask layout"""
    B, T, C, K = 2, 9, 8, 5
    u, w, b = R.gauss((B, T, 2 * C), 1), R.gauss((K, C), 2), R.gauss((C,), 3)
    conv = torch.nn.Conv1d(C, C, K, padding=K // 2, groups=C).double()
    with torch.no_grad():
        conv.weight.copy_(w.t().unsqueeze(1)); conv.bias.copy_(b)
    want = conv(torch.nn.functional.glu(u, -1).transpose(1, 2)).transpose(1, 2)
    assert torch.allclose(R.glu_dwconv_ref(u, w, b, 1, K // 2), want.detach(), atol=1e-12)
    causal = R.glu_dwconv_ref(u, w, b, 1, K - 1)
    g = torch.nn.functional.glu(u, -1)
    assert torch.allclose(causal[:, 0], b + w[K - 1] * g[:, 0], atol=1e-12), "causal: the first frame sees only itself, through the last tap"
    assert R.glu_dwconv_ref(u, w, b, 2, K // 2).shape[1] == (T - 1) // 2 + 1
    gamma, beta, da = R.gauss((C,), 4) + 1.5, R.gauss((C,), 5), R.gauss((B, T, C), 6)
    r = R.convmod_ref(u, w, b, gamma, beta, da, 1, K // 2, 1e-5)
    c = r["c"].reshape(-1, C)
    assert torch.allclose(c * r["ss"][0] + r["ss"][1], torch.nn.functional.batch_norm(c, None, None, gamma, beta, True, 0.1, 1e-5), atol=1e-12)
    assert torch.allclose(r["dbeta"], r["dz"].sum(0)) and torch.allclose(r["dgamma"], (r["dz"] * (c - r["ss"][2]) * r["ss"][3]).sum(0))
    mel, ws, bs = R.gauss((2, 10, 7), 7), R.gauss((3, 9), 8), R.gauss((3,), 9)
    c2 = torch.nn.Conv2d(1, 3, 3, stride=2, padding=1).double()
    with torch.no_grad():
        c2.weight.copy_(ws.view(3, 1, 3, 3)); c2.bias.copy_(bs)
    y, _ = R.audio_stem_ref(mel, ws, bs)
    assert torch.allclose(y, c2(mel.unsqueeze(1)).permute(0, 3, 1, 2).detach(), atol=1e-12) and y.shape == (2, 4, 3, 5)
    p = R.audio_stem_patches(mel)
    assert torch.allclose(torch.einsum("btfq,cq->btcf", p, ws) + bs.view(1, 1, 3, 1), y, atol=1e-12)
    # audio-stem backward against autograd through conv2d -> batch_norm -> swish
    wr, br, gr = ws.clone().requires_grad_(True), bs.clone().requires_grad_(True), (R.gauss((3,), 10) + 1.5).requires_grad_(True)
    yy = torch.nn.functional.conv2d(mel.unsqueeze(1), wr.view(3, 1, 3, 3), br, stride=2, padding=1)
    bt = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    a = R.swish(torch.nn.functional.batch_norm(yy, None, None, gr, bt, True, 0.1, 1e-5))
    da2 = R.gauss(tuple(a.shape), 11)
    a.backward(da2)
    yd = yy.detach().permute(0, 3, 1, 2)
    flat = yd.permute(0, 1, 3, 2).reshape(-1, 3)
    mean, var = flat.mean(0), flat.var(0, unbiased=False)
    rs = 1 / torch.sqrt(var + 1e-5)
    ss = torch.stack([gr.detach() * rs, -mean * gr.detach() * rs, mean, rs])
    n = float(flat.shape[0])
    d0 = R.stem_bwd_ref(mel, yd, da2.permute(0, 3, 1, 2), ss, gr.detach(), torch.zeros(6, dtype=torch.float64), n)["dstats"][0]
    refs = R.stem_bwd_ref(mel, yd, da2.permute(0, 3, 1, 2), ss, gr.detach(), d0, n)
    assert torch.allclose(refs["dw"][0], wr.grad, atol=1e-10) and torch.allclose(refs["dbias"][0], br.grad, atol=1e-10)
    assert torch.allclose(d0[3:], gr.grad, atol=1e-10) and torch.allclose(d0[:3], bt.grad, atol=1e-10)
    # bn_finalize_ref, bn_bwd_reduce_terms, pack_mask
    x = R.gauss((40, 6), 12) * 2 + 1
    rm, rv = torch.zeros(6, dtype=torch.float64), torch.ones(6, dtype=torch.float64)
    ss, rm1, rv1 = R.bn_finalize_ref(torch.cat([x.sum(0), (x * x).sum(0)]).view(1, -1), 40.0, torch.ones(6), torch.zeros(6), rm, rv, 0.1, 1e-5)
    rmt, rvt = rm.clone(), rv.clone()
    z = torch.nn.functional.batch_norm(x, rmt, rvt, None, None, True, 0.1, 1e-5)
    assert torch.allclose(x * ss[0] + ss[1], z, atol=1e-10) and torch.allclose(rm1, rmt) and torch.allclose(rv1, rvt)
    m = torch.zeros(2, 16, dtype=torch.bool); m[0, 0] = m[0, 9] = m[1, 7] = True
    assert R.pack_mask(m).tolist() == [1, 2, 128, 0]
    dout = R.gauss((40, 6), 13)
    t = R.bn_bwd_reduce_terms(dout, x, ss, 2, out=None)
    assert torch.equal(t[0], dout * (z > 0)) or torch.allclose(t[0], dout * (z > 0))


def _host_fp32_ratio(terms_fn, *args64):
    """the per-column metric of a plain fp32 host evaluation (torch fp32 sums) of a formula against its fp64 evaluation on the same (fp32-rounded) inputs"""
    a32 = [a.float() if torch.is_tensor(a) and a.dtype == torch.float64 else a for a in args64]
    a64 = [a.double() if torch.is_tensor(a) and a.dtype == torch.float32 else a for a in a32]
    ref, scale = terms_fn(*a64)
    got, _ = terms_fn(*a32)
    return R.worst(got, ref, scale)


def measure_host_fp32():
    """{formula: worst per-column ratio of the fp32 host evaluation over the shape lists}, Gaussian and positive inputs"""
    out = {}
    def upd(k, v):
        out[k] = max(out.get(k, 0.0), v)
    for mode in ("gauss", "positive"):
        for i, (M, C) in enumerate(R.SHAPES_COL):
            x = R.data(mode, (M, C), 11 + i)
            upd("colsum", _host_fp32_ratio(lambda t: R.reduce([t]), x))
            upd("bn_stats", _host_fp32_ratio(lambda t: R.reduce(R.stats_terms(t)), x))
            ss = torch.stack([torch.ones(C, dtype=torch.float64), 0.3 * R.gauss((C,), 1), 0.2 * R.gauss((C,), 2), 0.5 + R.gauss((C,), 3).abs()]).float().double()
            d = R.data(mode, (M, C), 101 + i)
            for act in (0, 1):
                upd("bn_bwd_reduce", _host_fp32_ratio(lambda a, b, act=act: R.bn_bwd_reduce_ref(a, b, ss, act), d, x))
        for i, shape in enumerate(R.SHAPES_DW):
            B, T, C, K, stride, causal = shape
            u, w, b = R.dw_inputs(mode, shape, i)
            upd("glu_dwconv stats", _host_fp32_ratio(lambda u, w, b: R.dw_stats_ref(u, w, b, stride, K - 1 if causal else K // 2)[1:], u, w, b))
        for i, shape in enumerate(R.SHAPES_STEM):
            x = R.stem_inputs(mode, shape, 700 + 10 * i)
            upd("audio stem stats", _host_fp32_ratio(lambda m, w, b: R.stem_fwd_ref(m, w, b)[1:], x["mel"], x["w"], x["bias"]))
            y = R.stem_fwd_ref(x["mel"].float().double(), x["w"].float().double(), x["bias"].float().double())[0]
            for k in ("dstats", "dw", "dbias"):
                upd("audio stem " + k, _host_fp32_ratio(lambda m, y, da, ss, g, ds, k=k: R.stem_bwd_ref(m, y, da, ss, g, ds, x["count"])[k],
                                                        x["mel"], y, x["da"], x["ss"], x["gamma"], x["dstats"]))
        for i, shape in enumerate(R.SHAPES_CONVMOD):
            B, T, C, K, stride, causal = shape
            if stride != 1 or mode != "gauss":              # (the convolution-module tests use Gaussian inputs only)
                continue
            x = R.convmod_inputs(mode, shape, i)
            padl = K - 1 if causal else K // 2
            f = [t.float().double() for t in (x["u"], x["w"], x["bias"], x["gamma"], x["beta"])]
            r = R.convmod_ref(*f, None, 1, padl, 1e-5)
            c, ss = r["c"].float().double(), r["ss"].float().double()
            for k in ("dstats", "dw", "dbias"):
                upd("convmod " + k, _host_fp32_ratio(lambda u, w, c, ss, g, da, k=k: R.convmod_bwd_ref(u, w, c, ss, g, da, padl)[k], f[0], f[1], c, ss, f[3], x["da"]))
    return out


def test_tolerance_is_8x_host_fp32():
    """R.TOL is 8 x the recorded worst per-column error of the plain fp32 host evaluation.  Re-measured here: torch's fp32 sums depend on the CPU's vector width and
    thread count, so the re-measurement may move by a small factor -- it must stay within 2 x of the record (then the tolerance is still >= 4 x a host
    evaluation), and the tolerance far below the size of one lost partial"""
    m = measure_host_fp32()
    assert sorted(m) == sorted(R.TOL)
    for k, v in sorted(m.items()):
        print("%-20s worst per-column ratio %.3g (recorded %.3g)   tolerance %.3g" % (k, v, R.HOST_FP32_WORST[k], R.TOL[k]))
        assert R.TOL[k] == 8 * R.HOST_FP32_WORST[k] and v <= 2 * R.HOST_FP32_WORST[k], (k, v, R.HOST_FP32_WORST[k])
    assert R.TOL_SUM < 1.0 / (2 * 2048), "one lost partial of the largest slot count must not fit under the tolerance"


def measure_du_fp32():
    """worst per-channel error (max |diff| / max |ref| per channel) of a plain fp32 host evaluation of the convolution-module backward's du"""
    worst = 0.0
    for mode in ("gauss",):
        for i, shape in enumerate(R.SHAPES_CONVMOD):
            B, T, C, K, stride, causal = shape
            if stride != 1:
                continue
            x = R.convmod_inputs(mode, shape, i)
            padl = K - 1 if causal else K // 2
            f = [t.float() for t in (x["u"], x["w"], x["bias"], x["gamma"], x["beta"])]
            r = R.convmod_ref(*[t.double() for t in f], None, 1, padl, 1e-5)
            c, ss, da = r["c"].float(), r["ss"].float(), x["da"].float()
            lo = R.convmod_bwd_ref(f[0], f[1], c, ss, f[3], da, padl)["du"]
            hi = R.convmod_bwd_ref(f[0].double(), f[1].double(), c.double(), ss.double(), f[3].double(), da.double(), padl)["du"]
            worst = max(worst, float(R.elem_ratio(lo, hi).max()))
    return worst


def test_du_fused_tolerance_is_8x_host_fp32():
    """the fused-against-unfused du tolerance of tests/test_gpu_convmod_bn.py is 8 x the recorded fp32 host error of the same formula (re-measured within 2 x)"""
    w = measure_du_fp32()
    print("convmod du: worst per-channel fp32 host error %.3g (recorded %.3g)" % (w, R.HOST_DU_FP32_WORST))
    assert w <= 2 * R.HOST_DU_FP32_WORST


def measure_kappa():
    x = R.variance_case(R.VAR_ROWS, 128).float()
    xb = x.double()
    mean, var = xb.mean(0), xb.var(0, unbiased=False)
    rel = (R.onepass_var_via_rstd_f32(x) - var).abs() / var
    const = rel / R.var_envelope(mean, var, 1.0)
    return [float(const[k::4].max()) for k in range(4)], [float(rel[k::4].max()) for k in range(4)]


def test_variance_kappa_is_4x_host_fp32():
    """KAPPA of the one-pass variance envelope |var - var_ref| / var_ref <= KAPPA eps (1 + mean^2 / var) is 4 x the constant of the host fp32 emulation"""
    const, rel = measure_kappa()
    for r, c, e in zip(R.VAR_RATIOS, const, rel):
        print("mean/std %5g: host fp32 one-pass relative variance error %.3g, constant %.3g" % (r, e, c))
    assert R.KAPPA == 4 * R.HOST_KAPPA_WORST and max(const) <= 1.5 * R.HOST_KAPPA_WORST, (const, R.KAPPA)
    t = torch.nn.functional.batch_norm
    x = R.variance_case(R.VAR_ROWS, 128).float()
    rm, rv = torch.zeros(128), torch.ones(128)
    t(x, rm, rv, None, None, True, 1.0, 1e-30)
    var = x.double().var(0, unbiased=True)
    assert float(((rv.double() - var).abs() / var).max()) < 1e-5, "the stable reference stays accurate where the one-pass formula does not"
