"""CPU: tests/gemm_exact_ref.py -- the operand sets of tests/test_gpu_gemm_exact.py leave a correct kernel no choice (check_exact with the unloosened LIMITS), its references
agree with independent formulas, and its tables (e4m3 bytes, dropout key, GELU tolerance, reachable instances) hold what they claim."""
import numpy as np
import pytest
import torch

from tests import conv_exact_ref as C
from tests import gemm_exact_ref as R
from tests import rowwise_ref as RW

SETS = R.all_operand_sets()


def test_ids_are_unique():
    ids = [cid for cid, _ in SETS]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("cid,build", SETS, ids=[cid for cid, _ in SETS])
def test_operand_set_is_exact(cid, build):
    """bf16 results are bf16 numbers of magnitude <= 256, fp32 results exact, every sum of |terms| below 2^24, at least 90 % of every compared tensor non-zero"""
    assert R.LIMITS is C.LIMITS and C.LIMITS == {"bf16_max": 256.0, "sum_max": float(1 << 24), "nonzero_min": 0.90}
    fig = R.check_exact(build()["check"])
    assert fig["nonzero_min"] >= 0.90


def test_every_reachable_nt_instance_has_a_case():
    assert sorted(set(c["kernel"] for c in R.NT_CASES)) == R.NT_REACHABLE and len(R.NT_REACHABLE) == 22
    assert {c["tile"] for c in R.FP8_CASES} == {"64,64,4", "128,64,2", "128,128,2"}
    for c in R.FP8_CASES:
        assert R.fp8_tile(c["M"], c["N"]) == c["tile"] and c["K"] % 16 == 0


def test_hand_written_3x3x2():
    """A [3][2], W [3][2], bias, ReLU, residual, alpha 0.5 by hand"""
    a = torch.tensor([[1., 2.], [-1., 0.], [2., -2.]], dtype=R.F64)
    w = torch.tensor([[1., 1.], [0., -1.], [-1., 1.]], dtype=R.F64)
    c = dict(R._NT_DEF, act=2, alpha=0.5)
    o = R.nt_reference(c, a, w, dict(bias=torch.tensor([0.5, 0., -1.], dtype=R.F64), res=torch.ones(3, 3, dtype=R.F64)))
    assert o["pre"].tolist() == [[3.5, -2., 0.], [-0.5, 0., 0.], [0.5, 2., -5.]]
    assert o["v"].tolist() == [[3.5, 0., 0.], [0., 0., 0.], [0.5, 2., 0.]]
    assert o["out"].tolist() == [[2.75, 1., 1.], [1., 1., 1.], [1.25, 2., 1.]]
    P = torch.tensor([[1., 2., 0.], [-1., 0., 2.]], dtype=R.F64)
    Q = torch.tensor([[1., -1., 2.], [2., 0., 1.]], dtype=R.F64)
    assert (P.t() @ Q + 0.5).tolist() == [[-0.5, -0.5, 1.5], [2.5, -1.5, 4.5], [4.5, 0.5, 2.5]]


@pytest.mark.parametrize("cid", ["plain4_tr_bias_relu_pre_res", "plain4_st_n_odd_dropout", "plain4_st_dact2_ldz", "gen_k266", "fp8_64_half_scale", "plain4_st_colsum_stats_wrap"])
def test_nt_reference_against_int64_einsum(cid):
    """the float64 reference against integer arithmetic: everything scaled by 4 is an int64"""
    c = next(c for c in R.NT_CASES + R.FP8_CASES if c["id"] == cid)
    o = R.nt_operands(c)
    acc4 = 4 * torch.einsum("mk,nk->mn", o["a"].long(), o["w"].long())
    if "sc" in o:
        acc4 = acc4 // 2
        assert o["sc"] == 0.5
    pre4 = acc4 + ((4 * o["bias"]).long() if "bias" in o else 0)
    assert torch.equal(pre4.double() / 4, o["pre"])
    v4 = torch.where(pre4 > 0, pre4, torch.zeros_like(pre4)) if c["act"] == 2 else pre4
    if c["drop"]:
        key = RW.drop_key(R.RNG, R.RNG_STREAM, R.DROP_P)
        keep = torch.from_numpy(RW.drop_keep(key, np.arange(c["M"] * c["N"], dtype=np.uint64))).view(c["M"], c["N"])
        v4 = v4 * 2 * keep.long()
    if c["dact"] == 2:
        v4 = v4 * (o["z"] > 0).long()
    alpha2 = int(2 * c["alpha"])
    out8 = alpha2 * v4 + (8 * o["res"]).long() if "res" in o else alpha2 * v4
    assert torch.equal(out8.double() / 8, o["out"])
    if c["colsum"]:
        assert torch.equal(v4.sum(0).double() / 4 + 0.5, o["colsum"])
    if c["stats"]:
        assert torch.equal(torch.stack([v4.sum(0).double() / 4, (v4 * v4).sum(0).double() / 16]), o["stats"])


def test_tn_references_against_int64_einsum():
    c = R.TN_CASES[0]
    o = R.tn_operands(c)
    assert torch.equal(torch.einsum("mi,mj->ij", o["P"].long(), o["Q"].long()).double() + c["init"], o["out"])
    o2 = R.tn_operands(c, alter=(1000, 5))
    diff = (o2["out"] != o["out"]).nonzero()
    assert set(diff[:, 0].tolist()) == {5} and diff[:, 1].tolist() == (o["Q"][1000] != 0).nonzero().view(-1).tolist()
    b = R.BATCHED_CASES[0]
    ob = R.batched_operands(b)
    for bi in range(b["B"]):
        for h in range(b["H"]):
            want = ob["P"][bi, h].long().t() @ ob["Q"][bi, :, h].long()
            assert torch.equal(want.double() + b["init"], ob["out"][bi, :, h])
    t = R.GROUPED_CASES[0][1][0]
    og = R.grouped_operands(t)
    assert torch.equal((og["P"].long().t() @ og["Q"].long()).double() + t["init"], og["out"]) and torch.equal(og["P"].sum(0) + 0.5, og["colsum"])


def test_step_rows():
    rows, n = R.step_rows(187, (25, 50, 2))
    assert rows[:3].tolist() == [0, 2, 4] and rows[25].item() == 50 and rows[186].item() == 7 * 50 + 11 * 2 and n == 400 and int(rows.max()) < n
    assert len(set(rows.tolist())) == 187


def test_dropout_at_one_half_is_exact():
    """p = 0.5: threshold 32768, kept scale exactly 2; the mask of the next stream is another mask"""
    k0, thr, scale = RW.drop_key(R.RNG, R.RNG_STREAM, R.DROP_P)
    assert thr == 32768 and scale == 2.0
    m = R.drop_mask(R.RNG, R.RNG_STREAM, R.DROP_P, (300, 71))
    assert set(m.unique().tolist()) == {0.0, 2.0} and 0.45 < float((m > 0).double().mean()) < 0.55
    other = R.drop_mask(R.RNG, R.RNG_STREAM + 1, R.DROP_P, (300, 71))
    assert 0.4 < float((m != other).double().mean()) < 0.6


def test_fp8_scale_is_exact():
    f = np.float32
    assert f(448) * (f(1) / f(448)) == f(1) and f(224) * (f(1) / f(448)) == f(0.5)


def test_e4m3_table_round_trips():
    v = torch.arange(-16, 17).double()
    b = R.e4m3_bytes(v)
    assert torch.equal(R.e4m3_value(b), v) and len(set(b.tolist())) == 33
    for n, code in enumerate(R.E4M3[1:], 1):          # sign 0, exponent floor(log2 n) + 7, three mantissa bits
        e = n.bit_length() - 1
        assert code == ((e + 7) << 3) | int((n / 2 ** e - 1) * 8) and (n / 2 ** e - 1) * 8 == int((n / 2 ** e - 1) * 8)
    if hasattr(torch, "float8_e4m3fn"):
        assert torch.equal(b.view(torch.float8_e4m3fn).double(), v)
        assert torch.equal(v.to(torch.float8_e4m3fn).view(torch.uint8)[17:], b[17:])


def test_gelu_tolerance_is_8x_host_fp32():
    """as tests/test_rowwise_ref.py: the re-measurement must stay within 2 x of the record"""
    m = R.measure_gelu_host_fp32()
    print("gelu worst host fp32 ratio %.3g (recorded %.3g) tolerance %.3g" % (m, R.GELU_HOST_FP32_WORST, R.TOL["gelu"]))
    assert R.TOL["gelu"] == 8 * R.GELU_HOST_FP32_WORST and 0 < m <= 2 * R.GELU_HOST_FP32_WORST
    assert R.TOL["swish"] == RW.TOL["act"] == R.TOL["dswish"] and max(R.TOL.values()) < 2.0 ** -18
    x = torch.linspace(-6, 6, 49, dtype=R.F64)
    assert torch.allclose(R.gelu_(x), torch.nn.functional.gelu(x), rtol=1e-13, atol=1e-15) and bool((R.gelu_mag(x) >= R.gelu_(x).abs()).all())


def test_relu_cases_see_both_zeros():
    z = R.nt_operands(next(c for c in R.NT_CASES if c["id"] == "plain4_tr_dact2"))["z"].view(-1)
    assert z[0] == 0 and torch.signbit(z[0]) and z[3] == 0 and not torch.signbit(z[3]) and bool((z > 0).any()) and bool((z < 0).any())
