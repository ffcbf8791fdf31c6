"""Host-only tests of tests/attention_ref.py: the fp64 forward against explicit triple loops and against the pad/reshape form of the relative term, the backward
formulas against fp64 autograd, the preconditions of the case table (max|s| < 32, the spikes, fp32 absorption of -1e9), the recorded host-model errors that the
tolerances are 8 x of, the coverage of every reachable kernel instance by the case table, and seeded faults that the judge must reject under those tolerances."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import attention_ref as A

D64 = torch.float64
SMALL = [dict(B=2, H=2, T=5, Tk=5, d=3, lens=[5, 3], q_full=4), dict(B=1, H=2, T=4, Tk=7, d=2, lens=[6], q_full=0), dict(B=2, H=1, T=6, Tk=6, d=4, mask=True),
         dict(B=2, H=1, T=3, Tk=3, d=2, lens=[0, 7], len_div=3, q_full=0)]


def small_inputs(c, seed=1):
    B, H, T, Tk, d = (c[n] for n in ("B", "H", "T", "Tk", "d"))
    R = Tk + T - 1
    g = lambda shape, k: A.RW.gauss(shape, seed * 100 + k)
    mask = None
    if c.get("mask"):
        mask = (torch.rand(B, T, Tk, generator=torch.Generator().manual_seed(seed)) < 0.6).float()
        mask[:, :, 1] = 1
        mask[-1, 2] = 0                                                    # an all-zero row
    return dict(q=g((B, T, H, d), 1), k=g((B, Tk, H, d), 2), v=g((B, Tk, H, d), 3), e=g((R, H, d), 4), dO=g((B, T, H, d), 5), de0=g((R, H, d), 6), scale=0.7,
                lens=c.get("lens"), len_div=c.get("len_div", 1), q_full=c.get("q_full", 0), mask=mask,
                keep=A.keep_mask(B, T, Tk, c.get("lens"), c.get("len_div", 1), c.get("q_full", 0), mask))


def close(a, b, tol=1e-11):
    return a.shape == b.shape and bool(((a - b).abs() <= tol * (1 + b.abs())).all())


@pytest.mark.parametrize("c", SMALL)
def test_forward_against_triple_loops(c):
    """s, P, O, (m, l) element by element from the definition; a masked key has probability exactly 0 and a row without kept keys is uniform over all Tk keys"""
    inp = small_inputs(c)
    r = A.evaluate(inp)
    B, H, T, Tk, d = (c[n] for n in ("B", "H", "T", "Tk", "d"))
    for b in range(B):
        for h in range(H):
            for i in range(T):
                if inp["mask"] is not None:
                    kept = [j for j in range(Tk) if inp["mask"][b, i, j] != 0]
                else:
                    klen = Tk if c.get("lens") is None else c["lens"][b] // c.get("len_div", 1)
                    kept = [j for j in range(Tk) if j < klen and i < (c.get("q_full") or T)]
                s = [0.7 * sum(float(inp["q"][b, i, h, x]) * (float(inp["k"][b, j, h, x]) + float(inp["e"][T - 1 - i + j, h, x])) for x in range(d)) for j in range(Tk)]
                assert all(abs(s[j] - float(r["s"][b, h, i, j])) < 1e-12 for j in range(Tk))
                if kept:
                    m = max(s[j] for j in kept)
                    w = [math.exp(s[j] - m) if j in kept else 0.0 for j in range(Tk)]
                else:
                    m, w = A.NEG, [1.0] * Tk
                l = sum(w)
                assert float(r["m"][b, h, i]) == pytest.approx(m, abs=1e-12) and float(r["l"][b, h, i]) == pytest.approx(l, rel=1e-12)
                assert bool(r["full_masked"][b, h, i]) == (not kept)
                for j in range(Tk):
                    assert float(r["P"][0][b, h, i, j]) == pytest.approx(w[j] / l, rel=1e-12, abs=0 if j not in kept and kept else 1e-300)
                for x in range(d):
                    assert float(r["O"][0][b, i, h, x]) == pytest.approx(sum(w[j] / l * float(inp["v"][b, j, h, x]) for j in range(Tk)), abs=1e-12)


def rel_to_abs(x):
    """the pad / reshape form of the re-indexing, written from its definition: [..][T][2T-1] -> [..][T][T].  One zero column on the right, flatten, T - 1 zeros
    at the end, view as [T+1][2T-1], keep rows < T and columns >= T - 1"""
    T = x.shape[-2]
    flat = F.pad(F.pad(x, (0, 1)).flatten(-2), (0, T - 1))
    return flat.view(x.shape[:-2] + (T + 1, 2 * T - 1))[..., :T, T - 1:]


def test_skew_is_rel_to_abs():
    T = 7
    x = A.RW.gauss((2, 3, T, 2 * T - 1), 3)
    assert torch.equal(A.gather_rel(x, A.skew_index(T, T)), rel_to_abs(x))
    inp = small_inputs(dict(B=2, H=2, T=6, Tk=6, d=3))
    r = A.evaluate(inp)
    qh, kh, eh = inp["q"].permute(0, 2, 1, 3), inp["k"].permute(0, 2, 1, 3), inp["e"].permute(1, 0, 2)
    assert close(r["s"], 0.7 * (qh @ kh.transpose(-1, -2) + rel_to_abs(torch.einsum("bhtd,hrd->bhtr", qh, eh))))
    y = A.RW.gauss((2, 5, 9), 4)
    idx = A.skew_index(5, 9)
    assert torch.equal(A.gather_rel(A.scatter_rel(y, idx, 13), idx), y) and float(A.scatter_rel(y, idx, 13).abs().sum()) == pytest.approx(float(y.abs().sum()))


@pytest.mark.parametrize("c", SMALL)
def test_backward_against_autograd(c):
    """dQ, dK, dV, dE (+ the pre-filled de) against fp64 autograd of softmax(masked s) V; rows without a kept key are uniform (a constant), so autograd sees them
    through V only -- for those rows the explicit formulas let the gradient flow through the scores too, as the kernels do, and are compared on the other rows' terms"""
    inp = small_inputs(c)
    r = A.evaluate(inp)
    live = ~r["full_masked"]                                              # [B][H][T]
    q, k, v, e = (inp[n].clone().requires_grad_(True) for n in ("q", "k", "v", "e"))
    B, T, H, d = q.shape
    Tk = k.shape[1]
    qh, kh, vh, eh = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3), e.permute(1, 0, 2)
    i, j = torch.arange(T)[:, None], torch.arange(Tk)[None, :]
    s = 0.7 * (qh @ kh.transpose(-1, -2) + torch.einsum("bhid,hijd->bhij", qh, eh[:, T - 1 - i + j]))
    keep = inp["keep"][:, None].expand(B, H, T, Tk)
    # the uniform rows enter as softmax(s + constant -1e9) = softmax(s) in exact arithmetic: differentiable through s, like the kernels' recomputation
    p = torch.softmax(torch.where(keep | ~live[..., None], s, torch.full_like(s, -math.inf)), -1)
    dead_rows = (~live).any()
    o = (p @ vh).permute(0, 2, 1, 3)
    if not dead_rows:
        assert close(o, r["O"][0])
        (o * inp["dO"]).sum().backward()
        for n, t in (("dQ", q), ("dK", k), ("dV", v)):
            assert close(r[n][0], t.grad, 1e-10), n
        assert close(r["dE"][0], inp["de0"] + e.grad, 1e-10)
    else:                                                                  # the live rows alone, with dO of the dead rows zeroed in both
        g = inp["dO"] * live.permute(0, 2, 1)[..., None]
        (o * g).sum().backward()
        r2 = A.evaluate(dict(inp, dO=g))
        for n, t in (("dQ", q), ("dK", k), ("dV", v)):
            assert close(r2[n][0], t.grad, 1e-10), n
        assert close(r2["dE"][0], inp["de0"] + e.grad, 1e-10)
        # and the dead rows by the formulas' own definition at the uniform point: dS = (dP - mean(dP)) * scale / Tk
        dP = inp["dO"].permute(0, 2, 1, 3) @ inp["v"].permute(0, 2, 1, 3).transpose(-1, -2)
        want = (dP - dP.mean(-1, keepdim=True)) * 0.7 / Tk
        assert close(r["dS"][0][~live], want[~live])
    assert close(r["dSrel"][0], A.scatter_rel(r["dS"][0], A.skew_index(T, Tk), Tk + T - 1))


def test_case_table_preconditions():
    """max|s| < 32 in fp64 (so fp32 addition of -1e9 absorbs every score, checked on the fp32 scores themselves), every spike reaches p >= 0.5 on its kept pair, the
    spiking first masked key has probability exactly 0, and the table has the shapes the kernels switch at"""
    for case in A.CASES:
        assert case["B"] <= 3 and case["H"] <= 3
        for dtype in ("f32", "bf16"):
            inp = A.make_inputs(case, dtype)
            r = A.evaluate(inp)
            assert float(r["s"].abs().max()) < 32, (case["name"], float(r["s"].abs().max()))
            assert bool(((r["s"].float() + torch.tensor(A.NEG, dtype=torch.float32)) == A.NEG).all()), case["name"]
            P = r["P"][0]
            for b, i, j in inp["spikes"]:
                assert bool(inp["keep"][b, i, j]) and float(P[b, :, i, j].min()) >= 0.5, (case["name"], dtype, b, i, j, float(P[b, :, i, j].min()))
            if case["spike"] and case["lens"] is not None:
                for b in range(case["B"]):
                    pairs, klen = A.spike_pairs(case, b)
                    if klen < case["Tk"] and pairs:
                        i = pairs[0][0]
                        assert float(r["s"][b, :, i, klen].min()) > 13 and float(P[b, :, i, klen].abs().max()) == 0.0
    Ts, ds = {c["T"] for c in A.CASES}, {c["d"] for c in A.CASES}
    assert Ts >= {1, 2, 31, 32, 33, 63, 64, 65, 97, 224, 225, 320, 321, 384, 385} and ds >= {1, 8, 16, 17, 45, 46, 48, 64, 65, 90, 96, 97, 150, 192}
    assert {c["T"] for c in A.CASES if c["d"] == 90 and c["mask"] is None and c["Tk"] == c["T"]} >= {128, 129, 192, 193, 224, 225}
    assert {c["Tk"] - c["T"] for c in A.CASES} >= {0, 1, 37, 64}
    assert {c["len_div"] for c in A.CASES} == {1, 3} and all(any(l % 3 for l in c["lens"]) for c in A.CASES if c["len_div"] == 3)
    assert {(c["mask"][0], c["mask"][1] == c["B"]) for c in A.CASES if c["mask"]} >= {("random", False), ("random", True), ("causal", True), ("zero_row", False), ("zero_row", True)}
    rel = set()
    for c in A.CASES:
        if c["lens"]:
            for l in c["lens"]:
                rel |= {("T", l // c["len_div"] - c["Tk"]), ("abs", l // c["len_div"])}
    assert rel >= {("T", 0), ("T", -1), ("T", -13), ("abs", 32), ("abs", 33), ("abs", 1), ("abs", 0)}
    assert {(c["q_full"] - c["T"]) if c["q_full"] >= c["T"] - 1 else c["q_full"] for c in A.CASES} >= {-1, 30, 1} and any(c["q_full"] == 0 for c in A.CASES)
    assert max(c["B"] * c["H"] * c["T"] for c in A.CASES) == 2 * 2 * 385


def test_lds_bounds_and_instance_coverage():
    """the T / d bounds of the MFMA paths re-derived from mfma_geom, and every instance that the dispatch can select is reached by a case"""
    last = lambda d, bwd, alias: max(T for T in range(1, 385) if (A.mfma_geom(T, d, bwd) or (0, 2))[1] == alias)
    assert (last(64, False, 0), last(64, False, 1), last(64, True, 0), last(64, True, 1)) == (320, 384, 320, 384)
    assert (last(90, False, 0), last(90, False, 1), last(90, True, 0), last(90, True, 1)) == (128, 224, 128, 192)
    assert A.mfma_geom(225, 90, False) is None and A.mfma_geom(193, 90, True) is None and A.mfma_geom(384, 64, True) is not None
    assert A.route("bf16", 300, 90, 300, False, False) == ("attn_rows<bf16,fwd>", "attn_rows<bf16,bwd>+cols<96>")
    assert A.route("bf16", 200, 90, 200, False, True) == ("attn_mfma_fwd<256,12,1,6>", "attn_rows<bf16,bwd>")
    assert A.route("bf16", 65, 1, 65, False, False, ld=3)[0] == "attn_rows<bf16,fwd>" and A.route("bf16", 65, 1, 65, False, False, ld=15)[0] == "attn_mfma_fwd<128,7,0,0>"
    assert A.route("bf16", 384, 8, 384, False, True, ld=8) == ("attn_mfma_fwd<128,12,1,0>", "attn_mfma_bwd<128,12,1,0>")
    fwd, rows, cols = set(), set(), set()
    for c in A.CASES:
        for dt in ("f32", "bf16"):
            f, b = A.case_route(c, dt)
            if f:
                fwd.add(f)
            if b:
                rows.add(b.split("+")[0])
                if "+cols" in b:
                    cols.add((dt, int(b.split("+cols<")[1][:-1])))
    assert fwd == set(A.REACHABLE_FWD), sorted(set(A.REACHABLE_FWD) ^ fwd)
    assert rows == set(A.REACHABLE_BWD_ROWS), sorted(set(A.REACHABLE_BWD_ROWS) ^ rows)
    assert cols == set(A.REACHABLE_COLS), sorted(set(A.REACHABLE_COLS) ^ cols)
    assert A.route("bf16", 33, 97, 33, False, False)[1] is None and A.route("f32", 33, 150, 33, False, True) == ("attn_rows<f32,fwd>", None)
    assert A.route("f32", 31, 192, 31, False, True) == (None, None) and (A.valu_lds(159, False), A.valu_lds(141, True)) == (163204, 162892) and A.valu_lds(160, False) > A.LDS_LIMIT < A.valu_lds(142, True)


@pytest.fixture(scope="module")
def measured():
    return A.measure_host()


def test_tolerance_is_8x_host_model(measured):
    """A.TOL is 8 x the recorded worst ratio of the host model of each kernel family's rounding points.  Re-measured here: torch's fp32 sums depend on the CPU's
    vector width and thread count, so the figure may move by a small factor; it must stay within 2 x of the record either way, or the record is stale"""
    for mdl in A.MODELS:
        for fam in A.FAMILIES:
            v, rec = measured[mdl][fam], A.HOST_WORST[mdl][fam]
            print("%-10s %-6s host worst %.3g (recorded %.3g)   tolerance %.3g" % (mdl, fam, v, rec, A.TOL[mdl][fam]))
            assert A.TOL[mdl][fam] == 8 * rec and rec / 2 <= v <= 2 * rec, (mdl, fam, v, rec)
    assert max(A.TOL["valu_f32"].values()) < 2.0 ** -13 and max(max(t.values()) for t in A.TOL.values()) < 2.0 ** -5, "no more than 8 bf16 roundings of an element's own terms"


FAULTS = ["drop_tile_last", "skew_off_by_one", "klen_inclusive", "ceil_len_div", "phantom_key", "no_inv_l", "masked_row_over_klen", "q_full_plus_one", "de_row_shift",
          "de_overwrite"]


@pytest.mark.parametrize("fault", FAULTS)
def test_judge_rejects_seeded_fault(fault):
    """each fault, seeded into the host model of BOTH dtypes' kernels, misses the committed tolerance on at least one case of the table -- in every model that the
    table runs (a tolerance wide enough to hide it in the bf16 models would pass here only through the fp32 one otherwise)"""
    caught = {m: [] for m in A.MODELS}
    for case in A.CASES:
        for dtype in ("f32", "bf16"):
            r, (fm, bm) = A.host_ratios(case, dtype, fault)
            for fam, w in r.items():
                mdl = fm if fam in ("O", "lse") else bm
                if not w <= A.TOL[mdl][fam]:
                    caught[mdl].append((case["name"], fam, w))
    for mdl in A.MODELS:
        print(fault, mdl, len(caught[mdl]), caught[mdl][:3])
        assert caught[mdl], (fault, mdl, "not rejected by any case")
