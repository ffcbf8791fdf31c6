"""Host-only tests of tests/loss_optim_ref.py: every fp64 reference of tests/test_gpu_loss_optim.py against something that does not share its code (the oracle's own
CTC recursion, a sum over all V^T paths, closed forms, torch.optim.Adam, explicit loops), the routing table against the restated launcher arithmetic, and the case
builders against what their rows claim to be."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import loss_optim_ref as R


# ---- CTC -----------------------------------------------------------------------------------------------------------------------------------------
def test_ctc_ref_equals_oracle_recursion_on_every_case_row():
    """oracle.avec_oracle.ctc_nll is an own log-space alpha recursion in fp32 (not aten): 1e-5 relative is 40 roundings of a sum of T <= 188 terms"""
    from oracle import avec_oracle as O
    for (T, Lmax, V), _ in R.CTC_SHAPES:
        x, il, tg, tl, feas = R.ctc_case(T, Lmax, V)
        nll, grad = R.ctc_ref(x, il, tg, tl, True)
        ora = O.ctc_nll(x, il, tg, tl).double()
        assert bool((nll[~feas] == 0).all()) and bool((ora[~feas] == 0).all())
        assert bool(((nll - ora).abs() <= 1e-5 * nll.abs() + 1e-6).all()), (T, Lmax, V, nll, ora)
        assert bool((nll[feas] > 0).all()) and bool(torch.isfinite(grad).all())


def test_ctc_case_rows_are_what_they_claim():
    want = dict(norepeat=True, exactfit=True, oneshort=False, allequal=True, empty=True, oneframe=True, peaky=True, noframes=False)
    for (T, Lmax, V), _ in R.CTC_SHAPES:
        x, il, tg, tl, feas = R.ctc_case(T, Lmax, V)
        assert x.shape == (len(R.CTC_ROWS), T, V) and int(tg.min()) >= 1 and int(tg.max()) < V
        for name, f in want.items():
            assert bool(feas[R.CTC_ROWS.index(name)]) == f, (T, Lmax, V, name)
        b = R.CTC_ROWS.index("exactfit")
        y = tg[b, :int(tl[b])]
        assert int(tl[b]) == Lmax and R.n_repeats(y) >= (3 if Lmax >= 6 else 1) and int(il[b]) == Lmax + R.n_repeats(y)
        assert torch.equal(tg[b + 1], tg[b]) and int(il[b + 1]) == int(il[b]) - 1
        b = R.CTC_ROWS.index("allequal")
        assert int(il[b]) == 2 * int(tl[b]) - 1 and len(set(tg[b, :int(tl[b])].tolist())) == 1 and int(tl[b]) >= 2
        assert int(tl[R.CTC_ROWS.index("norepeat")]) == Lmax and int(il[R.CTC_ROWS.index("random")]) == T
        b = R.CTC_ROWS.index("noframes")
        assert int(il[b]) == 0 and int(tl[b]) > 0
        b = R.CTC_ROWS.index("empty")
        assert int(il[b]) > 0 and int(tl[b]) == 0
        assert float(x[R.CTC_ROWS.index("peaky")].abs().max()) > 3 * float(x[0].abs().max())


def test_ctc_ref_edge_conventions():
    """what the GPU test relies on aten's double path for: infeasible -> 0 and a zero gradient under zero_infinity, inf without it; empty target -> the closed form
    -sum_t log p(blank); no frames -> 0; gradient rows beyond the length are zero"""
    T, Lmax, V = 60, 12, 40
    x, il, tg, tl, feas = R.ctc_case(T, Lmax, V)
    nll, grad = R.ctc_ref(x, il, tg, tl, True)
    lp = torch.log_softmax(x.double(), -1)
    for b, name in enumerate(R.CTC_ROWS):
        n = int(il[b])
        assert bool((grad[b, n:] == 0).all()), name
        if not feas[b]:
            assert float(nll[b]) == 0 and bool((grad[b] == 0).all()), name
    e = R.CTC_ROWS.index("empty")
    closed = -lp[e, :int(il[e]), 0].sum()
    assert abs(float(nll[e]) - float(closed)) <= 1e-12 * abs(float(closed))
    g_closed = torch.softmax(x[e, :int(il[e])].double(), -1)
    g_closed[:, 0] -= 1
    assert float((grad[e, :int(il[e])] - g_closed).abs().max()) < 1e-12
    o = R.CTC_ROWS.index("oneframe")
    assert abs(float(nll[o]) + float(lp[o, 0, int(tg[o, 0])])) < 1e-12
    nll0, grad0 = R.ctc_ref(x, il, tg, tl, False)
    assert bool(torch.isinf(nll0[~feas]).all()) and torch.equal(nll0[feas], nll[feas])
    assert float((grad0[feas] - grad[feas]).abs().max()) == 0


@pytest.mark.parametrize("T,target", [(1, [2]), (3, []), (4, [1, 1]), (3, [1, 1]), (5, [1, 2, 2]), (7, [3, 3, 1]), (7, [2, 1, 2, 3]), (6, [1, 1, 1]), (2, [1, 2, 3])])
def test_ctc_ref_equals_sum_over_all_paths(T, target):
    """V = 4, T <= 7: every one of the 4^T labellings, collapsed, in fp64 -- loss and gradient"""
    V, Lmax = 4, 4
    x = torch.randn(1, T, V, generator=torch.Generator().manual_seed(T * 10 + len(target))) * 2
    tg = torch.ones(1, Lmax, dtype=torch.int64)
    tg[0, :len(target)] = torch.tensor(target, dtype=torch.int64)
    nll, grad = R.ctc_ref(x, torch.tensor([T]), tg, torch.tensor([len(target)]), True)
    bn, bg = R.ctc_brute(x[0], target)
    assert R.ctc_feasible(T, target) == math.isfinite(bn)
    if math.isfinite(bn):
        assert abs(float(nll[0]) - bn) <= 1e-12 * abs(bn) and float((grad[0] - bg).abs().max()) < 1e-12
    else:
        assert float(nll[0]) == 0 and bool((grad[0] == 0).all())


def test_ctc_route_table():
    for (T, Lmax, V), want in R.CTC_SHAPES:
        k, nw, lds = R.ctc_route(T, Lmax, V)
        assert k + (" w%d" % nw if nw else "") == want, (T, Lmax, V)
    assert R.ctc_route(80, 32, 32)[2] == 65028 and R.ctc_route(80, 32, 40)[2] == 65540            # 4 bytes either side of what needs no opt-in
    assert R.ctc_route(100, 20, 256)[2] > 64 * 1024
    assert R.ctc_route(10, 3, 2100) == ("ctc_lds_kernel", 4, 34508) and 34508 + 12 * 2100 * 4 == 135308 > 128 * 1024
    assert R.ctc_route(140, 130, 40)[2] == 149852 <= 150 * 1024 < (160 * 301 + 160 + 3 * 301) * 4      # what alpha-in-LDS would need at (160, 150)
    assert 2 * 32 + 1 > 64 and 2 * 130 + 1 > 256 and 2 * 150 + 1 == 301
    # the shapes of the older test of tests/test_gpu_parity.py
    assert [R.ctc_route(T, L, 40)[0] for T, L in [(60, 12), (376, 36), (188, 45), (700, 70)]] == ["ctc_lds_kernel", "ctc_alpha_lds_kernel", "ctc_alpha_lds_kernel", "ctc_kernel"]
    assert R.ctc_multi_fits(100, 32, 6) and not R.ctc_multi_fits(376, 32, 36)


def test_row_rel_judges_every_utterance_on_its_own():
    ref = torch.zeros(3, 4, 5, dtype=torch.float64)
    ref[0] += 100.0
    ref[1] += 1e-3
    got = ref.clone()
    got[1, 2, 3] *= 1.01
    r = R.row_rel(got, ref)
    assert r[0] == 0 and abs(float(r[1]) - 0.01) < 1e-9 and r[2] == 0
    from tests.helpers import rel_err
    assert rel_err(got, ref) < 1e-6, "the batch-wide max-norm does not see it"
    got[2, 0, 0] = 1e-30
    assert math.isinf(float(R.row_rel(got, ref)[2])), "a row that must be zero must be exactly zero"
    got[0, 0, 0] = float("nan")
    assert math.isinf(float(R.row_rel(got, ref)[0]))


# ---- softmax cross-entropy ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,V", R.CE_SHAPES)
def test_softmax_ce_ref_equals_torch_on_valid_rows_and_zero_elsewhere(M, V):
    x, _ = R.ce_case(M, V)
    for y in R.ce_case_ys(M, V):
        loss, grad, mean = R.softmax_ce_ref(x, y)
        bad = (y < 0) | (y >= V)
        assert bool((loss[bad] == 0).all()) and bool((grad[bad] == 0).all())
        ok = ~bad
        if bool(ok.any()):
            xd = x[ok].double().requires_grad_(True)
            t = F.cross_entropy(xd, y[ok], reduction="none")
            t.sum().backward()
            assert float((loss[ok] - t.detach()).abs().max()) <= 1e-12 * max(1.0, float(t.detach().abs().max())) and float((grad[ok] - xd.grad).abs().max()) < 1e-12
        assert abs(float(mean) - float(loss.sum()) / M) < 1e-15 * max(1.0, abs(float(mean)))
    ys = torch.cat(R.ce_case_ys(M, V))
    assert {-100, -1, V} <= set(ys.tolist()) and float(x[0].abs().max()) > 30


def test_softmax_ce_ref_mean_counts_ignored_rows():
    x = torch.zeros(4, 8)
    loss, grad, mean = R.softmax_ce_ref(x, torch.tensor([1, -100, 8, 2]))
    assert abs(float(mean) - 2 * math.log(8) / 4) < 1e-15 and float(grad[0, 1]) == 1 / 8 - 1 and float(grad[0, 0]) == 1 / 8


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas,eps,wd,gscale", [((0.9, 0.98), 1e-9, 1e-6, 1.0), ((0.9, 0.999), 1e-8, 0.1, 0.25), ((0.9, 0.999), 1e-8, 0.0, 1.0)])
def test_adam_ref_equals_torch_optim_adam_over_20_steps(betas, eps, wd, gscale):
    """torch.optim.Adam in float64 with the fp32-rounded hyperparameters; the coupled weight decay and the gradient scale are applied to the gradient by hand"""
    n = 64
    p0, _, _, _ = R.adam_inputs(n, 3)
    p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([p], lr=0.0, betas=(R.f32(betas[0]), R.f32(betas[1])), eps=R.f32(eps), weight_decay=0.0)
    rp, rm, rv = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 21):
        g = R.adam_inputs(n, 100 + step)[1]
        lr = R.noam_lr(step)
        opt.param_groups[0]["lr"] = R.f32(lr)
        p.grad = g.double() * R.f32(gscale) + R.f32(wd) * p.detach()
        opt.step()
        rp, rm, rv = R.adam_ref(rp, g, rm, rv, step, lr, betas[0], betas[1], eps, wd, gscale)
        st = opt.state[p]
        assert float((rp - p.detach()).abs().max()) <= 1e-13 * float(p.detach().abs().max()), step
        assert R.scaled_err(rm, st["exp_avg"], R.TINY32) < 1e-12 and R.scaled_err(rv, st["exp_avg_sq"], R.TINY32) < 1e-12, step


def test_adam_ref_rounds_the_hyperparameters_like_the_abi():
    """beta2 = 0.999 is 0.99900001287... in fp32: at step 1 the bias correction 1 - beta2 differs by 1.3e-5 relative, the update by half of that"""
    p, g, m, v = R.adam_inputs(64, 5)
    a = R.adam_ref(p, g, m * 0, v * 0, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0)
    assert R.f32(0.999) != 0.999 and R.f32(0.5) == 0.5
    q = p.shape[0] // 4
    gd = g.double()[3 * q:]
    want_v = (1 - R.f32(0.999)) * gd * gd
    assert float(((a[2][3 * q:] - want_v).abs() / want_v).max()) < 1e-15
    naive_v = (1 - 0.999) * gd * gd
    assert float(((a[2][3 * q:] - naive_v).abs() / naive_v).max()) > 5e-6


def test_adam_inputs_hold_the_promised_magnitudes():
    p, g, m, v = R.adam_inputs(1028, 7)
    q = 257
    assert bool((g[:q] == 0).all()) and bool((v[:q] == 0).all()) and bool((m[1:q:2] == 0).all()) and bool((m[0:q:2] != 0).all())
    a = g[q:2 * q].abs()
    assert 1e-21 < float(a.median()) < 1e-19 and float((a * a).max()) < R.TINY32
    assert 1e3 < float(g[2 * q:3 * q].abs().median()) < 1e5 and bool((v[3 * q:] >= 0).all())


# ---- shadow refresh -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_shadow_ref_equals_explicit_loops(dtype):
    master, entries, n = R.shadow_case()
    table, total = R.shadow_table(entries)
    assert total == sum(R.shadow_blocks(e["A"], e["Tm"], e["C"]) for e in entries) and int(table[-1, 6]) + int(table[-1, 7]) == total
    for i in (5, 6, 8, 10, 11, 12):                         # (7, 3, 5), (6, 1, 4), the middle weight of the fused group, the padded-pitch entry, the two odd-offset entries: small enough for loops
        src, fwd, bwd, A, Tm, C, _, _, Cp, ldb = (int(v) for v in table[i])
        fp, fv, bp, bv = R.shadow_ref(master, table[i], dtype)
        want_f, want_b = {}, {}
        for a in range(A):
            for t in range(Tm):
                for c in range(C):
                    val = master[src + (a * Tm + t) * C + c].to(dtype)
                    want_f[fwd + (a * Tm + t) * C + c] = val
                    want_b[bwd + c * (ldb or Tm * A) + t * A + a] = val
        assert dict(zip(fp.tolist(), fv)) .keys() == want_f.keys() and all(torch.equal(v, want_f[k]) for k, v in zip(fp.tolist(), fv))
        assert dict(zip(bp.tolist(), bv)).keys() == want_b.keys() and all(torch.equal(v, want_b[k]) for k, v in zip(bp.tolist(), bv))


def test_shadow_case_images_are_disjoint_and_cover_the_listed_paths():
    master, entries, n = R.shadow_case()
    table, _ = R.shadow_table(entries)
    seen = torch.zeros(n, dtype=torch.int32)
    for row in table:
        fp, _, bp, _ = R.shadow_ref(master, row, torch.float32)
        for pos in (fp, bp):
            assert pos.numel() == 0 or (int(pos.min()) >= 0 and int(pos.max()) < n)
            seen[pos] += 1
    assert int(seen.max()) == 1, "no two images overlap"
    assert int((seen == 0).sum()) >= 64 * 3 + 5 * len(entries), "pad columns and gaps stay outside every image"
    assert int(seen[-7:].sum()) == 0 and int(seen[:8].sum()) == 0
    shapes = {(e["A"], e["Tm"], e["C"]) for e in entries}
    assert {(64, 1, 64), (130, 1, 72), (10, 1, 24), (64, 1, 245), (96, 9, 32), (7, 3, 5), (6, 1, 4), (8, 1, 12)} <= shapes
    pad = [e for e in entries if e.get("Cp", e["C"]) > e["C"]]
    assert len(pad) == 1 and pad[0]["Cp"] == 248 and pad[0]["bwd"] == -1
    fused = [e for e in entries if e.get("ldb") == 24]
    assert len(fused) == 3 and [e["bwd"] - fused[0]["bwd"] for e in fused] == [0, 8, 16] and all(e["ldb"] == 24 for e in fused)
    vec = lambda e: (((e["C"] | e["src"]) & 3) == 0, ((e["C"] | e["src"] | e["fwd"] | (e.get("Cp", 0) if e.get("Cp", 0) > e["C"] else e["Tm"] * e["C"])) & 3) == 0,
                     e["bwd"] >= 0 and ((e["A"] | e["bwd"] | (e.get("ldb") or e["Tm"] * e["A"])) & 3) == 0)
    paths = {vec(e) for e in entries}
    assert (True, True, True) in paths and (False, False, False) in paths and (True, True, False) in paths and (True, False, True) in paths
    assert len(entries) == 13
    pitch = entries[10]
    assert pitch["ldb"] > pitch["A"] and pitch["A"] % 4 and pitch["ldb"] % 4 == 0 and pitch["bwd"] % 4 == 0, "only A keeps this backward store element-wise"
    odd = entries[-1]
    assert odd["src"] % 2 and odd["fwd"] % 2 and odd["bwd"] % 2 and odd["A"] % 4 == 0 and odd["C"] % 4 == 0
