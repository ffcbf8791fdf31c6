"""No GPU: the host references of tests/grad_clip_ref.py against torch.nn.utils.clip_grad_norm_ and torch.optim.Adam in fp64, the C ABI of the gradient-norm and
clipped-Adam entry points (declared, exported, argument errors reported before any launch) and main.py's graph flags."""
import ctypes
import math
import os
import sys

import pytest
import torch

from avec_amd import lib as L
from avec_amd.lib import lib
from tests import grad_clip_ref as C
from tests import loss_optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("avec_grad_norm", "avec_grad_norm_workspace_bytes", "avec_grad_norm_blocks", "avec_adam_step_clipped")


@pytest.mark.parametrize("n", [4, 1028, 70000])
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
def test_norm_and_coef_reference_equal_clip_grad_norm_in_fp64(n, grad_scale):
    """clip_grad_norm_ on fp64 tensors holding g * grad_scale, split into three parameters: its return value is the norm, the factor it applied is the coef.  Both
    sides are fp64 evaluations of the same formula in another order of operations: 1e-12 relative."""
    g = R.adam_inputs(n, 60 + n)[1].double()
    norm = C.norm_ref(g, grad_scale)
    cuts = [0, n // 3, n // 2, n]
    for max_norm in (0.5 * norm, norm, 2.0 * norm, 1e-3):
        ps = [torch.nn.Parameter(torch.zeros(b - a, dtype=torch.float64)) for a, b in zip(cuts, cuts[1:]) if b > a]
        o = 0
        for p in ps:
            p.grad = g[o:o + p.numel()].clone() * R.f32(grad_scale)
            o += p.numel()
        total = float(torch.nn.utils.clip_grad_norm_(ps, R.f32(max_norm)))
        assert abs(total - norm) <= 1e-12 * norm, (total, norm)
        coef = C.coef_ref(norm, max_norm)
        got = torch.cat([p.grad for p in ps])
        want = g * R.f32(grad_scale) * coef
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (max_norm, coef)
        assert (coef < 1.0) == (R.f32(max_norm) < norm + C.EPS_CLIP)
    for max_norm in (0.0, -1.0, math.inf):
        assert C.coef_ref(norm, max_norm) == 1.0
    assert C.coef_ref(math.nan, 1.0) == 1.0 and C.coef_ref(math.inf, 1.0) == 1.0


@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adam_ref_at_the_effective_scale_equals_clip_then_adam_in_fp64(wd):
    """adam_ref with gscale := fp32(gscale * coef) against "scale, clip_grad_norm_, torch.optim.Adam" in fp64.  The two differ by the fp32 roundings of coef and of
    the product (2 x 2^-24 relative on the gradient term): every result is judged in units of the terms it is summed from (adam_scales), bound 4 roundings."""
    n, step, lr, b1, b2, eps, gs = 1028, 7, 1e-3, 0.9, 0.98, 1e-9, 0.25
    p0, g0, m0, v0 = R.adam_inputs(n, 71)
    norm = C.norm_ref(g0, gs)
    max_norm = 0.3 * norm
    coef32 = C.coef_f32(R.f32(norm), max_norm)
    geff = C.gscale_eff(gs, coef32)
    ref = R.adam_ref(p0, g0, m0, v0, step, lr, b1, b2, eps, wd, geff)
    p = torch.nn.Parameter(p0.double().clone())
    p.grad = g0.double() * R.f32(gs)
    torch.nn.utils.clip_grad_norm_([p], R.f32(max_norm))
    opt = torch.optim.Adam([p], lr=R.f32(lr), betas=(R.f32(b1), R.f32(b2)), eps=R.f32(eps), weight_decay=R.f32(wd))
    opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.double().clone(), "exp_avg_sq": v0.double().clone()}
    opt.step()
    su, sm, sv = R.adam_scales(p0, g0, m0, v0, step, lr, b1, b2, eps, wd, geff)
    st = opt.state[p]
    for name, got, want, s in (("update", p.detach() - p0.double(), ref[0] - p0.double(), su), ("m", st["exp_avg"], ref[1], sm), ("v", st["exp_avg_sq"], ref[2], sv)):
        e = float(((got - want).abs() / s).max())
        assert e <= 4 * R.EPS32, (name, e)


def test_header_declares_and_library_exports_the_new_entry_points():
    decl = L.declared_functions()
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in decl, name + " is not declared in include/avec_hip.h"
        assert hasattr(dll, name), name + " is not exported by libavec_hip.so"
    assert len(decl["avec_grad_norm"][1]) == 11 and len(decl["avec_adam_step_clipped"][1]) == 15
    assert len(decl["avec_adam_step_guarded"][1]) == 14 and len(decl["avec_adam_step"][1]) == 13, "the existing Adam entry points keep their signatures"
    assert lib.load().avec_version() == 4


def test_grid_and_workspace_size_functions():
    blocks, ws = lib.raw("avec_grad_norm_blocks"), lib.raw("avec_grad_norm_workspace_bytes")
    cap = blocks(1 << 40)
    assert 1 <= cap <= 65535 and blocks(4) == 1 and blocks(1024) == 1 and blocks(1028) == 2
    n_pass = 4 * 256 * cap                                     # one 16-byte load per lane of a full grid
    assert blocks(n_pass) == cap and blocks(n_pass - 1024) == cap - 1 and blocks(n_pass + 1200) == cap
    assert ws(4) == 8 and ws(n_pass) == 8 * cap and ws(1 << 40) == 8 * cap
    assert blocks(0) == 0 and blocks(-4) == 0


def test_argument_errors_come_back_before_any_launch():
    """made-up (aligned, non-NULL) addresses and no GPU in the process: a call that got as far as a launch would fail with a HIP error code, not with -1 and these
    messages"""
    g, ws, stats, flag = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    need = lib.raw("avec_grad_norm_workspace_bytes")(4096)
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*multiple of 4"):
        lib.grad_norm(g, 4094, 1.0, 1.0, 0, None, ws, need, stats, flag, None)
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*multiple of 4"):
        lib.grad_norm(g, 0, 1.0, 1.0, 0, None, ws, need, stats, flag, None)
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*stats"):
        lib.grad_norm(g, 4096, 1.0, 1.0, 0, None, ws, need, None, flag, None)
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*workspace"):
        lib.grad_norm(g, 4096, 1.0, 1.0, 0, None, ws, need - 8, stats, flag, None)
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*workspace"):
        lib.grad_norm(g, 4096, 1.0, 1.0, 0, None, None, need, stats, flag, None)
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*multiple of 4"):
        lib.adam_step_clipped(g, g, g, g, stats, 0.9, 0.98, 1e-9, 0.0, 1.0, 1, 6, None, stats, None)


def test_main_accepts_the_graph_flags():
    sys.path.insert(0, ROOT)
    try:
        import main
    finally:
        sys.path.remove(ROOT)
    a = main.build_parser().parse_args(["--use_graphs", "--graph_bucket_frames", "25"])
    assert a.use_graphs is True and a.graph_bucket_frames == 25 and a.graph_cache_size is None
    a = main.build_parser().parse_args(["--graph_cache_size", "3"])
    assert a.use_graphs is False and a.graph_bucket_frames is None and a.graph_cache_size == 3
    d = main.build_parser().parse_args([])
    assert d.mode == "training" and d.step_log_period == 100 and not d.no_eval_training, "no existing flag changed"
