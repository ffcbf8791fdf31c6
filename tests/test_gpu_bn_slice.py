"""GPU (-m gpu): the slice-streaming BatchNorm passes of avec_amd/csrc/norm.hip (bn_apply8s_kernel, bn_bwd_reduce8s_kernel, bn_bwd_apply8s_kernel) through the six
C entry points that dispatch to them, against the grid-stride kernels behind the same entry points and against fp64.

Both paths are reached in one process with avec_bn_slice_mode (the in-process form of AVEC_BN_SLICE): 0 = grid-stride kernels, 2 = slice kernels at every eligible
size -- the edges of the range guard lie far below the size from which the default dispatch (1) uses the slice kernels.  P (pieces per thread and unit), the grid
and the slice length come from avec_bn_slice_plan, not from constants copied here.  The apply passes cut a tensor into slices of a fixed length (one launch has
as many workgroups as that takes); the reduction (the bit-mask variant: the others have no slice kernel) walks long slices on a grid of at least 256 workgroups.

Shapes (shapes(C)), in 16-byte chunks n8 = M * C / 8, U = 256 * P, grid = the reduction's for a small tensor:
    M = 1            less than one unit; in the reduction 255 of 256 workgroups idle
    M = 37           odd, a ragged first unit
    M = 4099         odd; a ragged last slice, in the reduction slices shorter than one unit and idle workgroups behind the last
    grid * 6 U       whole units and whole slices only, in the reduction the steady-state loop twice in every workgroup
    ... + 37 rows    the same with a ragged last slice (reduction: a ragged unit at the end of every slice)
    grid * U + 3 U + one row      a few units above grid x unit
    grid * (2 U + 200)            reduction: three units per slice, the last ragged (the other exit of the walk)

Apply passes: bit-identical to the grid-stride kernels on random bf16 operands, every variant; dgamma / dbeta grow by exactly dstats once per launch.
Reduce: integer operands, mean 0, scale and rstd powers of two -- every partial sum is an fp32 number, so the sums equal the fp64 reference whatever the order
    (tests/colreduce_ref.py exact_or_die asserts the proviso); random operands within the bound of tests/test_gpu_colreduce.py::test_bn_bwd_reduce
    (R.TOL["bn_bwd_reduce"], per column against the sum of the terms' magnitudes), with the reduction workspace (NaN-filled before every launch) and without.
Bounds: every operand is a view into the middle of a larger buffer; around inputs NaN (mask bytes: 0xFF), around outputs a sentinel that must be unchanged.
"""
import ctypes

import pytest
import torch

from tests import colreduce_ref as R
from tests.test_gpu_colreduce import Ws, check

pytestmark = pytest.mark.gpu

BF16 = 1
PAD = 64                        # elements around every operand (a multiple of 16 bytes in every dtype used)
SENT16, SENT8 = 0x5A5B, 0xA5
CS = [64, 128, 256, 512]


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _lib():
    from avec_amd.lib import lib
    return lib


def stream():
    from avec_amd import runtime as rt
    return rt.stream()


def set_mode(mode):
    fn = _lib().raw("avec_bn_slice_mode")
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int]
    return fn(mode)


@pytest.fixture(autouse=True)
def _restore_mode():
    old = set_mode(-1)
    yield
    set_mode(old)


def plan(pas, M, C):
    """(takes the slice path, P, grid, slice) of pass 0 forward apply / 1 backward reduce / 2 backward apply in the mode in force"""
    fn = _lib().raw("avec_bn_slice_plan")
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint), ctypes.c_void_p]
    P, g, s = ctypes.c_int(0), ctypes.c_uint(0), ctypes.c_uint(0)
    ok = fn(pas, M, C, ctypes.byref(P), ctypes.byref(g), ctypes.byref(s), stream())
    return bool(ok), P.value, g.value, s.value


def shapes(C):
    set_mode(2)
    ps = [plan(p, 1, C) for p in range(3)]
    assert all(ok for ok, _, _, _ in ps), "mode 2 takes the slice path at every bf16 size"
    Us, grid = sorted({256 * P for _, P, _, _ in ps}), max(g for _, _, g, _ in ps)      # the grid of a small tensor (the least the plan gives)
    U, c8 = Us[-1], C // 8
    return [1, 37, 4099, grid * 6 * U // c8, grid * 6 * U // c8 + 37, (grid * U + 3 * U) // c8 + 1] + [grid * (2 * u + 200) // c8 for u in Us]


def test_the_shape_list_meets_every_edge_of_the_walk():
    """what the docstring says of shapes(), re-derived from the plan of the build under test for every pass"""
    for C in CS:
        Ms = shapes(C)
        for pas in range(3):
            seen = set()
            for M in Ms:
                ok, P, grid, sl = plan(pas, M, C)
                n8, U = M * C // 8, 256 * P
                assert ok and sl % 256 == 0 and sl % (C // 8) == 0 and grid * sl >= n8, (pas, M, C, P, grid, sl)
                busy = -(-n8 // sl)
                last = n8 - (busy - 1) * sl
                seen |= {"sub-unit"} if n8 < U else set()
                seen |= {"odd"} if M % 2 else set()
                seen |= {"whole"} if (n8 % U == 0 and last == sl) else set()
                seen |= {"ragged unit"} if (busy > 1 and sl % U) else set()
                seen |= {"ragged slice"} if (busy > 1 and last != sl) else set()
                if pas == 1:        # the reduction walks long slices on a fixed grid
                    assert grid % 256 == 0
                    seen |= {"idle"} if busy < grid else set()
                    seen |= {"steady state twice"} if sl >= 5 * U else set()
                    seen |= {"three units"} if 2 * U < sl < 3 * U else set()
                else:               # the apply passes: slices of fixed length, as many workgroups as it takes
                    assert grid == busy
            want = {"sub-unit", "odd", "whole", "ragged slice"} | ({"ragged unit", "idle", "steady state twice", "three units"} if pas == 1 else set())
            assert seen >= want, (C, pas, sorted(want - seen))
    set_mode(1)
    assert not any(plan(p, 4099, 64)[0] for p in range(3)), "small tensors keep the grid-stride kernels by default"
    assert all(plan(p, 3200 * 22 * 22, 64)[0] and plan(p, 3200 * 3 * 3, 512)[0] for p in range(3)), "the ResNet stages take the slice kernels by default"
    set_mode(0)
    assert not any(plan(p, 3200 * 22 * 22, 64)[0] for p in range(3))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# operands in the middle of larger buffers
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class Mid:
    """a tensor as a view into the middle of a larger buffer: `t` the view, `intact()` whether the surroundings still hold what they were filled with"""

    def __init__(self, n, dtype, fill):
        self.whole = torch.empty(n + 2 * PAD, dtype=dtype, device=dev())
        bits = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[dtype]
        self.bits = self.whole.view(bits)
        if isinstance(fill, float):
            self.whole.fill_(fill)
        else:
            self.bits.fill_(fill)
        self.ref = self.bits.clone()
        self.t = self.whole[PAD:PAD + n]
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return torch.equal(self.bits[:PAD], self.ref[:PAD]) and torch.equal(self.bits[-PAD:], self.ref[-PAD:])


def inp(x):
    """input operand: NaN around it (mask bytes: 0xFF)"""
    x = x.flatten()
    m = Mid(x.numel(), x.dtype, 0xFF if x.dtype == torch.uint8 else float("nan"))
    m.t.copy_(x)
    return m


def outp(n, dtype=torch.bfloat16):
    """output operand: the sentinel around AND inside it (a chunk the launch skips shows as a difference from the other path)"""
    return Mid(n, dtype, SENT8 if dtype == torch.uint8 else SENT16)


def gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def randn(shape, seed, dtype=torch.bfloat16):
    return torch.randn(shape, generator=gen(seed), device=dev()).to(dtype)


def coeffs(C, seed):
    """ss = [scale | shift | mean | rstd], gamma, dstats on random values"""
    ss = torch.randn(4 * C, generator=gen(seed), device=dev())
    ss[3 * C:] = ss[3 * C:].abs() + 0.5
    return ss, torch.randn(C, generator=gen(seed + 1), device=dev()), torch.randn(2 * C, generator=gen(seed + 2), device=dev())


def same_bits(a, b):
    return torch.equal(a.bits, b.bits)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# forward apply
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CS)
def test_apply_fwd_is_bit_identical_to_the_grid_stride_kernel(C):
    lib, st = _lib(), stream()
    for i, M in enumerate(shapes(C)):
        n = M * C
        y, res = inp(randn((M, C), 11 + i)), inp(randn((M, C), 21 + i))
        ss, rss = inp(coeffs(C, 31 + i)[0]), inp(coeffs(C, 41 + i)[0])
        variants = [("plain", act, r, None) for act in (0, 1, 2) for r in (None, res)] + [("mask", 2, r, q) for r, q in ((None, None), (res, None), (res, rss))]
        for entry, act, r, q in variants:
            got = {}
            for mode in (0, 2):
                set_mode(mode)
                out, mask = outp(n), outp(n // 8, torch.uint8)
                if entry == "plain":
                    lib.bn_apply_fwd(BF16, y.ptr(), ss.ptr(), r.ptr() if r else None, act, out.ptr(), M, C, st)
                else:
                    lib.bn_apply_fwd_mask(BF16, y.ptr(), ss.ptr(), r.ptr() if r else None, q.ptr() if q else None, out.ptr(), mask.ptr(), M, C, st)
                torch.cuda.synchronize()
                assert out.intact() and mask.intact(), ("a store outside the operand", entry, act, M, C, mode)
                got[mode] = (out, mask)
            case = (entry, act, r is not None, q is not None, M, C)
            assert same_bits(got[0][0], got[2][0]), ("out differs", case)
            assert same_bits(got[0][1], got[2][1]), ("mask differs", case)
            assert not bool(torch.isnan(got[2][0].t.float()).any()), ("NaN in the output: a read outside an operand", case)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# backward apply
# ---------------------------------------------------------------------------------------------------------------------------------------------------
BWD_SRC = [("none", 0), ("swish", 1), ("relu_pre", 2), ("relu_out", 2), ("mask", 2)]


@pytest.mark.parametrize("C", CS)
def test_bwd_apply_is_bit_identical_and_adds_the_affine_gradients_once(C):
    lib, st = _lib(), stream()
    for i, M in enumerate(shapes(C)):
        n = M * C
        dout, y, o = inp(randn((M, C), 51 + i)), inp(randn((M, C), 61 + i)), inp(randn((M, C), 71 + i))
        mk = inp(torch.randint(0, 256, (n // 8,), generator=gen(81 + i), device=dev(), dtype=torch.uint8))
        ssv, gv, dv = coeffs(C, 91 + i)
        ss, gamma, dstats = inp(ssv), inp(gv), inp(dv)
        for src, act in BWD_SRC:
            for want_dres in (False, True):
                for want_affine in (False, True):
                    got = {}
                    for mode in (0, 2):
                        set_mode(mode)
                        dy, dres = outp(n), outp(n)
                        dg, db = Mid(C, torch.float32, 0x7FC00001), Mid(C, torch.float32, 0x7FC00001)
                        dg.t.copy_(torch.arange(C, device=dev()) % 5 - 2.0)
                        db.t.copy_(torch.arange(C, device=dev()) % 3 - 1.0)
                        g0, b0 = dg.t.clone(), db.t.clone()
                        tail = (None, float(M), dy.ptr(), dres.ptr() if want_dres else None, dg.ptr() if want_affine else None, db.ptr() if want_affine else None, M, C, st)
                        if src == "mask":
                            lib.bn_bwd_apply_mask(BF16, dout.ptr(), y.ptr(), mk.ptr(), ss.ptr(), gamma.ptr(), dstats.ptr(), *tail)
                        else:
                            lib.bn_bwd_apply(BF16, dout.ptr(), y.ptr(), o.ptr() if src == "relu_out" else None, ss.ptr(), gamma.ptr(), dstats.ptr(), tail[0], tail[1], act, *tail[2:])
                        torch.cuda.synchronize()
                        case = (src, want_dres, want_affine, M, C, mode)
                        assert dy.intact() and dres.intact() and dg.intact() and db.intact(), ("a store outside the operand", case)
                        if want_affine:     # one fp32 addition per channel: the same rounding here and there
                            assert torch.equal(dg.t, g0 + dstats.t[C:]) and torch.equal(db.t, b0 + dstats.t[:C]), ("dgamma / dbeta did not grow by dstats exactly once", case)
                        else:
                            assert torch.equal(dg.t, g0) and torch.equal(db.t, b0), case
                        if not want_dres:
                            assert bool((dres.bits == SENT16).all()), ("dres written without being asked for", case)
                        got[mode] = (dy, dres)
                    case = (src, want_dres, want_affine, M, C)
                    assert same_bits(got[0][0], got[2][0]), ("dy differs", case)
                    assert same_bits(got[0][1], got[2][1]), ("dres differs", case)
                    assert not bool(torch.isnan(got[2][0].t.float()).any()), ("NaN in dy: a read outside an operand", case)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# backward reduce
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def exact_ss(C):
    """scale a power of two (the sign of scale * y + shift is the same in fp32 and fp64), mean 0, rstd a power of two"""
    c = torch.arange(C, dtype=torch.float64)
    sc = torch.tensor([0.5, 1.0, 2.0, -1.0], dtype=torch.float64)[(c % 4).long()]
    return torch.stack([sc, -0.75 * sc.sign(), torch.zeros(C, dtype=torch.float64), torch.tensor([0.5, 2.0, 1.0], dtype=torch.float64)[(c % 3).long()]])


def ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=gen(seed), device=dev()).double()


def run_reduce(ws, variant, act, dout, y, o, mk, ss, M, C):
    lib = _lib()
    dstats = Mid(2 * C, torch.float32, 0x7FC00001)
    dstats.t.fill_(-2.0)
    if variant == "mask":
        ws.run(lambda: lib.bn_bwd_reduce_mask(BF16, dout.ptr(), y.ptr(), mk.ptr(), ss.ptr(), dstats.ptr(), M, C, ws.stream))
    else:
        ws.run(lambda: lib.bn_bwd_reduce(BF16, dout.ptr(), y.ptr(), o.ptr() if variant == "relu_out" else None, ss.ptr(), act, dstats.ptr(), M, C, ws.stream))
    assert dstats.intact(), ("a store outside dstats", variant, M, C)
    assert not bool(torch.isnan(dstats.t).any()), ("NaN in the sums: a read outside an operand or a workspace slot nobody wrote", variant, M, C, ws.setup)
    return dstats.t


@pytest.mark.parametrize("setup", ["twopass", "atomics"])
@pytest.mark.parametrize("C", CS)
def test_bwd_reduce_of_integer_operands_equals_fp64(C, setup):
    set_mode(2)
    with Ws(setup) as ws:
        for i, M in enumerate(shapes(C)):
            d64, y64, o64 = ints((M, C), -3, 3, 101 + i), ints((M, C), 0, 3, 111 + i), ints((M, C), -1, 1, 121 + i)
            m64 = torch.randn((M, C), generator=gen(131 + i), device=dev()) > 0
            dout, y, o, mk = inp(d64.bfloat16()), inp(y64.bfloat16()), inp(o64.bfloat16()), inp(R.pack_mask(m64.cpu()).to(dev()))
            ss64 = exact_ss(C).to(dev())
            ss = inp(ss64.float())
            for variant, act in (("mask", 2),):                  # the variant with a slice kernel; the others stay on bn_bwd_reduce8_kernel (tests/test_gpu_colreduce.py)
                got = run_reduce(ws, variant, act, dout, y, o, mk, ss, M, C)
                ref = R.bn_bwd_reduce_ref(d64, y64, ss64, act, o64 if variant == "relu_out" else None, m64 if variant == "mask" else None)
                check("bn_bwd_reduce/" + variant, (M, C, "bf16", setup), "exact", got, (ref[0].cpu(), ref[1].cpu()), -2.0, 0.5)


@pytest.mark.parametrize("setup", ["twopass", "atomics"])
@pytest.mark.parametrize("C", CS)
def test_bwd_reduce_of_random_operands_stays_within_the_column_reduction_bound(C, setup):
    set_mode(2)
    with Ws(setup) as ws:
        for i, M in enumerate(shapes(C)):
            dout, y = inp(randn((M, C), 141 + i)), inp(randn((M, C), 151 + i))
            m64 = torch.randn((M, C), generator=gen(161 + i), device=dev()) > 0
            mk = inp(R.pack_mask(m64.cpu()).to(dev()))
            g = torch.randn((4, C), generator=gen(171 + i), device=dev(), dtype=torch.float64)
            c = torch.arange(C, device=dev())
            ss64 = torch.stack([torch.tensor([0.5, 1.0, 2.0, -1.0], dtype=torch.float64, device=dev())[c % 4], 0.3 * g[1], 0.2 * g[2], 0.5 + g[3].abs()]).float().double()
            ss = inp(ss64.float())
            d64, y64 = dout.t.double().view(M, C), y.t.double().view(M, C)
            for variant, act in (("mask", 2),):
                got = run_reduce(ws, variant, act, dout, y, None, mk, ss, M, C)
                ref = R.bn_bwd_reduce_ref(d64, y64, ss64, act, None, m64 if variant == "mask" else None)
                check("bn_bwd_reduce/" + variant, (M, C, "bf16", setup), "gauss", got, (ref[0].cpu(), ref[1].cpu()), -2.0)
