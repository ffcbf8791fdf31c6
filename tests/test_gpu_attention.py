"""GPU (-m gpu): the relative-position attention kernels of avec_amd/csrc/attention.hip (fp32 / bf16 VALU) and attention_mfma.hip (bf16 MFMA), called through the
C ABI (avec_relpos_attention_fwd / _bwd), element by element against the fp64 reference of tests/attention_ref.py (pinned on the host by tests/test_attention_ref.py).

Harness (that of tests/test_gpu_rowwise.py).  Inputs AND outputs are carved out of one device allocation pre-filled with the bit pattern 0x7FC0 (a NaN as bf16 and as
fp32) with gaps of at least 256 bytes: the bytes straight after the last row of every input are NaN, so a read past the end of a tensor poisons the result; after
every launch the gaps must be intact, every element the kernels owe must no longer be NaN, and everything else inside the output regions -- row-stride gaps, ldt / ldr
padding columns -- must still hold the pattern.  dsrel is pre-filled with zeros (its contract) and its out-of-band elements must come back as exact zeros; de is
pre-filled with known values and judged as an accumulation; with dsrel or Tk != T, dk / dv / de must be untouched.  The strided cases keep q | k | v fused in rows of
3 D + 8 elements, as the model does, with finite garbage in every row gap of every input, and run twice with different garbage: the outputs must be bit-identical
(dE, summed by atomics over the batch, only when B = 1).  NaN in row gaps is NOT tolerated by the MFMA kernels -- a precondition stated in csrc/attention.h.

Judgement, per element:  |got - ref| <= TOL[model][family] * scale (+ half a bf16 ulp for a bf16 output, + 2^-126), TOL = 8 x the worst ratio of the host model of
the kernel's rounding points over the same case table (attention_ref.HOST_WORST); the model is chosen by the kernel that ran.  m + log l is judged on rows with a
kept key; a row without one must have m == -1e9 and l == Tk exactly.

Every case asserts the kernel instance it was written for (avec_last_kernel() against attention_ref.route).  Instance -> case, bf16 (in f32 every case runs
attn_rows<f32,fwd> and attn_rows<f32,bwd>); attn_mfma_fwd and attn_mfma_bwd take the same template arguments <PITCH,NTM,ALIAS,DKS> except in the mixed band:
    <128,7,0,0>   T2_d8, T31_d16, T32_d17, T33_lens0             <128,7,0,3>   T33_d45, T33_d45_div3, T63_d46, T64_d48, strided_T65_d45
    <128,7,0,4>   T65_d64, T33_qfull, T224_d64                   <128,12,0,0>  T320_d16        <128,12,0,3>  T225_d45        <128,12,0,4>  T225_d64
    <128,12,1,0>  T384_d8       <128,12,1,3>  T384_d48           <128,12,1,4>  T321_d64
    <256,7,0,0>   T97_d65       <256,7,0,6>   T64_d96, T128_d90, strided_T33_d90_dsrel        <256,12,1,0>  T129_d65        <256,12,1,6>  T129_d90, T192_d90
    attn_mfma_fwd<256,12,1,6> with attn_rows<bf16,bwd>   T193_d90 (+cols<96>), T224_d90 (dsrel): the MFMA forward's (m, l) and O read by the VALU backward
    attn_rows<bf16,fwd> and <bf16,bwd>   T385_d64, T225_d90, strided_T225_d90, T33_d97, every mask_* and Tk_* case, and T1_d1 / T65_d1 (rows shorter than a head's padding)
    +cols<48>  T64_d48, T33_d45   +cols<64>  T65_d64, T385_d64   +cols<96>  T97_d65, T225_d90, T193_d90     (each in f32 and in bf16)
    rejected before any launch: T33_d97_reject (column pass, d > 96); T33_d150 backward and T31_d192 both ways (the VALU row kernels' LDS request passes 160 KB)
<256,12,0,*> is instantiated but cannot be selected (tests/test_attention_ref.py::test_lds_bounds_and_instance_coverage).

    family       valu_f32: host worst / tolerance / MI355X     valu_bf16: host worst / tolerance / MI355X     mfma_bf16: host worst / tolerance / MI355X
    O           1.90e-06 / 1.52e-05 / 2.45e-06         2.27e-07 / 1.82e-06 / 3.41e-07         2.38e-03 / 1.90e-02 / 2.38e-03
    m + log l   3.05e-07 / 2.44e-06 / 2.55e-07         8.78e-08 / 7.02e-07 / 1.19e-07         1.03e-07 / 8.24e-07 / 1.21e-07
    P           1.00e-05 / 8.00e-05 / 8.56e-06         2.03e-06 / 1.62e-05 / 1.44e-06         1.37e-06 / 1.10e-05 / 1.04e-06
    dS          2.47e-06 / 1.98e-05 / 2.24e-06         2.77e-03 / 2.22e-02 / 2.77e-03         9.02e-04 / 7.22e-03 / 9.02e-04
    dSrel       2.47e-06 / 1.98e-05 / 1.88e-06         2.77e-03 / 2.22e-02 / 2.32e-04         9.02e-04 / 7.22e-03 / 9.02e-04
    dQ          2.62e-07 / 2.10e-06 / 2.56e-07         1.54e-03 / 1.23e-02 / 1.54e-03         6.11e-04 / 4.89e-03 / 6.11e-04
    dK          4.04e-07 / 3.23e-06 / 2.49e-07         1.79e-03 / 1.43e-02 / 1.23e-03         6.41e-04 / 5.13e-03 / 6.41e-04
    dV          2.73e-06 / 2.18e-05 / 1.51e-06         3.64e-03 / 2.91e-02 / 3.15e-03         2.51e-03 / 2.01e-02 / 2.25e-03
    dE          3.87e-07 / 3.10e-06 / 2.50e-07         1.52e-03 / 1.22e-02 / 1.52e-03         9.75e-04 / 7.80e-03 / 9.75e-04
(MI355X worst ratios measured in this work, for the record only; no tolerance is derived from them.)
"""
import functools

import numpy as np
import pytest
import torch

from tests import attention_ref as A
from tests.test_gpu_rowwise import Carve, TD, launch, stream, _lib

pytestmark = pytest.mark.gpu

DT = A.RW.DT
NAMES = [c["name"] for c in A.CASES]


def last_kernel():
    return _lib().raw("avec_last_kernel")().decode()


@functools.lru_cache(maxsize=4)
def reference(name, dtype):
    """(inputs, fp64 reference) of a case: computed once and shared, never modified"""
    inp = A.make_inputs(A.CASE[name], dtype)
    return inp, A.evaluate(inp)


def strided(t, nrows, width, ld, col0=0):
    """[nrows][width] window of the flat tensor t with row stride ld, from element col0"""
    return torch.as_strided(t, (nrows, width), (ld, 1), t.storage_offset() + col0)


class Layout:
    """where every operand of a case lives inside one Carve: region index, row stride; q | k | v fused in one region when strided"""

    def __init__(self, case, dtype):
        B, H, T, d, Tk = (case[n] for n in ("B", "H", "T", "d", "Tk"))
        D, R, sd = H * d, Tk + T - 1, case["strided"]
        self.case, self.dtype, self.D, self.R = case, dtype, D, R
        self.fused = sd
        self.ld = 3 * D + 8 if sd else D
        self.ldo, self.lde, self.ldde = (D + 8, D + 16, D + 4) if sd else (D, D, D)
        self.lddq = self.ldd = self.ld
        self.ldt, self.ldr = (Tk + 3, R + 5) if sd else ((Tk + 7) // 8 * 8, (R + 7) // 8 * 8)      # unstrided: the model's own padding to a multiple of 8
        n = lambda rows, ld, w: (rows - 1) * ld + w                                            # a region ends with the last row: what follows is the sentinel
        Bm = case["mask"][1] if case["mask"] else 0
        specs = {"e": (n(R, self.lde, D), dtype), "dO": (n(B * T, self.ldo, D), dtype), "o": (n(B * T, self.ldo, D), dtype), "lse": (B * H * T * 2, "f32"),
                 "de": (n(R, self.ldde, D), "f32"), "pbuf": (n(B * H * T, self.ldt, Tk), dtype), "dsbuf": (n(B * H * T, self.ldt, Tk), dtype),
                 "dsrel": (n(H * B * T, self.ldr, R), dtype), "mask": (max(Bm, 1) * T * Tk, "f32"), "tail": (4096, "u8")}
        if self.fused:
            specs.update(qkv=(n(B * T, self.ld, 3 * D), dtype), dqkv=(n(B * T, self.ld, 3 * D), dtype))
        else:
            specs.update(q=(n(B * T, D, D), dtype), k=(n(B * Tk, D, D), dtype), v=(n(B * Tk, D, D), dtype), dq=(n(B * T, D, D), dtype), dk=(n(B * Tk, D, D), dtype),
                         dv=(n(B * Tk, D, D), dtype))
        self.names = [k for k in specs if k != "tail"] + ["tail"]
        self.c = Carve([specs[k] for k in self.names])

    def view(self, name):
        return self.c.views[self.names.index(name)]

    def pat(self, name):
        a, nb, dt = self.c.spans[self.names.index(name)]
        return self.c.pat[a:a + nb].view(TD[dt])

    def rows(self, name, nrows, width, ld, col0=0):
        return strided(self.view(name), nrows, width, ld, col0)

    def put(self, name, x2d, ld, col0=0, garbage=None):
        v = self.view(name)
        if garbage is not None and col0 == 0:
            g = torch.Generator().manual_seed(garbage)
            v.copy_((3 * torch.randn(v.numel(), generator=g)).to(v.dtype))
        self.rows(name, x2d.shape[0], x2d.shape[1], ld, col0).copy_(x2d.to(v.dtype))

    def only_owed_written(self, name, nrows, width, ld, col0=0):
        """everything of the region but the owed elements still holds the sentinel"""
        chk = self.view(name).clone()
        strided(chk, nrows, width, ld, col0).copy_(strided(self.pat(name), nrows, width, ld, col0))
        bits = torch.int16 if chk.element_size() == 2 else torch.int32
        return torch.equal(chk.view(bits), self.pat(name).view(bits))

    def untouched(self, name):
        bits = torch.int16 if self.view(name).element_size() == 2 else torch.int32
        return torch.equal(self.view(name).view(bits), self.pat(name).view(bits))


def run_case(case, dtype, garbage=None):
    """forward and backward launch of one case -> {name: host tensor in the reference's layout}, the kernel names, the raw owed bits (for the bit-identity check)"""
    from avec_amd.lib import Attn
    import ctypes
    lib, st = _lib(), stream()
    inp, _ = reference(case["name"], dtype)
    B, H, T, d, Tk = (case[n] for n in ("B", "H", "T", "d", "Tk"))
    L = Layout(case, dtype)
    D, R = L.D, L.R
    esz = 2 if dtype == "bf16" else 4
    gb = (lambda k: None) if garbage is None else (lambda k: garbage * 1000 + k)
    if L.fused:
        L.put("qkv", inp["q"].reshape(B * T, D), L.ld, 0, gb(1)); L.put("qkv", inp["k"].reshape(B * T, D), L.ld, D); L.put("qkv", inp["v"].reshape(B * T, D), L.ld, 2 * D)
        qp = L.view("qkv").data_ptr(); kp, vp = qp + D * esz, qp + 2 * D * esz
        dqp = L.view("dqkv").data_ptr(); dkp, dvp = dqp + D * esz, dqp + 2 * D * esz
    else:
        L.put("q", inp["q"].reshape(B * T, D), D); L.put("k", inp["k"].reshape(B * Tk, D), D); L.put("v", inp["v"].reshape(B * Tk, D), D)
        qp, kp, vp = (L.view(n).data_ptr() for n in ("q", "k", "v"))
        dqp, dkp, dvp = (L.view(n).data_ptr() for n in ("dq", "dk", "dv"))
    L.put("e", inp["e"].reshape(R, D), L.lde, 0, gb(2))
    L.put("dO", inp["dO"].reshape(B * T, D), L.ldo, 0, gb(3))
    L.rows("de", R, D, L.ldde).copy_(inp["de0"].reshape(R, D).float())
    L.rows("dsrel", H * B * T, R, L.ldr).zero_()
    de_before = L.view("de").clone()
    lens = None if case["lens"] is None else torch.tensor(case["lens"], dtype=torch.int64, device="cuda")
    a = Attn()
    a.q, a.k, a.v, a.ld, a.e, a.lde = qp, kp, vp, L.ld, L.view("e").data_ptr(), L.lde
    a.lens, a.len_div, a.q_full = (None if lens is None else lens.data_ptr()), case["len_div"], case["q_full"]
    if case["mask"]:
        L.view("mask").copy_(inp["mask"].reshape(-1).float())
        a.mask, a.mask_bstride = L.view("mask").data_ptr(), (T * Tk if case["mask"][1] > 1 else 0)
    a.o, a.ldo, a.lse = L.view("o").data_ptr(), L.ldo, L.view("lse").data_ptr()
    a.B, a.H, a.T, a.d, a.scale, a.Tk = B, H, T, d, inp["scale"], (Tk if Tk != T else 0)
    want_f, want_b = A.case_route(case, dtype)
    out, names = {}, {}
    raw_fwd, raw_bwd = lib.raw("avec_relpos_attention_fwd"), lib.raw("avec_relpos_attention_bwd")
    rc = []
    launch(L.c, lambda: rc.append(raw_fwd(DT[dtype], ctypes.byref(a), st)))
    if want_f is None:
        assert rc[0] != 0 and "LDS" in lib.raw("avec_last_error")().decode(), (rc, lib.raw("avec_last_error")().decode())
        assert L.untouched("o") and L.untouched("lse"), "a rejected forward wrote to its outputs"
        return None, (None, None), None
    assert rc[0] == 0, lib.raw("avec_last_error")().decode()
    names["fwd"] = last_kernel()
    assert L.only_owed_written("o", B * T, D, L.ldo), "o: written outside the owed elements"
    out["O"] = L.rows("o", B * T, D, L.ldo).cpu().view(B, T, H, d)
    lse = L.view("lse").cpu().view(B, H, T, 2)
    out["m"], out["l"] = lse[..., 0], lse[..., 1]
    raw = {"o": L.rows("o", B * T, D, L.ldo).clone(), "lse": L.view("lse").clone()}
    # ---- backward ----
    a.dout, a.dq, a.dk, a.dv, a.lddq, a.ldd = L.view("dO").data_ptr(), dqp, dkp, dvp, L.lddq, L.ldd
    a.de, a.ldde = L.view("de").data_ptr(), L.ldde
    a.pbuf, a.dsbuf, a.ldt = L.view("pbuf").data_ptr(), L.view("dsbuf").data_ptr(), L.ldt
    if case["dsrel"]:
        a.dsrel, a.ldr = L.view("dsrel").data_ptr(), L.ldr
    dsrel_before = L.view("dsrel").clone()
    rc = []
    launch(L.c, lambda: rc.append(raw_bwd(DT[dtype], ctypes.byref(a), st)))
    gname = "dqkv" if L.fused else None
    if want_b is None:
        msg = lib.raw("avec_last_error")().decode()
        assert rc[0] != 0 and ("column pass" in msg or "LDS" in msg), (rc, msg)
        for n in ([gname] if gname else ["dq", "dk", "dv"]) + ["pbuf", "dsbuf"]:
            assert L.untouched(n), (n, "a rejected backward wrote to its outputs")
        assert torch.equal(L.view("de").view(torch.int32), de_before.view(torch.int32)) and torch.equal(L.view("dsrel").view(torch.int16 if esz == 2 else torch.int32), dsrel_before.view(torch.int16 if esz == 2 else torch.int32))
        return out, (names["fwd"], None), raw
    assert rc[0] == 0, lib.raw("avec_last_error")().decode()
    names["bwd"] = last_kernel()
    cols = not case["dsrel"] and Tk == T
    for n in ("pbuf", "dsbuf"):
        assert L.only_owed_written(n, B * H * T, Tk, L.ldt), (n, "written outside the owed elements (ldt padding columns)")
    out["P"], out["dS"] = (L.rows(n, B * H * T, Tk, L.ldt).cpu().view(B, H, T, Tk) for n in ("pbuf", "dsbuf"))
    raw.update(P=L.rows("pbuf", B * H * T, Tk, L.ldt).clone(), dS=L.rows("dsbuf", B * H * T, Tk, L.ldt).clone())
    dq = L.rows("dqkv", B * T, D, L.ld) if L.fused else L.rows("dq", B * T, D, D)
    out["dQ"] = dq.cpu().view(B, T, H, d)
    raw["dQ"] = dq.clone()
    assert L.only_owed_written("dsrel", H * B * T, R, L.ldr), "dsrel: written into the ldr padding columns"
    bits = torch.int16 if esz == 2 else torch.int32
    if case["dsrel"]:
        rel = L.rows("dsrel", H * B * T, R, L.ldr)
        out["dSrel"] = rel.cpu().view(H, B, T, R).permute(1, 0, 2, 3)
        raw["dSrel"] = rel.clone()
    else:
        assert torch.equal(L.view("dsrel").view(bits), dsrel_before.view(bits)), "dsrel written although not given"
    if cols:
        if L.fused:
            assert L.only_owed_written("dqkv", B * T, 3 * D, L.ld), "dq | dk | dv: written into the row gaps"
            dk, dv = L.rows("dqkv", B * T, D, L.ld, D), L.rows("dqkv", B * T, D, L.ld, 2 * D)
        else:
            dk, dv = L.rows("dk", B * T, D, D), L.rows("dv", B * T, D, D)
        assert L.only_owed_written("de", R, D, L.ldde), "de: written into the row gaps"
        out["dK"], out["dV"], out["dE"] = dk.cpu().view(B, T, H, d), dv.cpu().view(B, T, H, d), L.rows("de", R, D, L.ldde).cpu().view(R, H, d)
        raw.update(dK=dk.clone(), dV=dv.clone())
        if B == 1:
            raw["dE"] = L.rows("de", R, D, L.ldde).clone()
    else:                                                                  # dk / dv / de belong to the caller's batched GEMMs
        assert torch.equal(L.view("de").view(torch.int32), de_before.view(torch.int32)), "de touched although the column pass does not run"
        if L.fused:
            assert L.only_owed_written("dqkv", B * T, D, L.ld), "dk / dv touched although the column pass does not run"
        else:
            assert L.untouched("dk") and L.untouched("dv"), "dk / dv touched although the column pass does not run"
            assert L.only_owed_written("dq", B * T, D, D)
    return out, (names["fwd"], names["bwd"]), raw


def judge(case, dtype, out, bwd_ran):
    """every family per element; prints one line per family (the record of the docstring table is read from these) and collects the misses"""
    _, ref = reference(case["name"], dtype)
    fm, bm = A.models_of(case, dtype)
    B, H, T, d, Tk = (case[n] for n in ("B", "H", "T", "d", "Tk"))
    fails = []
    for k, v in out.items():
        assert not bool(torch.isnan(v.float()).any()), (k, "an element the kernels owe is still NaN")
    live = ~ref["full_masked"]
    dead = ~live
    if bool(dead.any()):
        if not (bool((out["m"][dead] == A.NEG).all()) and bool((out["l"][dead] == Tk).all())):
            fails.append(("lse", "a row without a kept key must have m == -1e9 and l == Tk", out["m"][dead][:4].tolist(), out["l"][dead][:4].tolist()))
    fams = [("lse", fm, (out["m"].double() + out["l"].double().log())[live], ref["lse"][0][live], ref["lse"][1][live], "f32"), ("O", fm, out["O"], *ref["O"], dtype)]
    if bwd_ran:
        fams += [(f, bm, out[f], *ref[f], "f32" if f == "dE" else dtype) for f in ("P", "dS", "dSrel", "dQ", "dK", "dV", "dE") if f in out]
        for f in ("P", "dSrel"):                                            # zeros owed exactly: masked keys, out-of-band elements
            if f in out and not bool((out[f][ref[f][1] == 0] == 0).all()):
                fails.append((f, "an element owed as exact zero is not zero"))
    for fam, mdl, got, want, scale, odt in fams:
        if got.numel() == 0:
            continue
        r = A.RW.ratio(got, want, scale, odt)
        w, tol = float(r.max()), A.TOL[mdl][fam]
        print("ATTN_RATIO %-10s %-6s %.3g  tol %.3g  %s %s" % (mdl, fam, w, tol, case["name"], dtype))
        if not w <= tol:
            i = int(r.argmax())
            idx = [int(x) for x in np.unravel_index(i, tuple(got.shape))]
            fails.append((fam, mdl, "ratio %.3g > %.3g at %s of %s: got %r ref %r scale %r" % (w, tol, idx, list(got.shape), float(got.reshape(-1)[i]), float(want.reshape(-1)[i]),
                                                                                        float(scale.reshape(-1)[i]))))
    return fails


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_attention_case(name, dtype):
    """one case of attention_ref.CASES: kernel path, harness contracts, and every output family per element against fp64"""
    case = A.CASE[name]
    want = A.case_route(case, dtype)
    out, got_names, raw = run_case(case, dtype, garbage=1 if case["strided"] else None)
    assert got_names == want, ("kernel path", got_names, want)
    if out is None:
        return
    fails = judge(case, dtype, out, want[1] is not None)
    if case["strided"]:                                                    # other garbage in the row gaps of the inputs: the same bits
        out2, names2, raw2 = run_case(case, dtype, garbage=2)
        assert names2 == want
        for k in raw:
            if not torch.equal(raw[k].view(torch.int16 if raw[k].element_size() == 2 else torch.int32), raw2[k].view(torch.int16 if raw2[k].element_size() == 2 else torch.int32)):
                fails.append((k, "depends on the bytes in the row gaps of the inputs"))
    for f in fails:
        print("FAIL", name, dtype, f)
    assert not fails, fails[:6]
