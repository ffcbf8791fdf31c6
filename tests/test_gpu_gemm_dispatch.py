"""GPU (-m gpu): the host dispatch of the product family (csrc/gemm.hip, csrc/conv_s2.hip) chooses what it chose before.

Every case calls one C entry point on inputs from a seeded CPU generator and records
  * its return code and, for a refusal, the text of avec_last_error(),
  * the kernel instance reported by avec_last_kernel(),
  * a sha256 of the output bytes where the result is deterministic (every avec_gemm_nt / avec_gemm_nt_fp8 `out`, avec_gemm_tn_batched_store); what is summed with fp32
    atomics (stats, colsum, split-K avec_gemm_tn*, grouped products) is compared by kernel name only -- tests/test_gpu_parity.py and friends hold their numerics.
The records are compared for equality with tests/golden/gemm_dispatch.json.  Running this file as a script writes that file: do it once, on an MI355X, against the library
of the commit BEFORE a change to the dispatch (build it in a scratch tree and point AVEC_LIB_PATH at its libavec_hip.so), never against the library under test.
The cases run in table order in one process: avec_gemm_nt_fp8 notes no kernel name, so its record holds the name left by the case before it.

The shapes are the smallest on each side of a decision (tile choice at 383 / 384 tiles of 128 rows, the lean kernel's 4096-tile limit, ring depth at 512 / 513 tiles and
K = 384 / 392, the shifted-window kernel's e256 > e128 crossing, the grouped kernel's tile at 95 / 96, ...).

Not set up here, and why:
  * gemm_nt_glds_kernel with 64-byte rows (<.., 3 or 4, 1, 64>) and with FC = 1 on the 128-row tiles: a bf16 convolution that qualifies goes to gemm_nt_conv_lean_kernel
    first unless AVEC_NO_LEAN_CONV is set (or its weights exceed 4 GiB), and the 64 x 64 tile is only chosen below 1536 tiles unless AVEC_NT_RB=64 is; the library reads both
    once per process.  The 1535 / 1536-tile cases below pin that the tile count alone does not switch the row width of a product that the lean kernels take.
  * which of its three tiles avec_gemm_nt_fp8 takes: the entry point notes no kernel name, and the output bytes do not depend on the tile (every element is the same
    fp32 sum over K in the same order).  The fp8 cases on both sides of the two thresholds pin return code and result only.
  * gemm_tn_tr_kernel with Q32 = 0: the gathered operand needs more than 2^31 elements (4 GiB, with a matching P).
  * the KT = 64 gemm_tn_tr_kernel instances (AVEC_TN_KT), AVEC_TN_WGS, AVEC_SHIFT_BM, AVEC_NO_*: read once per process; the tests that set them in child processes stay
    where they are (tests/test_gpu_round3.py, tests/test_gpu_round5.py).
"""
import ctypes
import hashlib
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_dispatch.json")
F32, BF16 = 0, 1
PLAIN, FWD, BWD = 0, 1, 2

_state = {}


def _env():
    """torch, the library and the seeded pool of input values, once"""
    if not _state:
        import torch
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        from avec_amd import lib as L
        g = torch.Generator().manual_seed(20240607)
        _state.update(torch=torch, L=L, dev=torch.device("cuda:0"), pool=torch.randn(1 << 22, generator=g) * 0.5,
                      bits=torch.randint(0, 256, (1 << 20,), generator=g, dtype=torch.uint8), pos=0)
    return _state


def _vals(n, dtype, off=0):
    """n seeded values on the device, in a buffer whose data pointer is `off` elements behind an aligned address (64 spare elements behind the last)"""
    s = _env(); torch = s["torch"]
    pool = s["pool"]
    start = s["pos"] % 4093; s["pos"] += 7919
    reps = (start + n + pool.numel() - 1) // pool.numel()
    src = (pool if reps == 1 else pool.repeat(reps))[start:start + n]
    buf = torch.zeros(n + off + 64, dtype=dtype, device=s["dev"])
    buf[off:off + n].copy_(src.to(dtype))
    return buf[off:off + n]


def _zeros(n, dtype, off=0):
    s = _env()
    return s["torch"].zeros(n + off + 64, dtype=dtype, device=s["dev"])[off:off + n]


def _bits(n):
    """n seeded bytes on the device"""
    s = _env()
    return s["bits"].repeat(n // s["bits"].numel() + 1)[:n].to(s["dev"])


def _sha(t):
    s = _env()
    s["torch"].cuda.synchronize()
    return hashlib.sha256(t.contiguous().view(s["torch"].uint8).cpu().numpy().tobytes()).hexdigest()


def _record(rc, out=None):
    s = _env(); raw = s["L"].lib.raw
    s["torch"].cuda.synchronize()
    rec = {"rc": int(rc), "kernel": raw("avec_last_kernel")().decode()}
    if rc != 0:
        rec["error"] = raw("avec_last_error")().decode()
    elif out is not None:
        rec["sha256"] = _sha(out)
    return rec


def _ptr(t):
    return None if t is None else t.data_ptr()


def _conv(H, W, C, KH, KW, stride, pad, OH, OW):
    return dict(H=H, W=W, C=C, KH=KH, KW=KW, stride=stride, pad=pad, OH=OH, OW=OW)


def nt(dtype=BF16, M=64, N=64, K=64, mode=PLAIN, conv=None, imgs=0, a_f32=0, lda=None, ldw=None, step=None, off_a=0, off_w=0, off_out=0, out_f32=0, bias=False, act=0,
       colsum=False, stats=False, res=None, res_rows=None, res_mask=False, res_cls0=0, null=None, drop_p=0.0, bnb=False, ldo=None, ldres=None, call_n=None):
    """one avec_gemm_nt call.  conv: geometry of the gathered source (imgs images); res: None, "act" or "f32"; call_n: the N of the call itself (buffers keep the size N gives)"""
    s = _env(); torch = s["torch"]; L = s["L"]
    adt = torch.bfloat16 if dtype == BF16 else torch.float32
    rows = L.Rows()
    if conv is None:
        lda = K if lda is None else lda
        rows.ld = lda
        src_rows = M
        if step:
            rows.rows_out, rows.rows_in, rows.step = step          # (rows_out, rows_in, step)
            src_rows = (M // step[0] + 1) * step[1]
        if lda > 4 * K:      # rows far apart (lean_rows_past_32bit: 64 rows x (2^25 + 8) bf16 = 4 GiB, the smallest operand beyond 32-bit byte offsets): uninitialised
            # storage, only the K elements of every row are written (and read)
            A = torch.empty(src_rows * lda + 64, dtype=adt, device=s["dev"])[:src_rows * lda]
            A.as_strided((src_rows, K), (lda, 1)).copy_(_vals(src_rows * K, adt).view(src_rows, K))
        else:
            A = _vals(src_rows * lda, torch.float32 if a_f32 else adt, off_a)
    else:
        for k, v in conv.items():
            setattr(rows, k, v)
        pix = conv["H"] * conv["W"] if mode == FWD else conv["OH"] * conv["OW"]
        A = _vals(imgs * pix * conv["C"], torch.float32 if a_f32 else adt, off_a)
    ldw = K if ldw is None else ldw
    Wt = _vals(N * ldw, adt, off_w)
    ldo = N if ldo is None else ldo
    out = _zeros(M * ldo, torch.float32 if out_f32 else adt, off_out)
    ep = L.Epilogue(); ep.out = _ptr(out); ep.ldo = ldo; ep.out_f32 = out_f32; ep.alpha = 1.0; ep.act = act; ep.drop_p = drop_p
    keep = [A, Wt, out]
    if bias:
        keep.append(_vals(N, torch.float32)); ep.bias = _ptr(keep[-1])
    if colsum:
        keep.append(_zeros(N, torch.float32)); ep.colsum = _ptr(keep[-1])
    if stats:
        keep.append(_zeros(64 * 2 * N, torch.float32)); ep.stats = _ptr(keep[-1])
    if res:
        ldres = N if ldres is None else ldres
        keep.append(_vals((M if res_rows is None else res_rows) * ldres, adt if res == "act" else torch.float32)); ep.res = _ptr(keep[-1]); ep.ldres = ldres; ep.res_act = 1 if res == "act" else 0
    if res_mask:
        keep.append(_bits((M * N + 7) // 8 + 64)); ep.res_mask = _ptr(keep[-1])
    if bnb:
        keep.append(_vals(M * N, adt)); ep.bnb_y = _ptr(keep[-1]); ep.ldby = N
    ep.res_cls0 = res_cls0
    a_ptr, w_ptr, ep_ref, rows_ref = _ptr(A), _ptr(Wt), ctypes.byref(ep), ctypes.byref(rows)
    if null == "A": a_ptr = None
    if null == "W": w_ptr = None
    if null == "ep": ep_ref = None
    if null == "rows": rows_ref = None
    if null == "out": ep.out = None
    rc = L.lib.raw("avec_gemm_nt")(dtype, a_ptr, rows_ref, mode, a_f32, w_ptr, ldw, M, N if call_n is None else call_n, K, ep_ref, None)
    return _record(rc, out)


def conv1(imgs, S, C, N, mode, stride=1, **kw):
    """1 x 1 convolution over S x S images (gemm_nt_conv_lean_kernel on the 128-row tiles, the LDS-DMA kernel below them)"""
    O = (S - 1) // stride + 1
    M = imgs * (O * O if mode == FWD else S * S)
    return nt(M=M, N=N, K=C, mode=mode, conv=_conv(S, S, C, 1, 1, stride, 0, O, O), imgs=imgs, **kw)


def conv3(imgs, S, C, N, mode, stride=1, **kw):
    """3 x 3 convolution, pad 1 (conv3x3_shift_kernel at stride 1, conv3x3_s2_* at stride 2)"""
    O = (S - 1) // stride + 1
    M = imgs * (O * O if mode == FWD else S * S)
    return nt(M=M, N=N, K=9 * C, mode=mode, conv=_conv(S, S, C, 3, 3, stride, 1, O, O), imgs=imgs, **kw)


def fp8(M, N, K=64, null=None, lda=None, drop_p=0.0):
    s = _env(); torch = s["torch"]; L = s["L"]
    lda = K if lda is None else lda
    byt = lambda n: _bits(n + 64) % 0x70 | ((_bits(n + 71)[7:] & 1) << 7)      # finite e4m3 codes of either sign
    A, Wt = byt(M * lda), byt(N * K)
    amax = _zeros(2, torch.float32) + 1.5
    out = _zeros(M * N, torch.bfloat16)
    ep = L.Epilogue(); ep.out = _ptr(out); ep.ldo = N; ep.alpha = 1.0; ep.drop_p = drop_p
    rc = L.lib.raw("avec_gemm_nt_fp8")(None if null == "A" else _ptr(A), lda, _ptr(Wt), K, M, N, K, _ptr(amax), amax.data_ptr() + 4, ctypes.byref(ep), None)
    return _record(rc, out)


def tn(dtype=BF16, M=256, I=64, J=64, mode=PLAIN, conv=None, imgs=0, q_f32=0, ldp=None, ldq=None, off_p=0, off_q=0, colsum=None, entry="tn", nb=(1, 1), null=None, call_j=None):
    """avec_gemm_tn / _bias / _batched / _batched_store.  Batches lie behind one another (strides = whole matrices)"""
    s = _env(); torch = s["torch"]; L = s["L"]
    adt = torch.bfloat16 if dtype == BF16 else torch.float32
    nbatch = nb[0] * nb[1]
    ldp = I if ldp is None else ldp
    P = _vals(nbatch * M * ldp, adt, off_p)
    rows = L.Rows()
    if conv is None:
        ldq = J if ldq is None else ldq
        rows.ld = ldq
        Q = _vals(nbatch * M * ldq, torch.float32 if q_f32 else adt, off_q)
    else:
        for k, v in conv.items():
            setattr(rows, k, v)
        Q = _vals(imgs * conv["H"] * conv["W"] * conv["C"], adt, off_q)
    O = _zeros(nbatch * I * J, adt if entry == "store" else torch.float32)
    raw = L.lib.raw
    p_ptr = None if null == "P" else _ptr(P)
    if entry == "tn":
        rc = raw("avec_gemm_tn")(dtype, p_ptr, ldp, _ptr(Q), None if null == "rows" else ctypes.byref(rows), mode, q_f32, _ptr(O), J, M, I, J if call_j is None else call_j, None)
    elif entry == "bias":
        cs = _zeros(I, torch.float32) if colsum else None
        rc = raw("avec_gemm_tn_bias")(dtype, p_ptr, ldp, _ptr(Q), ctypes.byref(rows), mode, q_f32, _ptr(O), J, _ptr(cs), M, I, J, None)
    else:
        st6 = (ctypes.c_longlong * 6)(nb[1] * M * ldp, M * ldp, nb[1] * M * ldq, M * ldq, nb[1] * I * J, I * J)
        if null == "odd_stride": st6[0] += 1
        name = "avec_gemm_tn_batched_store" if entry == "store" else "avec_gemm_tn_batched"
        rc = raw(name)(dtype, p_ptr, ldp, _ptr(Q), ldq, _ptr(O), J, M, I, J, nb[0], nb[1], None if null == "strides" else st6, None)
    return _record(rc, O if entry == "store" else None)


def multi(problems, n=None, null=None):
    """avec_gemm_tn_batched_multi over (M, I, J, nbatch, store) problems"""
    s = _env(); torch = s["torch"]; L = s["L"]
    items = (L.TnBatched * max(len(problems), 1))(); keep = []
    for k, (M, I, J, nbatch, store) in enumerate(problems):
        P, Q = _vals(nbatch * M * I, torch.bfloat16), _vals(nbatch * M * J, torch.bfloat16)
        O = _zeros(nbatch * I * J, torch.bfloat16 if store else torch.float32)
        st6 = (ctypes.c_longlong * 6)(0, M * I, 0, M * J, 0, I * J)
        keep += [P, Q, O, st6]
        t = items[k]; t.P = _ptr(P); t.ldp = I; t.Q = _ptr(Q); t.ldq = J; t.ldo = J; t.M = M; t.I = I; t.J = J; t.nb_outer = 1; t.nb_inner = nbatch
        t.strides6 = None if null == "strides" else st6
        if store: t.O_act = _ptr(O)
        else: t.O = _ptr(O)
    rc = L.lib.raw("avec_gemm_tn_batched_multi")(BF16, ctypes.byref(items), len(problems) if n is None else n, None)
    return _record(rc)


def grouped(shapes, dtype=BF16, n=None, M=256):
    """avec_gemm_tn_grouped over (I, J) products of M rows"""
    s = _env(); torch = s["torch"]; L = s["L"]
    items = (L.TnItem * max(len(shapes), 1))(); keep = []
    for k, (I, J) in enumerate(shapes):
        P, Q, O = _vals(M * I + 8, torch.bfloat16), _vals(M * J + 8, torch.bfloat16), _zeros(I * J, torch.float32)
        keep += [P, Q, O]
        t = items[k]; t.P = _ptr(P); t.Q = _ptr(Q); t.O = _ptr(O); t.ldp = I; t.ldq = J; t.ldo = J; t.M = M; t.I = I; t.J = J
    rc = L.lib.raw("avec_gemm_tn_grouped")(dtype, ctypes.byref(items), len(shapes) if n is None else n, None)
    return _record(rc)


C3 = _conv(8, 8, 64, 3, 3, 1, 1, 8, 8)
CASES = [
    # ---- launch_nt: tile choice ----------------------------------------------------------------------------------------------------------
    ("nt_tile_t128_384", nt, dict(M=128 * 384, N=128, K=16)),                      # 384 tiles of 128 x 128: the big tile
    ("nt_tile_t128_383_lean", nt, dict(M=128 * 383, N=128, K=16)),                 # 383: lean 64 x 64 (1532 tiles, two-stage ring)
    ("nt_tile_n64_never_128", nt, dict(M=128 * 384, N=64, K=16)),                  # N <= 64 never takes 128 x 128; lean
    ("nt_tile_128x64_384", nt, dict(M=128 * 384, N=64, K=12)),                     # K = 8n + 4 is not lean: 384 tiles of 128 x 64
    ("nt_tile_128x64_383", nt, dict(M=128 * 383, N=64, K=12)),                     # 383: 64 x 64, lean kernel with the K tail
    ("nt_tile_lean_4096", nt, dict(M=64 * 4096, N=64, K=8)),                       # 4096 tiles of 64 x 64: still lean
    ("nt_tile_lean_4097", nt, dict(M=64 * 4096 + 1, N=64, K=8)),                   # 4097: the general 128 x 64 kernel
    ("nt_tile_f32_128x128", nt, dict(dtype=F32, M=128 * 384, N=128, K=8)),
    ("nt_tile_f32_128x64", nt, dict(dtype=F32, M=128 * 384, N=64, K=8)),
    ("nt_tile_f32_64x64", nt, dict(dtype=F32, M=100, N=72, K=8)),
    # ---- lean plain kernel ---------------------------------------------------------------------------------------------------------------
    ("lean_ring2_513", nt, dict(M=64 * 513, N=64, K=384)),
    ("lean_ring4_512", nt, dict(M=64 * 512, N=64, K=384)),
    ("lean_ring4_k392", nt, dict(M=64 * 513, N=64, K=392)),
    ("lean_ring2_staged_out_unaligned", nt, dict(M=64 * 513, N=64, K=16, off_out=4)),
    ("lean_ring4_staged_colsum", nt, dict(M=300, N=72, K=64, colsum=True)),
    ("lean_ring4_staged_stats", nt, dict(M=300, N=72, K=64, stats=True)),
    ("lean_tr_bias_swish_res", nt, dict(M=300, N=72, K=64, bias=True, act=1, res="f32")),
    ("lean_tr_out_f32", nt, dict(M=300, N=72, K=64, out_f32=1)),
    ("lean_staged_n_odd", nt, dict(M=300, N=70, K=64)),
    ("lean_ktail", nt, dict(M=300, N=72, K=180, lda=180, ldw=180)),
    ("lean_a_unaligned", nt, dict(M=300, N=72, K=64, off_a=2)),                     # the DMA takes any source address
    ("lean_rows_past_32bit", nt, dict(M=64, N=64, K=64, lda=(1 << 25) + 8)),         # 64 rows x 2^25 elements x 2 bytes = 2^32: the general LDS-DMA kernel
    ("plain_step2_aligned", nt, dict(M=256, N=64, K=64, step=(32, 64, 2))),         # strided row source: not lean
    ("plain_step2_unaligned", nt, dict(M=256, N=64, K=64, step=(32, 64, 2), off_a=2)),
    # ---- LDS-DMA kernel (gemm_nt_glds_kernel) --------------------------------------------------------------------------------------------
    ("glds_plain_128x128_ktail", nt, dict(M=128 * 384, N=128, K=12)),
    ("glds_plain_1535_tiles", nt, dict(M=128 * 307, N=640, K=16)),                  # 1535 tiles of 128 x 128
    ("glds_plain_1536_tiles", nt, dict(M=128 * 384, N=512, K=16)),                  # 1536: plain products keep 128-byte rows
    ("glds_f32_plain_aligned", nt, dict(dtype=F32, M=200, N=72, K=32)),
    ("glds_conv_fc0_fwd", nt, dict(M=40 * 64, N=64, K=32, mode=FWD, conv=_conv(8, 8, 32, 1, 1, 1, 0, 8, 8), imgs=40)),      # 32 channels: not the fast gather
    ("glds_conv_fc0_bwd", nt, dict(M=40 * 64, N=64, K=32, mode=BWD, conv=_conv(8, 8, 32, 1, 1, 1, 0, 8, 8), imgs=40)),
    ("glds_conv_fc1_fwd_64x64", conv1, dict(imgs=40, S=8, C=64, N=64, mode=FWD)),
    ("glds_conv_fc1_bwd_64x64", conv1, dict(imgs=40, S=8, C=64, N=64, mode=BWD)),
    ("glds_conv_fc1_f32_fwd", nt, dict(dtype=F32, M=40 * 64, N=64, K=32, mode=FWD, conv=_conv(8, 8, 32, 1, 1, 1, 0, 8, 8), imgs=40)),
    ("glds_conv_fc1_f32_bwd_128x128", nt, dict(dtype=F32, M=768 * 64, N=128, K=32, mode=BWD, conv=_conv(8, 8, 32, 1, 1, 1, 0, 8, 8), imgs=768)),
    ("glds_conv_perm2_bwd_64x64", conv1, dict(imgs=40, S=8, C=64, N=64, mode=BWD, stride=2)),       # parity-class order
    # ---- register-staged kernel (gemm_nt_kernel) -----------------------------------------------------------------------------------------
    ("gen_f32src_aligned", nt, dict(M=300, N=72, K=64, a_f32=1)),
    ("gen_f32src_unaligned", nt, dict(M=300, N=72, K=64, a_f32=1, off_a=1)),
    ("gen_f32src_128x128", nt, dict(M=128 * 384, N=128, K=16, a_f32=1)),
    ("gen_f32src_128x64", nt, dict(M=128 * 384, N=64, K=16, a_f32=1)),
    ("gen_bf16_k_mod8_2", nt, dict(M=300, N=72, K=66, lda=66, ldw=66)),              # K = 8n + 2: neither DMA kernel
    ("gen_bf16_k_mod8_2_128x64", nt, dict(M=128 * 384, N=64, K=10, lda=10, ldw=10)),
    ("gen_f32_unaligned", nt, dict(dtype=F32, M=200, N=72, K=32, off_a=1)),
    ("gen_f32_unaligned_128x128", nt, dict(dtype=F32, M=128 * 384, N=128, K=8, off_w=1)),
    ("gen_conv_fwd_unaligned", nt, dict(M=40 * 64, N=64, K=64, mode=FWD, conv=_conv(8, 8, 64, 1, 1, 1, 0, 8, 8), imgs=40, off_a=2)),
    ("gen_conv_bwd_unaligned", nt, dict(M=40 * 64, N=64, K=64, mode=BWD, conv=_conv(8, 8, 64, 1, 1, 1, 0, 8, 8), imgs=40, off_a=2)),
    ("gen_conv_fwd_f32flag_aligned", nt, dict(M=40 * 64, N=64, K=64, mode=FWD, conv=_conv(8, 8, 64, 1, 1, 1, 0, 8, 8), imgs=40, a_f32=1)),
    ("gen_conv_f32_fwd_unaligned", nt, dict(dtype=F32, M=40 * 64, N=64, K=32, mode=FWD, conv=_conv(8, 8, 32, 1, 1, 1, 0, 8, 8), imgs=40, off_w=1)),
    ("gen_conv_f32_bwd_unaligned", nt, dict(dtype=F32, M=40 * 64, N=64, K=32, mode=BWD, conv=_conv(8, 8, 32, 1, 1, 1, 0, 8, 8), imgs=40, off_w=1)),
    # ---- gemm_nt_conv_lean_kernel (1 x 1 convolutions on the 128-row tiles) ---------------------------------------------------------------
    ("clean_fwd_128_tr", conv1, dict(imgs=768, S=8, C=64, N=128, mode=FWD, stats=True)),
    ("clean_fwd_128_staged", conv1, dict(imgs=768, S=8, C=64, N=128, mode=FWD, bias=True)),
    ("clean_bwd_128_tr", conv1, dict(imgs=768, S=8, C=64, N=128, mode=BWD, res="act")),
    ("clean_bwd_128_staged", conv1, dict(imgs=768, S=8, C=64, N=128, mode=BWD, res="f32")),
    ("clean_fwd_64_tr", conv1, dict(imgs=768, S=8, C=64, N=64, mode=FWD)),
    ("clean_fwd_64_staged", conv1, dict(imgs=768, S=8, C=64, N=64, mode=FWD, out_f32=1)),
    ("clean_bwd_64_tr", conv1, dict(imgs=768, S=8, C=64, N=64, mode=BWD)),
    ("clean_bwd_64_staged", conv1, dict(imgs=768, S=8, C=64, N=64, mode=BWD, act=2)),
    ("clean_1535_tiles", conv1, dict(imgs=3070, S=8, C=64, N=128, mode=FWD)),
    ("clean_1536_tiles", conv1, dict(imgs=3072, S=8, C=64, N=128, mode=FWD)),
    ("clean_bwd_perm2_s2", conv1, dict(imgs=3072, S=8, C=64, N=128, mode=BWD, stride=2)),
    ("clean_res_mask_tr", conv1, dict(imgs=768, S=8, C=64, N=128, mode=BWD, res="act", res_mask=True)),
    ("clean_res_mask_rejected_staged", conv1, dict(imgs=768, S=8, C=64, N=128, mode=BWD, res="act", res_mask=True, off_out=4)),
    ("gen_res_mask_rejected", conv1, dict(imgs=40, S=8, C=64, N=64, mode=BWD, res="act", res_mask=True)),
    # ---- conv3x3_shift_kernel -----------------------------------------------------------------------------------------------------------
    ("shift_128x64_fwd", conv3, dict(imgs=12, S=8, C=32, N=64, mode=FWD)),
    ("shift_128x64_bwd", conv3, dict(imgs=12, S=8, C=32, N=64, mode=BWD, res="act")),
    # tile height: e128 = t128 / (rounds of 768), e256 = 1.08 * t256 / (rounds of 512); 256 rows when e256 > e128
    ("shift_1_tile_256", conv3, dict(imgs=2, S=8, C=32, N=128, mode=FWD)),                      # 1 / 768 vs 1.08 * 1 / 512
    ("shift_2_tiles_128", conv3, dict(imgs=4, S=8, C=32, N=128, mode=FWD)),                     # 2 / 768 vs 1.08 * 1 / 512
    ("shift_3_tiles_256_by_factor", conv3, dict(imgs=6, S=8, C=32, N=128, mode=FWD)),           # 3 / 768 = 2 / 512: the factor 1.08 decides
    ("shift_768_tiles_128_fwd", conv3, dict(imgs=1536, S=8, C=32, N=128, mode=FWD, stats=True)),  # 768 / 768 vs 1.08 * 384 / 512
    ("shift_768_tiles_128_bwd", conv3, dict(imgs=1536, S=8, C=32, N=128, mode=BWD, res="act")),
    ("shift_769_tiles_256_fwd_tr", conv3, dict(imgs=1538, S=8, C=32, N=128, mode=FWD, stats=True)),   # 769 / 1536 vs 1.08 * 385 / 512
    ("shift_769_tiles_256_bwd_tr", conv3, dict(imgs=1538, S=8, C=32, N=128, mode=BWD, res="act")),
    ("shift_769_tiles_256_fwd_staged", conv3, dict(imgs=1538, S=8, C=32, N=128, mode=FWD, bias=True)),
    ("shift_769_tiles_256_bwd_staged", conv3, dict(imgs=1538, S=8, C=32, N=128, mode=BWD, res="f32")),
    ("shift_res_mask_tr", conv3, dict(imgs=12, S=8, C=32, N=128, mode=BWD, res="act", res_mask=True)),      # the mask forces the 256-row register-direct instance
    ("shift_res_mask_rejected_n64", conv3, dict(imgs=12, S=8, C=32, N=64, mode=BWD, res="act", res_mask=True)),
    ("shift_res_mask_rejected_staged", conv3, dict(imgs=12, S=8, C=32, N=128, mode=BWD, res="act", res_mask=True, off_out=4)),
    ("shift_w32_falls_through", conv3, dict(imgs=2, S=32, C=32, N=64, mode=FWD)),                # W > 31
    # ---- conv3x3_s2_* -------------------------------------------------------------------------------------------------------------------
    ("s2_fwd_even_128", conv3, dict(imgs=20, S=12, C=32, N=128, mode=FWD, stride=2, stats=True)),
    ("s2_fwd_odd_128", conv3, dict(imgs=20, S=11, C=32, N=128, mode=FWD, stride=2)),
    ("s2_fwd_even_64", conv3, dict(imgs=20, S=12, C=32, N=64, mode=FWD, stride=2)),
    ("s2_fwd_odd_64", conv3, dict(imgs=20, S=11, C=32, N=64, mode=FWD, stride=2)),
    ("s2_bwd_even_128", conv3, dict(imgs=20, S=12, C=32, N=128, mode=BWD, stride=2, res="act")),
    ("s2_bwd_odd_128", conv3, dict(imgs=20, S=11, C=32, N=128, mode=BWD, stride=2)),
    ("s2_bwd_even_64", conv3, dict(imgs=20, S=12, C=32, N=64, mode=BWD, stride=2)),
    ("s2_bwd_odd_64", conv3, dict(imgs=20, S=11, C=32, N=64, mode=BWD, stride=2, res="act")),
    ("s2_bwd_res_cls0", conv3, dict(imgs=20, S=11, C=64, N=64, mode=BWD, stride=2, res="act", res_cls0=1, res_rows=20 * 36)),
    ("s2_wide_falls_to_class_glds", conv3, dict(imgs=4, S=32, C=64, N=64, mode=BWD, stride=2)),       # OW = 16 > 15: parity-class order in the LDS-DMA kernel
    ("s2_wide_res_cls0_class_glds", conv3, dict(imgs=4, S=32, C=64, N=64, mode=BWD, stride=2, res="act", res_cls0=1, res_rows=4 * 256)),
    ("s2_res_cls0_rejected_alignment", conv3, dict(imgs=4, S=32, C=64, N=64, mode=BWD, stride=2, res="act", res_cls0=1, res_rows=4 * 256, off_a=2)),
    ("s2_fwd_bias_falls_through", conv3, dict(imgs=20, S=12, C=64, N=64, mode=FWD, stride=2, bias=True)),
    # ---- avec_gemm_nt_fp8 ---------------------------------------------------------------------------------------------------------------
    ("fp8_64x64", fp8, dict(M=300, N=128)),
    ("fp8_128x64", fp8, dict(M=128 * 384, N=64, K=16)),
    ("fp8_128x64_383", fp8, dict(M=128 * 383, N=64, K=16)),
    ("fp8_128x128", fp8, dict(M=128 * 384, N=128, K=16)),
    # ---- avec_gemm_tn* ------------------------------------------------------------------------------------------------------------------
    ("tn_64x64_tr", tn, dict(M=256, I=64, J=72)),
    ("tn_big_by_tiles_tr", tn, dict(M=256, I=128 * 6, J=128 * 8)),                 # 48 tiles of 128 x 128
    ("tn_47_tiles_64x64", tn, dict(M=256, I=128, J=128 * 47)),
    ("tn_big_by_m_tr", tn, dict(M=32768, I=128, J=128)),
    ("tn_m_32767_64x64", tn, dict(M=32767, I=128, J=128)),
    ("tn_wide_tr", tn, dict(M=32768, I=64, J=128)),
    ("tn_wide_not_below_m", tn, dict(M=32767, I=64, J=128)),
    ("tn_conv_tr_q32", tn, dict(M=40 * 64, I=64, J=576, mode=FWD, conv=C3, imgs=40)),
    ("tn_conv_big_tr", tn, dict(M=512 * 64, I=128, J=576, mode=FWD, conv=C3, imgs=512)),
    ("tn_conv_wide_tr", tn, dict(M=512 * 64, I=64, J=576, mode=FWD, conv=C3, imgs=512)),
    ("tn_conv_unaligned_generic", tn, dict(M=40 * 64, I=64, J=576, mode=FWD, conv=C3, imgs=40, off_p=2)),
    ("tn_conv_big_pixels_generic", tn, dict(M=2 * 72 * 72, I=64, J=72, mode=FWD, conv=_conv(72, 72, 8, 3, 3, 1, 1, 72, 72), imgs=2)),      # more than 4096 pixels per image
    ("tn_plain_unaligned_generic", tn, dict(M=256, I=64, J=72, off_q=2)),
    ("tn_plain_f32src", tn, dict(M=256, I=64, J=72, q_f32=1)),
    ("tn_plain_f32src_unaligned", tn, dict(M=256, I=64, J=72, q_f32=1, off_q=1)),
    ("tn_plain_big_unaligned_generic", tn, dict(M=256, I=128 * 6, J=128 * 8, off_p=2)),
    ("tn_f32_64x64_aligned", tn, dict(dtype=F32, M=256, I=64, J=72)),
    ("tn_f32_64x64_unaligned", tn, dict(dtype=F32, M=256, I=64, J=72, off_q=1)),
    ("tn_f32_big", tn, dict(dtype=F32, M=256, I=128 * 6, J=128 * 8)),
    ("tn_f32_conv", tn, dict(dtype=F32, M=40 * 64, I=64, J=288, mode=FWD, conv=_conv(8, 8, 32, 3, 3, 1, 1, 8, 8), imgs=40)),
    ("tn_bias_fused_tr", tn, dict(M=256, I=64, J=72, entry="bias", colsum=True)),
    ("tn_bias_separate_pass", tn, dict(M=256, I=64, J=72, entry="bias", colsum=True, off_q=2)),       # the kernel without fused sums: column-sum pass first
    ("tn_batched", tn, dict(M=64, I=48, J=48, entry="batched", nb=(2, 3))),
    ("tn_batched_big", tn, dict(M=64, I=128, J=128, entry="batched", nb=(6, 8))),
    ("tn_store_batched", tn, dict(M=64, I=48, J=48, entry="store", nb=(2, 3))),
    ("tn_store_single_aligned", tn, dict(M=64, I=64, J=64, entry="store")),                         # Oact keeps an aligned product off the transposed-read kernel
    ("tn_store_big", tn, dict(M=64, I=128, J=128, entry="store", nb=(6, 8))),
    # ---- avec_gemm_tn_batched_multi -----------------------------------------------------------------------------------------------------
    ("multi_three_join", multi, dict(problems=[(64, 48, 48, 4, False), (64, 48, 48, 4, False), (64, 40, 48, 4, True)])),
    ("multi_one_joins_one_alone", multi, dict(problems=[(64, 128, 128, 48, False), (64, 48, 48, 4, False)])),
    ("multi_none_joins", multi, dict(problems=[(64, 128, 128, 48, False)])),
    # ---- avec_gemm_tn_grouped -----------------------------------------------------------------------------------------------------------
    ("grouped_t128_96", grouped, dict(shapes=[(384, 128)] * 32)),
    ("grouped_t128_95", grouped, dict(shapes=[(384, 128)] * 31 + [(256, 128)])),
    ("grouped_odd_widths", grouped, dict(shapes=[(180, 180), (90, 44)], M=1000)),
    # ---- argument checks: return code and avec_last_error text -------------------------------------------------------------------------
    ("err_nt_dtype", nt, dict(dtype=2)),
    ("err_nt_null_a", nt, dict(null="A")),
    ("err_nt_null_out", nt, dict(null="out")),
    ("err_nt_null_rows", nt, dict(null="rows")),
    ("err_nt_dims", nt, dict(call_n=0)),
    ("err_nt_mode", nt, dict(mode=3)),
    ("err_nt_k_small", nt, dict(K=6, lda=8, ldw=8)),
    ("err_nt_ldw_odd", nt, dict(K=64, ldw=65)),
    ("err_nt_lda_odd", nt, dict(K=64, lda=65)),
    ("err_nt_f32src_k", nt, dict(K=66, lda=66, ldw=66, a_f32=1)),
    ("err_nt_conv_c", nt, dict(M=64, N=64, K=36, mode=FWD, conv=_conv(8, 8, 4, 3, 3, 1, 1, 8, 8), imgs=1)),
    ("err_nt_conv_k", nt, dict(M=64, N=64, K=64, mode=FWD, conv=_conv(8, 8, 8, 3, 3, 1, 1, 8, 8), imgs=1)),
    ("err_nt_res_mask_plain", nt, dict(res="act", res_mask=True)),
    ("err_nt_res_cls0_stride1", conv3, dict(imgs=12, S=8, C=32, N=64, mode=BWD, res="act", res_cls0=1)),
    ("err_nt_bnb_without_stats", nt, dict(bnb=True)),
    ("err_nt_dropout_no_rng", nt, dict(drop_p=0.5)),
    ("err_fp8_null", fp8, dict(M=64, N=64, null="A")),
    ("err_fp8_lda", fp8, dict(M=64, N=64, lda=72)),
    ("err_fp8_dropout_no_rng", fp8, dict(M=64, N=64, drop_p=0.5)),
    ("err_tn_dtype", tn, dict(dtype=2)),
    ("err_tn_null", tn, dict(null="P")),
    ("err_tn_dims", tn, dict(call_j=0)),
    ("err_tn_mode", tn, dict(mode=BWD, conv=C3, imgs=4)),
    ("err_tn_i_small", tn, dict(I=6, ldp=6)),
    ("err_tn_ldq_odd", tn, dict(J=64, ldq=65)),
    ("err_tn_conv_c", tn, dict(M=64, I=64, J=36, mode=FWD, conv=_conv(8, 8, 4, 3, 3, 1, 1, 8, 8), imgs=1)),
    ("err_tn_f32src_j", tn, dict(J=66, ldq=66, q_f32=1)),
    ("err_tn_batch_stride_odd", tn, dict(M=64, I=48, J=48, entry="batched", nb=(2, 3), null="odd_stride")),
    ("err_tn_bias_i", tn, dict(I=66, ldp=66, entry="bias", colsum=True)),
    ("err_tn_batched_null_strides", tn, dict(M=64, I=48, J=48, entry="batched", null="strides")),
    ("err_tn_store_null_strides", tn, dict(M=64, I=48, J=48, entry="store", null="strides")),
    ("err_multi_count", multi, dict(problems=[(64, 48, 48, 4, False)], n=4)),
    ("err_multi_null_strides", multi, dict(problems=[(64, 48, 48, 4, False)], null="strides")),
    ("err_grouped_count", grouped, dict(shapes=[(64, 64)], n=33)),
    ("err_grouped_item", grouped, dict(shapes=[(64, 64)], dtype=F32)),
]
IDS = [c[0] for c in CASES]


def run_all():
    assert len(set(IDS)) == len(IDS)
    out = {}
    for cid, fn, kw in CASES:
        out[cid] = fn(**kw)
    return out


@pytest.fixture(scope="module")
def results():
    return run_all()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_file_holds_exactly_the_case_table(golden):
    assert sorted(golden) == sorted(IDS)


@pytest.mark.parametrize("cid", IDS)
def test_dispatch_matches_recorded(results, golden, cid):
    """same return code, same error text, same kernel instance, same output bytes as the library the golden file was recorded from"""
    assert results[cid] == golden[cid], cid


if __name__ == "__main__":
    rec = run_all()
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    for cid in IDS:
        print("%-36s %3d  %s%s" % (cid, rec[cid]["rc"], rec[cid]["kernel"], "  | " + rec[cid]["error"] if "error" in rec[cid] else ""))
