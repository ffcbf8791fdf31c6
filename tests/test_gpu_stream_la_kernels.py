"""GPU (-m gpu): the look-ahead streaming entry points (avec_relpos_attention_stream_la, avec_glu_dwconv_stream_la, avec_stream_window, avec_stream_window_advance;
avec_amd/csrc/attention.hip, convmod.hip), called through the C ABI push by push, element by element against the chunked fp64 references of
tests/stream_la_ref.py (pinned to the offline formulas on the host by tests/test_stream_la_ref.py).

Harness (that of tests/test_gpu_stream_kernels.py): every operand, output and state buffer is carved out of one allocation pre-filled with the NaN pattern 0x7FC0,
with sentinel gaps; the state buffers have exactly their stated size and start as NaN: a restart must hide them by position alone.  B = 3 slots per push: slot 0 runs
with full windows and every commit count from 0 to Tq, slot 1 is restarted in the middle, slot 2 has so few valid rows that (where Wq - L allows) a query keeps no key
and must read back as zeros, and commits nothing in every second push (its state must come back bit-identical).  Window rows at or past n hold finite garbage.

Judgement, per element of EVERY window row (the reference defines the rows at or past n too):  |got - ref| <= TOL * scale (+ half a bf16 ulp for a bf16 output,
+ 2^-126), TOL = attention_ref.TOL[valu_f32 | valu_bf16]["O"] and stream_ref.CONV_TOL, the project's; the rings and the context after every push equal the
reference's wherever it defines them.  No figure comes from a GPU run.
"""
import pytest
import torch

from tests import attention_ref as A
from tests import stream_la_ref as LR
from tests import stream_ref as SR
from tests.test_gpu_rowwise import Carve, TD, _lib, stream
from tests.test_gpu_stream_kernels import judge, run

pytestmark = pytest.mark.gpu
RW = A.RW
DT = RW.DT
I64 = lambda v: v.view(torch.int64)


def commits(Tq):
    return list(range(Tq + 1)) if Tq <= 6 else [0, 1, Tq // 2, Tq - 1, Tq]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("Wq", [3, 6, 40])
@pytest.mark.parametrize("L,R", [(0, 1), (3, 2), (6, 5), (70, 2)])
@pytest.mark.parametrize("d", [8, 24])
def test_relpos_attention_stream_la_per_element(d, L, R, Wq, dtype):
    B, H, esz, div = 3, 2, TD[dtype].itemsize, 2               # div = 2: the counters run at twice the stage's rate, as behind a stride-2 boundary
    Tq = Wq - min(R, Wq - 1)
    D, cap = H * d, L + Tq
    lib = _lib()
    sd = 8000 + 31 * d + 7 * L + 3 * R + Wq
    sg = 2.0 ** 0.25
    E = RW.rd(RW.gauss((L + R + 1, H, d), sd + 5) * sg, dtype)
    scale = float(torch.tensor(1.0 / d ** 0.5, dtype=torch.float32))
    cbytes = lib.raw("avec_relpos_attention_stream_state_bytes")(DT[dtype], B, H, d, L, Tq)
    assert cbytes == B * cap * D * esz
    c = Carve([(B * Wq * 3 * D, dtype), ((L + R + 1) * D, dtype), (cbytes // esz, dtype), (cbytes // esz, dtype), (B * Wq * D, dtype), (8 * B, "u8"), (8 * B, "u8"), (8 * B, "u8"), (B, "u8")])
    qkv_d, e_d, kc_d, vc_d, o_d = c.views[:5]
    pos_d, nv_d, nc_d, rs_d = I64(c.views[5]), I64(c.views[6]), I64(c.views[7]), c.views[8]
    e_d.copy_(E.reshape(-1))
    ref = LR.AttnStreamLA(B, H, d, L, R, Tq)
    written = torch.zeros(B, cap, dtype=torch.bool)
    tol = A.TOL["valu_f32" if dtype == "f32" else "valu_bf16"]["O"]
    cs = commits(Tq)
    pushes = 2 * len(cs) + 2
    n2 = max(Wq - L - 1, 0) if Wq - L >= 2 else 1              # slot 2: with n < Wq - L the rows >= n + L keep no key
    worst, empty_rows, q0 = 0.0, 0, qkv_d.data_ptr()
    for pi in range(pushes):
        c0 = cs[pi % len(cs)]
        c1 = cs[(pi + 2) % len(cs)]
        n = [Wq, min(Wq, c1 + (pi % 3)), 0 if pi % 4 == 3 else n2]
        cm = [c0, min(c1, n[1]), 0 if pi % 2 else min(n[2], 1, Tq)]
        reset = set(range(B)) if pi == 0 else ({1} if pi == pushes // 2 else set())
        q, k, v = (RW.rd(RW.gauss((B, Wq, H, d), sd + 10 * pi + j) * (sg if j < 2 else 1.0), dtype) for j in range(3))
        for b in range(B):
            k[b, n[b]:], v[b, n[b]:] = 2.0, 2.0                    # finite garbage: a key at or past n is left out whatever the row holds
        qkv_d.copy_(torch.cat([q.reshape(B * Wq, D), k.reshape(B * Wq, D), v.reshape(B * Wq, D)], 1).reshape(-1))
        p_before = [0 if b in reset else ref.pos[b] for b in range(B)]
        pos_d.copy_(torch.tensor([p * div for p in ref.pos], dtype=torch.int64))       # (a restarted slot's counter is stale: the flag hides it)
        nv_d.copy_(torch.tensor([max(x * div - 1, 0) for x in n], dtype=torch.int64))  # odd counts: a stage takes ceil(nvalid / div) rows
        nc_d.copy_(torch.tensor([x * div for x in cm], dtype=torch.int64))
        rs_d.copy_(torch.tensor([1 if b in reset else 0 for b in range(B)], dtype=torch.uint8))
        before = (kc_d.clone(), vc_d.clone())
        run(c, lambda: lib.relpos_attention_stream_la(DT[dtype], q0, q0 + D * esz, q0 + 2 * D * esz, 3 * D, e_d.data_ptr(), D, kc_d.data_ptr(), vc_d.data_ptr(), cbytes,
                                                      pos_d.data_ptr(), rs_d.data_ptr(), nv_d.data_ptr(), nc_d.data_ptr(), div, o_d.data_ptr(), D, B, H, Wq, Tq, d, L, R, scale,
                                                      stream()))
        assert lib.raw("avec_last_kernel")().decode() == "attn_stream_la<%s>" % dtype
        want, sc = ref.push(q, k, v, E, scale, n, cm, reset)
        got = o_d.view(B, Wq, H, d)
        kc, vc = kc_d.view(B, cap, H, d).cpu(), vc_d.view(B, cap, H, d).cpu()
        for b in range(B):
            worst = max(worst, judge((pi, b), got[b], want[b], sc[b], dtype, tol))
            none = [i for i in range(Wq) if i >= n[b] + L]          # no window key within L behind it, and (i >= L) no ring column either
            empty_rows += len(none)
            assert none == [] or not bool(got[b, none].float().abs().max() > 0), (pi, b, "a query that keeps no key must give zeros")
            if cm[b] == 0:
                for now, bef in ((kc_d, before[0]), (vc_d, before[1])):
                    assert torch.equal(now.view(B, -1)[b].view(torch.uint8), bef.view(B, -1)[b].view(torch.uint8)), (pi, b, "the rings of a slot that committed no row changed")
            for i in range(cm[b]):
                written[b, (p_before[b] + i) % cap] = True
            m = written[b]
            assert torch.equal(kc[b][m].double(), ref.kc[b][m]) and torch.equal(vc[b][m].double(), ref.vc[b][m]), (pi, b, "ring rows")
    assert empty_rows > 0 or Wq - L < 2
    print("relpos_attention_stream_la d=%d L=%d R=%d Wq=%d Tq=%d %s: %d pushes, worst ratio %.3g (tolerance %.3g), %d rows without a key" % (d, L, R, Wq, Tq, dtype, pushes, worst, tol, empty_rows))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("C,K,s,Wq", [(C, K, s, Wq) for C in (8, 36) for K in (3, 15) for s in (1, 2) for Wq in (4, 12)])
def test_glu_dwconv_stream_la_per_element(C, K, s, Wq, dtype):
    B, To, esz, div = 3, Wq // s, TD[dtype].itemsize, 2
    Tq = Wq - 2
    lib = _lib()
    sd = 9500 + 131 * C + 17 * K + 5 * s + Wq
    w = RW.rd(RW.gauss((K, C), sd + 1) * 0.4, "f32")
    bias = RW.rd(RW.coef(C, 1) * 0.3, "f32")
    ss = RW.rd(torch.stack([RW.coef(C, 2, positive=True), RW.coef(C, 3) * 0.5]), "f32")
    sbytes = lib.raw("avec_glu_dwconv_stream_state_bytes")(DT[dtype], B, C, K)
    c = Carve([(B * Wq * 2 * C, dtype), (K * C, "f32"), (C, "f32"), (2 * C, "f32"), (B * To * C, dtype), (sbytes // esz, dtype), (8 * B, "u8"), (8 * B, "u8"), (B, "u8")])
    u_d, w_d, b_d, ss_d, out_d, st_d = c.views[:6]
    pos_d, nc_d, rs_d = I64(c.views[6]), I64(c.views[7]), c.views[8]
    w_d.copy_(w.reshape(-1)), b_d.copy_(bias), ss_d.copy_(ss.reshape(-1))
    ref = SR.ConvStream(B, C, K)
    cs = sorted({0, 2, Tq})
    pushes = 3 * len(cs) + 2 + (K - 1) // 2                        # slot 0 commits more than K - 1 rows in all: the whole context turns over
    worst = 0.0
    for pi in range(pushes):
        cm = [cs[(pi + 1) % len(cs)], cs[pi % len(cs)], 2 if pi == 0 else 0]
        reset = set(range(B)) if pi == 0 else ({1} if pi == pushes // 2 else set())
        u = RW.rd(RW.gauss((B, Wq, 2 * C), sd + 10 * pi) * 1.5, dtype)
        u_d.copy_(u.reshape(-1))
        pos_d.copy_(torch.tensor([p * div for p in ref.pos], dtype=torch.int64))
        nc_d.copy_(torch.tensor([x * div for x in cm], dtype=torch.int64))
        rs_d.copy_(torch.tensor([1 if b in reset else 0 for b in range(B)], dtype=torch.uint8))
        before = st_d.clone()
        run(c, lambda: lib.glu_dwconv_stream_la(DT[dtype], u_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), ss_d.data_ptr(), out_d.data_ptr(), st_d.data_ptr(), sbytes,
                                                pos_d.data_ptr(), rs_d.data_ptr(), nc_d.data_ptr(), div, B, Wq, C, K, s, stream()))
        want, scale = ref.push(u, w, bias, ss, s, cm, reset)
        got = out_d.view(B, To, C)
        stv, bef = st_d.view(B, K - 1, 2 * C).cpu(), before.view(B, K - 1, 2 * C).cpu()
        for b in range(B):
            worst = max(worst, judge((pi, b), got[b], want[b], scale[b], dtype, SR.CONV_TOL))
            if cm[b] == 0:
                assert torch.equal(stv[b].view(torch.uint8), bef[b].view(torch.uint8)), (pi, b, "the context of a slot that committed no row changed")
            live = min(ref.pos[b], K - 1)                               # context rows at positions >= 0
            if live:
                assert torch.equal(stv[b, K - 1 - live:].double(), ref.ctx[b, K - 1 - live:]), (pi, b, "carried context rows")
    assert ref.pos[0] > K - 1
    print("glu_dwconv_stream_la C=%d K=%d s=%d Wq=%d %s: %d pushes, worst ratio %.3g (tolerance %.3g)" % (C, K, s, Wq, dtype, pushes, worst, SR.CONV_TOL))


@pytest.mark.parametrize("Tc,LAe,S,D", [(2, 2, 2, 5), (4, 6, 2, 32), (8, 2, 1, 300), (4, 24, 4, 8)])
def test_stream_window_and_advance_exact(Tc, LAe, S, D):
    """the two control launches over a schedule with restarts, short last chunks and an ended slot that is offered frames: X, the counts, the carried tail (where the
    reference defines it), pend, pos, ended, the consumed flags -- all exact (copies and integer arithmetic)"""
    utts = [[23, 9], [5], [16, 30]]
    B, W = len(utts), Tc + LAe
    lib = _lib()
    data = [[RW.rd(RW.gauss((T, D), 10 * b + u), "f32") for u, T in enumerate(ut)] for b, ut in enumerate(utts)]
    c = Carve([(B * Tc * D, "f32"), (B * LAe * D, "f32"), (B * W * D, "f32")] + [(8 * B, "u8")] * 6 + [(B, "u8")] * 3)
    x_d, tail_d, X_d = c.views[:3]
    pend_d, pos_d, nn_d, nv_d, nc_d, em_d = (I64(v) for v in c.views[3:9])
    last_d, rs_d, end_d = c.views[9:12]
    win = LR.Window(B, Tc, LAe, S, (D,))
    for pi, row in enumerate(LR.schedule(utts, Tc)):
        x = SR.chunk_of(data, [r[:4] for r in row], Tc, 3.0)
        last, reset = {b for b, r in enumerate(row) if r[4]}, {b for b, r in enumerate(row) if r[3]}
        n_new = [Tc if r[0] is None else r[2] for r in row]             # (an ended slot is offered Tc frames and takes none)
        x_d.copy_(x.reshape(-1)), nn_d.copy_(torch.tensor(n_new, dtype=torch.int64))
        last_d.copy_(torch.tensor([1 if b in last else 0 for b in range(B)], dtype=torch.uint8))
        rs_d.copy_(torch.tensor([1 if b in reset else 0 for b in range(B)], dtype=torch.uint8))
        run(c, lambda: lib.stream_window(x_d.data_ptr(), tail_d.data_ptr(), X_d.data_ptr(), pend_d.data_ptr(), nn_d.data_ptr(), last_d.data_ptr(), rs_d.data_ptr(), end_d.data_ptr(),
                                         nv_d.data_ptr(), nc_d.data_ptr(), em_d.data_ptr(), B, Tc, LAe, D, S, stream()))
        X, nvalid, ncommit, emit = win.begin(x, n_new, last, reset)
        assert torch.equal(X_d.view(B, W, D).cpu().double(), X), pi
        assert (nv_d.tolist(), nc_d.tolist(), em_d.tolist()) == (nvalid, ncommit, emit), pi
        run(c, lambda: lib.stream_window_advance(X_d.data_ptr(), tail_d.data_ptr(), pend_d.data_ptr(), pos_d.data_ptr(), nv_d.data_ptr(), nc_d.data_ptr(), last_d.data_ptr(),
                                                 rs_d.data_ptr(), end_d.data_ptr(), B, W, LAe, D, stream()))
        win.advance(X)
        assert (pend_d.tolist(), pos_d.tolist(), [bool(e) for e in end_d.tolist()]) == (win.pend, win.pos, win.ended), pi
        assert not bool(last_d.any()) and not bool(rs_d.any()), (pi, "the flags are consumed")
        tail = tail_d.view(B, LAe, D).cpu().double()
        for b in range(B):
            assert torch.equal(tail[b, :win.pend[b]], win.tail[b, :win.pend[b]]), (pi, b, "carried tail")
