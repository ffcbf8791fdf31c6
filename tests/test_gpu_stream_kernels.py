"""GPU (-m gpu): avec_glu_dwconv_stream and avec_relpos_attention_stream (avec_amd/csrc/convmod.hip, attention.hip), called through the C ABI push by push,
element by element against the chunked fp64 references of tests/stream_ref.py (pinned to the offline formulas on the host by tests/test_stream_ref.py).

Harness (that of tests/test_gpu_rowwise.py): every operand, output and state buffer is carved out of one allocation pre-filled with the NaN pattern 0x7FC0, with
sentinel gaps; the state buffers have exactly their stated size (avec_*_state_bytes), so a byte written beyond it lands in a gap.  The state starts as NaN: a slot's
restart must hide it by position alone.  Every push: B slots, a restart of slot 1 in push 2, a short final chunk, a slot that has run out and takes 0 frames
(its state must come back bit-identical); rows past chunk_len hold finite garbage.  After every push the position counters, the consumed restart flags and every state
row written so far are compared exactly (the state is a copy of the operands), the gaps must be intact.

Judgement, per element of the rows a slot took:  |got - ref| <= TOL * scale (+ half a bf16 ulp for a bf16 output, + 2^-126).
    convolution  TOL = 8 x 1.0e-7, the worst ratio of the host fp32 evaluation of the same formula over this case table (stream_ref.measure_conv_host: 9.92e-8)
    attention    TOL = attention_ref.TOL[valu_f32 | valu_bf16]["O"] = 8 x 1.90e-6 | 8 x 2.27e-7: the arithmetic is attn_rows_kernel's
No figure comes from a GPU run.
"""
import pytest
import torch

from tests import attention_ref as A
from tests import stream_ref as SR
from tests.test_gpu_rowwise import Carve, TD, _lib, stream

pytestmark = pytest.mark.gpu
RW = A.RW
DT = RW.DT


def run(c, fn):
    try:
        fn()
        torch.cuda.synchronize()
    except Exception as e:              # a failed launch or a device fault: nothing more is started on this device in this session
        pytest.exit("GPU launch failed, session ended: %r" % (e,), returncode=3)
    assert c.intact(), "written outside the outputs / beyond the stated state size"


def judge(tag, got, ref, scale, dtype, tol):
    got = got.detach().cpu()
    assert not bool(torch.isnan(got.float()).any()), (tag, "an element the kernel owes is NaN")
    r = RW.ratio(got, ref, scale, dtype)
    w = float(r.max())
    assert w <= tol, (tag, "ratio %.3g > %.3g at flat index %d" % (w, tol, int(r.argmax())))
    return w


class Ctl:
    """pos / chunk_len (int64) and reset (bytes) regions of a Carve, driven by a schedule row; avec_stream_advance ends the push"""

    def __init__(self, c, i_pos, i_len, i_reset, B):
        self.pos, self.clen, self.reset = c.views[i_pos].view(torch.int64), c.views[i_len].view(torch.int64), c.views[i_reset]
        self.pos.zero_()
        self.reset.zero_()
        self.B = B

    def set(self, row, mult=1):
        self.clen.copy_(torch.tensor([r[2] * mult for r in row], dtype=torch.int64))
        self.reset.copy_(torch.tensor([1 if r[3] else 0 for r in row], dtype=torch.uint8))

    def advance(self, full):
        _lib().stream_advance(self.pos.data_ptr(), self.reset.data_ptr(), self.clen.data_ptr(), full, self.B, stream())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("C,K,s,Tq", SR.CONV_CASES)
def test_glu_dwconv_stream_per_element(C, K, s, Tq, dtype):
    B, To, esz = 3, Tq // s, TD[dtype].itemsize
    lib = _lib()
    data, w, bias, ss = SR.conv_inputs(C, K, s, Tq, dtype)
    sbytes = lib.raw("avec_glu_dwconv_stream_state_bytes")(DT[dtype], B, C, K)
    assert sbytes == B * (K - 1) * 2 * C * esz
    c = Carve([(B * Tq * 2 * C, dtype), (K * C, "f32"), (C, "f32"), (2 * C, "f32"), (B * To * C, dtype), (sbytes // esz, dtype), (8 * B, "u8"), (8 * B, "u8"), (B, "u8")])
    u_d, w_d, b_d, ss_d, out_d, st_d = c.views[:6]
    ctl = Ctl(c, 6, 7, 8, B)
    w_d.copy_(w.reshape(-1)), b_d.copy_(bias), ss_d.copy_(ss.reshape(-1))
    ref = SR.ConvStream(B, C, K)
    sched = SR.schedule(SR.CONV_UTTS(Tq), Tq)
    assert len(sched) >= 3 and sched[1][1][3] and any(0 < r[2] < Tq for row in sched for r in row) and any(r[0] is None for r in sched[-1])
    worst, div = 0.0, 2                     # div = 2: the counters run at twice the stage's rate, as behind a stride-2 boundary
    for pi, row in enumerate(sched):
        n = [r[2] for r in row]
        reset = {b for b, r in enumerate(row) if r[3]}
        uc = SR.chunk_of(data, row, Tq, 3.0)
        u_d.copy_(uc.reshape(-1))
        ctl.set(row, div)
        before = st_d.clone()
        run(c, lambda: lib.glu_dwconv_stream(DT[dtype], u_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), ss_d.data_ptr(), out_d.data_ptr(), st_d.data_ptr(), sbytes,
                                             ctl.pos.data_ptr(), ctl.reset.data_ptr(), ctl.clen.data_ptr(), div, B, Tq, C, K, s, stream()))
        run(c, lambda: ctl.advance(Tq * div))
        want, scale = ref.push(uc, w, bias, ss, s, n, reset)
        got = out_d.view(B, To, C)
        stv, bef = st_d.view(B, K - 1, 2 * C).cpu(), before.view(B, K - 1, 2 * C).cpu()
        for b in range(B):
            rows = -(-n[b] // s)
            if rows:
                worst = max(worst, judge((pi, b), got[b, :rows], want[b, :rows], scale[b, :rows], dtype, SR.CONV_TOL))
            if n[b] == 0:
                assert torch.equal(stv[b].view(torch.uint8), bef[b].view(torch.uint8)), (pi, b, "the state of a slot that took no frame changed")
            live = min(ref.pos[b], K - 1)                                   # context rows at positions >= 0
            if live:
                assert torch.equal(stv[b, K - 1 - live:].double(), ref.ctx[b, K - 1 - live:]), (pi, b, "carried context rows")
        assert ctl.pos.tolist() == [p * div for p in ref.pos] and not bool(ctl.reset.any()), (pi, ctl.pos.tolist(), ref.pos)
    print("glu_dwconv_stream C=%d K=%d s=%d Tq=%d %s: %d pushes, worst ratio %.3g (tolerance %.3g)" % (C, K, s, Tq, dtype, len(sched), worst, SR.CONV_TOL))


ATTN_CASES = [(d, L, Tq) for d in (8, 45, 64, 90) for L in (0, 1, 5, 70) for Tq in (1, 3, 16)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d,L,Tq", ATTN_CASES)
def test_relpos_attention_stream_per_element(d, L, Tq, dtype):
    B, H, esz = 2, 2, TD[dtype].itemsize
    D, cap = H * d, L + Tq
    lib = _lib()
    utts = [[3 * cap + Tq + 1], [Tq, 2 * Tq + max(Tq // 2, 1)]]            # slot 0 wraps its ring three times and ends short; slot 1 restarts in push 2, ends short, runs out
    sd = 7000 + 31 * d + 7 * L + Tq
    sg = 2.0 ** 0.25
    data = [[[RW.rd(RW.gauss((T, H, d), sd + 100 * b + 10 * u + j) * (sg if j < 2 else 1.0), dtype) for j in range(3)] for u, T in enumerate(ut)] for b, ut in enumerate(utts)]
    part = lambda j: [[x[j] for x in ub] for ub in data]
    E = RW.rd(RW.gauss((L + 1, H, d), sd + 5) * sg, dtype)
    scale = float(torch.tensor(1.0 / d ** 0.5, dtype=torch.float32))
    cbytes = lib.raw("avec_relpos_attention_stream_state_bytes")(DT[dtype], B, H, d, L, Tq)
    assert cbytes == B * cap * D * esz
    c = Carve([(B * Tq * 3 * D, dtype), ((L + 1) * D, dtype), (cbytes // esz, dtype), (cbytes // esz, dtype), (B * Tq * D, dtype), (8 * B, "u8"), (8 * B, "u8"), (B, "u8")])
    qkv_d, e_d, kc_d, vc_d, o_d = c.views[:5]
    ctl = Ctl(c, 5, 6, 7, B)
    e_d.copy_(E.reshape(-1))
    ref = SR.AttnStream(B, H, d, L, Tq)
    written = torch.zeros(B, cap, dtype=torch.bool)
    tol = A.TOL["valu_f32" if dtype == "f32" else "valu_bf16"]["O"]
    sched = SR.schedule(utts, Tq)
    assert len(sched) >= 3 and sched[1][1][3] and sum(r[0][2] for r in sched) > 3 * cap
    worst, q0 = 0.0, qkv_d.data_ptr()
    for pi, row in enumerate(sched):
        n = [r[2] for r in row]
        reset = {b for b, r in enumerate(row) if r[3]}
        q, k, v = (SR.chunk_of(part(j), row, Tq, 2.0) for j in range(3))
        qkv_d.copy_(torch.cat([q.reshape(B * Tq, D), k.reshape(B * Tq, D), v.reshape(B * Tq, D)], 1).reshape(-1))
        ctl.set(row)
        before = (kc_d.clone(), vc_d.clone())
        run(c, lambda: lib.relpos_attention_stream(DT[dtype], q0, q0 + D * esz, q0 + 2 * D * esz, 3 * D, e_d.data_ptr(), D, kc_d.data_ptr(), vc_d.data_ptr(), cbytes,
                                                   ctl.pos.data_ptr(), ctl.reset.data_ptr(), ctl.clen.data_ptr(), 1, o_d.data_ptr(), D, B, H, Tq, d, L, scale, stream()))
        assert lib.raw("avec_last_kernel")().decode() == "attn_stream<%s>" % dtype
        p_before = list(ref.pos)
        run(c, lambda: ctl.advance(Tq))
        want, sc = ref.push(q, k, v, E, scale, n, reset)
        got = o_d.view(B, Tq, H, d)
        kc, vc = kc_d.view(B, cap, H, d).cpu(), vc_d.view(B, cap, H, d).cpu()
        for b in range(B):
            if n[b]:
                worst = max(worst, judge((pi, b), got[b, :n[b]], want[b, :n[b]], sc[b, :n[b]], dtype, tol))
            else:
                for now, bef in ((kc_d, before[0]), (vc_d, before[1])):
                    assert torch.equal(now.view(B, -1)[b].view(torch.uint8), bef.view(B, -1)[b].view(torch.uint8)), (pi, b, "the rings of a slot that took no frame changed")
            p0 = 0 if b in reset else p_before[b]
            for i in range(n[b]):
                written[b, (p0 + i) % cap] = True
            if pi % 16 == 0 or pi >= len(sched) - 2:
                m = written[b]
                assert torch.equal(kc[b][m].double(), ref.kc[b][m]) and torch.equal(vc[b][m].double(), ref.vc[b][m]), (pi, b, "ring rows")
        assert ctl.pos.tolist() == ref.pos and not bool(ctl.reset.any()), (pi, ctl.pos.tolist(), ref.pos)
    print("relpos_attention_stream d=%d L=%d Tq=%d %s: %d pushes, worst ratio %.3g (tolerance %.3g)" % (d, L, Tq, dtype, len(sched), worst, tol))
