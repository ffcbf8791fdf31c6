"""Launchers over the C ABI (raw pointers + sizes) and the autograd Functions that compose them.

Every Function writes parameter gradients straight into `param.grad` (accumulating; the flat gradient
arena when the model owns one) and returns None for them, so the backward pass is a fixed sequence of
HIP launches on the current stream (graph-capturable)."""
import collections
import ctypes
import os

import torch

from . import fp8
from . import runtime as rt
from .lib import (ACT_GELU, ACT_NONE, ACT_RELU, ACT_SWISH, BF16, LN_GROUP_MAX, ROWS_CONV_BWD, ROWS_CONV_FWD, ROWS_PLAIN, ROWS_STEM3D, TN_GROUP_MAX, WGRAD_GROUP_MAX, Attn, Epilogue, LnItem, Rows, TnBatched, TnItem,
                  WgradItem, lib)

_byref = ctypes.byref


class KernelTimer:
    """HIP-event timing of the GEMM-family launches (bench.py roofline): events are recorded on the launch stream around each
    launch while enabled; durations are read after the timed region."""
    NAMES = {(0, ROWS_CONV_FWD): "gemm_nt<conv_fwd>", (0, ROWS_CONV_BWD): "gemm_nt<conv_bwd_data>", (0, ROWS_STEM3D): "gemm_nt<stem3d>",
             (0, ROWS_PLAIN): "gemm_nt<plain>", (1, ROWS_CONV_FWD): "gemm_tn<conv_wgrad>", (1, ROWS_STEM3D): "gemm_tn<stem3d_wgrad>",
             (1, ROWS_PLAIN): "gemm_tn<plain>", (2, 0): "conv3x3_slab<fwd>", (2, 1): "conv3x3_slab<bwd_data>", (2, 2): "conv3x3_slab<wgrad>"}

    def __init__(self):
        self.enabled = False
        self.records = []

    def reset(self, enabled):
        self.enabled, self.records = enabled, []

    def start(self):
        """the event in front of a launch; None while disabled, which stop() ignores: launch sites bracket unconditionally"""
        if not self.enabled:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def stop(self, e0, key, flops, abytes=0.0):
        """abytes: ALGORITHMIC bytes of the launch (operands once + results once), next to the PMC traffic in the roofline rows"""
        if e0 is None:
            return
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        name = lib.raw("avec_last_kernel")()                  # the kernel instance the entry point chose (api.hip)
        self.records.append((key, flops, e0, e1, name.decode() if name else "", float(abytes)))

    def bracket_overhead_us(self, n=200):
        """what an event pair around NOTHING measures (the record / timestamp cost that every bracketed launch carries): calibrated live, subtracted from the per-launch
        durations so that they agree with rocprofv3's kernel durations of the graph-replayed step (round 3: 16.0 us here vs 13.0 us there for the dominant row)"""
        evs = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); b.record()
            evs.append((a, b))
        torch.cuda.synchronize()
        d = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
        return d[len(d) // 2]

    def summary(self, peak_tflops, steps=1):
        """`roofline` object of bench.py: one row per kernel INSTANCE (rocprofv3's kernel names), the top row = the kernel with the largest total time;
        `families` groups the same launches by addressing mode.  FLOPs are algorithmic (2 x MACs of the product the launch stands for: structurally
        zero taps of a strided backward-data convolution are not counted)."""
        if not self.records:
            return None
        torch.cuda.synchronize()
        ovh = self.bracket_overhead_us() * 1e-6
        agg, rows = {}, {}
        for key, flops, e0, e1, name, ab in self.records:
            dt = max(e0.elapsed_time(e1) * 1e-3 - ovh, 1e-7)
            a = agg.setdefault(key, [0.0, 0.0, 0])
            a[0] += dt; a[1] += flops; a[2] += 1
            r = rows.setdefault(name or self.NAMES.get(key, str(key)), [0.0, 0.0, 0, 0.0])
            r[0] += dt; r[1] += flops; r[2] += 1; r[3] += ab

        def row(name, v):
            return {"kernel": name, "launches_per_step": round(v[2] / steps, 1), "avg_us": round(1e6 * v[0] / v[2], 2), "ms_per_step": round(1e3 * v[0] / steps, 3),
                    "alg_gflop_per_launch": round(v[1] / v[2] / 1e9, 3), "alg_bytes_per_launch": round(v[3] / v[2]), "tflops": round(v[1] / v[0] / 1e12, 1),
                    "frac": round(v[1] / v[0] / 1e12 / peak_tflops, 4)}
        ordered = sorted(rows.items(), key=lambda kv: -kv[1][0])
        top_name, top = ordered[0]
        t_all = sum(v[0] for v in rows.values()); f_all = sum(v[1] for v in rows.values())
        achieved = top[1] / top[0] / 1e12
        return {"bound": "mfma", "kernel": top_name, "achieved": round(achieved, 2), "peak": peak_tflops, "unit": "TFLOP/s",
                "frac": round(achieved / peak_tflops, 5), "traffic": None, "launches": round(top[2] / steps, 1), "avg_launch_ms": round(1e3 * top[0] / top[2], 5),
                "alg_gflop_per_launch": round(top[1] / top[2] / 1e9, 3), "alg_bytes_per_launch": round(top[3] / top[2]),
                "event_bracket_overhead_us": round(ovh * 1e6, 2),
                "rows": [row(n, v) for n, v in ordered[:8]],
                "gemm_family_total": {"ms_per_step": round(1e3 * t_all / steps, 3), "tflops": round(f_all / t_all / 1e12, 1), "frac": round(f_all / t_all / 1e12 / peak_tflops, 4)},
                "families": {self.NAMES.get(k, str(k)): {"ms_total": round(1e3 * v[0] / steps, 3), "tflops": round(v[1] / v[0] / 1e12, 2), "launches": round(v[2] / steps, 1)}
                             for k, v in sorted(agg.items(), key=lambda kv: -kv[1][0])}}


KERNEL_TIMER = KernelTimer()


def _p(t):
    return None if t is None else t.data_ptr()


def _rng(device, drop_p=1.0):
    """the RNG state pointer for a launch that drops with probability drop_p; None when it draws nothing (launches that always draw leave drop_p out)"""
    return rt.rng_state(device).data_ptr() if drop_p > 0 else None


# ---- step stamps (measurement aid, AVEC_STAMPS=1): wall-clock marks written by one-wave kernels at named points of the forward and backward passes, on whatever stream the
# point runs on -- they replay with the captured graph, so tools/step_stamps.py sees the real overlap of the two branch streams without a profiler ----
STAMPS = {"on": os.environ.get("AVEC_STAMPS", "0") == "1", "buf": None, "names": []}


def stamp(name):
    if not STAMPS["on"]:
        return
    if STAMPS["buf"] is None:
        STAMPS["buf"] = torch.zeros(256, dtype=torch.int64, device="cuda")
    if name not in STAMPS["names"]:
        STAMPS["names"].append(name)
    lib.stamp(STAMPS["buf"].data_ptr(), STAMPS["names"].index(name), rt.stream())


class StampFn(torch.autograd.Function):
    """identity; stamps `name:f` when the forward pass gets here and `name:b` when the gradient comes back"""

    @staticmethod
    def forward(ctx, x, name):
        ctx.name = name
        stamp(name + ":f")
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        stamp(ctx.name + ":b")
        return g, None


def mark(x, name):
    return StampFn.apply(x, name) if (STAMPS["on"] and torch.is_tensor(x) and x.requires_grad) else (stamp(name + ":f") or x)


def grad_of(p):
    """fp32 gradient buffer of a parameter (same physical layout), created on first use."""
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    return p.grad


def empty(shape, dtype, ref):
    """uninitialised device tensor.  16-bit matrices whose row is not a whole number of 16-byte chunks (the 180-channel audio stage) get 16 readable bytes behind
    the last row: the LDS-DMA kernels fetch whole chunks (avec_gemm_tn_grouped)."""
    if dtype == torch.bfloat16 and len(shape) == 2 and shape[1] % 8:
        n = shape[0] * shape[1]
        return torch.empty(n + 8, dtype=dtype, device=ref.device)[:n].view(shape)
    return torch.empty(shape, dtype=dtype, device=ref.device)


def _chunk_readable(t, ld, width, rows):
    """rows of `width` 16-bit elements at stride `ld`: may the kernels read whole 8-element chunks behind the last row?"""
    if width % 8 == 0 and ld % 8 == 0 and t.data_ptr() % 16 == 0:
        return True
    if ld >= (width + 7) // 8 * 8:
        return True
    st = t.untyped_storage()
    end = (t.storage_offset() + (rows - 1) * ld + (width + 7) // 8 * 8) * t.element_size()
    return end <= st.nbytes()


def rows_plain(ld, rows_out=1, rows_in=1, step=0):
    r = Rows()
    r.ld, r.rows_out, r.rows_in, r.step = ld, rows_out, rows_in, step
    return r


def rows_conv(H, W, C, KH, KW, stride, pad, OH, OW):
    r = Rows()
    r.H, r.W, r.C, r.KH, r.KW, r.stride, r.pad, r.OH, r.OW = H, W, C, KH, KW, stride, pad, OH, OW
    return r


def gemm_nt_fp8(A, ent, out, M, N, K, *, bias=None, act=ACT_NONE, out_pre=None, drop_p=0.0, sid=0, res=None, alpha=1.0, out_f32=False, ldo=None):
    """forward Linear product on e4m3 operands (avec_amd/fp8.py): quantize the bf16 activation with its own max|x|, then avec_gemm_nt_fp8"""
    Kp = ent.Kp
    q = torch.empty((M, Kp), dtype=torch.uint8, device=A.device)
    lib.fp8_quantize(rt.dt(), A.data_ptr(), K, q.data_ptr(), Kp, M, K, ent.a_amax, 1, rt.stream())
    ep = Epilogue()
    ep.out, ep.ldo, ep.out_f32 = out.data_ptr(), (N if ldo is None else ldo), int(out_f32)
    if out_pre is not None:
        ep.out_pre, ep.ldpre = out_pre.data_ptr(), N
    ep.bias, ep.act, ep.alpha = _p(bias), act, alpha
    if drop_p > 0.0:
        ep.drop_p, ep.rng, ep.rng_stream = drop_p, _rng(out.device, drop_p), sid
    if res is not None:
        ep.res, ep.ldres, ep.res_act = res.data_ptr(), N, 0
    ev = KERNEL_TIMER.start()
    lib.gemm_nt_fp8(q.data_ptr(), Kp, ent.wq, Kp, M, N, Kp, ent.a_amax, ent.w_amax, _byref(ep), rt.stream())
    KERNEL_TIMER.stop(ev, (0, 0), 2.0 * M * N * K)
    return out


def gemm_nt(A, W, out, M, N, K, *, rows=None, mode=ROWS_PLAIN, a_f32=False, ldw=None, bias=None, act=ACT_NONE, out_pre=None,
            drop_p=0.0, sid=0, res=None, res_act=False, alpha=1.0, dact_z=None, dact=0, colsum=None, stats=None, out_f32=False,
            ldo=None, ldres=None, dtype=None, flops=None, bnb=None, res_cls0=False, abytes=None, res_mask=None):
    ep = Epilogue()
    ep.out, ep.ldo, ep.out_f32 = out.data_ptr(), (N if ldo is None else ldo), int(out_f32)
    if out_pre is not None:
        ep.out_pre, ep.ldpre = out_pre.data_ptr(), N
    ep.bias = _p(bias)
    ep.act = act
    if drop_p > 0.0:
        ep.drop_p, ep.rng, ep.rng_stream = drop_p, _rng(out.device, drop_p), sid
    if res is not None:
        ep.res, ep.ldres, ep.res_act, ep.res_cls0 = res.data_ptr(), (N if ldres is None else ldres), int(res_act), int(res_cls0)
        if res_mask is not None:
            ep.res_mask = res_mask.data_ptr()
    ep.alpha = alpha
    if dact_z is not None:
        ep.dact_z, ep.ldz, ep.dact = dact_z.data_ptr(), N, dact
    ep.colsum, ep.stats = _p(colsum), _p(stats)
    if bnb is not None:       # BatchNorm-backward fusion (avec_hip.h): (y, ss | None, mask tensor | None, replicated stats)
        ep.bnb_y, ep.ldby, ep.stats = bnb.y.data_ptr(), N, bnb.stats.data_ptr()
        if bnb.mask_z is not None:
            ep.dact_z, ep.ldz, ep.dact, ep.bnb_mask = bnb.mask_z.data_ptr(), N, 2, 0
        else:
            ep.bnb_ss, ep.bnb_mask = bnb.ss.data_ptr(), 1
    if rows is None:
        rows = rows_plain(K)
    ev = KERNEL_TIMER.start()
    lib.gemm_nt(rt.dt() if dtype is None else dtype, A.data_ptr(), _byref(rows), mode, int(a_f32), W.data_ptr(),
                K if ldw is None else ldw, M, N, K, _byref(ep), rt.stream())
    esz = A.element_size()
    KERNEL_TIMER.stop(ev, (0, mode), 2.0 * M * N * K if flops is None else flops,
                      ((M * K + N * K) * esz + M * N * (4 if out_f32 else esz)) if abytes is None else abytes)
    return out


# (The module-level switches of this file are plain constants, not environment switches (DEFER_WGRAD alone also reads AVEC_DEFER_WGRAD); each alternative is kept for
# the test or tool that flips it in-process: DEFER_WGRAD tests/test_gpu_backward_state.py; LN_PAIR tests/test_gpu_round4.py; RELU_BITMASK, SHORTCUT_SUBGRID,
# GROUP_WGRAD128, BNB_FUSE tests/test_gpu_round3.py; CONVMOD_BN_FUSE tests/test_gpu_convmod_bn.py; STEM3D_DIRECT, STEM3P, STEM3P_FUSED_WGRAD tests/test_gpu_parity.py
# and tools/bench_stem.py.)
# ---- deferred parameter gradients ------------------------------------------------------------------------------------------------------------
# Weight gradients (dW = dY^T X), bias gradients and LayerNorm gamma/beta gradients only feed the optimizer: nothing in the backward chain waits for
# them.  Launched one by one they are ~45 % of a conformer block's backward launches, each latency-bound (a few hundred workgroups, 12-21 us).  Inside a
# backward pass they are therefore QUEUED per stream (the operand tensors stay referenced) and submitted as grouped launches (avec_gemm_tn_grouped,
# avec_layernorm_param_grads_grouped: one grid over the tiles of up to 32 / 40 products) when a queue fills, at the explicit flush points (end of the audio
# branch, before an early gradient all-reduce) and by a final autograd callback when the backward pass ends.  ops.DEFER_WGRAD = False restores immediate launches.
DEFER_WGRAD = os.environ.get("AVEC_DEFER_WGRAD", "1") != "0"


# one kind of queued launch: its ctypes item, the most items one launch takes, the grouped entry point (lib name) and the dtype argument in front of its items (a
# callable, or None: the entry point takes none), the KERNEL_TIMER key (None: not timed), the ALGORITHMIC bytes of one item, and whether a push that fills a group
# launches it at once
_QueueKind = collections.namedtuple("_QueueKind", "item group_max launcher dtype timer_key abytes flush_when_full")


def _wgrad3x3_bytes(it):
    return 2.0 * 2 * it.images * it.H * it.W * it.C + 4.0 * 9 * it.C * it.C      # x, dy once (bf16) + dW once (fp32)


# in launch order.  cw / cw64: 3x3 weight gradients of the wide ResNet layers / of the 64-channel layers, launched when the pass is through
_QUEUE_KINDS = {
    "tn": _QueueKind(TnItem, TN_GROUP_MAX, "gemm_tn_grouped", lambda: BF16, (1, ROWS_PLAIN), lambda it: 2.0 * it.M * (it.I + it.J) + 4.0 * it.I * it.J, True),      # P, Q once (bf16) + dW once (fp32)
    "ln": _QueueKind(LnItem, LN_GROUP_MAX, "layernorm_param_grads_grouped", rt.dt, None, None, True),
    "cw": _QueueKind(WgradItem, WGRAD_GROUP_MAX, "wgrad3x3_c128_grouped", None, (2, 2), _wgrad3x3_bytes, False),
    "cw64": _QueueKind(WgradItem, WGRAD_GROUP_MAX, "wgrad3x3_c64_grouped", None, (2, 2), _wgrad3x3_bytes, False),
}


class _PendingGrads:
    """the queued launches of one stream: items and algorithmic FLOPs per kind, and the operand tensors (`keep`) that must outlive the launches"""
    __slots__ = ("stream", "items", "flops", "keep")

    def __init__(self, stream):
        self.stream = stream
        self.clear()

    def clear(self):
        self.items, self.flops, self.keep = {k: [] for k in _QUEUE_KINDS}, dict.fromkeys(_QUEUE_KINDS, 0.0), []

    def push(self, kind, item, keep, flops=0.0):
        self.items[kind].append(item)
        self.keep += keep
        self.flops[kind] += flops
        if _QUEUE_KINDS[kind].flush_when_full and len(self.items[kind]) >= _QUEUE_KINDS[kind].group_max:
            self.flush((kind,))

    def flush(self, kinds=None):
        """submit on the CURRENT stream (the queue's own stream during the pass; the caller's stream, which has joined every branch, at the end of it)"""
        cur = torch.cuda.current_stream()
        if cur.cuda_stream != self.stream.cuda_stream:
            for t in self.keep:
                t.record_stream(cur)
        for kind in (_QUEUE_KINDS if kinds is None else kinds):
            k, items = _QUEUE_KINDS[kind], self.items[kind]
            if not items:
                continue
            ev = KERNEL_TIMER.start() if k.timer_key is not None else None
            for i in range(0, len(items), k.group_max):
                chunk = items[i:i + k.group_max]
                getattr(lib, k.launcher)(*(() if k.dtype is None else (k.dtype(),)), (k.item * len(chunk))(*chunk), len(chunk), rt.stream())
            if ev is not None:          # (the byte count walks the items: only while timing)
                KERNEL_TIMER.stop(ev, k.timer_key, self.flops[kind], sum(k.abytes(it) for it in items))
            self.items[kind], self.flops[kind] = [], 0.0
        if not any(self.items.values()):
            self.keep = []


class _BackwardPass:
    """everything one backward pass leaves between its autograd nodes"""
    __slots__ = ("task", "queues", "prep", "ln2", "pos", "bn_ready")

    def __init__(self, task):
        self.task = task
        self.queues = {}        # stream handle -> _PendingGrads
        self.prep = {}          # address of a LayerNorm's dx -> the prepared gradient made with it (see _take_prep)
        self.ln2 = {}           # address of a feed-forward module's dx -> the dx of the LayerNorm in front of it (see LN_PAIR)
        self.pos = {}           # _PosGroupEntry -> [the group's shared dE accumulator, layers still to arrive] (see _pos_group_backward)
        self.bn_ready = {}      # address of a ResNet block's dx -> the completed BatchNorm-backward request of the block in front (see ResNetBlockFn)

    def pending(self):
        """the queue of the current stream"""
        st = torch.cuda.current_stream()
        q = self.queues.get(st.cuda_stream)
        if q is None:
            q = self.queues[st.cuda_stream] = _PendingGrads(st)
        return q


_PASS = None


def _pass():
    """state of the backward pass that is running; None outside one"""
    global _PASS
    task = torch._C._current_graph_task_id()
    if task == -1:
        return None
    if _PASS is None or _PASS.task != task:
        # first use in this backward pass.  A state that is still here belongs to a pass that never reached its end-of-pass callback (it raised midway): its
        # queued products, hand-overs and group counters belong to another batch and must not reach this step's gradients -- dropped as a whole
        _PASS = _BackwardPass(task)
        torch.autograd.Variable._execution_engine.queue_callback(_flush_at_end)      # flush whatever is left when the pass ends
    return _PASS


def _in_backward():
    return DEFER_WGRAD and torch._C._current_graph_task_id() != -1


def reset_backward_state():
    """forget everything a backward pass leaves between its nodes (queued parameter-gradient products, hand-over tables, position-group counters): called when a pass
    was aborted (a graph capture that failed midway) before the step is run again"""
    global _PASS
    _PASS = None


def flush_param_grads(all_streams=False):
    """submit the queued parameter-gradient work of the current stream (all_streams: of every stream, on the current one)"""
    if _PASS is None:
        return
    if all_streams:
        for q in list(_PASS.queues.values()):
            q.flush()
        return
    q = _PASS.queues.get(torch.cuda.current_stream().cuda_stream)
    if q is not None:
        q.flush()


def _flush_at_end():
    global _PASS
    flush_param_grads(all_streams=True)
    _PASS = None


def gemm_tn(P, Q, O, M, I, J, *, ldp=None, q_rows=None, q_mode=ROWS_PLAIN, q_f32=False, ldo=None, dtype=None, p_colsum=None, side=False):
    """O[I][J] (fp32) += P[M][I]^T Q[M][J];  optionally p_colsum[I] += column sums of P (the bias gradient, fused into the same launch).
    side=True (weight gradients): may be queued for a grouped launch (see above) / launched on the side stream (runtime.wgrad_fork)."""
    if q_rows is None:
        q_rows = rows_plain(J)
    if side and q_mode == ROWS_PLAIN and q_f32 and dtype is None and rt.compute_dtype() == "bf16" and _in_backward() and Q.dim() == 2 and Q.dtype == torch.float32:
        # fp32 activations (a layer fed by the residual stream): one cast launch, then the product joins the grouped launch like any other -- instead of a
        # launch of its own on the register-staged kernel plus a column-sum / col_finalize pair for its bias (same rounding: that kernel casts while staging)
        Qb = empty((Q.shape[0], J), rt.act_dtype(), Q)
        lib.cast_rows(rt.dt(), Q.data_ptr(), q_rows.ld, Qb.data_ptr(), J, Q.shape[0], J, rt.stream())
        Q, q_f32, q_rows = Qb, False, rows_plain(J, q_rows.rows_out, q_rows.rows_in, q_rows.step)
    if side and q_mode == ROWS_PLAIN and not q_f32 and dtype is None and rt.compute_dtype() == "bf16" and _in_backward():
        it = TnItem()
        it.P, it.Q, it.O, it.p_colsum = P.data_ptr(), Q.data_ptr(), O.data_ptr(), _p(p_colsum)
        it.ldp, it.ldq, it.ldo, it.M, it.I, it.J = (I if ldp is None else ldp), q_rows.ld, (J if ldo is None else ldo), M, I, J
        it.q_rows_out, it.q_rows_in, it.q_step = q_rows.rows_out, q_rows.rows_in, q_rows.step
        if lib.raw("avec_gemm_tn_grouped_ok")(BF16, _byref(it)) and _chunk_readable(P, it.ldp, I, M) and _chunk_readable(Q, it.ldq, J, M):
            _pass().pending().push("tn", it, [P, Q], 2.0 * M * I * J)
            return
    ev = KERNEL_TIMER.start()
    st = rt.stream()
    if side and not KERNEL_TIMER.enabled:
        sd = rt.wgrad_fork(P, Q)
        st = st if sd is None else sd.cuda_stream
    lib.gemm_tn_bias(rt.dt() if dtype is None else dtype, P.data_ptr(), I if ldp is None else ldp, Q.data_ptr(), _byref(q_rows), q_mode,
                     int(q_f32), O.data_ptr(), J if ldo is None else ldo, _p(p_colsum), M, I, J, st)
    KERNEL_TIMER.stop(ev, (1, q_mode), 2.0 * M * I * J, (M * I + M * J) * 2.0 + I * J * 4.0)


def layernorm_fwd(x, w, b, M, D, out_f32, eps):
    y = empty((M, D), torch.float32 if out_f32 else rt.act_dtype(), x)
    mean = empty((M,), torch.float32, x)
    rstd = empty((M,), torch.float32, x)
    lib.layernorm_fwd(rt.dt(), x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), int(out_f32), mean.data_ptr(), rstd.data_ptr(), M, D, eps,
                      rt.stream())
    return y, mean, rstd


# ---- the first launch of a module's backward, folded into the last launch of the module behind it -----------------------------------------------------
# Every residual module computes  out = x + alpha * Dropout(f(LN(x)))  and starts its backward with  dacc = act(alpha * dropmask * dy)  (avec_grad_prep: ~100
# launches per step).  dy is the dx that the NEXT module's LayerNorm backward wrote a moment ago -- so that kernel writes dacc as a second output
# (avec_layernorm_bwd_prep).  Forward: a module tags its output tensor with (alpha, drop_p, rng stream); the consumer module remembers the tag of its input.
# Backward: the consumer's LayerNorm backward produces the prepared gradient and leaves it under dx's address; the producer module takes it if the address, the
# backward pass, the shape and its own (alpha, drop_p, stream) all match, and launches grad_prep otherwise (gradient accumulated from several consumers, ...).
def _tag_prep(out, alpha, drop_p, sid):
    out._avec_prep = (float(alpha), float(drop_p), int(sid))
    return out


def _prep_request(x):
    return getattr(x, "_avec_prep", None)


def _take_prep(dy, M, N, alpha, drop_p, sid):
    p = _pass()
    r = None if p is None else p.prep.pop(dy.data_ptr(), None)
    if r is not None and r[1:] == (M, N, float(alpha), float(drop_p), int(sid)) and r[0].dtype == rt.act_dtype():
        return r[0]
    return None


def layernorm_bwd(dy, dy_f32, x, mean, rstd, w, b, M, D, dres=None, prep=None):
    """prep = (alpha, drop_p, rng stream) of the module whose output this LayerNorm normalised: also produce its prepared gradient (see above)"""
    dx = empty((M, D), torch.float32, x)
    gw, gb = grad_of(w), grad_of(b)
    if D <= 1024 and D % 4 == 0 and _in_backward():          # (the dx-only kernel and the grouped launch use 4-wide accesses) dx now (one wave per row); d(gamma), d(beta) with the other queued parameter gradients
        if prep is not None:
            pt = empty((M, D), rt.act_dtype(), x)
            alpha, drop_p, sid = prep
            lib.layernorm_bwd_prep(rt.dt(), dy.data_ptr(), int(dy_f32), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), dx.data_ptr(), _p(dres),
                                   pt.data_ptr(), alpha, drop_p, _rng(x.device, drop_p), sid, M, D, rt.stream())
            _pass().prep[dx.data_ptr()] = (pt, M, D, alpha, drop_p, sid)
        else:
            lib.layernorm_bwd(rt.dt(), dy.data_ptr(), int(dy_f32), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), dx.data_ptr(), _p(dres),
                              None, None, M, D, rt.stream())
        defer_ln_param_grads(dy, dy_f32, x, mean, rstd, w, b, M, D)
        return dx
    lib.layernorm_bwd(rt.dt(), dy.data_ptr(), int(dy_f32), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), w.data_ptr(), dx.data_ptr(), _p(dres),
                      gw.data_ptr(), gb.data_ptr(), M, D, rt.stream())
    return dx


def layernorm_bwd_pair(dy2, x2, mean2, rstd2, w2, b2, dres2, x1, mean1, rstd1, w1, req1, ctx1, M, D):
    """LayerNorm backward of a module's pre-norm (dy2: act, residual gradient dres2) AND of the LayerNorm that produced its input (LayerNormFn ctx1; req1 = the prepared
    gradient wanted by the module in front of that one): one launch; returns dx2 and leaves dx1 for LayerNormFn.backward (see LN_PAIR)"""
    dx2, dx1 = empty((M, D), torch.float32, x2), empty((M, D), torch.float32, x2)
    pt, alpha, drop_p, sid = None, 1.0, 0.0, 0
    if req1 is not None:
        pt = empty((M, D), rt.act_dtype(), x2)
        alpha, drop_p, sid = req1
        _pass().prep[dx1.data_ptr()] = (pt, M, D, alpha, drop_p, sid)
    lib.layernorm_bwd2(rt.dt(), dy2.data_ptr(), x2.data_ptr(), mean2.data_ptr(), rstd2.data_ptr(), w2.data_ptr(), dres2.data_ptr(), dx2.data_ptr(),
                       x1.data_ptr(), mean1.data_ptr(), rstd1.data_ptr(), w1.data_ptr(), dx1.data_ptr(), _p(pt), alpha, drop_p, _rng(x2.device, drop_p), sid, M, D,
                       rt.stream())         # (drop_p is 0 without a request)
    _pass().ln2[dx2.data_ptr()] = (dx1, ctx1, dx2, dx2._version)
    defer_ln_param_grads(dy2, False, x2, mean2, rstd2, w2, b2, M, D)
    return dx2


def grad_prep(dout, M, N, alpha=1.0, drop_p=0.0, sid=0, dbias=None):
    dacc = empty((M, N), rt.act_dtype(), dout)
    lib.grad_prep(rt.dt(), dout.data_ptr(), N, dacc.data_ptr(), alpha, drop_p, _rng(dout.device, drop_p), sid, _p(dbias), M, N, rt.stream())
    return dacc


def colsum(x, ld, out, M, N):
    lib.colsum(rt.dt(), x.data_ptr(), ld, out.data_ptr(), M, N, rt.stream())


def _f32c(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()




# ============================================================================================
# Linear family
# ============================================================================================
def linear_fwd(x2d, weight, bias, M, *, in_f32, out_f32, act=ACT_NONE, out_pre=None, drop_p=0.0, sid=0, res=None, alpha=1.0,
               rows=None, K=None):
    sh = rt.shadow(weight)
    N, Kw = sh.A, sh.Tm * sh.C
    out = empty((M, N), torch.float32 if out_f32 else rt.act_dtype(), x2d)
    ent = fp8.entry(weight, Kw) if (rows is None and not in_f32 and sh.group is None) else None
    if ent is not None and ent.N == N:
        return gemm_nt_fp8(x2d, ent, out, M, N, Kw, bias=bias, act=act, out_pre=out_pre, drop_p=drop_p, sid=sid, res=res, alpha=alpha, out_f32=out_f32)
    gemm_nt(x2d, sh.fwd, out, M, N, Kw, rows=rows, a_f32=in_f32, bias=bias, act=act, out_pre=out_pre, drop_p=drop_p, sid=sid,
            res=res, alpha=alpha, out_f32=out_f32)
    return out


def linear_bwd_weight(dacc, x2d, weight, M, *, q_f32=False, q_rows=None, ldp=None, bias=None):
    """dW += dacc^T x;  with `bias`: db += column sums of dacc, out of the same GEMM launch"""
    sh = rt.shadow(weight)
    gemm_tn(dacc, x2d, grad_of(weight), M, sh.A, sh.Tm * sh.C, q_f32=q_f32, q_rows=q_rows, ldp=ldp, p_colsum=None if bias is None else grad_of(bias), side=True)


def linear_bwd_input(dacc, weight, M, *, out_f32, res=None, res_act=False, dact_z=None, dact=0, drop_p=0.0, sid=0, colsum_to=None, lda=None, out=None):
    sh = rt.shadow(weight)
    N, K = sh.Tm * sh.C, sh.A            # bwd shadow is [C*Tm][A]
    if out is None:
        out = empty((M, N), torch.float32 if out_f32 else rt.act_dtype(), dacc)
    gemm_nt(dacc, sh.bwd, out, M, N, K, rows=rows_plain(K if lda is None else lda), ldw=sh.ldb, res=res, res_act=res_act, dact_z=dact_z, dact=dact,
            drop_p=drop_p, sid=sid, colsum=colsum_to, out_f32=out_f32)
    return out


class LinearFn(torch.autograd.Function):
    """layers.Linear.forward (nnet/layers.py:64-76): y = x W^T + b.  x fp32 or act; y fp32 or act."""

    @staticmethod
    def forward(ctx, x, weight, bias, in_f32, out_f32):
        rt.require_gpu(x)
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        M = x2.shape[0]
        y = linear_fwd(x2, weight, bias, M, in_f32=in_f32, out_f32=out_f32)
        ctx.saved = (x2, weight, bias, in_f32, out_f32, M, shp)
        return y.view(*shp[:-1], y.shape[-1])

    @staticmethod
    def backward(ctx, dy):
        x2, weight, bias, in_f32, out_f32, M, shp = ctx.saved
        N = weight.shape[0]
        dy = dy.reshape(M, N)
        dy = dy if dy.is_contiguous() else dy.contiguous()
        dacc = grad_prep(dy, M, N) if out_f32 else dy
        linear_bwd_weight(dacc, x2, weight, M, q_f32=in_f32, bias=bias)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = linear_bwd_input(dacc, weight, M, out_f32=in_f32).view(shp)
        return dx, None, None, None, None


def linear(x, weight, bias, out_f32=True):
    """x fp32 (converted while staging in bf16 mode) or act; returns fp32 by default."""
    if rt.compute_dtype() == "f32":
        return LinearFn.apply(x.float(), weight, bias, False, True)
    if x.dtype == torch.float32:
        return LinearFn.apply(x, weight, bias, True, out_f32)
    return LinearFn.apply(x.to(rt.act_dtype()), weight, bias, False, out_f32)


# ---- two consecutive LayerNorms as one launch per pass (round 4) --------------------------------------------------------------------------------------------
# The LayerNorm that closes a ConformerBlock is followed at once by the pre-norm of the next block's first feed-forward module: rows are independent, so the closing
# norm's launch also produces the next one's output (avec_layernorm_fwd2) and leaves it on its result tensor; FeedForwardFn picks it up when the tensor, the
# parameters and eps are the ones it was made for.  Backward: the feed-forward module's LayerNorm backward also runs the closing norm's (avec_layernorm_bwd2) and
# leaves dx1 under the address of the gradient it returns; LayerNormFn.backward takes it if that very tensor comes back from autograd (one consumer), else computes.
LN_PAIR = True


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm over the last dim of an fp32 tensor -> fp32.  nxt = (weight, bias, eps) of a LayerNorm that will read the result next (see above)."""

    @staticmethod
    def forward(ctx, x, w, b, eps, nxt=None):
        rt.require_gpu(x)
        shp = x.shape
        pair = None
        x2 = _f32c(x.reshape(-1, shp[-1]))
        M, D = x2.shape
        if nxt is not None and LN_PAIR and D <= 512 and D % 4 == 0:
            w2, b2, eps2 = nxt
            y, mean, rstd = empty((M, D), torch.float32, x2), empty((M,), torch.float32, x2), empty((M,), torch.float32, x2)
            h2, mean2, rstd2 = empty((M, D), rt.act_dtype(), x2), empty((M,), torch.float32, x2), empty((M,), torch.float32, x2)
            lib.layernorm_fwd2(rt.dt(), x2.data_ptr(), w.data_ptr(), b.data_ptr(), eps, y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                               w2.data_ptr(), b2.data_ptr(), eps2, h2.data_ptr(), mean2.data_ptr(), rstd2.data_ptr(), M, D, rt.stream())
            pair = (h2, mean2, rstd2, w2.data_ptr(), float(eps2), M, D, ctx)
        else:
            y, mean, rstd = layernorm_fwd(x2, w, b, M, D, True, eps)
        ctx.saved = (x2, mean, rstd, w, b, M, D, shp, _prep_request(x))
        out = y.view(shp)
        if pair is not None:
            out._avec_ln2 = pair
        return out

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd, w, b, M, D, shp, req = ctx.saved
        p = _pass()
        if p is not None:
            r = p.ln2.pop(dy.data_ptr(), None)
            # the feed-forward module behind has done this LayerNorm's backward already -- valid only if dy still IS its dx2 (same storage, not accumulated into since:
            # a second consumer of this norm's output makes autograd add its gradient in place, which bumps the version counter)
            if r is not None and r[1] is ctx and dy.dtype == torch.float32 and dy.is_contiguous() and (dy is r[2] or dy._base is r[2]) and r[2]._version == r[3]:
                defer_ln_param_grads(dy.reshape(M, D), True, x2, mean, rstd, w, b, M, D)
                return r[0].view(shp), None, None, None, None
        dx = layernorm_bwd(_f32c(dy.reshape(M, D)), True, x2, mean, rstd, w, b, M, D, prep=req)
        return dx.view(shp), None, None, None, None


class ActivationFn(torch.autograd.Function):
    """stand-alone Swish / ReLU / GLU(dim=-1) (nnet/activations.py:39-69) on fp32 device tensors"""

    @staticmethod
    def forward(ctx, x, act, dim):
        rt.require_gpu(x)
        assert act in (1, 2, 3)
        assert act != 3 or dim in (-1, x.dim() - 1), "GLU over the last axis"
        x2 = _f32c(x)
        C = x2.shape[-1] // 2 if act == 3 else x2.shape[-1]
        assert act != 3 or x2.shape[-1] == 2 * C, "GLU needs an even last axis"
        rows = x2.numel() // x2.shape[-1]
        y = torch.empty(x2.shape[:-1] + (C,), dtype=torch.float32, device=x2.device)
        lib.act_f32(act, x2.data_ptr(), None, y.data_ptr(), rows, C, 0, rt.stream())
        ctx.saved = (x2, act, rows, C)
        return y.to(x.dtype) if x.dtype != torch.float32 else y

    @staticmethod
    def backward(ctx, dy):
        x2, act, rows, C = ctx.saved
        dyc = _f32c(dy)
        dx = torch.empty_like(x2)
        lib.act_f32(act, x2.data_ptr(), dyc.data_ptr(), dx.data_ptr(), rows, C, 1, rt.stream())
        return dx, None, None


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, sid):
        x = _f32c(x)
        y = torch.empty_like(x)
        lib.dropout_f32(x.data_ptr(), y.data_ptr(), p, _rng(x.device), sid, x.numel(), rt.stream())
        ctx.saved = (p, sid)
        return y

    @staticmethod
    def backward(ctx, dy):
        p, sid = ctx.saved
        dy = _f32c(dy)
        dx = torch.empty_like(dy)
        lib.dropout_f32(dy.data_ptr(), dx.data_ptr(), p, _rng(dy.device), sid, dy.numel(), rt.stream())
        return dx, None, None


# ============================================================================================
# FeedForwardModule (nnet/modules.py:257-289) fused with its macaron residual (nnet/blocks.py:292,301)
#   y = x + alpha * Drop(W2 Drop(Swish(W1 LN(x) + b1)) + b2)
# ============================================================================================
def defer_ln_param_grads(dy, dy_f32, x, mean, rstd, w, b, M, D):
    """queue d(gamma), d(beta) of a LayerNorm whose input gradient was computed elsewhere (inside a backward pass), or compute them now"""
    it = LnItem()
    it.dy, it.x, it.mean, it.rstd, it.dgamma, it.dbeta = dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), grad_of(w).data_ptr(), grad_of(b).data_ptr()
    it.M, it.D, it.dy_f32 = M, D, int(dy_f32)
    if _in_backward() and D % 4 == 0 and D <= 1024:
        _pass().pending().push("ln", it, [dy, x, mean, rstd])
    else:
        lib.layernorm_param_grads_grouped(rt.dt(), (LnItem * 1)(it), 1, rt.stream())


class FeedForwardFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ln_w, ln_b, w1, b1, w2, b2, eps, alpha, drop_p, sid1, sid2):
        rt.require_gpu(x)
        shp = x.shape
        x2 = _f32c(x.reshape(-1, shp[-1]))
        M, D = x2.shape
        F = w1.shape[0]
        adt = rt.act_dtype()
        ln_prev = None
        pre = getattr(x, "_avec_ln2", None)
        if pre is not None and pre[3] == ln_w.data_ptr() and pre[4] == float(eps) and pre[5:7] == (M, D) and x2.data_ptr() == x.data_ptr() and pre[0].dtype == adt:
            h0, mean, rstd = pre[0], pre[1], pre[2]          # made by the LayerNorm launch that produced x (LayerNormFn, nxt)
            ln_prev = pre[7]
        else:
            h0, mean, rstd = layernorm_fwd(x2, ln_w, ln_b, M, D, False, eps)
        z = empty((M, F), adt, x2)
        h1 = linear_fwd(h0, w1, b1, M, in_f32=False, out_f32=False, act=ACT_SWISH, out_pre=z, drop_p=drop_p, sid=sid1)
        y = linear_fwd(h1, w2, b2, M, in_f32=False, out_f32=True, drop_p=drop_p, sid=sid2, res=x2, alpha=alpha)
        ctx.saved = (x2, mean, rstd, h0, z, h1, ln_w, ln_b, w1, b1, w2, b2, alpha, drop_p, sid1, sid2, M, D, F, shp)
        ctx.prep_req = _prep_request(x)
        ctx.ln_prev = ln_prev
        return _tag_prep(y.view(shp), alpha, drop_p, sid2)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd, h0, z, h1, ln_w, ln_b, w1, b1, w2, b2, alpha, drop_p, sid1, sid2, M, D, F, shp = ctx.saved
        dy = _f32c(dy.reshape(M, D))
        dacc = _take_prep(dy, M, D, alpha, drop_p, sid2)
        if dacc is None:
            dacc = grad_prep(dy, M, D, alpha=alpha, drop_p=drop_p, sid=sid2)
        linear_bwd_weight(dacc, h1, w2, M, bias=b2)
        dz = linear_bwd_input(dacc, w2, M, out_f32=False, dact_z=z, dact=ACT_SWISH, drop_p=drop_p, sid=sid1)
        linear_bwd_weight(dz, h0, w1, M, bias=b1)
        dh0 = linear_bwd_input(dz, w1, M, out_f32=False)
        pv = ctx.ln_prev
        if pv is not None and _in_backward() and D <= 512 and D % 4 == 0 and dh0.dtype == rt.act_dtype():
            x1, mean1, rstd1, w1n, b1n, M1, D1, shp1, req1 = pv.saved
            if (M1, D1) == (M, D):
                return (layernorm_bwd_pair(dh0, x2, mean, rstd, ln_w, ln_b, dy, x1, mean1, rstd1, w1n, req1, pv, M, D).view(shp),) + (None,) * 11
        dx = layernorm_bwd(dh0, False, x2, mean, rstd, ln_w, ln_b, M, D, dres=dy, prep=ctx.prep_req)
        return (dx.view(shp),) + (None,) * 11


# ============================================================================================
# AttentionModule (nnet/modules.py:320-339) with RelPos1d / RelPosPatch1d attention (nnet/attentions.py:280-382)
#   y = x + Drop(Wo . Attn(LN(x)) + bo)
# ============================================================================================
_PE_CACHE = {}


def rel_pos_table(T, D, device):
    """RelativeSinusoidalPositionalEncoding rows p = T-1 .. -(T-1) (nnet/embeddings.py:117-126,152), act dtype."""
    key = (T, D, str(device), rt.compute_dtype())
    if key not in _PE_CACHE:
        pos = torch.arange(T - 1, -T, -1, dtype=torch.float32).unsqueeze(1)
        inv = 10000 ** (2 * torch.arange(0, D // 2, dtype=torch.float32).unsqueeze(0) / D)
        ang = pos / inv
        pe = torch.zeros(2 * T - 1, D)
        pe[:, 0::2] = ang.sin()
        pe[:, 1::2] = ang.cos()
        _PE_CACHE[key] = pe.to(device=device, dtype=rt.act_dtype()).contiguous()
    return _PE_CACHE[key]


def _attn_args(qkv, e, lens, len_div, mask, o, lse, B, H, T, d, D, q_full=0, *, kv=None, Tk=0, scale=None):
    """the forward fields of an Attn.  qkv: packed [B*T][3D] = q | k | v; or, with kv = (k, v, row stride) -- the key/value-cache form, Tk keys per sequence --, q
    alone at the same row stride.  scale: 1 / sqrt(d) unless given."""
    a = Attn()
    a.q_full = q_full
    if kv is None:
        esz = qkv.element_size()
        a.q, a.k, a.v, a.ld = qkv.data_ptr(), qkv.data_ptr() + D * esz, qkv.data_ptr() + 2 * D * esz, 3 * D
    else:
        a.q, a.k, a.v, a.ld = qkv.data_ptr(), kv[0].data_ptr(), kv[1].data_ptr(), kv[2]
    a.e, a.lde = e.data_ptr(), (e.stride(0) if e.dim() == 2 else D)      # (a column slice of a stack's fused position projections: row stride L * D)
    a.lens, a.len_div = _p(lens), len_div
    if mask is not None:
        a.mask, a.mask_bstride = mask.data_ptr(), (T * (Tk or T) if mask.shape[0] > 1 else 0)
    a.o, a.ldo, a.lse = o.data_ptr(), D, lse.data_ptr()
    a.B, a.H, a.T, a.d, a.scale, a.Tk = B, H, T, d, (1.0 / d ** 0.5 if scale is None else scale), Tk
    return a


def _pad8(n):
    return (n + 7) // 8 * 8


def _attn_backward(a, do, dq, dsrel, de=None, products=False, one_launch=False):
    """avec_relpos_attention_bwd on the forward Attn `a` (of _attn_args), then -- products -- dK = dS^T Q and dV = P^T dO per (batch, head) and dE_h = sum_b skew(dS)^T Q
    as batched TN MFMA GEMMs with fp32 accumulation: one_launch puts the three into one (avec_gemm_tn_batched_multi), else two stores and one accumulation.
    The buffers are the caller's: do [B*T][D] act; dq the dQ rows (with products: the first third of a packed [B*T][3D] dQ | dK | dV, row stride dq.stride(0)); de fp32
    [2T-1][D] rows, zeroed or holding a sum to add to; dsrel [H][B*T][_pad8(T + Tk - 1)] act, zeroed.  Returns the (P, dS) scratch [2][B*H][T][_pad8(Tk)].
    `do` NEEDS 16 READABLE BYTES BEHIND ITS LAST ROW when d is no multiple of 8 (d = 45, 90): dV reads dO per head in whole 16-byte chunks (gemm_tn_batched: J = d
    rounded up to the vector width), so the last head's last chunk ends up to 12 bytes behind the row -- in the last row, behind the tensor."""
    B, H, T, d = a.B, a.H, a.T, a.d
    D, esz = H * d, do.element_size()
    a.dout = do.data_ptr()
    a.dq, a.lddq = dq.data_ptr(), dq.stride(0)
    if products:
        a.dk, a.dv, a.ldd = a.dq + D * esz, a.dq + 2 * D * esz, a.lddq
        a.de, a.ldde = de.data_ptr(), de.stride(0)
    Tld = _pad8(a.Tk or T)
    scratch = empty((2, B * H, T, Tld), do.dtype, do)                # P and dS of every (batch, head), row stride padded to 8
    a.pbuf, a.dsbuf, a.ldt = scratch.data_ptr(), scratch.data_ptr() + scratch[0].numel() * esz, Tld
    a.dsrel, a.ldr = dsrel.data_ptr(), dsrel.shape[2]
    lib.relpos_attention_bwd(rt.dt(), _byref(a), rt.stream())
    if not products:
        return scratch
    # dK and dV: one workgroup per (batch, head, tile) reduces over all T rows and stores straight into the K / V thirds of the packed gradient (no zero-filled
    # fp32 staging, no atomics, no cast pass); dE sums over the batch, so it keeps the accumulate form
    L6 = ctypes.c_longlong * 6
    sK, sV, sE = L6(H * T * Tld, T * Tld, T * a.ld, d, T * a.ldd, d), L6(H * T * Tld, T * Tld, T * D, d, T * a.ldd, d), L6(0, B * T * a.ldr, 0, d, 0, d)
    # (P, ldp, Q, ldq, O, ldo, M, I, J, outer batch, inner batch, strides)
    pK = (a.dsbuf, Tld, a.q, a.ld, a.dk, a.ldd, T, T, d, B, H, sK)
    pV = (a.pbuf, Tld, a.dout, D, a.dv, a.ldd, T, T, d, B, H, sV)
    pE = (a.dsrel, a.ldr, a.q, a.ld, a.de, a.ldde, B * T, 2 * T - 1, d, 1, H, sE)
    if one_launch:
        it = (TnBatched * 3)()
        for t, p, out in zip(it, (pK, pV, pE), ("O_act", "O_act", "O")):
            t.P, t.ldp, t.Q, t.ldq, _, t.ldo, t.M, t.I, t.J, t.nb_outer, t.nb_inner, t.strides6 = p
            setattr(t, out, p[4])
        lib.gemm_tn_batched_multi(rt.dt(), it, 3, rt.stream())
    else:
        lib.gemm_tn_batched_store(rt.dt(), *pK, rt.stream())
        lib.gemm_tn_batched_store(rt.dt(), *pV, rt.stream())
        lib.gemm_tn_batched(rt.dt(), *pE, rt.stream())
    return scratch


# ---- position projections of a whole stack in one launch ---------------------------------------------------------------------------------------------------
# E_l = pos_layer_l(PE) depends on weights only (nnet/attentions.py:289, nnet/embeddings.py:158: the reference recomputes it per block AND per batch element).
# The pos_layer weights of the consecutive blocks of a stage are laid out back to back in the arena (nnet.ConformerInterCTC declares them with rt.fuse_linears), so
# ONE product PE [2T-1][D] x W_all^T [D][L D] gives every block's E as a column slice, and in backward the L gradients dE_l accumulate in one [2T-1][L D] buffer that
# takes ONE cast and ONE weight-gradient product when the last of them has arrived: 2 (L - 1) launches less per stage and pass.  Versioned by the arena's shadow
# refresh counter (E follows the weights), per sequence length.
_POS_CACHE = {}
_POS_EPOCH = [0]


class _PosGroupEntry:
    __slots__ = ("e_all", "pe", "L", "D", "Tp", "capture")


def invalidate_pos_cache():
    """Forget every cached E: the next forward pass computes it again.  A capture that holds no shadow refresh (Model.make_graphed_micro_step) calls this first, so
    that E is computed INSIDE its graph and follows the weights on every replay -- an entry built by an earlier capture lives in that graph's pool and is filled only
    when that graph replays."""
    _POS_CACHE.clear()
    _POS_EPOCH[0] += 1


def _pos_group_entry(wp, Tp, D, device):
    """-> (entry, index of this layer inside its group) or (None, 0)"""
    if rt.compute_dtype() != "bf16":
        return None, 0
    grp = rt.fused_group(wp)
    if grp is None or len(grp.weights) < 2 or fp8.enabled():
        return None, 0
    idx = next((k for k, w in enumerate(grp.weights) if w is wp), None)
    if idx is None:
        return None, 0
    arena = wp._avec_shadow.arena
    key = (id(grp), Tp, str(device))
    ent = _POS_CACHE.get(key)
    ver = (getattr(arena, "refresh_count", 0), torch.cuda.current_stream().cuda_stream)
    if ent is None or ent[0] != ver:
        L = len(grp.weights)
        e = _PosGroupEntry()
        e.L, e.D, e.Tp, e.pe = L, D, Tp, rel_pos_table(Tp, D, device)
        e.capture = _POS_EPOCH[0] if torch.cuda.is_current_stream_capturing() else None
        e.e_all = empty((2 * Tp - 1, L * D), rt.act_dtype(), e.pe)
        gemm_nt(e.pe, grp.fwd, e.e_all, 2 * Tp - 1, L * D, D, bias=grp.bias)
        _POS_CACHE[key] = ent = (ver, e, grp)
        if len(_POS_CACHE) > 64:
            for k in list(_POS_CACHE)[:32]:
                _POS_CACHE.pop(k, None)
    elif ent[1].capture is not None and torch.cuda.is_current_stream_capturing():
        assert ent[1].capture == _POS_EPOCH[0], "E built inside one captured graph must not be served to a later capture"
    return ent[1], idx


def _pos_group_backward(entry, wp):
    """one layer of the group has accumulated its dE: when all have, cast once and queue ONE weight-gradient product for the whole group"""
    acc = _pass().pos[entry]
    acc[1] -= 1
    if acc[1] > 0:
        return
    de_all = _pass().pos.pop(entry)[0]
    grp = rt.fused_group(wp)
    R, W = 2 * entry.Tp - 1, entry.L * entry.D
    dea = empty((R, W), rt.act_dtype(), de_all)
    lib.cast_rows(rt.dt(), de_all.data_ptr(), W, dea.data_ptr(), W, R, W, rt.stream())
    gemm_tn(dea, entry.pe, grp.wgrad, R, W, entry.D, p_colsum=grp.bgrad, side=True)


def qkv_project(h, wb, M, D, fp8_ok=False):
    """h [M, D] act -> Q | K | V [M, 3D] act.  wb = ((wq, wk, wv), (bq, bk, bv)).  One GEMM when the arena laid the three weights back to back, else three GEMMs
    into column slices of the one buffer.  fp8_ok (the training forward only): the grouped product may take the weights' fp8 entry."""
    (wq, wk, wv), bs = wb
    qkv = empty((M, 3 * D), rt.act_dtype(), h)
    grp = rt.fused_group(wq)          # (no test of the biases: ParamArena forms a group only when every bias exists)
    if grp is not None and grp.weights[1] is wk and grp.weights[2] is wv:
        ent = fp8.entry(wq, D) if fp8_ok else None
        if ent is not None and ent.N == 3 * D:
            gemm_nt_fp8(h, ent, qkv, M, 3 * D, D, bias=grp.bias)
        else:
            gemm_nt(h, grp.fwd, qkv, M, 3 * D, D, bias=grp.bias)
    else:
        for i, (w, b) in enumerate(zip((wq, wk, wv), bs)):
            gemm_nt(h, rt.shadow(w).fwd, qkv[:, i * D:], M, D, D, bias=b, ldo=3 * D)
    return qkv


class AttentionModuleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lens, mask, ln_w, ln_b, wq, bq, wk, bk, wv, bv, wo, bo, wp, bp, H, patch, eps, drop_p, sid, residual):
        rt.require_gpu(x)
        B, T, D = x.shape
        M, d, adt = B * T, D // H, rt.act_dtype()
        x2 = _f32c(x.reshape(-1, D))
        if ln_w is not None:
            h, mean, rstd = layernorm_fwd(x2, ln_w, ln_b, M, D, False, eps)
        else:                      # bare attention layer (forwardQKV called directly): no pre-norm
            mean = rstd = None
            h = empty((M, D), adt, x2)
            lib.cast_rows(rt.dt(), x2.data_ptr(), D, h.data_ptr(), D, M, D, rt.stream())
        if patch > 1:
            Tp = (T + patch - 1) // patch
            hp = empty((B * Tp, D), adt, x2)
            lib.patch_pool_fwd(rt.dt(), h.data_ptr(), hp.data_ptr(), B, T, D, patch, rt.stream())
        else:
            Tp, hp = T, h
        Mp = B * Tp
        if mask is not None:      # dense (B or 1,1,T,T) float mask as the reference API; patch variant min-pools it on the host side
            mask = mask.reshape(mask.shape[0], T, T) if patch == 1 else _pool_mask(mask, T, patch)
            mask = mask.float().contiguous()
        qkv = qkv_project(hp, ((wq, wk, wv), (bq, bk, bv)), Mp, D, fp8_ok=True)
        pg, pgi = _pos_group_entry(wp, Tp, D, x.device)
        if pg is not None:
            pe, e = pg.pe, pg.e_all[:, pgi * D:(pgi + 1) * D]          # this block's slice of the stack's position projections (one launch per stage and pass)
        else:
            pe = rel_pos_table(Tp, D, x.device)
            e = linear_fwd(pe, wp, bp, 2 * Tp - 1, in_f32=False, out_f32=False)
        o = empty((Mp, D), adt, x2)
        lse = empty((B * H, Tp, 2), torch.float32, x2)
        q_full = T // patch if (patch > 1 and mask is None) else 0
        a = _attn_args(qkv, e, lens, patch, mask, o, lse, B, H, Tp, d, D, q_full)
        lib.relpos_attention_fwd(rt.dt(), _byref(a), rt.stream())
        res = x2 if residual else None
        if patch > 1:
            oo = linear_fwd(o, wo, bo, Mp, in_f32=False, out_f32=False)
            base = x2 if residual else torch.zeros_like(x2)
            y = empty((M, D), torch.float32, x2)
            lib.patch_unpool_add(rt.dt(), oo.data_ptr(), base.data_ptr(), y.data_ptr(), drop_p, _rng(x.device, drop_p), sid, B, T, D, patch, rt.stream())
        else:
            y = linear_fwd(o, wo, bo, M, in_f32=False, out_f32=True, drop_p=drop_p, sid=sid, res=res, alpha=1.0)
        ctx.saved = (x2, mean, rstd, h, hp, qkv, pe, e, o, lse, lens, mask, ln_w, ln_b, wq, bq, wk, bk, wv, bv, wo, bo, wp, bp,
                     H, patch, drop_p, sid, residual, B, T, Tp, D)
        ctx.pos_group = (pg, pgi)
        ctx.prep_req = _prep_request(x)
        return _tag_prep(y.view(B, T, D), 1.0, drop_p, sid) if patch == 1 else y.view(B, T, D)

    @staticmethod
    def backward(ctx, dy):
        (x2, mean, rstd, h, hp, qkv, pe, e, o, lse, lens, mask, ln_w, ln_b, wq, bq, wk, bk, wv, bv, wo, bo, wp, bp,
         H, patch, drop_p, sid, residual, B, T, Tp, D) = ctx.saved
        M, Mp, d, adt = B * T, B * Tp, D // H, rt.act_dtype()
        dy = _f32c(dy.reshape(M, D))
        if patch > 1:
            doo = empty((Mp, D), adt, dy)
            lib.patch_unpool_bwd(rt.dt(), dy.data_ptr(), doo.data_ptr(), drop_p, _rng(dy.device, drop_p), sid, B, T, D, patch, rt.stream())
        else:
            doo = _take_prep(dy, M, D, 1.0, drop_p, sid)
            if doo is None:
                doo = grad_prep(dy, M, D, drop_p=drop_p, sid=sid)
        linear_bwd_weight(doo, o, wo, Mp, bias=bo)
        do = torch.empty(Mp * D + 8, dtype=adt, device=dy.device)[:Mp * D].view(Mp, D)          # 16 readable bytes behind the last row (see _attn_backward)
        do = linear_bwd_input(doo, wo, Mp, out_f32=False, out=do)
        dqkv = empty((Mp, 3 * D), adt, dy)
        pg, pgi = ctx.pos_group
        if pg is not None:
            acc = _pass().pos.get(pg)
            if acc is None:                          # first layer of the group to reach its backward: the shared [2T-1][L D] accumulator (pre-zeroed pool)
                acc = _pass().pos[pg] = [rt.zeros_scratch((2 * Tp - 1) * pg.L * D, dy.device).view(2 * Tp - 1, pg.L * D), pg.L]
            de = acc[0][:, pgi * D:(pgi + 1) * D]
        else:
            de = rt.zeros_scratch((2 * Tp - 1) * D, dy.device).view(2 * Tp - 1, D)      # pre-zeroed pool: no fill launch per layer (-0.15 ms per step)
        a = _attn_args(qkv, e, lens, patch, mask, o, lse, B, H, Tp, d, D, T // patch if (patch > 1 and mask is None) else 0)
        n_rel = H * B * Tp * _pad8(2 * Tp - 1)                       # zero-initialised, from the step's pre-zeroed pool (was a fill launch per layer on the dependent chain)
        if adt == torch.bfloat16:
            dsrel = rt.zeros_scratch((n_rel + 1) // 2, dy.device).view(torch.bfloat16)[:n_rel].view(H, B * Tp, -1)
        else:
            dsrel = rt.zeros_scratch(n_rel, dy.device).view(H, B * Tp, -1)
        _attn_backward(a, do, dqkv, dsrel, de, products=True, one_launch=True)
        dhp = None
        grp = rt.fused_group(wq)
        if grp is not None and grp.weights[1] is wk and grp.weights[2] is wv and bq is not None:
            gemm_tn(dqkv, hp, grp.wgrad, Mp, 3 * D, D, p_colsum=grp.bgrad, side=True)                    # d(Wq|Wk|Wv), d(bq|bk|bv)
            dhp = empty((Mp, D), adt, dy)
            gemm_nt(dqkv, grp.bwd, dhp, Mp, D, 3 * D)                                            # d(input) = dQ Wq + dK Wk + dV Wv
        else:
            for i, (w, b) in enumerate(((wq, bq), (wk, bk), (wv, bv))):
                g = dqkv[:, i * D:]
                linear_bwd_weight(g, hp, w, Mp, ldp=3 * D, bias=b)
                dhp = linear_bwd_input(g, w, Mp, out_f32=False, lda=3 * D, res=dhp, res_act=True, out=dhp)
        if pg is not None:
            _pos_group_backward(pg, wp)
        else:
            dea = empty((2 * Tp - 1, D), adt, dy)
            lib.cast_rows(rt.dt(), de.data_ptr(), D, dea.data_ptr(), D, 2 * Tp - 1, D, rt.stream())
            linear_bwd_weight(dea, pe, wp, 2 * Tp - 1, bias=bp)
        if patch > 1:
            dh = empty((M, D), adt, dy)
            lib.patch_pool_bwd(rt.dt(), dhp.data_ptr(), dh.data_ptr(), B, T, D, patch, rt.stream())
        else:
            dh = dhp
        if ln_w is not None:
            dx = layernorm_bwd(dh, False, x2, mean, rstd, ln_w, ln_b, M, D, dres=dy if residual else None, prep=ctx.prep_req)
        else:
            dx = dy.clone() if residual else torch.zeros_like(dy)
            lib.to_f32_rows(rt.dt(), dh.data_ptr(), D, dx.data_ptr(), D, M, D, 1, rt.stream())
        return (dx.view(B, T, D),) + (None,) * 20


class RelPosCoreFn(torch.autograd.Function):
    """softmax((Q K^T + rel_to_abs(Q E^T)) * scale + mask) V per (batch, head) on packed activation-dtype operands (the core of nnet/attentions.py:299-315 /
    :621-640 without the projections): qkv [B*T][3*H*d] = q | k | v, e [2T-1][H*d] (row r <-> relative offset T-1-r) -> o [B*T][H*d].
    Used by the Transformer-XL style / grouped attention classes, whose u / v biases and frame grouping are expressed on the operands."""

    @staticmethod
    def forward(ctx, qkv, e, lens, len_div, mask, B, H, T, d, scale):
        rt.require_gpu(qkv)
        D, adt = H * d, rt.act_dtype()
        assert qkv.dtype == adt and e.dtype == adt and qkv.is_contiguous() and e.is_contiguous() and qkv.shape == (B * T, 3 * D) and e.shape == (2 * T - 1, D)
        assert d % 2 == 0, "the batched-GEMM backward needs an even head width (pad the operands)"
        if mask is not None:
            mask = mask.reshape(mask.shape[0], T, T).float().contiguous()
        o = empty((B * T, D), adt, qkv)
        lse = empty((B * H, T, 2), torch.float32, qkv)
        a = _attn_args(qkv, e, lens, len_div, mask, o, lse, B, H, T, d, D, scale=scale)
        lib.relpos_attention_fwd(rt.dt(), _byref(a), rt.stream())
        ctx.saved = (qkv, e, o, lse, lens, len_div, mask, B, H, T, d, scale)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, e, o, lse, lens, len_div, mask, B, H, T, d, scale = ctx.saved
        D, adt = H * d, rt.act_dtype()
        do = do.to(adt).contiguous()
        dqkv = empty((B * T, 3 * D), adt, do)
        de = torch.zeros((2 * T - 1, D), dtype=torch.float32, device=do.device)
        a = _attn_args(qkv, e, lens, len_div, mask, o, lse, B, H, T, d, D, scale=scale)
        dsrel = torch.zeros((H, B * T, _pad8(2 * T - 1)), dtype=adt, device=do.device)
        _attn_backward(a, do, dqkv, dsrel, de, products=True)
        return dqkv, de.to(adt), None, None, None, None, None, None, None, None


def relpos_core_infer(q, k, v, e, lens, mask, B, H, T, Tk, d, scale, want_probs=False):
    """inference form with a key/value cache: q [B*T][H*d], k / v [B*Tk][H*d] (Tk >= T), e [Tk+T-1][H*d], optional dense mask (Bm, T, Tk) -> o [B*T][H*d]
    (and the attention probabilities (B, H, T, Tk) when asked: the reference returns them next to the updated cache, nnet/attentions.py:552)"""
    rt.require_gpu(q)
    D, adt = H * d, rt.act_dtype()
    for t in (q, k, v, e):
        assert t.dtype == adt and t.is_contiguous()
    assert q.shape == (B * T, D) and k.shape == (B * Tk, D) and v.shape == (B * Tk, D) and e.shape == (Tk + T - 1, D)
    if mask is not None:
        mask = mask.reshape(mask.shape[0], T, Tk).float().contiguous()
    o = empty((B * T, D), adt, q)
    lse = empty((B * H, T, 2), torch.float32, q)
    a = _attn_args(q, e, lens, 1, mask, o, lse, B, H, T, d, D, kv=(k, v, D), Tk=Tk, scale=scale)
    lib.relpos_attention_fwd(rt.dt(), _byref(a), rt.stream())
    if not want_probs:
        return o, None
    dq = empty((B * T, D), adt, q)
    zero = torch.zeros((B * T, D), dtype=adt, device=q.device)
    dsrel = torch.zeros((H, B * T, _pad8(Tk + T - 1)), dtype=adt, device=q.device)
    scratch = _attn_backward(a, zero, dq, dsrel)                      # the row pass recomputes the probabilities from (max, sum) and stores them
    return o, scratch[0].view(B, H, T, -1)[..., :Tk].float()


def _pool_mask(mask, T, P):
    """reference min-pool of the padded (B,1,T,T) mask (nnet/attentions.py:140-171,357-362) -- exact 0/1 index work on the host side API path"""
    pad = (P - T % P) % P
    m = torch.nn.functional.pad(mask.reshape(mask.shape[0], 1, T, T).float(), (0, pad, 0, pad), value=0.0)
    Tp = (T + pad) // P
    return m.reshape(m.shape[0], Tp, P, Tp, P).amin(dim=(2, 4))


# ============================================================================================
# ConvolutionModule (nnet/modules.py:341-385) fused with the block's conv residual (nnet/blocks.py:273-277,298)
#   y = R(x) + Drop(PW2(Swish(BN(DW(GLU(PW1(LN(x))))))))     R = identity | strided k=1 conv
# ============================================================================================
class BNState:
    """scratch for one BatchNorm application: stats [2C+1] (sum | sumsq | count) and ss [4C]"""

    NREP = 64      # AVEC_STAT_REPLICAS: the GEMM epilogue spreads its statistic atomics over this many [2C] copies

    def __init__(self, C, ref):
        self.stats = rt.zeros_scratch(self.NREP * 2 * C, ref.device)
        self.red = None
        self.ss = torch.empty(4 * C, dtype=torch.float32, device=ref.device)
        self.C = C


RELU_BITMASK = True    # ResNet block ends: the backward pass reads a 1-bit ReLU mask instead of the saved block output (0: reads `out`)
def bn_finalize(bn, st, count, training):
    """bn: module with weight/bias/running_mean/running_var/num_batches_tracked/momentum/eps"""
    C = st.C
    cptr = None
    sptr, nrep = st.stats.data_ptr(), st.NREP
    if training and rt.sync_batchnorm():
        # SyncBatchNorm: collapse the replicas, append the local count, sum over ranks (one small RCCL all-reduce)
        st.red = rt.sync_bn_stats(st.stats, st.NREP, C, count, key=(id(bn), "f"))
        sptr, nrep, cptr = st.red.data_ptr(), 1, st.red.data_ptr() + 2 * C * 4
    lib.bn_finalize(sptr, nrep, cptr, float(count), bn.weight.data_ptr(), bn.bias.data_ptr(), *_bn_running(bn, training), bn.eps, st.ss.data_ptr(), C, int(training),
                    rt.stream())
    return cptr


def _bn_running(bn, training):
    """(running_mean, running_var, num_batches_tracked pointers, momentum) as the finalize kernels take them: null without tracked statistics; the batch counter
    only moves in training"""
    track = bn.track_running_stats and bn.running_mean is not None
    return (bn.running_mean.data_ptr() if track else None, bn.running_var.data_ptr() if track else None,
            bn.num_batches_tracked.data_ptr() if (track and training) else None, bn.momentum if bn.momentum is not None else 0.1)


def bn_backward(bn, st, cptr, count, dout, y, out, act, M, want_dres=False, pre=None, mask=None):
    """pre: a completed BnbFuse -- `dout` is already masked and its (sum d, sum d*y) sit in pre.stats: no reduction pass, the apply pass reads d and y only
    mask: the ReLU mask of `out` as one bit per element (avec_bn_apply_fwd_mask): read instead of `out`"""
    C = st.C
    adt = rt.act_dtype()
    dstats = rt.zeros_scratch(2 * C, dout.device)
    if pre is not None:
        lib.bn_bwd_finalize(pre.stats.data_ptr(), BNState.NREP, st.ss.data_ptr(), dstats.data_ptr(), C, rt.stream())
        act, out, want_dres, mask = ACT_NONE, None, False, None
    elif mask is not None:
        lib.bn_bwd_reduce_mask(rt.dt(), dout.data_ptr(), y.data_ptr(), mask.data_ptr(), st.ss.data_ptr(), dstats.data_ptr(), M, C, rt.stream())
    else:
        lib.bn_bwd_reduce(rt.dt(), dout.data_ptr(), y.data_ptr(), _p(out), st.ss.data_ptr(), act, dstats.data_ptr(), M, C, rt.stream())
    dstats, gw, gb = _bn_sync_grads(bn, dstats, C)
    dy = empty((M, C), adt, dout)
    dres = empty((M, C), adt, dout) if want_dres else None
    if mask is not None:
        lib.bn_bwd_apply_mask(rt.dt(), dout.data_ptr(), y.data_ptr(), mask.data_ptr(), st.ss.data_ptr(), bn.weight.data_ptr(), dstats.data_ptr(), cptr, float(count),
                              dy.data_ptr(), _p(dres), _p(gw), _p(gb), M, C, rt.stream())
    else:
        lib.bn_bwd_apply(rt.dt(), dout.data_ptr(), y.data_ptr(), _p(out), st.ss.data_ptr(), bn.weight.data_ptr(), dstats.data_ptr(), cptr, float(count), act,
                         dy.data_ptr(), _p(dres), _p(gw), _p(gb), M, C, rt.stream())
    return dy, (dout if pre is not None else dres)


def _add_local_affine_grads(dstats, gw, gb, C, key):
    """SyncBatchNorm: d(gamma), d(beta) are the LOCAL sums (the gradient all-reduce averages them like any other parameter, as torch's
    SyncBatchNorm does); only the statistics entering dx are global.  Adds the local sums, then all-reduces `dstats`.
    Returns (dstats to use -- the global sums when synchronised --, whether it synchronised)."""
    if not rt.sync_batchnorm():
        return dstats, False
    from . import peer
    px = peer.active()
    if px is not None and dstats.is_cuda and dstats.is_contiguous() :
        return px.all_reduce_sum_fused(dstats, 1, 2 * C, None, key, dgamma=gw, dbeta=gb, C=C), True      # local affine gradients added inside the exchange kernel
    lib.bn_affine_grads(dstats.data_ptr(), gw.data_ptr(), gb.data_ptr(), C, rt.stream())
    return rt.all_reduce_small(dstats, key), True


def _bn_sync_grads(bn, dstats, C):
    """the step between the two passes of a training-mode BatchNorm backward: dstats = the local [sum d | sum d*y].  Returns (the dstats the apply pass reads,
    d(gamma), d(beta) accumulators for it to add to).  SyncBatchNorm: the global sums, and (None, None) -- the affine gradients are already added from the LOCAL
    sums; the kernel must not add the global ones."""
    gw, gb = grad_of(bn.weight), grad_of(bn.bias)
    dstats, synced = _add_local_affine_grads(dstats, gw, gb, C, (id(bn), "b"))
    return (dstats, None, None) if synced else (dstats, gw, gb)


def dw_pad_left(conv):
    """zero frames in front of the sequence for the depthwise conv (nnet/layers.py:137-156): "same" = K // 2, "causal" = K - 1"""
    K = conv.kernel_size[0]
    kind = getattr(conv, "padding_type", "same")
    if kind == "causal":
        return K - 1
    assert kind == "same", "the fused convolution module supports 'same' and 'causal' padding, got %r" % (kind,)
    return K // 2

CONVMOD_BN_FUSE = True      # conformer convolution module: BatchNorm finalize straight from the depthwise kernel's partial sums


class ConvModuleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, _anchor, mod, res_conv, drop_p, sid, training):
        """mod: ConvolutionModule (layers: 0 LN, 1 pw1, 3 dw, 4 BN, 6 pw2);  res_conv: strided k=1 Conv1d or None"""
        rt.require_gpu(x)
        B, T, D = x.shape
        ln, pw1, dw, bn, pw2 = mod.layers[0], mod.layers[1], mod.layers[3], mod.layers[4], mod.layers[6]
        Dp, K, stride = dw.weight.shape[0], dw.weight.shape[2], dw.stride[0]
        To = (T - 1) // stride + 1
        M, Mo, adt = B * T, B * To, rt.act_dtype()
        x2 = _f32c(x.reshape(M, D))
        h, mean, rstd = layernorm_fwd(x2, ln.weight, ln.bias, M, D, False, ln.eps)
        u = linear_fwd(h, pw1.weight, pw1.bias, M, in_f32=False, out_f32=False)
        c = empty((Mo, Dp), adt, x2)
        st = BNState(Dp, x2)
        use_batch = training and not getattr(bn, "frozen", False)
        if use_batch and not rt.sync_batchnorm() and CONVMOD_BN_FUSE:
            # local batch statistics: the finalize reads the depthwise kernel's column-reduction partials (one launch less in the block's dependent chain)
            lib.glu_dwconv_fwd_bn(rt.dt(), u.data_ptr(), dw.weight.data_ptr(), _p(dw.bias), c.data_ptr(), st.stats.data_ptr(), B, T, Dp, K, stride, dw_pad_left(dw),
                                  bn.weight.data_ptr(), bn.bias.data_ptr(), *_bn_running(bn, use_batch), bn.eps, st.ss.data_ptr(), rt.stream())
            cptr = None
        else:
            lib.glu_dwconv_fwd(rt.dt(), u.data_ptr(), dw.weight.data_ptr(), _p(dw.bias), c.data_ptr(), st.stats.data_ptr() if use_batch else None,
                               B, T, Dp, K, stride, dw_pad_left(dw), rt.stream())
            cptr = bn_finalize(bn, st, Mo, use_batch)
        a = empty((Mo, Dp), adt, x2)
        lib.bn_apply_fwd(rt.dt(), c.data_ptr(), st.ss.data_ptr(), None, ACT_SWISH, a.data_ptr(), Mo, Dp, rt.stream())
        if res_conv is not None:
            rs = res_conv.stride[0]
            R = linear_fwd(x2, res_conv.weight, res_conv.bias, Mo, in_f32=(adt != torch.float32), out_f32=True,
                           rows=rows_plain(D, To, T, rs) if rs > 1 else None)
        else:
            R = x2
        y = linear_fwd(a, pw2.weight, pw2.bias, Mo, in_f32=False, out_f32=True, drop_p=drop_p, sid=sid, res=R, alpha=1.0)
        ctx.saved = (x2, mean, rstd, h, u, c, a, st, cptr, use_batch, mod, res_conv, drop_p, sid, B, T, To, D, Dp, K, stride)
        ctx.prep_req = _prep_request(x)
        return _tag_prep(y.view(B, To, Dp), 1.0, drop_p, sid)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd, h, u, c, a, st, cptr, use_batch, mod, res_conv, drop_p, sid, B, T, To, D, Dp, K, stride = ctx.saved
        ln, pw1, dw, bn, pw2 = mod.layers[0], mod.layers[1], mod.layers[3], mod.layers[4], mod.layers[6]
        M, Mo, adt = B * T, B * To, rt.act_dtype()
        dy = _f32c(dy.reshape(Mo, Dp))
        dacc = _take_prep(dy, Mo, Dp, 1.0, drop_p, sid)
        if dacc is None:
            dacc = grad_prep(dy, Mo, Dp, drop_p=drop_p, sid=sid)
        linear_bwd_weight(dacc, a, pw2.weight, Mo, bias=pw2.bias)
        da = linear_bwd_input(dacc, pw2.weight, Mo, out_f32=False)
        du = empty((M, 2 * Dp), adt, dy)
        if use_batch and CONVMOD_BN_FUSE and stride == 1 and not rt.sync_batchnorm():
            # local batch statistics, stride 1: the reduction pass, then the BatchNorm-backward arithmetic inside the depthwise kernel's staging pass (no apply launch, no dc tensor)
            dstats = rt.zeros_scratch(2 * Dp, da.device)
            lib.bn_bwd_reduce(rt.dt(), da.data_ptr(), c.data_ptr(), None, st.ss.data_ptr(), ACT_SWISH, dstats.data_ptr(), Mo, Dp, rt.stream())
            lib.dwconv_glu_bwd_bn(rt.dt(), da.data_ptr(), c.data_ptr(), st.ss.data_ptr(), bn.weight.data_ptr(), dstats.data_ptr(), float(Mo), u.data_ptr(), dw.weight.data_ptr(),
                                  du.data_ptr(), grad_of(dw.weight).data_ptr(), None if dw.bias is None else grad_of(dw.bias).data_ptr(),
                                  grad_of(bn.weight).data_ptr(), grad_of(bn.bias).data_ptr(), B, T, Dp, K, dw_pad_left(dw), rt.stream())
        else:
            if use_batch:
                dc, _ = bn_backward(bn, st, cptr, Mo, da, c, None, ACT_SWISH, Mo)
            else:   # eval / frozen statistics: dc = da * swish'(pre) * scale  -> reuse the apply kernel with zero batch terms
                dc = _bn_eval_backward(bn, st, da, c, ACT_SWISH, Mo)
            lib.dwconv_glu_bwd(rt.dt(), dc.data_ptr(), u.data_ptr(), dw.weight.data_ptr(), du.data_ptr(), grad_of(dw.weight).data_ptr(),
                               None if dw.bias is None else grad_of(dw.bias).data_ptr(), B, T, Dp, K, stride, dw_pad_left(dw), rt.stream())
        linear_bwd_weight(du, h, pw1.weight, M, bias=pw1.bias)
        dh = linear_bwd_input(du, pw1.weight, M, out_f32=False)
        if res_conv is None:
            dx = layernorm_bwd(dh, False, x2, mean, rstd, ln.weight, ln.bias, M, D, dres=dy, prep=ctx.prep_req)
        else:
            rs = res_conv.stride[0]
            dx = layernorm_bwd(dh, False, x2, mean, rstd, ln.weight, ln.bias, M, D)
            dracc = grad_prep(dy, Mo, Dp)
            linear_bwd_weight(dracc, x2, res_conv.weight, Mo, q_f32=(adt != torch.float32), q_rows=rows_plain(D, To, T, rs) if rs > 1 else None, bias=res_conv.bias)
            dxr = linear_bwd_input(dracc, res_conv.weight, Mo, out_f32=True)
            lib.strided_rows_add(dx.data_ptr(), dxr.data_ptr(), B, T, To, D, rs, rt.stream())
        return dx.view(B, T, D), None, None, None, None, None, None


def _bn_eval_backward(bn, st, dout, y, act, M, out=None):
    """BatchNorm backward with fixed (running) statistics: dy = dr * scale; the batch-mean terms vanish (dstats = 0)."""
    C = st.C
    dstats = torch.zeros(2 * C, dtype=torch.float32, device=dout.device)
    dstats2 = torch.zeros(2 * C, dtype=torch.float32, device=dout.device)
    lib.bn_bwd_reduce(rt.dt(), dout.data_ptr(), y.data_ptr(), _p(out), st.ss.data_ptr(), act, dstats2.data_ptr(), M, C, rt.stream())
    dy = empty((M, C), rt.act_dtype(), dout)
    lib.bn_bwd_apply(rt.dt(), dout.data_ptr(), y.data_ptr(), _p(out), st.ss.data_ptr(), bn.weight.data_ptr(), dstats.data_ptr(), None, 1.0, act,
                     dy.data_ptr(), None, None, None, M, C, rt.stream())
    # parameter gradients from the true sums
    grad_of(bn.weight).add_(dstats2[C:])
    grad_of(bn.bias).add_(dstats2[:C])
    return dy


# ============================================================================================
# InterCTCResModule (nnet/modules.py:395-400):  logits = P1 x;  y = x + P2 softmax(logits)
# ============================================================================================
class InterCTCFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        rt.require_gpu(x)
        B, T, D = x.shape
        M, V = B * T, w1.shape[0]
        x2 = _f32c(x.reshape(M, D))
        conv = rt.act_dtype() != torch.float32
        logits = linear_fwd(x2, w1, b1, M, in_f32=conv, out_f32=True)
        probs = empty((M, V), rt.act_dtype(), x2)
        lib.softmax_fwd(rt.dt(), logits.data_ptr(), probs.data_ptr(), M, V, rt.stream())
        y = linear_fwd(probs, w2, b2, M, in_f32=False, out_f32=True, res=x2, alpha=1.0)
        ctx.saved = (x2, logits, probs, w1, b1, w2, b2, B, T, D, V, conv)
        return y.view(B, T, D), logits.view(B, T, V)

    @staticmethod
    def backward(ctx, dy, dlogits_ext):
        x2, logits, probs, w1, b1, w2, b2, B, T, D, V, conv = ctx.saved
        M = B * T
        dy = _f32c(dy.reshape(M, D))
        dacc = grad_prep(dy, M, D)
        linear_bwd_weight(dacc, probs, w2, M, bias=b2)
        dprobs = linear_bwd_input(dacc, w2, M, out_f32=False)
        dl = empty((M, V), torch.float32, dy)
        dext = None if dlogits_ext is None else _f32c(dlogits_ext.reshape(M, V))
        lib.softmax_bwd(rt.dt(), dprobs.data_ptr(), logits.data_ptr(), dl.data_ptr(), _p(dext), M, V, rt.stream())
        dla = grad_prep(dl, M, V)
        linear_bwd_weight(dla, x2, w1, M, q_f32=conv, bias=b1)
        dx = linear_bwd_input(dla, w1, M, out_f32=True, res=dy)
        return dx.view(B, T, D), None, None, None, None


# ============================================================================================
# FusionModule (nnet/modules.py:421-426): cat -> Linear -> Swish -> Linear
# ============================================================================================
class FusionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, v, w1, b1, w2, b2):
        rt.require_gpu(a)
        B, T, Da = a.shape
        Dv = v.shape[-1]
        M, F, adt = B * T, w1.shape[0], rt.act_dtype()
        a2, v2 = _f32c(a.reshape(M, Da)), _f32c(v.reshape(M, Dv))
        xc = empty((M, Da + Dv), adt, a2)
        lib.cast_rows(rt.dt(), a2.data_ptr(), Da, xc.data_ptr(), Da + Dv, M, Da, rt.stream())
        lib.cast_rows(rt.dt(), v2.data_ptr(), Dv, xc.data_ptr() + Da * xc.element_size(), Da + Dv, M, Dv, rt.stream())
        z = empty((M, F), adt, a2)
        h = linear_fwd(xc, w1, b1, M, in_f32=False, out_f32=False, act=ACT_SWISH, out_pre=z)
        y = linear_fwd(h, w2, b2, M, in_f32=False, out_f32=True)
        ctx.saved = (xc, z, h, w1, b1, w2, b2, B, T, Da, Dv, F)
        return y.view(B, T, -1)

    @staticmethod
    def backward(ctx, dy):
        xc, z, h, w1, b1, w2, b2, B, T, Da, Dv, F = ctx.saved
        M, N = B * T, w2.shape[0]
        dy = _f32c(dy.reshape(M, N))
        dacc = grad_prep(dy, M, N)
        linear_bwd_weight(dacc, h, w2, M, bias=b2)
        dz = linear_bwd_input(dacc, w2, M, out_f32=False, dact_z=z, dact=ACT_SWISH)
        linear_bwd_weight(dz, xc, w1, M, bias=b1)
        sh = rt.shadow(w1)                     # bwd shadow [Da+Dv][F]: rows 0..Da-1 -> d(audio), rest -> d(video)
        da = empty((M, Da), torch.float32, dy)
        dv = empty((M, Dv), torch.float32, dy)
        gemm_nt(dz, sh.bwd, da, M, Da, F, out_f32=True)
        gemm_nt(dz, sh.bwd[Da * F:], dv, M, Dv, F, out_f32=True)
        return da.view(B, T, Da), dv.view(B, T, Dv), None, None, None, None


# ============================================================================================
# CTC loss (nnet/losses.py:311-334) -> batch mean
# ============================================================================================
class CTCLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, logit_len, targets, target_len, blank, zero_infinity):
        rt.require_gpu(logits)
        B, T, V = logits.shape
        lg = _f32c(logits)
        tg = targets.to(device=lg.device, dtype=torch.int64).contiguous()
        if tg.dim() == 1:
            tg = tg.view(B, -1)
        Lmax = tg.shape[1]
        il = logit_len.to(device=lg.device, dtype=torch.int64).contiguous()
        tl = target_len.to(device=lg.device, dtype=torch.int64).contiguous()
        nll = empty((B,), torch.float32, lg)
        mean = torch.zeros((), dtype=torch.float32, device=lg.device)
        need_grad = ctx.needs_input_grad[0]
        grad = empty((B, T, V), torch.float32, lg) if need_grad else None
        ws = empty((lib.raw("avec_ctc_workspace_floats")(B, T, max(Lmax, 1)),), torch.float32, lg)
        lib.ctc_loss(lg.data_ptr(), il.data_ptr(), tg.data_ptr(), tl.data_ptr(), nll.data_ptr(), mean.data_ptr(), _p(grad), ws.data_ptr(),
                     B, T, V, Lmax, blank, int(zero_infinity), rt.stream())
        ctx.saved = (grad, B)
        ctx.nll = nll
        return mean

    @staticmethod
    def backward(ctx, dloss):
        grad, B = ctx.saved
        out = torch.empty_like(grad)
        dl = dloss.float().contiguous()
        lib.scale_by_scalar(grad.data_ptr(), dl.data_ptr(), 1.0 / B, out.data_ptr(), grad.numel(), rt.stream())
        return out, None, None, None, None, None


class CTCLossMultiFn(torch.autograd.Function):
    """n CTC heads over the same batch and labels in one launch (avec_ctc_loss_multi): apply(blank, zero_infinity, targets, target_len, weights, logits_0, len_0, ...)
    -> (sum_i weights[i] * loss_i, loss_0, ..., loss_{n-1}); the individual batch-mean losses are returned for logging (not differentiable), the weighted sum
    carries the gradient: backward is one scaling launch for all heads.  Same arithmetic per head as CTCLossFn (the kernel body is shared)."""

    @staticmethod
    def forward(ctx, blank, zero_infinity, targets, target_len, weights, *flat):
        n = len(flat) // 2
        logits, lens = [_f32c(t) for t in flat[0::2]], flat[1::2]
        rt.require_gpu(logits[0])
        B, _, V = logits[0].shape
        dev = logits[0].device
        tg = targets.to(device=dev, dtype=torch.int64).contiguous()
        if tg.dim() == 1:
            tg = tg.view(B, -1)
        Lmax = tg.shape[1]
        tl = target_len.to(device=dev, dtype=torch.int64).contiguous()
        ils = [l.to(device=dev, dtype=torch.int64).contiguous() for l in lens]
        nll = torch.empty((n, B), dtype=torch.float32, device=dev)
        means = rt.zeros_scratch(n + 1, dev)                 # [n]: the weighted total, accumulated by the same launch (was a rocBLAS dot + fill + add on the critical chain)
        grads = [empty(tuple(lg.shape), torch.float32, lg) if ctx.needs_input_grad[5 + 2 * i] else None for i, lg in enumerate(logits)]
        arr_p = lambda ptrs: (ctypes.c_void_p * n)(*ptrs)
        Ts = (ctypes.c_int * n)(*[lg.shape[1] for lg in logits])
        lib.ctc_loss_multi(n, arr_p([lg.data_ptr() for lg in logits]), arr_p([l.data_ptr() for l in ils]), Ts, arr_p([nll[i].data_ptr() for i in range(n)]),
                           arr_p([means[i:].data_ptr() for i in range(n)]), arr_p([g.data_ptr() if g is not None else None for g in grads]),
                           tg.data_ptr(), tl.data_ptr(), (ctypes.c_float * n)(*[float(x) for x in weights]), means[n:].data_ptr(), B, V, Lmax, blank, int(zero_infinity), rt.stream())
        total = means[n]
        ctx.set_materialize_grads(False)                     # (the n logging outputs never receive a gradient: no zero-filled scalars made for them in backward)
        ctx.saved = (grads, B, n, [float(x) for x in weights])
        ctx.keep = (logits, ils, tg, tl, nll)
        outs = tuple(means[i] for i in range(n))
        ctx.mark_non_differentiable(*outs)
        return (total,) + outs

    @staticmethod
    def backward(ctx, dtotal, *_unused):
        grads, B, n, weights = ctx.saved
        out = [None, None, None, None, None]
        if dtotal is None:
            return tuple(out + [None, None] * n)
        dt = dtotal.float().contiguous()
        live = [i for i in range(n) if grads[i] is not None]
        outs = {i: torch.empty_like(grads[i]) for i in live}
        if live:                                             # one scaling launch for all heads
            k = len(live)
            lib.scale_by_scalar_multi(k, (ctypes.c_void_p * k)(*[grads[i].data_ptr() for i in live]), (ctypes.c_void_p * k)(*[outs[i].data_ptr() for i in live]),
                                      (ctypes.c_longlong * k)(*[grads[i].numel() for i in live]), (ctypes.c_float * k)(*[weights[i] / B for i in live]), dt.data_ptr(), rt.stream())
        for i in range(n):
            out += [outs.get(i), None]
        return tuple(out)


_WCACHE = {}


def ctc_multi_fits(T, V, Lmax):
    return bool(lib.raw("avec_ctc_loss_multi_fits")(int(T), int(V), int(Lmax)))


class TimeMeanFn(torch.autograd.Function):
    """mean over the time axis of fp32 (B, T, V) logits (VisualEfficientConformerCE.forward, nnet/models_zoo.py:41) = the channels-last average pool"""

    @staticmethod
    def forward(ctx, x):
        from .lib import F32
        rt.require_gpu(x)
        B, T, V = x.shape
        x = _f32c(x)
        y = empty((B, V), torch.float32, x)
        lib.avgpool_fwd(F32, x.data_ptr(), y.data_ptr(), B, T, V, rt.stream())
        ctx.saved = (B, T, V)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .lib import F32
        B, T, V = ctx.saved
        dy = _f32c(dy)
        dx = empty((B, T, V), torch.float32, dy)
        lib.avgpool_bwd(F32, dy.data_ptr(), dx.data_ptr(), B, T, V, rt.stream())
        return dx


class SoftmaxCEFn(torch.autograd.Function):
    """mean over rows of cross-entropy(logits[M,V], targets[M]) with ignore_index (losses.SoftmaxCrossEntropy, nnet/losses.py:258-290)"""

    @staticmethod
    def forward(ctx, logits, targets, ignore_index):
        rt.require_gpu(logits)
        M, V = logits.shape
        lg = _f32c(logits)
        tg = targets.to(device=lg.device, dtype=torch.int64).contiguous()
        loss = empty((M,), torch.float32, lg)
        mean = torch.zeros((), dtype=torch.float32, device=lg.device)
        grad = empty((M, V), torch.float32, lg) if ctx.needs_input_grad[0] else None
        lib.softmax_ce(lg.data_ptr(), tg.data_ptr(), int(ignore_index), loss.data_ptr(), mean.data_ptr(), _p(grad), M, V, rt.stream())
        ctx.saved = (grad, M)
        return mean

    @staticmethod
    def backward(ctx, dloss):
        grad, M = ctx.saved
        out = torch.empty_like(grad)
        lib.scale_by_scalar(grad.data_ptr(), dloss.float().contiguous().data_ptr(), 1.0 / M, out.data_ptr(), grad.numel(), rt.stream())
        return out, None, None


# ============================================================================================
# convolutions on channels-last activations (ResNet-18 front-end, nnet/blocks.py:29-91, nnet/networks.py:32-146)
# ============================================================================================
def conv2d_fwd(x, weight, N, H, W, Cin, stride, stats=None):
    """x: act [N,H,W,Cin] (contiguous NHWC); weight: Conv2d param (physical [Cout][KH][KW][Cin]); 'same' zero padding ((k-1)//2)."""
    Cout, KH, KW = weight.shape[0], weight.shape[2], weight.shape[3]
    pad = (KH - 1) // 2
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = N * OH * OW
    sh = rt.shadow(weight)
    y = empty((M, Cout), rt.act_dtype(), x)
    if _slab_conv(H, W, Cin, Cout, KH, KW, stride):
        ev = KERNEL_TIMER.start()
        lib.conv3x3_c64(x.data_ptr(), sh.fwd.data_ptr(), y.data_ptr(), None, _p(stats), N, H, W, 0, rt.stream())
        KERNEL_TIMER.stop(ev, (2, 0), 2.0 * M * Cout * KH * KW * Cin, 2.0 * (N * H * W * Cin + Cout * KH * KW * Cin + M * Cout))
        return y, OH, OW
    gemm_nt(x, sh.fwd, y, M, Cout, KH * KW * Cin, rows=rows_conv(H, W, Cin, KH, KW, stride, pad, OH, OW), mode=ROWS_CONV_FWD, stats=stats,
            abytes=2.0 * (N * H * W * Cin + Cout * KH * KW * Cin + M * Cout))
    return y, OH, OW


SHORTCUT_SUBGRID = True        # ResNet projection shortcuts: input gradient on the subsampled grid (res_cls0)
GROUP_WGRAD128 = True          # the wide layers' weight gradients as one grouped launch at the end of the backward pass


def _slab_conv(H, W, Cin, Cout, KH, KW, stride):
    """ResNet stage 1 (3x3, stride 1, 64 -> 64 channels, 22x22 images), bf16: weights resident in LDS + one image slab per iteration (csrc/conv3x3.hip)"""
    return rt.act_dtype() == torch.bfloat16 and bool(lib.raw("avec_conv3x3_c64_supported")(H, W, Cin, Cout, KH, KW, stride))


class BnbFuse:
    """request to fold a BatchNorm(+ReLU) backward reduction into the epilogue of the product that computes its output gradient:
    y = the BatchNorm input, mask_z = saved post-ReLU activation (mask z > 0) or None (mask from scale*y + shift > 0 with `ss`), stats = replicated [sum d | sum d*y]"""
    __slots__ = ("y", "ss", "mask_z", "stats", "done")

    def __init__(self, y, ss, mask_z, C):
        self.y, self.ss, self.mask_z, self.done = y, ss, mask_z, False
        self.stats = rt.zeros_scratch(BNState.NREP * 2 * C, y.device)


# BatchNorm-backward reductions inside the backward-data epilogues (ResNet stages 2-4).  Correct (tests/test_gpu_round3.py) but SLOWER in the step (25.32 vs 25.07 ms, same box):
# the extra y / mask tile loads sit on the critical path of each workgroup's epilogue while the stand-alone reductions run at 0.5 of the HBM peak.  Opt-in.
BNB_FUSE = False


def conv2d_bwd(dy, x, weight, N, H, W, Cin, stride, OH, OW, need_dx=True, dx_res=None, bnb=None, dx_res_cls0=False, dx_res_mask=None):
    """dx_res_cls0: dx_res holds rows for the (even row, even column) input pixels only (stride-2 layers, bf16: include/avec_hip.h res_cls0)
    dx_res_mask: one bit per element of dx_res (the ReLU mask written by avec_bn_apply_fwd_mask): dx = conv^T(dy) + (bit ? dx_res : 0) (see res_mask_ok)"""
    Cout, KH, KW = weight.shape[0], weight.shape[2], weight.shape[3]
    pad = (KH - 1) // 2
    M = N * OH * OW
    sh = rt.shadow(weight)
    slab64 = _slab_conv(H, W, Cin, Cout, KH, KW, stride) and H * (W + 1) <= 512
    wide = not slab64 and rt.act_dtype() == torch.bfloat16 and bool(lib.raw("avec_wgrad3x3_c128_supported")(H, W, Cin, Cout, KH, KW, stride))
    if slab64 or wide:
        if GROUP_WGRAD128 and _in_backward():
            # queued: one grouped launch for all the layers of a kind when the backward pass is through (the final atomics of a launch of its own are ~30 % of it)
            it = WgradItem()
            it.x, it.dy, it.dw, it.images, it.C, it.H, it.W = x.data_ptr(), dy.data_ptr(), grad_of(weight).data_ptr(), N, Cin, H, W
            _pass().pending().push("cw64" if slab64 else "cw", it, [x, dy], 2.0 * M * Cout * KH * KW * Cin)
        else:
            ev = KERNEL_TIMER.start()
            if slab64:
                lib.wgrad3x3_c64(x.data_ptr(), dy.data_ptr(), grad_of(weight).data_ptr(), N, H, W, rt.stream())
            else:
                lib.wgrad3x3_c128(x.data_ptr(), dy.data_ptr(), grad_of(weight).data_ptr(), N, Cin, H, W, rt.stream())
            KERNEL_TIMER.stop(ev, (2, 2), 2.0 * M * Cout * KH * KW * Cin)
    else:
        gemm_tn(dy, x, grad_of(weight), M, Cout, KH * KW * Cin, q_rows=rows_conv(H, W, Cin, KH, KW, stride, pad, OH, OW), q_mode=ROWS_CONV_FWD, side=True)
    if not need_dx:
        return None
    dx = empty((N * H * W, Cin), rt.act_dtype(), dy)
    if _slab_conv(H, W, Cin, Cout, KH, KW, stride):
        ev = KERNEL_TIMER.start()
        if dx_res_mask is not None:
            lib.conv3x3_c64_res_masked(dy.data_ptr(), sh.bwd.data_ptr(), dx.data_ptr(), dx_res.data_ptr(), dx_res_mask.data_ptr(), N, H, W, 1, rt.stream())
        else:
            lib.conv3x3_c64(dy.data_ptr(), sh.bwd.data_ptr(), dx.data_ptr(), _p(dx_res), None, N, H, W, 1, rt.stream())
        KERNEL_TIMER.stop(ev, (2, 1), 2.0 * N * H * W * Cin * KH * KW * Cout, 2.0 * (2 * N * H * W * Cin + Cout * KH * KW * Cin + M * Cout))
        return dx
    # algorithmic work of the backward-data product: one MAC per (output pixel, tap, Cin, Cout) -- for stride 2 three of four taps of the implicit GEMM
    # over input pixels are structurally zero and are skipped by the parity-class kernel: they are not counted
    fuse = bnb if (bnb is not None and BNB_FUSE and rt.act_dtype() == torch.bfloat16 and Cin % 4 == 0) else None
    gemm_nt(dy, sh.bwd, dx, N * H * W, Cin, KH * KW * Cout, rows=rows_conv(H, W, Cout, KH, KW, stride, pad, OH, OW), mode=ROWS_CONV_BWD,
            res=dx_res, res_act=True, flops=2.0 * N * OH * OW * Cout * KH * KW * Cin, bnb=fuse, res_cls0=dx_res_cls0, res_mask=dx_res_mask,
            abytes=2.0 * (N * H * W * Cin * (2 if dx_res is not None else 1) + Cout * KH * KW * Cin + M * Cout))
    if fuse is not None:
        fuse.done = True
    return dx


def res_mask_ok(H, W, Cin, Cout, stride):
    """can conv2d_bwd add a bit-masked residual for this 3x3 layer?  The stage-1 slab kernel, or the shifted-window kernel with its register-direct epilogue (csrc/gemm.hip)"""
    if rt.act_dtype() != torch.bfloat16 or stride != 1 or Cin != Cout:
        return False
    return _slab_conv(H, W, Cin, Cout, 3, 3, 1) or (Cin >= 128 and Cin % 32 == 0 and W <= 31)


class ResNetBlockFn(torch.autograd.Function):
    """x: act NHWC [N,H,W,Cin] -> act NHWC [N,OH,OW,Cout]"""

    # BatchNorm-backward fusion across blocks: a block whose output feeds ONLY the next block (chain=True, set by nnet.ResNet) registers (y2, out, ss2) under its
    # output's address; the next block's backward folds the mask + (sum d, sum d*y2) reduction of that BatchNorm into the epilogue of the product that computes its
    # input gradient and leaves the completed request under the gradient's address (in the pass state) for the producer block's backward
    _CHAIN = {}

    @staticmethod
    def forward(ctx, x, _anchor, blk, training, chain=False):
        rt.require_gpu(x)
        N, H, W, Cin = x.shape
        conv1, bn1, conv2, bn2 = blk.layers[0], blk.layers[1], blk.layers[3], blk.layers[4]
        stride = conv1.stride[0]
        Cout = conv1.weight.shape[0]
        adt = rt.act_dtype()
        x = x.contiguous()
        st1, st2 = BNState(Cout, x), BNState(Cout, x)
        y1, OH, OW = conv2d_fwd(x, conv1.weight, N, H, W, Cin, stride, stats=st1.stats if training else None)
        Mo = N * OH * OW
        c1 = bn_finalize(bn1, st1, Mo, training)
        a1 = empty((Mo, Cout), adt, x)
        lib.bn_apply_fwd(rt.dt(), y1.data_ptr(), st1.ss.data_ptr(), None, ACT_RELU, a1.data_ptr(), Mo, Cout, rt.stream())
        y2, _, _ = conv2d_fwd(a1, conv2.weight, N, OH, OW, Cout, 1, stats=st2.stats if training else None)
        c2 = bn_finalize(bn2, st2, Mo, training)
        has_proj = not isinstance(blk.residual, torch.nn.Identity)
        yr = str_ = cr = None
        if has_proj:
            convr, bnr = blk.residual[0], blk.residual[1]
            str_ = BNState(Cout, x)
            yr, _, _ = conv2d_fwd(x, convr.weight, N, H, W, Cin, stride, stats=str_.stats if training else None)
            cr = bn_finalize(bnr, str_, Mo, training)
        use_mask = RELU_BITMASK and training and Cout % 8 == 0 and Cout <= 2048 and Mo * Cout // 8 < (1 << 31)
        if has_proj and not use_mask:
            r = empty((Mo, Cout), adt, x)
            lib.bn_apply_fwd(rt.dt(), yr.data_ptr(), str_.ss.data_ptr(), None, ACT_NONE, r.data_ptr(), Mo, Cout, rt.stream())
        elif not has_proj:
            r = x
        out = empty((Mo, Cout), adt, x)
        ctx.relu_mask = None
        if use_mask:
            # the backward pass needs `out` only as a ReLU mask: one bit per element, written here, instead of re-reading the tensor twice (reduction + apply pass);
            # a projection shortcut is normalised on the fly from its raw convolution output (no tensor, no launch of its own)
            ctx.relu_mask = torch.empty(Mo * Cout // 8, dtype=torch.uint8, device=x.device)
            lib.bn_apply_fwd_mask(rt.dt(), y2.data_ptr(), st2.ss.data_ptr(), (yr if has_proj else r).data_ptr(), str_.ss.data_ptr() if has_proj else None, out.data_ptr(),
                                  ctx.relu_mask.data_ptr(), Mo, Cout, rt.stream())
        else:
            lib.bn_apply_fwd(rt.dt(), y2.data_ptr(), st2.ss.data_ptr(), r.data_ptr(), ACT_RELU, out.data_ptr(), Mo, Cout, rt.stream())
        ctx.saved = (x, y1, a1, y2, yr, out, st1, st2, str_, c1, c2, cr, blk, training, N, H, W, Cin, Cout, OH, OW, stride, has_proj)
        ctx.chain = bool(chain and training and BNB_FUSE and rt.act_dtype() == torch.bfloat16)
        if ctx.chain:
            if len(ResNetBlockFn._CHAIN) > 64:
                ResNetBlockFn._CHAIN.clear()
            ResNetBlockFn._CHAIN[out.data_ptr()] = (y2, out, st2, Cout)
        return out.view(N, OH, OW, Cout)

    @staticmethod
    def backward(ctx, dout):
        x, y1, a1, y2, yr, out, st1, st2, str_, c1, c2, cr, blk, training, N, H, W, Cin, Cout, OH, OW, stride, has_proj = ctx.saved
        conv1, bn1, conv2, bn2 = blk.layers[0], blk.layers[1], blk.layers[3], blk.layers[4]
        Mo = N * OH * OW
        dout = dout.reshape(Mo, Cout).to(rt.act_dtype()).contiguous()
        assert training, "ResNetBlock backward is implemented for training-mode BatchNorm"
        ResNetBlockFn._CHAIN.pop(out.data_ptr(), None)
        pre2 = _pass().bn_ready.pop(dout.data_ptr(), None) if ctx.chain else None      # the consumer block already masked dout and reduced it against y2
        if pre2 is not None and pre2.y is not y2:
            raise RuntimeError("ResNetBlock backward: a fused BatchNorm-backward request does not belong to this block (the block output has another consumer?)")
        # the gradient that passed the block's final ReLU is needed twice more (second BatchNorm's backward above all, then as the residual branch's gradient): with the bit
        # mask at hand nobody needs it as a tensor -- the consumers below apply the mask themselves
        lazy_dres = (not BNB_FUSE and ctx.relu_mask is not None and pre2 is None and
                     (has_proj or (conv1.weight.shape[2] == 3 and res_mask_ok(H, W, Cin, Cout, stride) and not KERNEL_TIMER.enabled)))
        dy2, dres = bn_backward(bn2, st2, c2, Mo, dout, y2, out, ACT_RELU, Mo, want_dres=not lazy_dres, pre=pre2, mask=ctx.relu_mask)
        f1 = BnbFuse(y1, st1.ss, None, Cout)        # BatchNorm 1 + ReLU: the mask comes from the pre-activation itself
        da1 = conv2d_bwd(dy2, a1, conv2.weight, N, OH, OW, Cout, 1, OH, OW, bnb=f1)
        dy1, _ = bn_backward(bn1, st1, c1, Mo, da1, y1, None, ACT_RELU, Mo, pre=f1 if f1.done else None)      # no residual before this ReLU: the mask is recomputed from y1 (one tensor less to read)
        need_dx = ctx.needs_input_grad[0]
        prev = ResNetBlockFn._CHAIN.get(x.data_ptr()) if need_dx else None
        fx = BnbFuse(prev[0], prev[2].ss, prev[1], prev[3]) if prev is not None else None
        if has_proj:
            convr, bnr = blk.residual[0], blk.residual[1]
            if lazy_dres:
                dyr, _ = bn_backward(bnr, str_, cr, Mo, dout, yr, None, ACT_NONE, Mo, mask=ctx.relu_mask)      # (mask variant: d = bit ? dout : 0, no activation of its own)
            else:
                dyr, _ = bn_backward(bnr, str_, cr, Mo, dres, yr, None, ACT_NONE, Mo)
            kr = convr.weight.shape[2]
            if (SHORTCUT_SUBGRID and need_dx and stride == 2 and kr == 1 and rt.act_dtype() == torch.bfloat16 and Cin % 64 == 0 and Cout % 64 == 0
                    and conv1.weight.shape[2] == 3 and not _slab_conv(H, W, Cin, Cout, 3, 3, stride)):
                # the 1x1 / stride-2 shortcut sends its gradient to the (even, even) input pixels only: a plain product on the subsampled grid, added by the 3x3
                # layer's backward-data epilogue to its class-0 tiles -- instead of a full-size, three-quarters-zero tensor written and read back
                conv2d_bwd(dyr, x, convr.weight, N, H, W, Cin, stride, OH, OW, need_dx=False)
                dxs = empty((Mo, Cin), rt.act_dtype(), dyr)
                gemm_nt(dyr, rt.shadow(convr.weight).bwd, dxs, Mo, Cin, Cout)
                dx = conv2d_bwd(dy1, x, conv1.weight, N, H, W, Cin, stride, OH, OW, need_dx=True, dx_res=dxs, bnb=fx, dx_res_cls0=True)
            else:
                dx = conv2d_bwd(dyr, x, convr.weight, N, H, W, Cin, stride, OH, OW, need_dx=need_dx)
                dx = conv2d_bwd(dy1, x, conv1.weight, N, H, W, Cin, stride, OH, OW, need_dx=need_dx, dx_res=dx, bnb=fx)
        else:
            if lazy_dres:
                dx = conv2d_bwd(dy1, x, conv1.weight, N, H, W, Cin, stride, OH, OW, need_dx=need_dx, dx_res=dout, dx_res_mask=ctx.relu_mask, bnb=fx)
            else:
                dx = conv2d_bwd(dy1, x, conv1.weight, N, H, W, Cin, stride, OH, OW, need_dx=need_dx, dx_res=dres, bnb=fx)
        if fx is not None and fx.done:
            _pass().bn_ready[dx.data_ptr()] = fx
        return (dx.view(N, H, W, Cin) if dx is not None else None), None, None, None, None


STEM3D_DIRECT = True      # direct (no im2col) bf16 visual-stem kernels
STEM3P_FUSED_WGRAD = True  # ... and the weight gradient computed from the recomputed tiles in the same kernel (no dz tensor)
STEM3P = True                    # ... with the max pool inside the convolution kernel and the pre-pool tensor recomputed in backward (stem3p.hip)


class VideoStemFn(torch.autograd.Function):
    """Conv3d(1->C,(5,7,7),s(1,2,2),'same',bias) + BatchNorm3d + ReLU + MaxPool3d((1,3,3),s(1,2,2),'same')
    video fp32 [B,T,H,W] -> act NHWC [B*T, H/4, W/4, C]      (nnet/networks.py:459-470)"""

    @staticmethod
    def forward(ctx, video, _anchor, conv, bn, training):
        rt.require_gpu(video)
        B, T, H, W = video.shape
        C = conv.weight.shape[0]
        v = _f32c(video)
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        M = B * T * OH * OW
        sh = rt.shadow(conv.weight)
        st = BNState(C, v)
        K, Kp = sh.Tm * sh.C, sh.Cp
        y = empty((M, C), rt.act_dtype(), v)
        if (STEM3P and STEM3D_DIRECT and rt.compute_dtype() == "bf16" and C == 64 and K == 245 and lib.raw("avec_stem3p_supported")(B, T, H, W)
                and lib.raw("avec_stem3d_supported")(B, T, H, W)):
            # round 3 (stem3p.hip): the max pool runs on the raw conv output inside the convolution kernel (BatchNorm + ReLU is monotone per channel); the
            # 793 MB pre-pool tensor never reaches memory, the backward pass recomputes it
            w8 = torch.zeros((C, 36, 8), dtype=sh.fwd.dtype, device=v.device)         # (kd,kh) rows: zero slot, then the 7 taps
            w8[:, :35, 1:] = sh.fwd.view(C, Kp)[:, :K].view(C, 35, 7)
            vb = v.to(torch.bfloat16)
            PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
            zp = torch.empty((B * T, PH, PW, C), dtype=torch.bfloat16, device=v.device)
            idx = torch.empty((B * T, PH, PW, C), dtype=torch.uint8, device=v.device)
            lib.stem3p_fwd(vb.data_ptr(), w8.data_ptr(), _p(conv.bias), bn.weight.data_ptr(), zp.data_ptr(), idx.data_ptr(), st.stats.data_ptr() if training else None,
                           B, T, H, W, rt.stream())
            cp = bn_finalize(bn, st, M, training)
            out = torch.empty_like(zp)
            lib.bn_apply_fwd(rt.dt(), zp.data_ptr(), st.ss.data_ptr(), None, ACT_RELU, out.data_ptr(), B * T * PH * PW, C, rt.stream())
            ctx.saved = (v, None, idx, st, cp, conv, bn, ("p", vb, w8, zp, PH, PW), B, T, OH, OW, C, M, K, training, None)
            return out
        if STEM3D_DIRECT and rt.compute_dtype() == "bf16" and C == 64 and K == 245 and lib.raw("avec_stem3d_supported")(B, T, H, W):
            # direct kernels (stem3d.hip): the input band is staged in LDS, no im2col matrix in HBM
            w8 = torch.zeros((C, 36, 8), dtype=sh.fwd.dtype, device=v.device)         # (kd,kh) rows of 7 taps + a zero slot (stem3d.hip)
            w8[:, :35, :7] = sh.fwd.view(C, Kp)[:, :K].view(C, 35, 7)
            lib.stem3d_fwd(v.data_ptr(), w8.data_ptr(), 288, _p(conv.bias), y.data_ptr(), st.stats.data_ptr() if training else None, B, T, H, W, rt.stream())
            r = None
        else:
            # im2col once (shared by the forward GEMM and the weight-gradient GEMM), then a plain MFMA GEMM with K padded to Kp
            A = empty((M, Kp), rt.act_dtype(), v)
            lib.stem_im2col(rt.dt(), v.data_ptr(), A.data_ptr(), B, T, H, W, Kp, rt.stream())
            gemm_nt(A, sh.fwd, y, M, C, Kp, bias=conv.bias, stats=st.stats if training else None)
            r = A
        cp = bn_finalize(bn, st, M, training)
        PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
        out = empty((B * T, PH, PW, C), rt.act_dtype(), v)
        idx = torch.empty((B * T, PH, PW, C), dtype=torch.uint8, device=v.device)
        ymax = torch.empty_like(out) if (training and C % 8 == 0) else None           # winners' pre-BN values: the backward statistics pass then reads pooled-size tensors only
        lib.stem_pool_fwd(rt.dt(), y.data_ptr(), st.ss.data_ptr(), out.data_ptr(), idx.data_ptr(), _p(ymax), B * T, OH, OW, C, rt.stream())
        ctx.saved = (v, y, idx, st, cp, conv, bn, r, B, T, OH, OW, C, M, K, training, ymax)
        return out

    @staticmethod
    def backward(ctx, dpool):
        v, y, idx, st, cp, conv, bn, r, B, T, OH, OW, C, M, K, training, ymax = ctx.saved
        assert training, "VideoStem backward is implemented for training-mode BatchNorm"
        dpool = dpool.to(rt.act_dtype()).contiguous()
        if isinstance(r, tuple):                                # stem3p: ReLU mask + BatchNorm-backward sums over the pooled tensor, then dz from the RECOMPUTED conv output
            _, vb, w8, zp, PH, PW = r
            H, W = v.shape[2], v.shape[3]
            dstats = torch.zeros(2 * C, dtype=torch.float32, device=v.device)
            # dpool is masked IN PLACE: it is the first ResNet block's dx (99 MB), which nothing else reads -- a hook or retain_grad on the stem's output sees the masked gradient
            lib.stem3p_reduce(dpool.data_ptr(), zp.data_ptr(), st.ss.data_ptr(), dstats.data_ptr(), B * T, PH, PW, rt.stream())
            dstats, gw, gb = _bn_sync_grads(bn, dstats, C)
            if STEM3P_FUSED_WGRAD and lib.raw("avec_stem3p_wgrad_supported")(B, T, H, W):
                # recompute + routing + weight gradient in ONE kernel: neither z nor dz exist in memory
                lib.stem3p_wgrad(vb.data_ptr(), w8.data_ptr(), _p(conv.bias), dpool.data_ptr(), idx.data_ptr(), st.ss.data_ptr(), bn.weight.data_ptr(), dstats.data_ptr(), cp, float(M),
                                 grad_of(conv.weight).data_ptr(), _p(gw), _p(gb), B, T, H, W, rt.stream())
            else:
                dy = empty((M, C), rt.act_dtype(), v)
                lib.stem3p_dz(vb.data_ptr(), w8.data_ptr(), _p(conv.bias), dpool.data_ptr(), idx.data_ptr(), st.ss.data_ptr(), bn.weight.data_ptr(), dstats.data_ptr(), cp, float(M),
                              dy.data_ptr(), _p(gw), _p(gb), B, T, H, W, rt.stream())
                lib.stem3d_wgrad(v.data_ptr(), dy.data_ptr(), grad_of(conv.weight).data_ptr(), B, T, H, W, rt.stream())
            if conv.bias is not None:
                grad_of(conv.bias)
            stamp("v_stem_end:b")
            return None, None, None, None, None
        dstats = torch.zeros(2 * C, dtype=torch.float32, device=v.device)

        def common(ds):          # what both phases of avec_stem_pool_bwd take; ds: the sums phase 0 writes / phase 1 reads
            return dpool.data_ptr(), idx.data_ptr(), y.data_ptr(), st.ss.data_ptr(), bn.weight.data_ptr(), ds.data_ptr(), cp, float(M)
        if ymax is not None:
            lib.stem_pool_bwd_reduce_pooled(rt.dt(), dpool.data_ptr(), idx.data_ptr(), ymax.data_ptr(), st.ss.data_ptr(), dstats.data_ptr(), B * T, OH, OW, C, rt.stream())
        else:
            lib.stem_pool_bwd(rt.dt(), *common(dstats), 0, None, None, None, B * T, OH, OW, C, rt.stream())
        dstats, gw, gb = _bn_sync_grads(bn, dstats, C)
        dy = empty((M, C), rt.act_dtype(), v)
        lib.stem_pool_bwd(rt.dt(), *common(dstats), 1, dy.data_ptr(), _p(gw), _p(gb), B * T, OH, OW, C, rt.stream())
        if r is None:
            H, W = v.shape[2], v.shape[3]
            lib.stem3d_wgrad(v.data_ptr(), dy.data_ptr(), grad_of(conv.weight).data_ptr(), B, T, H, W, rt.stream())
        else:
            gemm_tn(dy, r, grad_of(conv.weight), M, C, K, q_rows=rows_plain(r.shape[1]), side=True)
        if conv.bias is not None:
            grad_of(conv.bias)   # d(bias) before training-mode BatchNorm is analytically zero: left at 0
        return None, None, None, None, None


class AvgPoolFn(torch.autograd.Function):
    """GlobalAvgPool2d on act NHWC [N,H,W,C] -> act [N,C]"""

    @staticmethod
    def forward(ctx, x):
        N, H, W, C = x.shape
        x = x.contiguous()
        y = empty((N, C), x.dtype, x)
        lib.avgpool_fwd(rt.dt(), x.data_ptr(), y.data_ptr(), N, H * W, C, rt.stream())
        ctx.saved = (N, H, W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, H, W, C = ctx.saved
        dy = dy.to(rt.act_dtype()).contiguous()
        dx = empty((N, H, W, C), dy.dtype, dy)
        lib.avgpool_bwd(rt.dt(), dy.data_ptr(), dx.data_ptr(), N, H * W, C, rt.stream())
        return dx


class AudioStemFn(torch.autograd.Function):
    """Conv2d(1->C,3x3,s2,'same') + BatchNorm2d + Swish on mel [B,80,F] -> act [B, T', C*40]   (nnet/networks.py:359-377)"""

    @staticmethod
    def forward(ctx, mel, _anchor, conv, bn, training):
        rt.require_gpu(mel)
        B, NM, F = mel.shape
        C = conv.weight.shape[0]
        mel = _f32c(mel)
        Fo, To = (NM - 1) // 2 + 1, (F - 1) // 2 + 1
        adt = rt.act_dtype()
        y = empty((B * To, C * Fo), adt, mel)
        st = BNState(C, mel)
        lib.audio_stem_conv_fwd(rt.dt(), mel.data_ptr(), conv.weight.data_ptr(), _p(conv.bias), y.data_ptr(), st.stats.data_ptr() if training else None,
                                B, NM, F, C, rt.stream())
        count = B * To * Fo
        cp = bn_finalize(bn, st, count, training)
        a = empty((B, To, C * Fo), adt, mel)
        lib.audio_stem_act_fwd(rt.dt(), y.data_ptr(), st.ss.data_ptr(), a.data_ptr(), B, NM, F, C, rt.stream())
        ctx.saved = (mel, y, st, cp, count, conv, bn, B, NM, F, C, training)
        return a

    @staticmethod
    def backward(ctx, da):
        mel, y, st, cp, count, conv, bn, B, NM, F, C, training = ctx.saved
        assert training, "AudioStem backward is implemented for training-mode BatchNorm"
        flush_param_grads()                                   # last node of the audio branch: its queued parameter gradients go out on this (the branch's) stream
        da = da.to(rt.act_dtype()).contiguous()
        dstats = torch.zeros(2 * C, dtype=torch.float32, device=mel.device)

        def common(ds):          # what both phases of avec_audio_stem_bwd take; ds: the sums phase 0 writes / phase 1 reads
            return da.data_ptr(), y.data_ptr(), mel.data_ptr(), st.ss.data_ptr(), bn.weight.data_ptr(), ds.data_ptr(), cp, float(count)
        lib.audio_stem_bwd(rt.dt(), *common(dstats), 0, None, None, None, None, B, NM, F, C, rt.stream())
        dstats, gw, gb = _bn_sync_grads(bn, dstats, C)
        lib.audio_stem_bwd(rt.dt(), *common(dstats), 1, grad_of(conv.weight).data_ptr(), None if conv.bias is None else grad_of(conv.bias).data_ptr(),
                           _p(gw), _p(gb), B, NM, F, C, rt.stream())
        stamp("a_stem_end:b")
        arena = rt.arena_of(bn)
        if arena is not None and getattr(arena, "_early_armed", False) and getattr(arena, "_audio_range", None):
            lo, hi = arena._audio_range                       # the stem is the first op of the audio encoder: its backward is the last one of that branch
            arena._audio_range = None
            arena.early_all_reduce(lo, hi)
        return None, None, None, None, None


# ============================================================================================
# mel front-end (no gradient): AudioPreprocessing.forward (nnet/preprocessing.py:57-85)
# ============================================================================================
def mel_spectrogram(audio, window, dft, fb, n_fft, win, hop, n_mels):
    """audio fp32 [B,L]; window [win]; dft fp32 [2*nb][win] (cos rows then -sin rows); fb [nb][n_mels] -> [B,n_mels,L//hop+1] fp32"""
    rt.require_gpu(audio)
    B, L = audio.shape
    audio = _f32c(audio)
    F = L // hop + 1
    frames = empty((B * F, win), torch.float32, audio)
    lib.mel_frames(audio.data_ptr(), window.data_ptr(), frames.data_ptr(), B, L, n_fft, win, hop, rt.stream())
    return mel_from_frames(frames, dft, fb, B, F, n_mels)


def spec_augment_(mel, lens, mF, Fp, mT, pS, sid):
    B, NM, F = mel.shape
    lens_ = None if lens is None else lens.to(device=mel.device, dtype=torch.int64).contiguous()
    lib.specaugment(mel.data_ptr(), _p(lens_), B, NM, F, mF, Fp, mT, pS, _rng(mel.device), sid, rt.stream())
    return mel


def len_affine(lengths, sub, div, add):
    """floor((lengths - sub) / div) + add on an int64 length vector: one launch on the device (three ATen launches otherwise), plain torch on the host"""
    if torch.is_tensor(lengths) and lengths.is_cuda and lengths.dtype == torch.int64 and lengths.is_contiguous() and lengths.numel() > 0:
        out = torch.empty_like(lengths)
        lib.len_affine(lengths.data_ptr(), out.data_ptr(), lengths.numel(), sub, div, add, rt.stream())
        return out
    return torch.div(lengths - sub, div, rounding_mode="floor") + add


def argmax_rows(logits):
    lead, V = logits.shape[:-1], logits.shape[-1]
    lg = _f32c(logits)
    out = torch.empty(lead, dtype=torch.int64, device=lg.device)
    lib.argmax_rows(lg.data_ptr(), out.data_ptr(), out.numel(), V, rt.stream())
    return out


def weight_average(avg, p, mode, wa=0.0, wp=0.0):
    """One launch over two flat fp32 arenas of the same size (a multiple of 4 elements): mode 0 avg = p, mode 1 avg = avg + wp * (p - avg), mode 2
    avg = (wa * avg) + (wp * p), every operation a single correctly rounded fp32 one (include/avec_hip.h).  In place on `avg`; graph-capturable."""
    rt.require_gpu(avg)
    rt.require_gpu(p)
    if not (avg.dtype == p.dtype == torch.float32 and avg.dim() == p.dim() == 1 and avg.is_contiguous() and p.is_contiguous() and avg.numel() == p.numel()):
        raise RuntimeError("weight_average: two flat contiguous fp32 buffers of the same size are needed (got %s %s and %s %s)"
                           % (tuple(avg.shape), avg.dtype, tuple(p.shape), p.dtype))
    lib.weight_average(avg.data_ptr(), p.data_ptr(), int(mode), float(wa), float(wp), avg.numel(), rt.stream())
    return avg


def grad_norm_workspace(n, device):
    """the fp64 partial sums of ops.grad_norm for an arena of n elements (a few KB: one per workgroup of the first launch)"""
    return torch.empty(max(int(lib.raw("avec_grad_norm_workspace_bytes")(int(n))), 8) // 8, dtype=torch.float64, device=device)


def grad_norm(grad, workspace, stats, flag, grad_scale=1.0, max_norm=None, skip_nonfinite=False, skip_in=None):
    """Global L2 norm of the flat fp32 gradient arena times `grad_scale`, and torch.nn.utils.clip_grad_norm_'s factor for `max_norm` (None: 1), on the device:
    stats (fp32 [2]) = {norm, coef}, flag (int32 [2]) = {skip this step, steps skipped so far} (include/avec_hip.h).  Two launches, no atomics, no host
    synchronisation, graph-capturable; the optimizer launch reads both (Adam.launch_step(clip=True))."""
    rt.require_gpu(grad)
    if not (grad.dtype == torch.float32 and grad.dim() == 1 and grad.is_contiguous() and stats.dtype == torch.float32 and stats.numel() >= 2
            and flag.dtype == torch.int32 and flag.numel() >= 2 and (skip_in is None or skip_in.dtype == torch.int32)):
        raise RuntimeError("grad_norm: a flat contiguous fp32 arena, fp32 stats[2] and int32 flag[2] are needed (got %s %s, %s, %s)"
                           % (tuple(grad.shape), grad.dtype, stats.dtype, flag.dtype))
    lib.grad_norm(grad.data_ptr(), grad.numel(), float(grad_scale), 0.0 if max_norm is None else float(max_norm), int(bool(skip_nonfinite)), _p(skip_in),
                  workspace.data_ptr(), workspace.numel() * workspace.element_size(), stats.data_ptr(), flag.data_ptr(), rt.stream())
    return stats


def ctc_beam_search(logits, lengths, beam, tmp=1.0, lm=None, alpha=0.6, beta=1.0):
    """CTC prefix beam search (blank 0) of logits [B, T, V] with lengths [B], optionally fused with an n-gram LM (avec_amd.ngram.NGramLM):
    one launch for the whole batch.  Returns tokens [B, beam, T] int32, out_len [B, beam] int32, score [B, beam] (ranking score, best first) and
    ctc_logp [B, beam]; empty slots have score -inf and length 0.  alpha / beta are ignored without an LM."""
    B, T, V = logits.shape
    lg = _f32c(logits)
    dev = lg.device
    lens = lengths.to(device=dev, dtype=torch.int64).contiguous()
    st = rt.stream()
    ws = torch.empty(lib.raw("avec_ctc_beam_workspace_bytes")(B, T, beam), dtype=torch.uint8, device=dev)
    tokens = torch.empty(B, beam, T, dtype=torch.int32, device=dev)
    out_len = torch.empty(B, beam, dtype=torch.int32, device=dev)
    score = torch.empty(B, beam, dtype=torch.float32, device=dev)
    ctc_logp = torch.empty(B, beam, dtype=torch.float32, device=dev)
    use_lm = lm is not None and lm.usable
    lm_arg = _byref(lm.device_struct(dev)) if use_lm else None
    oov = lm.oov_logprob if use_lm else 0.0
    lib.ctc_beam_search(lg.data_ptr(), lens.data_ptr(), B, T, V, beam, 1.0 / tmp, lm_arg, alpha if use_lm else 0.0, beta if use_lm else 0.0, oov,
                        ws.data_ptr(), ws.numel(), tokens.data_ptr(), out_len.data_ptr(), score.data_ptr(), ctc_logp.data_ptr(), st)
    return tokens, out_len, score, ctc_logp


def _slot_vec(op, name, t, B, dev, mask=False, convert=False):
    """A per-slot control vector of a streaming op: None, or a contiguous tensor [B] on the GPU `dev`, int64 counts or (mask) a uint8 / bool mask.  Returns it;
    anything else raises, unless `convert` (ctc_beam_stream's chunk_len) asks for the counts to be brought into that form."""
    if t is None or (t.is_cuda and t.device == dev and t.is_contiguous() and t.numel() == B and (t.dtype in (torch.uint8, torch.bool) if mask else t.dtype == torch.int64)):
        return t
    if convert:
        return t.to(device=dev, dtype=torch.int64).contiguous().view(B)
    raise ValueError("%s: %s must be a contiguous %s [%d] on the device" % (op, name, "uint8 / bool mask" if mask else "int64 tensor", B))


class CTCBeamStreamState:
    """Everything a streaming beam search keeps between pushes (ops.ctc_beam_stream), allocated once: the beam state and backpointer rows of avec_ctc_beam_stream,
    the outputs it writes when it emits, and a reset flag buffer.  batch utterance slots, `beam` beams, at most max_frames frames per utterance.  A zero-filled
    state is a reset one."""

    def __init__(self, batch, beam, max_frames, device=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.B, self.W, self.Tcap = int(batch), int(beam), int(max_frames)
        if self.B < 1 or self.Tcap < 1 or not 1 <= self.W <= 64:
            raise ValueError("CTCBeamStreamState: batch %d, beam %d (1..64), max_frames %d" % (self.B, self.W, self.Tcap))
        self.state = torch.zeros(lib.raw("avec_ctc_beam_state_bytes")(self.B, self.W), dtype=torch.uint8, device=dev)
        self.backptr = torch.empty(lib.raw("avec_ctc_beam_workspace_bytes")(self.B, self.Tcap, self.W), dtype=torch.uint8, device=dev)
        self.tokens = torch.zeros(self.B, self.W, self.Tcap, dtype=torch.int32, device=dev)
        self.out_len = torch.zeros(self.B, self.W, dtype=torch.int32, device=dev)
        self.score = torch.full((self.B, self.W), float("-inf"), dtype=torch.float32, device=dev)
        self.ctc_logp = torch.full((self.B, self.W), float("-inf"), dtype=torch.float32, device=dev)
        self.stable_len = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.reset_flags = torch.zeros(self.B, dtype=torch.uint8, device=dev)


def ctc_beam_stream(st, logits, chunk_len=None, reset=None, tmp=1.0, lm=None, alpha=0.6, beta=1.0, emit=True):
    """One push of the streaming CTC prefix beam search: `st` (a CTCBeamStreamState) consumes the chunk logits [B, Tc, V]; utterance b takes chunk_len[b] frames
    (int64 [B] on the device; None: all Tc), clamped so that it never holds more than st.Tcap.  reset: None, or a uint8 / bool mask [B] on the device whose set
    slots restart from the empty prefix before the chunk.  tmp, lm, alpha, beta as ops.ctc_beam_search, the same for every push of a session.  With emit the
    state's tokens [B, W, Tcap], out_len, score, ctc_logp hold what ops.ctc_beam_search gives on the frames pushed so far (bit for bit) and stable_len [B] the
    length of the common prefix of the live beams, which no later frame can change; they are returned (views of st, overwritten by the next emitting push).
    One launch, no host synchronisation, no allocation beyond the fp32 conversion of the chunk."""
    B, Tc, V = logits.shape
    if B != st.B:
        raise ValueError("ctc_beam_stream: chunk of %d utterances for a state of %d" % (B, st.B))
    lg = _f32c(logits)
    dev = st.state.device
    if lg.device != dev:
        raise ValueError("ctc_beam_stream: chunk on %s, state on %s" % (lg.device, dev))
    chunk_len = _slot_vec("ctc_beam_stream", "chunk_len", chunk_len, B, dev, convert=True)
    _slot_vec("ctc_beam_stream", "reset", reset, B, dev, mask=True)
    use_lm = lm is not None and lm.usable
    lm_arg = _byref(lm.device_struct(dev)) if use_lm else None
    oov = lm.oov_logprob if use_lm else 0.0
    lib.ctc_beam_stream(lg.data_ptr(), _p(chunk_len), _p(reset), B, Tc, V, st.W, st.Tcap, 1.0 / tmp, lm_arg, alpha if use_lm else 0.0, beta if use_lm else 0.0, oov,
                        st.state.data_ptr(), st.state.numel(), st.backptr.data_ptr(), st.backptr.numel(), st.tokens.data_ptr(), st.out_len.data_ptr(),
                        st.score.data_ptr(), st.ctc_logp.data_ptr(), st.stable_len.data_ptr(), 1 if emit else 0, rt.stream())
    return (st.tokens, st.out_len, st.score, st.ctc_logp, st.stable_len) if emit else None


class CTCBeamRingState:
    """Everything an endless streaming beam search keeps between pushes (ops.ctc_beam_stream_ring), allocated once: the beam state, the `window` backpointer rows and
    the commit log of avec_ctc_beam_stream_ring, the outputs it writes when it emits, and a reset flag buffer.  batch utterance slots, `beam` beams, a commit log of
    log_frames (token, frame) entries per slot.  A zero-filled state is a reset one."""

    def __init__(self, batch, beam, window, log_frames, device=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.B, self.W, self.window, self.log_frames = int(batch), int(beam), int(window), int(log_frames)
        if self.B < 1 or self.window < 2 or self.log_frames < 1 or not 1 <= self.W <= 64:
            raise ValueError("CTCBeamRingState: batch %d, beam %d (1..64), window %d (>= 2), log_frames %d" % (self.B, self.W, self.window, self.log_frames))
        self.state = torch.zeros(lib.raw("avec_ctc_beam_ring_state_bytes")(self.B, self.W), dtype=torch.uint8, device=dev)
        self.backptr = torch.empty(lib.raw("avec_ctc_beam_ring_workspace_bytes")(self.B, self.window, self.W), dtype=torch.uint8, device=dev)
        self.log = torch.zeros(self.B, self.log_frames, 2, dtype=torch.int32, device=dev)
        self.tokens = torch.zeros(self.B, self.W, self.window, dtype=torch.int32, device=dev)
        self.frames = torch.zeros(self.B, self.W, self.window, dtype=torch.int32, device=dev)
        self.out_len = torch.zeros(self.B, self.W, dtype=torch.int32, device=dev)
        self.score = torch.full((self.B, self.W), float("-inf"), dtype=torch.float32, device=dev)
        self.ctc_logp = torch.full((self.B, self.W), float("-inf"), dtype=torch.float32, device=dev)
        self.stable_len = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.info = torch.zeros(self.B, 4, dtype=torch.int32, device=dev)
        self.reset_flags = torch.zeros(self.B, dtype=torch.uint8, device=dev)

    def header(self):
        """[B, 8] int32 view of the state: {live beams, frames consumed, tag, window, base, ccount, dropped, commits} as the last push left them"""
        return self.state.view(torch.int32).view(self.B, -1)[:, -8:]


def ctc_beam_stream_ring(st, logits, chunk_len=None, reset=None, tmp=1.0, lm=None, alpha=0.6, beta=1.0, emit=True):
    """One push of the endless streaming CTC prefix beam search (window-limited: include/avec_hip.h, avec_ctc_beam_stream_ring): `st` (a CTCBeamRingState) consumes the
    chunk logits [B, Tc, V]; utterance b takes chunk_len[b] frames (int64 [B] on the device; None: all Tc) and no push is ever too long.  reset, tmp, lm, alpha, beta as
    ops.ctc_beam_stream.  History older than the window is committed to st.log as the frames pass (entry k % log_frames = committed token k and its frame).  With emit
    the state's tokens and frames [B, W, window] hold every beam's tail after the committed tokens and the frame that emitted each, out_len the tail lengths, score
    and ctc_logp the beams' scores, stable_len [B] = committed tokens + the common prefix of the tails, info [B, 4] = {base, ccount, dropped, commits}; they are returned
    (views of st, overwritten by the next emitting push).  One launch, no host synchronisation, no allocation beyond the fp32 conversion of the chunk."""
    B, Tc, V = logits.shape
    if B != st.B:
        raise ValueError("ctc_beam_stream_ring: chunk of %d utterances for a state of %d" % (B, st.B))
    lg = _f32c(logits)
    dev = st.state.device
    if lg.device != dev:
        raise ValueError("ctc_beam_stream_ring: chunk on %s, state on %s" % (lg.device, dev))
    chunk_len = _slot_vec("ctc_beam_stream_ring", "chunk_len", chunk_len, B, dev, convert=True)
    _slot_vec("ctc_beam_stream_ring", "reset", reset, B, dev, mask=True)
    use_lm = lm is not None and lm.usable
    lm_arg = _byref(lm.device_struct(dev)) if use_lm else None
    oov = lm.oov_logprob if use_lm else 0.0
    lib.ctc_beam_stream_ring(lg.data_ptr(), _p(chunk_len), _p(reset), B, Tc, V, st.W, st.window, st.log_frames, 1.0 / tmp, lm_arg, alpha if use_lm else 0.0,
                             beta if use_lm else 0.0, oov, st.state.data_ptr(), st.state.numel(), st.backptr.data_ptr(), st.backptr.numel(), st.log.data_ptr(),
                             st.log.numel() * 4, st.tokens.data_ptr(), st.frames.data_ptr(), st.out_len.data_ptr(), st.score.data_ptr(), st.ctc_logp.data_ptr(),
                             st.stable_len.data_ptr(), st.info.data_ptr(), 1 if emit else 0, rt.stream())
    return (st.tokens, st.frames, st.out_len, st.score, st.ctc_logp, st.stable_len, st.info) if emit else None


def ctc_align(logits, logits_len, targets, target_len, blank=0, tier=0):
    """CTC forced alignment (Viterbi) of targets [B, Lmax] (target_len [B]) to logits [B, T, V] (logits_len [B]): one launch for the whole batch, no host
    synchronisation.  Returns path [B, T] int32 (the token of every frame, -1 past logits_len), spans [B, Lmax, 2] int32 ((first frame, last frame + 1) of every
    target token, -1 past target_len), score [B] (log-probability of the best path) and token_logp [B, Lmax]; an utterance that cannot be aligned has score -inf,
    path and spans -1 (include/avec_hip.h: avec_ctc_align).  tier: 0 auto, 1 all-LDS, 2 workspace (same results bit for bit)."""
    rt.require_gpu(logits)
    B, T, V = logits.shape
    lg = _f32c(logits)
    dev = lg.device
    tg = targets.to(device=dev, dtype=torch.int64)
    if tg.dim() == 1:
        tg = tg.view(B, -1)
    tg = tg.contiguous()
    Lmax = tg.shape[1]
    il = logits_len.to(device=dev, dtype=torch.int64).contiguous()
    tl = target_len.to(device=dev, dtype=torch.int64).contiguous()
    ws = torch.empty(max(16, lib.raw("avec_ctc_align_workspace_bytes")(B, T, Lmax)), dtype=torch.uint8, device=dev)
    path = torch.empty(B, T, dtype=torch.int32, device=dev)
    spans = torch.empty(B, Lmax, 2, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    token_logp = torch.empty(B, Lmax, dtype=torch.float32, device=dev)
    lib.ctc_align(lg.data_ptr(), il.data_ptr(), _p(tg), tl.data_ptr(), B, T, V, Lmax, blank, tier, ws.data_ptr(), ws.numel(),
                  path.data_ptr(), _p(spans), score.data_ptr(), _p(token_logp), rt.stream())
    return path, spans, score, token_logp


def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def video_tta_batch(video, n, flip_mask):
    """The clip batch of test-time augmentation for ONE encoder pass: video (B, T, H, W, 1) fp32 -> (B * n, T, H, W, 1), clip b * n + k = video[b] mirrored along W when
    bit k of flip_mask is set, video[b] otherwise (avec_video_tta_batch: every input row read once, written n times).  Inference only."""
    _inference_only("ops.video_tta_batch", video)
    rt.require_gpu(video)
    if video.dim() != 5 or video.shape[-1] != 1:
        raise ValueError("ops.video_tta_batch: video of shape %s, expected (B, T, H, W, 1)" % (tuple(video.shape),))
    n, flip_mask = int(n), int(flip_mask)
    if not 1 <= n <= 32 or flip_mask < 0 or flip_mask >> n:
        raise ValueError("ops.video_tta_batch: n = %d (1..32), flip_mask = %s (bits below n only)" % (n, bin(flip_mask)))
    B, T, H, W, _ = video.shape
    x = _aligned16(_f32c(video))
    y = torch.empty(B * n, T, H, W, 1, dtype=torch.float32, device=x.device)
    lib.video_tta_batch(x.data_ptr(), y.data_ptr(), B, T * H, W, n, flip_mask, rt.stream())
    return y


def ctc_tta_pick(tokens, out_len, score, n, best_slot=None):
    """Per utterance the winner among its n augmentations, on the device (avec_ctc_tta_pick; one launch, no host synchronisation).  tokens [S, W, T] int32,
    out_len [S, W] int32, score [S, W] of ops.ctc_beam_search on S = B * n rows (row b * n + k = augmentation k of utterance b).  best_slot [B] int64 (optional):
    the winning slot in [0, n * W), ops.lm_rescore's `best`; without it the augmentation whose best beam scores highest (first maximum) and beam 0.
    Returns best_aug [B], best_beam [B], ids [B, T] (zero past ids_len), ids_len [B] (all int64) and best_score [B]."""
    rt.require_gpu(tokens)
    S, W, T = tokens.shape
    n = int(n)
    if n < 1 or S % n:
        raise ValueError("ops.ctc_tta_pick: %d rows are not a whole number of utterances of %d augmentations" % (S, n))
    B, dev = S // n, tokens.device
    if tuple(out_len.shape) != (S, W) or tuple(score.shape) != (S, W):
        raise ValueError("ops.ctc_tta_pick: tokens %s, out_len %s, score %s" % (tuple(tokens.shape), tuple(out_len.shape), tuple(score.shape)))
    tk, ol, sc = tokens.to(torch.int32).contiguous(), out_len.to(device=dev, dtype=torch.int32).contiguous(), _f32c(score.to(dev))
    if best_slot is not None:
        best_slot = best_slot.to(device=dev, dtype=torch.int64).contiguous().view(-1)
        if best_slot.numel() != B:
            raise ValueError("ops.ctc_tta_pick: best_slot of %d entries for %d utterances" % (best_slot.numel(), B))
    best_aug, best_beam, ids_len = (torch.empty(B, dtype=torch.int64, device=dev) for _ in range(3))
    ids = torch.empty(B, T, dtype=torch.int64, device=dev)
    best_score = torch.empty(B, dtype=torch.float32, device=dev)
    lib.ctc_tta_pick(tk.data_ptr(), ol.data_ptr(), sc.data_ptr(), _p(best_slot), B, n, W, T, best_aug.data_ptr(), best_beam.data_ptr(), ids.data_ptr(),
                     ids_len.data_ptr(), best_score.data_ptr(), rt.stream())
    return best_aug, best_beam, ids, ids_len, best_score


def ngram_rows(lm, contexts):
    """ln P(. | ctx) [n, V] on the device for a list of token histories (oldest first, -1 = <s>): avec_ngram_rows"""
    dev = torch.device("cuda", torch.cuda.current_device())
    n, L = len(contexts), max(1, max((len(c) for c in contexts), default=1))
    ctx = torch.zeros(n, L, dtype=torch.int32)
    for i, c in enumerate(contexts):
        if len(c):
            ctx[i, :len(c)] = torch.tensor(list(c), dtype=torch.int32)
    ctx, clen = ctx.to(dev), torch.tensor([len(c) for c in contexts], dtype=torch.int32, device=dev)
    rows = torch.empty(n, lm.V, dtype=torch.float32, device=dev)
    lib.ngram_rows(_byref(lm.device_struct(dev)), ctx.data_ptr(), clen.data_ptr(), n, L, lm.oov_logprob, rows.data_ptr(), rt.stream())
    return rows


# ============================================================================================
# Transformer-LM (GPT) rescoring of the beam -- csrc/lm.hip.  Inference only: no autograd Functions, no backward kernels.
# ============================================================================================
CAUSAL_HEAD_DIM = 64


def _inference_only(what, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError("%s is an inference path (it has no backward kernels): call it under torch.no_grad(), or with inputs and parameters that do not "
                           "require grad -- a graph-less result would silently train nothing" % what)


def embed_pos(ids, weight, pos, out_f32=True):
    """x[n, t] = weight[ids[n, t]] + pos[t]: nn.Embedding followed by SinPosEmbedding / PosEmbedding1d (pos: [>= L, D] or [1, >= L, D], fp32) in one launch.
    ids [N, L] integer -> [N, L, D] fp32 (the residual stream) or, with out_f32=False, the compute dtype."""
    _inference_only("ops.embed_pos", weight, pos)
    rt.require_gpu(weight)
    N, L = ids.shape
    V, D = weight.shape
    pos = pos.reshape(-1, D)
    if pos.shape[0] < L:
        raise ValueError("ops.embed_pos: %d positions for sequences of %d tokens (max_pos_encoding)" % (pos.shape[0], L))
    ids = ids.to(device=weight.device, dtype=torch.int64).contiguous()
    w, p = _f32c(weight.detach()), _f32c(pos.detach())
    out = torch.empty(N, L, D, dtype=torch.float32 if out_f32 else rt.act_dtype(), device=weight.device)
    lib.embed_pos(rt.dt(), ids.data_ptr(), w.data_ptr(), p.data_ptr(), out.data_ptr(), int(out_f32), N, L, V, D, rt.stream())
    return out


def causal_attention(qkv, N, H, L, lens=None):
    """softmax(Q K^T / sqrt(d) + causal) V per (sequence, head) on the fused projection qkv [N * L, 3 * H * d] (compute dtype, Q | K | V) -> [N * L, H * d].
    The mask is computed from the indices (Mask(right_context=0)); lens [N] (optional) lets whole 32-row query tiles past a sequence's length be skipped
    (written as zeros).  Only d = 64 (GPT-Small 768 / 12, GPT-Medium 1024 / 16) has a kernel: other head widths raise NotImplementedError."""
    _inference_only("ops.causal_attention", qkv)
    rt.require_gpu(qkv)
    M, W3 = qkv.shape
    d = W3 // (3 * H)
    if d != CAUSAL_HEAD_DIM or 3 * H * d != W3:
        raise NotImplementedError("ops.causal_attention: head width %d (row of %d over %d heads); the causal attention kernel supports d = %d only" % (d, W3, H, CAUSAL_HEAD_DIM))
    assert qkv.dtype == rt.act_dtype() and qkv.is_contiguous() and M == N * L, (qkv.dtype, qkv.shape, N, L)
    o = empty((M, H * d), rt.act_dtype(), qkv)
    lens_t = None if lens is None else lens.to(device=qkv.device, dtype=torch.int64).contiguous()
    lib.causal_attention(rt.dt(), qkv.data_ptr(), W3, _p(lens_t), o.data_ptr(), H * d, N, H, L, d, 1.0 / d ** 0.5, rt.stream())
    return o


def lm_head_workspace_bytes(R, V, D):
    return lib.raw("avec_lm_head_nll_workspace_bytes")(R, V, D)


def lm_head_nll(h, weight, bias, tgt):
    """nll[r] = logsumexp_v(h[r] . weight[v] + bias[v]) - (h[r] . weight[tgt[r]] + bias[tgt[r]]), fp32, 0 where tgt[r] = -1: head Linear + log_softmax + gather as
    one kernel that never writes the [R, V] logits.  h [R, D] compute dtype; weight: the head's (registered) Linear weight [V, D]."""
    _inference_only("ops.lm_head_nll", h, weight, bias)
    rt.require_gpu(h)
    sh = rt.shadow(weight)
    V, D = sh.A, sh.C
    R = h.shape[0]
    assert h.dtype == rt.act_dtype() and h.is_contiguous() and h.shape[1] == D and sh.Tm == 1, (h.dtype, h.shape, D)
    tgt = tgt.to(device=h.device, dtype=torch.int64).contiguous().view(-1)
    assert tgt.numel() == R, (tgt.shape, R)
    b = bias.detach() if bias is not None else torch.zeros(V, dtype=torch.float32, device=h.device)
    nbytes = lm_head_workspace_bytes(R, V, D)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=h.device) if nbytes else None
    nll = torch.empty(R, dtype=torch.float32, device=h.device)
    lib.lm_head_nll(rt.dt(), h.data_ptr(), D, sh.fwd.data_ptr(), sh.Cp, b.data_ptr(), tgt.data_ptr(), nll.data_ptr(), R, V, D, _p(ws), nbytes, rt.stream())
    return nll


def lm_segment_sum(nll, lens):
    """nll [S, L] (row (s, t) scores token t + 1), lens [S] tokens incl. <sos> / <eos> -> [S] sums over t < lens - 1"""
    S, L = nll.shape
    lens = lens.to(device=nll.device, dtype=torch.int64).contiguous()
    out = torch.empty(S, dtype=torch.float32, device=nll.device)
    lib.lm_segment_sum(_f32c(nll).data_ptr(), lens.data_ptr(), S, L, out.data_ptr(), rt.stream())
    return out


def lm_attention_module(x2, N, L, ln, att, lens=None):
    """x + attention(LN(x)) of a pre-norm TransformerBlock on the fp32 residual rows x2 [N * L, D]: LayerNorm, one Q|K|V product, the causal core, output
    projection with the residual in its epilogue"""
    M, D = x2.shape
    h, _, _ = layernorm_fwd(x2, ln.weight, ln.bias, M, D, False, ln.eps)
    q, k, v = att.query_layer, att.key_layer, att.value_layer
    qkv = qkv_project(h, ((q.weight, k.weight, v.weight), (q.bias, k.bias, v.bias)), M, D)
    o = causal_attention(qkv, N, att.num_heads, L, lens)
    return linear_fwd(o, att.output_layer.weight, att.output_layer.bias, M, in_f32=False, out_f32=True, res=x2, alpha=1.0)


def lm_ffn_module(x2, ln, l1, l2, act=ACT_GELU):
    """x + Linear(act(Linear(LN(x)))) on the fp32 residual rows: the activation (GELU, exact erf form) and the residual are GEMM epilogues"""
    M, D = x2.shape
    h, _, _ = layernorm_fwd(x2, ln.weight, ln.bias, M, D, False, ln.eps)
    u = linear_fwd(h, l1.weight, l1.bias, M, in_f32=False, out_f32=False, act=act)
    return linear_fwd(u, l2.weight, l2.bias, M, in_f32=False, out_f32=True, res=x2, alpha=1.0)


def lm_rescore(model, ids, lens, beam_score, alpha, beta, B):
    """One scoring pass for all B * K hypotheses of a batch: neural = model.score(ids, lens) (nll sums [B * K]), then on the device
    total = beam_score - alpha * neural + beta * beta * (lens - 1) (this repository's higher-is-better convention; beta enters squared as in the reference,
    nnet/decoders.py:231,234) and best = the first maximum per utterance; slots with lens == 0 or beam_score == -inf never win.
    Returns best [B] int64, total [B, K], neural [B, K]."""
    S = ids.shape[0]
    K = S // B
    assert K * B == S and beam_score.numel() == S and lens.numel() == S
    with torch.no_grad():
        neural = model.score(ids, lens)
    dev = neural.device
    neural = _f32c(neural.view(-1))
    lens = lens.to(device=dev, dtype=torch.int64).contiguous()
    beam = _f32c(beam_score.to(dev).view(-1))
    total = torch.empty(S, dtype=torch.float32, device=dev)
    best = torch.empty(B, dtype=torch.int64, device=dev)
    lib.lm_rescore_select(neural.data_ptr(), lens.data_ptr(), beam.data_ptr(), float(alpha), float(beta), B, K, total.data_ptr(), best.data_ptr(), rt.stream())
    return best, total.view(B, K), neural.view(B, K)


# ============================================================================================
# Streaming encoder (nnet.ConformerStreamSession): the two stateful kernels of a causal Conformer stack run chunk by chunk (include/avec_hip.h)
# ============================================================================================
def _stream_ctl(name, pos, reset, chunk_len, B):
    _slot_vec(name, "pos", pos, B, pos.device)
    _slot_vec(name, "reset", reset, B, pos.device, mask=True)
    _slot_vec(name, "chunk_len", chunk_len, B, pos.device)


def glu_dwconv_stream_state(B, C, K, device):
    """zero-filled left context of ops.glu_dwconv_stream: [B, K - 1, 2C] in the activation dtype"""
    return torch.zeros(B, K - 1, 2 * C, dtype=rt.act_dtype(), device=device)


def glu_dwconv_stream(u, w, bias, ss, state, pos, reset=None, chunk_len=None, div=1, stride=1):
    """One chunk of the convolution module's middle: Swish(BatchNorm_eval(depthwise_causal(GLU([carried context | u])))) in one launch.  u [B, Tq, 2C] act (the
    pointwise conv's output), w the depthwise weight (tap-major [K][C] in memory), ss the eval-mode scale | shift of the BatchNorm ([>= 2C] fp32, ops.bn_finalize),
    state [B, K - 1, 2C] act, updated in place; pos / reset / chunk_len / div as include/avec_hip.h.  Returns [B, Tq / stride, C] act.  No synchronisation."""
    rt.require_gpu(u)
    B, Tq, C2 = u.shape
    C, K = C2 // 2, w.shape[-1]
    adt = rt.act_dtype()
    if not (u.dtype == adt and u.is_contiguous() and state.dtype == adt and state.is_contiguous() and ss.dtype == torch.float32 and ss.numel() >= 2 * C):
        raise ValueError("glu_dwconv_stream: u and state contiguous in the activation dtype %s, ss fp32 [>= 2C] (got %s, %s, %s)" % (adt, u.dtype, state.dtype, ss.dtype))
    _stream_ctl("glu_dwconv_stream", pos, reset, chunk_len, B)
    if Tq % stride:
        raise ValueError("glu_dwconv_stream: %d frames per chunk is not a multiple of the stride %d" % (Tq, stride))
    out = empty((B * (Tq // stride), C), adt, u)
    lib.glu_dwconv_stream(rt.dt(), u.data_ptr(), w.data_ptr(), _p(bias), ss.data_ptr(), out.data_ptr(), state.data_ptr() if state.numel() else None,
                          state.numel() * state.element_size(), pos.data_ptr(), _p(reset), _p(chunk_len), int(div), B, Tq, C, K, int(stride), rt.stream())
    return out.view(B, Tq // stride, C)


def relpos_attention_stream_state(B, H, d, L, Tq, device):
    """the key and value rings of ops.relpos_attention_stream: two [B, L + Tq, H * d] tensors in the activation dtype"""
    return (torch.zeros(B, L + Tq, H * d, dtype=rt.act_dtype(), device=device), torch.zeros(B, L + Tq, H * d, dtype=rt.act_dtype(), device=device))


def relpos_attention_stream(qkv, e, kcache, vcache, pos, reset=None, chunk_len=None, div=1, *, B, H, L):
    """Relative-position attention of one chunk over the band 0 <= p_i - p_j <= L.  qkv [B * Tq, 3D] act (the fused q | k | v projection of the chunk), e [L + 1, D] act
    (row delta = pos_layer(PE(delta)), possibly a column slice), kcache / vcache [B, L + Tq, D] act rings (the chunk's rows are appended).  Returns o [B * Tq, D] act."""
    rt.require_gpu(qkv)
    M, D3 = qkv.shape
    D, Tq = D3 // 3, M // B
    d, adt = D // H, rt.act_dtype()
    if not (qkv.dtype == adt and qkv.is_contiguous() and e.dtype == adt and e.shape[0] == L + 1 and e.stride(1) == 1 and kcache.dtype == adt and vcache.dtype == adt
            and kcache.is_contiguous() and vcache.is_contiguous() and tuple(kcache.shape) == tuple(vcache.shape) == (B, L + Tq, D) and B * Tq == M and H * d == D):
        raise ValueError("relpos_attention_stream: qkv [B Tq, 3D], e [L + 1, D], kcache / vcache [B, L + Tq, D] in the activation dtype %s (got %s %s, %s %s, %s %s)"
                         % (adt, tuple(qkv.shape), qkv.dtype, tuple(e.shape), e.dtype, tuple(kcache.shape), kcache.dtype))
    _stream_ctl("relpos_attention_stream", pos, reset, chunk_len, B)
    o = empty((M, D), adt, qkv)
    esz = qkv.element_size()
    lib.relpos_attention_stream(rt.dt(), qkv.data_ptr(), qkv.data_ptr() + D * esz, qkv.data_ptr() + 2 * D * esz, 3 * D, e.data_ptr(), e.stride(0), kcache.data_ptr(), vcache.data_ptr(),
                                kcache.numel() * esz, pos.data_ptr(), _p(reset), _p(chunk_len), int(div), o.data_ptr(), D, B, H, Tq, d, L, 1.0 / d ** 0.5, rt.stream())
    return o


def stream_advance(pos, reset, chunk_len, full):
    """end of a push: pos = (reset ? 0 : pos) + min(chunk_len, full) in place, and the reset flags are cleared (consumed); one launch"""
    _stream_ctl("stream_advance", pos, reset, chunk_len, pos.numel())
    lib.stream_advance(pos.data_ptr(), _p(reset), _p(chunk_len), int(full), pos.numel(), rt.stream())
    return pos


# ---- with look-ahead (nnet.ConformerLookaheadStreamSession): a window of W = Tc + LAe frames per push, of which only the committed ones reach the state --------------
class StreamWindowState:
    """What the look-ahead session carries per slot, on the device: the tail of input frames heard and not final yet [B, LAe, D] fp32, pend (frames in it), pos
    (committed input frames), the `ended` flag, and the counts a push's first launch writes for the others: nvalid, ncommit, emit (include/avec_hip.h).  Never cleared:
    the first push restarts every slot."""

    def __init__(self, B, Tc, LAe, D, S, device):
        self.B, self.Tc, self.LAe, self.D, self.S = int(B), int(Tc), int(LAe), int(D), int(S)
        self.tail = torch.zeros(B, max(LAe, 1), D, dtype=torch.float32, device=device)
        self.pend, self.pos, self.nvalid, self.ncommit, self.emit = (torch.zeros(B, dtype=torch.int64, device=device) for _ in range(5))
        self.ended = torch.zeros(B, dtype=torch.uint8, device=device)


def stream_window(st, x_new, n_new=None, last=None, reset=None):
    """first launch of a push: x_new [B, Tc, D] fp32 -> the window X [B, Tc + LAe, D] fp32 = [tail[:pend] | x_new[:n_new] | zeros]; st.nvalid / ncommit / emit are written"""
    rt.require_gpu(x_new)
    if not (x_new.dtype == torch.float32 and x_new.is_contiguous() and tuple(x_new.shape) == (st.B, st.Tc, st.D)):
        raise ValueError("stream_window: x_new fp32 contiguous [%d, %d, %d] (got %s %s)" % (st.B, st.Tc, st.D, tuple(x_new.shape), x_new.dtype))
    dev = st.pend.device
    _slot_vec("stream_window", "n_new", n_new, st.B, dev)
    _slot_vec("stream_window", "last", last, st.B, dev, mask=True)
    _slot_vec("stream_window", "reset", reset, st.B, dev, mask=True)
    X = empty((st.B, st.Tc + st.LAe, st.D), torch.float32, x_new)
    lib.stream_window(x_new.data_ptr(), st.tail.data_ptr(), X.data_ptr(), st.pend.data_ptr(), _p(n_new), _p(last), _p(reset), st.ended.data_ptr(), st.nvalid.data_ptr(),
                      st.ncommit.data_ptr(), st.emit.data_ptr(), st.B, st.Tc, st.LAe, st.D, st.S, rt.stream())
    return X


def stream_window_advance(st, X, last=None, reset=None):
    """last launch of a push: tail <- X[ncommit : nvalid], pend, pos and `ended` move on, the reset / last flags are cleared (consumed)"""
    dev = st.pend.device
    _slot_vec("stream_window_advance", "last", last, st.B, dev, mask=True)
    _slot_vec("stream_window_advance", "reset", reset, st.B, dev, mask=True)
    if not (X.dtype == torch.float32 and X.is_contiguous() and tuple(X.shape) == (st.B, st.Tc + st.LAe, st.D)):
        raise ValueError("stream_window_advance: X fp32 contiguous [%d, %d, %d] (got %s %s)" % (st.B, st.Tc + st.LAe, st.D, tuple(X.shape), X.dtype))
    lib.stream_window_advance(X.data_ptr(), st.tail.data_ptr(), st.pend.data_ptr(), st.pos.data_ptr(), st.nvalid.data_ptr(), st.ncommit.data_ptr(), _p(last), _p(reset),
                              st.ended.data_ptr(), st.B, st.Tc + st.LAe, st.LAe, st.D, rt.stream())


def glu_dwconv_stream_la(u, w, bias, ss, state, pos, reset, ncommit, div=1, stride=1):
    """ops.glu_dwconv_stream on a window u [B, Wq, 2C]: every row is convolved, the first ncommit / div enter the carried context.  Returns [B, Wq / stride, C] act."""
    rt.require_gpu(u)
    B, Wq, C2 = u.shape
    C, K = C2 // 2, w.shape[-1]
    adt = rt.act_dtype()
    if not (u.dtype == adt and u.is_contiguous() and state.dtype == adt and state.is_contiguous() and ss.dtype == torch.float32 and ss.numel() >= 2 * C):
        raise ValueError("glu_dwconv_stream_la: u and state contiguous in the activation dtype %s, ss fp32 [>= 2C] (got %s, %s, %s)" % (adt, u.dtype, state.dtype, ss.dtype))
    _stream_ctl("glu_dwconv_stream_la", pos, reset, ncommit, B)
    if Wq % stride:
        raise ValueError("glu_dwconv_stream_la: %d window rows is not a multiple of the stride %d" % (Wq, stride))
    out = empty((B * (Wq // stride), C), adt, u)
    lib.glu_dwconv_stream_la(rt.dt(), u.data_ptr(), w.data_ptr(), _p(bias), ss.data_ptr(), out.data_ptr(), state.data_ptr() if state.numel() else None,
                             state.numel() * state.element_size(), pos.data_ptr(), _p(reset), _p(ncommit), int(div), B, Wq, C, K, int(stride), rt.stream())
    return out.view(B, Wq // stride, C)


def relpos_attention_stream_la(qkv, e, kcache, vcache, pos, reset, nvalid, ncommit, div=1, *, B, H, L, R):
    """Relative-position attention of a window over the band -R <= p_i - p_j <= L.  qkv [B * Wq, 3D] act, e [L + R + 1, D] act (row delta + R = pos_layer(PE(delta))),
    kcache / vcache [B, L + Tq, D] act rings of ops.relpos_attention_stream_state (the first ncommit / div rows are appended).  Returns o [B * Wq, D] act."""
    rt.require_gpu(qkv)
    M, D3 = qkv.shape
    D, Wq = D3 // 3, M // B
    d, adt = D // H, rt.act_dtype()
    Tq = kcache.shape[1] - L if kcache.dim() == 3 else 0
    if not (qkv.dtype == adt and qkv.is_contiguous() and e.dtype == adt and e.shape[0] == L + R + 1 and e.stride(1) == 1 and kcache.dtype == adt and vcache.dtype == adt
            and kcache.is_contiguous() and vcache.is_contiguous() and tuple(kcache.shape) == tuple(vcache.shape) == (B, L + Tq, D) and 0 < Tq <= Wq and B * Wq == M and H * d == D):
        raise ValueError("relpos_attention_stream_la: qkv [B Wq, 3D], e [L + R + 1, D], kcache / vcache [B, L + Tq, D] (Tq <= Wq) in the activation dtype %s (got %s %s, %s %s, %s %s)"
                         % (adt, tuple(qkv.shape), qkv.dtype, tuple(e.shape), e.dtype, tuple(kcache.shape), kcache.dtype))
    _stream_ctl("relpos_attention_stream_la", pos, reset, nvalid, B)
    _slot_vec("relpos_attention_stream_la", "ncommit", ncommit, B, pos.device)
    o = empty((M, D), adt, qkv)
    esz = qkv.element_size()
    lib.relpos_attention_stream_la(rt.dt(), qkv.data_ptr(), qkv.data_ptr() + D * esz, qkv.data_ptr() + 2 * D * esz, 3 * D, e.data_ptr(), e.stride(0), kcache.data_ptr(),
                                   vcache.data_ptr(), kcache.numel() * esz, pos.data_ptr(), _p(reset), _p(nvalid), _p(ncommit), int(div), o.data_ptr(), D, B, H, Wq, Tq, d, L, R,
                                   1.0 / d ** 0.5, rt.stream())
    return o


# ============================================================================================
# Streamed audio front-end (nnet.AudioFrontStreamSession): waveform chunks -> the stem's rows with the offline arithmetic (include/avec_hip.h, csrc/audio_stream.hip)
# ============================================================================================
def audio_stream_state(B, device):
    """what ops.mel_frames_stream / audio_stream_advance carry between pushes: per slot the sample tail, the sample counter and the `ended` flag (one uint8 blob of
    avec_audio_stream_state_bytes; never cleared: the first push restarts every slot)"""
    return torch.empty(lib.raw("avec_audio_stream_state_bytes")(int(B)), dtype=torch.uint8, device=device)


def _front_stream_ctl(name, x, state, count_name, counts, reset, last, layout_ok, layout):
    """what the launches of a streamed front-end check of their input x (layout_ok: the caller's verdict on its layout, described by `layout`), the state blob and
    the per-slot count / reset / last vectors"""
    if not (layout_ok and state.dtype == torch.uint8 and state.is_contiguous() and state.device == x.device):
        raise ValueError("%s: %s and a uint8 state blob on its device (got %s %s, %s)" % (name, layout, tuple(x.shape), x.dtype, state.dtype))
    B = x.shape[0]
    _slot_vec(name, count_name, counts, B, x.device)
    _slot_vec(name, "reset", reset, B, x.device, mask=True)
    _slot_vec(name, "last", last, B, x.device, mask=True)


def _wave_layout(wave):
    return wave.dim() == 2 and wave.dtype == torch.float32 and wave.stride(1) == 1, "wave fp32 [B, W] with unit sample stride"


def mel_frames_stream(wave, window, state, n_samples=None, reset=None, last=None, *, Tmax, n_fft, win, hop, out=None):
    """The framing launch of one push: wave [B, W] fp32 (slot b takes its first n_samples[b] samples; default all W) behind the carried tail -> (frames
    [B * (2 Tmax + 1), win] fp32: the windowed mel frames 2 E0 - 1 .. 2 E1 - 1, zeros elsewhere; out_len [B] int64 = E1 - E0 stem frames; meta [B, 2] int64 for
    ops.audio_stem_stream).  Reads the state only: ops.audio_stream_advance ends the push.  out: (frames, out_len, meta) to write into.  No synchronisation."""
    rt.require_gpu(wave)
    _front_stream_ctl("mel_frames_stream", wave, state, "n_samples", n_samples, reset, last, *_wave_layout(wave))
    B, W = wave.shape
    if out is None:
        out = (empty((B * (2 * Tmax + 1), win), torch.float32, wave), torch.empty(B, dtype=torch.int64, device=wave.device),
               torch.empty(B, 2, dtype=torch.int64, device=wave.device))
    frames, out_len, meta = out
    if not (frames.dtype == torch.float32 and frames.is_contiguous() and frames.numel() == B * (2 * Tmax + 1) * win and out_len.dtype == meta.dtype == torch.int64
            and out_len.is_contiguous() and meta.is_contiguous() and out_len.numel() == B and meta.numel() == 2 * B):
        raise ValueError("mel_frames_stream: out = (frames fp32 [B (2 Tmax + 1), win], out_len int64 [B], meta int64 [B, 2]), contiguous")
    lib.mel_frames_stream(wave.data_ptr(), wave.stride(0), window.data_ptr(), frames.data_ptr(), state.data_ptr(), state.numel(), _p(n_samples), _p(reset), _p(last),
                          out_len.data_ptr(), meta.data_ptr(), B, W, int(Tmax), int(n_fft), int(win), int(hop), rt.stream())
    return frames, out_len, meta


def mel_from_frames(frames, dft, fb, B, F, n_mels):
    """windowed frames [B * F, win] fp32 -> log-mel [B, n_mels, F] fp32: the DFT GEMM and the power / mel / log kernel of ops.mel_spectrogram, unchanged"""
    from .lib import F32
    M, win = frames.shape
    nb = dft.shape[0] // 2
    spec = empty((M, 2 * nb), torch.float32, frames)
    gemm_nt(frames, dft, spec, M, 2 * nb, win, out_f32=True, dtype=F32)
    out = empty((B, n_mels, F), torch.float32, frames)
    lib.mel_power_log(spec.data_ptr(), fb.data_ptr(), out.data_ptr(), B, F, nb, n_mels, rt.stream())
    return out


def audio_stem_stream(mel, w, bias, ss, out_len, meta, C, out=None):
    """mel [B, n_mels, 2 Tmax + 1] fp32 (the push's log-mel columns) -> [B, Tmax, C * n_mels / 2] act: Conv2d(1 -> C, 3x3, s2) + bias, eval-mode BatchNorm (ss: the
    scale | shift of ops.bn_finalize), Swish, one launch; rows at or past out_len are zeros."""
    rt.require_gpu(mel)
    B, NM, Fmax = mel.shape
    if not (mel.dtype == torch.float32 and mel.is_contiguous() and Fmax % 2 == 1 and ss.dtype == torch.float32 and ss.numel() >= 2 * C and w.dtype == torch.float32
            and w.is_contiguous() and w.numel() == 9 * C):
        raise ValueError("audio_stem_stream: mel fp32 [B, n_mels, 2 Tmax + 1] contiguous, w fp32 [C, 1, 3, 3], ss fp32 [>= 2C] (got %s %s, %s, %s)"
                         % (tuple(mel.shape), mel.dtype, tuple(w.shape), tuple(ss.shape)))
    Tmax = (Fmax - 1) // 2
    if out is None:
        out = torch.empty(B, Tmax, C * (NM // 2), dtype=rt.act_dtype(), device=mel.device)
    elif not (out.dtype == rt.act_dtype() and out.is_contiguous() and tuple(out.shape) == (B, Tmax, C * (NM // 2))):
        raise ValueError("audio_stem_stream: out must be contiguous [B, Tmax, C n_mels / 2] in the activation dtype")
    lib.audio_stem_stream(rt.dt(), mel.data_ptr(), w.data_ptr(), _p(bias), ss.data_ptr(), out.data_ptr(), out_len.data_ptr(), meta.data_ptr(), B, NM, Tmax, C, rt.stream())
    return out


def audio_stream_advance(wave, state, n_samples=None, reset=None, last=None, *, n_fft, win, hop):
    """end of a push: the tail becomes the samples the next frames still need, n += n_samples, ended |= last, in place; the reset and last flags are cleared (consumed)"""
    rt.require_gpu(wave)
    _front_stream_ctl("audio_stream_advance", wave, state, "n_samples", n_samples, reset, last, *_wave_layout(wave))
    B, W = wave.shape
    lib.audio_stream_advance(wave.data_ptr(), wave.stride(0), state.data_ptr(), state.numel(), _p(n_samples), _p(reset), _p(last), B, W, int(n_fft), int(win), int(hop), rt.stream())
    return state


# ============================================================================================
# Streamed visual stem (nnet.VisualFrontStreamSession): video chunks -> the pooled NHWC frames with the offline arithmetic (include/avec_hip.h, csrc/video_stream.hip)
# ============================================================================================
def video_stream_state(B, H, W, device):
    """what ops.video_stem_stream / video_stream_advance carry between pushes: per slot a ring of the last 4 input frames in the compute dtype, the frame counter and
    the `ended` flag (one uint8 blob of avec_video_stream_state_bytes; never cleared: the first push restarts every slot)"""
    n = lib.raw("avec_video_stream_state_bytes")(rt.dt(), int(B), int(H), int(W))
    if n <= 0:
        raise ValueError("video_stream_state: no state for B=%d frames of %dx%d (W must be a multiple of 8)" % (B, H, W))
    return torch.empty(n, dtype=torch.uint8, device=device)


def video_stem_w8(weight):
    """Conv3d weight [64, 1, 5, 7, 7] -> [64][36][8] in the compute dtype as VideoStemFn packs it for stem3p.hip: per (kd, kh) row a zero slot, then the 7 taps; row 35
    zero.  A session packs once, not once per push."""
    if tuple(weight.shape) != (64, 1, 5, 7, 7):
        raise ValueError("video_stem_w8: weight %s is not the [64, 1, 5, 7, 7] stem convolution" % (tuple(weight.shape),))
    w8 = torch.zeros((64, 36, 8), dtype=rt.act_dtype(), device=weight.device)
    w8[:, :35, 1:] = weight.detach().reshape(64, 35, 7).to(rt.act_dtype())
    return w8


def _video_layout(chunk):
    return chunk.dim() == 4 and chunk.dtype == torch.float32 and chunk[0].is_contiguous(), "chunk fp32 [B, Tin, H, W] with contiguous slots"


def video_stem_stream(chunk, state, w8, bias, ss, n_frames=None, reset=None, last=None, *, Tmax, out=None):
    """The stem launch of one push: chunk [B, Tin, H, W] fp32 (slot b takes its first n_frames[b] frames; default all Tin) behind the carried ring -> (frames
    [Tmax, B, PH, PW, 64] act, FRAME-major: local output frame r of slot b in row r * B + b, zeros at or past out_len; out_len [B] int64).  Conv3d + bias, eval-mode
    BatchNorm (ss: the scale | shift of ops.bn_finalize), ReLU and the 3x3 / s2 max pool in one launch; w8 from ops.video_stem_w8.  Reads the state only:
    ops.video_stream_advance ends the push.  out: (frames, out_len) to write into.  No synchronisation."""
    rt.require_gpu(chunk)
    _front_stream_ctl("video_stem_stream", chunk, state, "n_frames", n_frames, reset, last, *_video_layout(chunk))
    B, Tin, H, W = chunk.shape
    adt = rt.act_dtype()
    if not (w8.dtype == adt and w8.is_contiguous() and tuple(w8.shape) == (64, 36, 8) and ss.dtype == torch.float32 and ss.numel() >= 128 and ss.is_contiguous()
            and (bias is None or (bias.dtype == torch.float32 and bias.numel() == 64 and bias.is_contiguous()))):
        raise ValueError("video_stem_stream: w8 [64, 36, 8] in the compute dtype %s (ops.video_stem_w8), bias fp32 [64], ss fp32 [>= 128] (got %s %s, %s)"
                         % (adt, tuple(w8.shape), w8.dtype, tuple(ss.shape)))
    PH, PW = ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1
    if out is None:
        out = (torch.empty(int(Tmax), B, PH, PW, 64, dtype=adt, device=chunk.device), torch.empty(B, dtype=torch.int64, device=chunk.device))
    frames, out_len = out
    if not (frames.dtype == adt and frames.is_contiguous() and tuple(frames.shape) == (int(Tmax), B, PH, PW, 64) and out_len.dtype == torch.int64 and out_len.is_contiguous()
            and out_len.numel() == B):
        raise ValueError("video_stem_stream: out = (frames [Tmax, B, PH, PW, 64] in the activation dtype, out_len int64 [B]), contiguous")
    lib.video_stem_stream(rt.dt(), chunk.data_ptr(), chunk.stride(0), state.data_ptr(), state.numel(), _p(n_frames), _p(reset), _p(last), w8.data_ptr(), _p(bias), ss.data_ptr(),
                          frames.data_ptr(), out_len.data_ptr(), B, Tin, int(Tmax), H, W, rt.stream())
    return frames, out_len


def video_stream_advance(chunk, state, n_frames=None, reset=None, last=None):
    """end of a push: the chunk's last min(n_frames, 4) frames go into their ring slots, n += n_frames, ended |= last, in place; the reset and last flags are cleared
    (consumed).  A launch of its own behind the stem launch, whose workgroups read the ring slots it overwrites."""
    rt.require_gpu(chunk)
    _front_stream_ctl("video_stream_advance", chunk, state, "n_frames", n_frames, reset, last, *_video_layout(chunk))
    B, Tin, H, W = chunk.shape
    lib.video_stream_advance(rt.dt(), chunk.data_ptr(), chunk.stride(0), state.data_ptr(), state.numel(), _p(n_frames), _p(reset), _p(last), B, Tin, H, W, rt.stream())
    return state


# ============================================================================================
# Streamed audio-visual fusion input (nnet.AudioVisualStreamSession): the branches' rows paired across pushes -> the first fusion Linear's operand (csrc/av_stream.hip)
# ============================================================================================
def av_fuse_stream_state(B, Da, Dv, cap, device):
    """what ops.av_fuse_stream carries between pushes: per slot two rings of `cap` rows in the activation dtype and three int64 counters (one uint8 blob of
    avec_av_fuse_stream_state_bytes; never cleared: the first push restarts every slot)"""
    n = lib.raw("avec_av_fuse_stream_state_bytes")(rt.dt(), int(B), int(Da), int(Dv), int(cap))
    if n <= 0:
        raise ValueError("av_fuse_stream_state: no state for B=%d rows of %d | %d, cap=%d (the widths must be multiples of 4)" % (B, Da, Dv, cap))
    return torch.empty(n, dtype=torch.uint8, device=device)


def av_fuse_stream(a, a_len, v, v_len, state, reset=None, max_emit=1, *, out=None):
    """One launch: a [B, Ra, Da] / v [B, Rv, Dv] fp32 (slot b appends its first a_len[b] / v_len[b] rows; int64 [B] on the device) behind the carried rings ->
    (xc [B, max_emit, Da + Dv] act: the oldest unpaired rows [audio | video], zeros at or past pair_len; pair_len [B] int64).  reset: uint8 flags [B], consumed
    (cleared) by the launch.  cap is read off the state's size.  out: (xc, pair_len) to write into.  No synchronisation."""
    rt.require_gpu(a)
    if not (a.dim() == 3 and v.dim() == 3 and a.dtype == torch.float32 and v.dtype == torch.float32 and a.is_contiguous() and v.is_contiguous() and a.shape[0] == v.shape[0]
            and v.device == a.device and state.dtype == torch.uint8 and state.is_contiguous() and state.device == a.device):
        raise ValueError("av_fuse_stream: a [B, Ra, Da] and v [B, Rv, Dv] fp32, contiguous, with a uint8 state blob on their device (got %s %s, %s %s, %s)"
                         % (tuple(a.shape), a.dtype, tuple(v.shape), v.dtype, state.dtype))
    B, Ra, Da = a.shape
    _, Rv, Dv = v.shape
    _slot_vec("av_fuse_stream", "a_len", a_len, B, a.device)
    _slot_vec("av_fuse_stream", "v_len", v_len, B, a.device)
    _slot_vec("av_fuse_stream", "reset", reset, B, a.device, mask=True)
    if a_len is None or v_len is None:
        raise ValueError("av_fuse_stream: a_len and v_len are required (int64 [B] on the device)")
    adt, max_emit = rt.act_dtype(), int(max_emit)
    esz = 2 if adt == torch.bfloat16 else 4
    cap = (state.numel() - 24 * B) // (B * (Da + Dv) * esz)         # the library checks the size exactly: a state of another shape is an argument error
    if out is None:
        out = (torch.empty(B, max_emit, Da + Dv, dtype=adt, device=a.device), torch.empty(B, dtype=torch.int64, device=a.device))
    xc, pair_len = out
    if not (xc.dtype == adt and xc.is_contiguous() and tuple(xc.shape) == (B, max_emit, Da + Dv) and pair_len.dtype == torch.int64 and pair_len.is_contiguous()
            and pair_len.numel() == B):
        raise ValueError("av_fuse_stream: out = (xc [B, max_emit, Da + Dv] in the activation dtype, pair_len int64 [B]), contiguous")
    lib.av_fuse_stream(rt.dt(), a.data_ptr(), a_len.data_ptr(), v.data_ptr(), v_len.data_ptr(), state.data_ptr(), state.numel(), _p(reset), xc.data_ptr(), pair_len.data_ptr(),
                       B, Ra, Rv, Da, Dv, cap, max_emit, rt.stream())
    return xc, pair_len
