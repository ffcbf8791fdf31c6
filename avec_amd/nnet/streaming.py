"""Streaming sessions: models run chunk by chunk over a fixed number of utterance slots.  None has a counterpart in the reference; the factories (.stream_front() /
.stream() of the encoders, ConformerInterCTC.stream, CTCBeamSearchDecoder.stream) stay with the classes they wrap.  A session owns its device state; nothing is added to
a module tree or a state_dict.

    _StreamSession                      B slots, `_first`, flag vectors uploaded only when a flag is set
      _CapturableSession                a push is a fixed sequence of launches: the device side of push, capture()
        ConformerStreamSession          a causal Conformer stack
          ConformerLookaheadStreamSession a stack with right_context > 0: a window of chunk + look-ahead per push, only the final frames are committed
        _FrontStreamSession             a front-end: count / last / reset controls, their host mirror, the schedule rules (_controls) and _commit
          AudioFrontStreamSession       waveform chunks -> stem frames
          VisualFrontStreamSession      video chunks -> ResNet features
      AudioVisualStreamSession          both branch sessions -> row pairing -> the fusion stack
      CTCBeamStreamSession              the beam search over logit chunks, up to max_frames per slot
      CTCBeamRingStreamSession          the beam search over logit chunks without a frame limit: a window of backpointer rows, older history committed
    _BranchStreamSession                a front session -> the stack -> the head; a last push's tail of up to TAIL frames goes through _push_again
      AudioStreamSession (TAIL 1), VisualStreamSession (TAIL 2)"""
import torch
import torch.nn as nn

from .. import ops
from .. import runtime as rt
from . import attentions, normalizations
from .captured import CapturedStep

__all__ = ["slot_mask", "ConformerStreamSession", "ConformerLookaheadStreamSession", "AudioFrontStreamSession", "AudioStreamSession", "VisualFrontStreamSession", "VisualStreamSession",
           "AudioVisualStreamSession", "CTCBeamStreamSession", "CTCBeamRingStreamSession"]


def slot_mask(flags, B):
    """reset / last as passed to a push (None, a list of slot indices, a host bool mask [B], or a tensor of either) -> a bool list [B]"""
    if flags is None:
        return [False] * B
    r = flags.cpu().tolist() if torch.is_tensor(flags) else list(flags)
    if len(r) == B and all(isinstance(v, bool) for v in r):
        return r
    mask = [False] * B
    for k in r:
        mask[int(k)] = True
    return mask


class _StreamSession:
    """What every session keeps: B slots, `_first` (the first push restarts every slot), device state allocated by the first push (it knows the device; the
    subclass's _allocate(dev)) and uint8 flag vectors that a push uploads only when some flag is set."""

    def __init__(self, batch_size):
        self.B = int(batch_size)
        self.state = None
        self._first = True

    def _reset_mask(self, reset):
        """the first push restarts every slot; later, None stays None (nothing to upload, nothing to check)"""
        if self._first:
            return [True] * self.B
        return None if reset is None else slot_mask(reset, self.B)

    def _flags(self, dev):
        return torch.zeros(self.B, dtype=torch.uint8, device=dev)

    @staticmethod
    def _raise_flags(buf, mask):
        """upload a flag vector only when some flag is set (the push's last launch clears it again: no memset afterwards) -> buf, or None when none is"""
        if mask is None or not any(mask):
            return None
        return buf.copy_(torch.tensor(mask, dtype=torch.uint8), non_blocking=True)

    def _ensure_state(self, dev):
        if self.state is None:
            self._allocate(dev)


class _CapturableSession(_StreamSession):
    """A session over an eval-mode `module` whose push is a fixed sequence of launches: the tail of push and capture() for the subclass's _upload(*controls) (flag
    and count vectors to the device), _run(x) (the eager launches), _static_input(dev) (a zero input and a first push's controls) and _forget() (reset whatever
    the host mirrors of the warm-up pushes)."""

    def __init__(self, module, batch_size):
        super().__init__(batch_size)
        self.module = module
        self._capture = None               # the CapturedStep of one push, after capture()

    def _push(self, x, *controls):
        """the device side of a push: flag and count uploads, then the input copy and the replay, or the eager launches"""
        with torch.no_grad():
            self._ensure_state(x.device)
            self._upload(*controls)
            self._first = False
            if self._capture is not None:
                self._capture.load((x,), ())
                return self._capture.replay()
            return self._run(x)

    def capture(self, device=None):
        """Capture one push as a graph on static input / count / flag buffers; push then copies into them and replays (the device counters make every replay
        advance).  Call it on a fresh session, before the first push; the warm-up pushes it runs are forgotten (the next push restarts every slot).  After it the
        results of a push are static tensors that the next push overwrites."""
        if self._capture is not None:
            return self
        if not self._first:
            raise RuntimeError("capture: call it before the first push of the session")
        p = next(self.module.parameters())
        dev = torch.device(device) if device is not None else p.device
        rt.require_gpu(p)
        with torch.no_grad(), torch.cuda.device(dev):
            self._ensure_state(dev)
            x, controls = self._static_input(dev)
            cap = CapturedStep((x,))
            x = cap.inputs[0]
            self._upload(*controls)
            cap.warm_up(lambda: self._run(x), 2)        # weight shadows, lazy kernel attributes, allocator
            cap.capture(lambda: self._run(x))
        self._capture = cap
        self._forget()
        return self


class ConformerStreamSession(_CapturableSession):
    """ConformerInterCTC.stream(): a causal stack run chunk by chunk.  After any sequence of push calls the rows a slot has produced equal the rows that
    stack(x, lengths) produces offline (eval mode, the same Mask) on the frames pushed so far for that slot, up to floating-point summation order, for every split
    into chunks.  Everything row-wise (LayerNorm, the feed-forward and pointwise products, the InterCTC modules, the strided k=1 residual) runs through the offline
    eval-path launchers; the depthwise convolution's left context and the attention's keys / values are carried by ops.glu_dwconv_stream / relpos_attention_stream in
    buffers this object owns.  Per slot a frame counter lives on the device; a restart only sets a flag that the kernels read: whatever the buffers hold from
    before the restart is older than the counter and counts as absent."""

    LOOKAHEAD = False                      # what _check is told: a right_context > 0 is refused

    def __init__(self, stack, batch_size, chunk_frames):
        super().__init__(stack, batch_size)
        self.stack, self.Tc = stack, int(chunk_frames)
        self.plan = self._check(stack, self.LOOKAHEAD)
        self.S = 1
        for p in self.plan:
            self.S *= p["stride"]
        if self.B < 1:
            raise ValueError("stream: batch_size %d" % self.B)
        if self.Tc < 1 or self.Tc % self.S:
            raise ValueError("stream: chunk_frames = %d must be a positive multiple of the stack's total stride %d (every push then yields whole output frames at every stage)"
                             % (self.Tc, self.S))
        for p in self.plan:
            if p["K"] - 1 + self.Tc // p["div"] > 96:
                raise ValueError("stream: chunk_frames = %d is %d frames at a stage with a %d-tap convolution: at most %d (the kernel holds context + chunk in LDS)"
                                 % (self.Tc, self.Tc // p["div"], p["K"], 97 - p["K"]))
        self._short = [False] * self.B     # host mirror of "this slot's last chunk was short" (the contract check of host-list chunk lengths: no sync)

    @staticmethod
    def _check(stack, lookahead=False):
        """-> per block {div, stride, L, R, K}; raises before anything is launched"""
        if stack.training:
            raise RuntimeError("stream: the stack is in training mode (BatchNorm batch statistics and dropout are not functions of the past): call .eval() first")
        m = stack.mask
        if not isinstance(m, attentions.Mask):
            raise NotImplementedError("stream: the stack needs a streaming Mask(left_context=L, right_context=0), got mask=%r" % (m,))
        if m.left_context is None:
            raise NotImplementedError("stream: left_context=None would need an unbounded key/value cache; give the Mask an integer left_context")
        if not isinstance(m.left_context, int) or m.left_context < 0:
            raise NotImplementedError("stream: left_context=%r must be an integer >= 0" % (m.left_context,))
        if m.right_context != 0 and not lookahead:
            raise NotImplementedError("stream: right_context=%r needs look-ahead buffering (only right_context=0 is streamed)" % (m.right_context,))
        if not isinstance(m.right_context, int) or m.right_context < 0:
            raise NotImplementedError("stream: right_context=%r must be an integer >= 0" % (m.right_context,))
        if (m.mask_start or 0) > 1:
            raise NotImplementedError("stream: mask_start=%r opens a block of future keys at the start of the utterance (only mask_start <= 1 is causal)" % (m.mask_start,))
        plan, div = [], 1
        for i, blk in enumerate(stack.conformer_blocks):
            att = blk.self_att_module.attention
            if isinstance(att, attentions.RelPosPatch1dMultiHeadAttention):
                raise NotImplementedError("stream: block %d uses RelPosPatch1dMultiHeadAttention (patch attention): under a causal mask the min-pooled patch mask hides a patch "
                                          "from itself, its first patch row keeps no key and the offline kernels then average over ALL keys of the utterance, future ones "
                                          "included -- not a function of the past, so no chunked form can equal it" % i)
            if isinstance(att, attentions.RelPosMultiHeadSelfAttention):
                raise NotImplementedError("stream: block %d uses grouped / Transformer-XL attention (%s): its `hidden` cache grows without bound and is not streamed here"
                                          % (i, type(att).__name__))
            if type(att) is not attentions.RelPos1dMultiHeadAttention:
                raise NotImplementedError("stream: block %d attention %s is not RelPos1dMultiHeadAttention" % (i, type(att).__name__))
            dw, bn = blk.conv_module.layers[3], blk.conv_module.layers[4]
            if getattr(dw, "padding_type", "same") != "causal":
                raise NotImplementedError("stream: block %d depthwise conv has padding=%r: only padding='causal' depends on the past alone" % (i, getattr(dw, "padding_type", "same")))
            if not (bn.track_running_stats and bn.running_mean is not None):
                raise NotImplementedError("stream: block %d BatchNorm keeps no running statistics" % i)
            if lookahead and getattr(att, "causal", False):
                raise NotImplementedError("stream: block %d attention is causal=True, whose position table has no row for a future key (the stack's constructor refuses it "
                                          "with right_context > 0)" % i)
            plan.append({"div": div, "stride": blk.stride, "L": m.left_context // div, "R": m.right_context // div, "K": dw.kernel_size[0]})
            div *= blk.stride
        return plan

    # ---- device state ----------------------------------------------------------------------------------------------------------------------------------------------
    def _allocate_controls(self, dev):
        self.pos = torch.zeros(self.B, dtype=torch.int64, device=dev)
        self.reset_flags = self._flags(dev)
        self.clen = torch.full((self.B,), self.Tc, dtype=torch.int64, device=dev)
        self._clen_full = True

    @staticmethod
    def _pos_rows(p, D, dev):
        """the sinusoid rows of E[delta], delta = 0 .. L: the first L + 1 rows of the offline table are the positions L .. 0, the same for every T"""
        return ops.rel_pos_table(p["L"] + 1, D, dev)[:p["L"] + 1].flip(0)

    def _allocate(self, dev):
        B = self.B
        self._allocate_controls(dev)
        self.state = []                    # per block: E table, key / value rings, conv context, BatchNorm scale | shift
        for p, blk in zip(self.plan, self.stack.conformer_blocks):
            att, dw, bn = blk.self_att_module.attention, blk.conv_module.layers[3], blk.conv_module.layers[4]
            D, H, L, Tq = att.dim_model, att.num_heads, p["L"], self.Tc // p["div"]
            C = dw.weight.shape[0]
            pe = self._pos_rows(p, D, dev)                 # E = pos_layer(PE(delta)), projected once
            e = ops.linear_fwd(pe, att.pos_layer.weight, att.pos_layer.bias, pe.shape[0], in_f32=False, out_f32=False)
            kc, vc = ops.relpos_attention_stream_state(B, H, D // H, L, Tq, dev)
            st = ops.BNState(C, pe)
            ops.bn_finalize(bn, st, 1, False)              # eval mode: scale | shift from the running statistics
            self.state.append({"e": e, "kc": kc, "vc": vc, "ss": st.ss, "ctx": ops.glu_dwconv_stream_state(B, C, p["K"], dev)})

    # ---- one push, eager: a fixed sequence of launches on the current stream ------------------------------------------------------------------------------------
    def _attention(self, p, st, blk, x):
        mod = blk.self_att_module
        att, ln = mod.attention, mod.norm
        B, Tq, D = x.shape
        M = B * Tq
        x2 = ops._f32c(x.reshape(M, D))
        h, _, _ = ops.layernorm_fwd(x2, ln.weight, ln.bias, M, D, False, ln.eps)
        q, k, v = att.query_layer, att.key_layer, att.value_layer
        qkv = ops.qkv_project(h, ((q.weight, k.weight, v.weight), (q.bias, k.bias, v.bias)), M, D)
        o = self._attend(p, st, qkv, B, att.num_heads)
        return ops.linear_fwd(o, att.output_layer.weight, att.output_layer.bias, M, in_f32=False, out_f32=True, res=x2, alpha=1.0).view(B, Tq, D)

    def _conv(self, p, st, blk, x):
        mod = blk.conv_module
        ln, pw1, dw, pw2 = mod.layers[0], mod.layers[1], mod.layers[3], mod.layers[6]
        res_conv = None if isinstance(blk.conv_res, nn.Identity) else blk.conv_res
        B, Tq, D = x.shape
        Dp, s = dw.weight.shape[0], p["stride"]
        To = Tq // s
        M, Mo, adt = B * Tq, B * To, rt.act_dtype()
        x2 = ops._f32c(x.reshape(M, D))
        h, _, _ = ops.layernorm_fwd(x2, ln.weight, ln.bias, M, D, False, ln.eps)
        u = ops.linear_fwd(h, pw1.weight, pw1.bias, M, in_f32=False, out_f32=False)
        a = self._dwconv(p, st, u.view(B, Tq, 2 * Dp), dw, s)
        if res_conv is not None:
            rs = res_conv.stride[0]
            R = ops.linear_fwd(x2, res_conv.weight, res_conv.bias, Mo, in_f32=(adt != torch.float32), out_f32=True, rows=ops.rows_plain(D, To, Tq, rs) if rs > 1 else None)
        else:
            R = x2
        return ops.linear_fwd(a.view(Mo, Dp), pw2.weight, pw2.bias, Mo, in_f32=False, out_f32=True, res=R, alpha=1.0).view(B, To, Dp)

    # the two stateful launches and the two ends of a push: what the look-ahead session replaces
    def _attend(self, p, st, qkv, B, H):
        return ops.relpos_attention_stream(qkv, st["e"], st["kc"], st["vc"], self.pos, self.reset_flags, self.clen, p["div"], B=B, H=H, L=p["L"])

    def _dwconv(self, p, st, u, dw, s):
        return ops.glu_dwconv_stream(u, dw.weight, dw.bias, st["ss"], st["ctx"], self.pos, self.reset_flags, self.clen, p["div"], s)

    def _begin(self, x):
        """-> (the rows every block runs on, the input-rate count per slot that becomes out_len)"""
        return x, self.clen

    def _end(self, x):
        ops.stream_advance(self.pos, self.reset_flags, self.clen, self.Tc)

    def _run(self, x):
        stack = self.stack
        x, first = self._begin(x)
        x0, lengths, inter, j = x, first, {}, 0
        for i, (p, st, blk) in enumerate(zip(self.plan, self.state, stack.conformer_blocks)):
            x = blk.ff_module1.residual_forward(x, 0.5)
            x = self._attention(p, st, blk, x)
            x = self._conv(p, st, blk, x)
            x = blk.ff_module2.residual_forward(x, 0.5)
            if isinstance(blk.norm, nn.LayerNorm):
                x = normalizations.torch_layer_norm_forward(blk.norm, x, getattr(blk, "_next_ln", None))
            logits = None
            if i + 1 in stack.interctc_blocks:
                x, logits = stack.interctc_modules[j](x)
                j += 1
            if p["stride"] > 1:
                lengths = ops.len_affine(lengths, 1, p["stride"], 1)
            if logits is not None:
                inter[stack.loss_prefix + "_" + str(i)] = [logits, lengths]
        if lengths is first:
            lengths = lengths.clone()
        self._end(x0)
        return x, lengths, inter

    # ---- host side of a push -----------------------------------------------------------------------------------------------------------------------------------------
    def _controls(self, chunk_len, reset):
        B = self.B
        mask = self._reset_mask(reset)
        host_len = None
        if chunk_len is not None and not torch.is_tensor(chunk_len):
            host_len = [int(v) for v in chunk_len]
            if len(host_len) != B or any(v < 0 or v > self.Tc for v in host_len):
                raise ValueError("push: chunk_len %r for %d slots of at most %d frames" % (host_len, B, self.Tc))
        if not torch.is_tensor(chunk_len):
            for b in range(B):                # (a slot that has ended may idle: further chunks of 0 frames change nothing)
                if self._short[b] and not (mask is not None and mask[b]) and (self.Tc if host_len is None else host_len[b]) > 0:
                    raise RuntimeError("push: slot %d ended with a short chunk and was not reset: a chunk shorter than chunk_frames is legal only as the last one "
                                       "of an utterance (pass reset=[%d] with the next utterance's first chunk)" % (b, b))
        return mask, host_len

    def _upload(self, mask, host_len, chunk_len):
        self._raise_flags(self.reset_flags, mask)
        if torch.is_tensor(chunk_len):
            self.clen.copy_(chunk_len.view(self.B), non_blocking=True)
            self._clen_full = False
            self._short = [False] * self.B           # a device tensor's contract is the caller's
        elif host_len is not None:
            full = all(v == self.Tc for v in host_len)
            if not (full and self._clen_full):
                self.clen.copy_(torch.tensor(host_len, dtype=torch.int64), non_blocking=True)
            self._clen_full = full
            self._short = [v < self.Tc for v in host_len]
        else:
            if not self._clen_full:
                self.clen.fill_(self.Tc)
                self._clen_full = True
            self._short = [False] * self.B

    def _static_input(self, dev):
        D0 = self.stack.conformer_blocks[0].ff_module1.layers[0].normalized_shape[0]
        return torch.zeros(self.B, self.Tc, D0, dtype=torch.float32, device=dev), ([True] * self.B, None, None)

    def _forget(self):
        self._short = [False] * self.B

    def push(self, x_chunk, chunk_len=None, reset=None):
        """x_chunk [B, Tc, D] (the stack's input features) -> (y [B, Tc / S, D_out] fp32, out_len [B] int64 on the device, inter: the offline forward's dict
        loss_prefix_i -> [logits chunk, lengths]).  Slot b takes the first chunk_len[b] frames (a Python list or an int64 device tensor [B]; default all Tc); fewer
        than Tc is legal only as the slot's last chunk before a reset -- until then the slot may only idle on chunks of 0 frames (checked on the host for a list; the
        caller's contract for a device tensor).  Rows at or past
        chunk_len are computed from whatever was passed and never reach the carried state.  reset: slots to restart before this chunk, a list of indices or a host
        bool mask [B]; the first push restarts every slot.  No host synchronisation after the first push; after capture() the results are static tensors that the
        next push overwrites."""
        self._check_chunk(x_chunk)
        mask, host_len = self._controls(chunk_len, reset)
        return self._push(x_chunk, mask, host_len, chunk_len)

    def _check_chunk(self, x_chunk):
        if x_chunk.dim() != 3 or x_chunk.shape[0] != self.B or x_chunk.shape[1] != self.Tc:
            raise ValueError("push: chunk %s for a session of %d slots x %d frames" % (tuple(x_chunk.shape), self.B, self.Tc))
        rt.require_gpu(x_chunk)
        if self.stack.training:
            raise RuntimeError("push: the stack went back to training mode; call .eval()")


class ConformerLookaheadStreamSession(ConformerStreamSession):
    """ConformerInterCTC.stream(lookahead=True): a stack with Mask(left_context=L, right_context=R > 0) run chunk by chunk.  The attention of a block behind total
    stride div sees R // div future frames at its own rate, R // div * div input frames; nothing else in a block looks ahead.  With LA the sum of these over the blocks,
    the stack's rows for input frames < n - LA depend on input frames < n alone.  `lookahead` = LAe is LA rounded up to the total stride, `window` = W = Tc + LAe.
    Every push runs the stack on a window per slot: the pend <= LAe frames carried from earlier pushes, then the new chunk, n valid frames in all.  A running slot
    commits c = max(0, n - LAe) of them: the first c / div key / value rows of each attention go to its ring, the first c / div pre-GLU rows of each convolution to its
    context, the first c / S output rows are emitted, and the other n - c frames stay in the carried tail and are computed again in the next push.  A slot flagged
    `last` emits all ceil(n / S) rows (offline the key-padding mask hides what lies past the length: there is no future) and then idles until it is restarted.  The
    rows a slot has emitted equal the offline forward's, which they trail by LAe input frames; shapes and launches are fixed, so capture() works as on the plain
    session.  ops.stream_window / stream_window_advance build and advance the window; pend, pos and `ended` live on the device with a host mirror for the
    contract check of host-list counts."""

    LOOKAHEAD = True

    def __init__(self, stack, batch_size, chunk_frames):
        super().__init__(stack, batch_size, chunk_frames)
        la = sum(p["R"] * p["div"] for p in self.plan)
        self.lookahead = -(-la // self.S) * self.S
        self.window = self.Tc + self.lookahead
        for i, p in enumerate(self.plan):
            if p["K"] - 1 + self.window // p["div"] > 96:
                raise ValueError("stream: block %d (total stride %d): the window of %d + %d frames is %d rows there and its %d-tap convolution holds context + window in "
                                 "LDS: at most %d rows" % (i, p["div"], self.Tc, self.lookahead, self.window // p["div"], p["K"], 97 - p["K"]))
        self._up = None                            # what self._count holds
        self._forget()

    def _forget(self):
        B = self.B
        self._pend, self._pos, self._ended = [0] * B, [0] * B, [False] * B      # host mirror of the device counters (None: unknown after device-tensor counts)

    # ---- device state ----------------------------------------------------------------------------------------------------------------------------------------------
    def _allocate_controls(self, dev):
        D0 = self.stack.conformer_blocks[0].ff_module1.layers[0].normalized_shape[0]
        self.win = ops.StreamWindowState(self.B, self.Tc, self.lookahead, D0, self.S, dev)
        self.pos = self.win.pos
        self.reset_flags, self.last_flags = self._flags(dev), self._flags(dev)
        self._count = torch.zeros(self.B, dtype=torch.int64, device=dev)

    @staticmethod
    def _pos_rows(p, D, dev):
        """the sinusoid rows of E[delta + R], delta = -R .. L: row T - 1 - delta of the offline table of any T > max(L, R)"""
        L, R = p["L"], p["R"]
        T = max(L, R) + 1
        return ops.rel_pos_table(T, D, dev)[T - 1 - L:T + R].flip(0)

    # ---- one push --------------------------------------------------------------------------------------------------------------------------------------------------
    def _attend(self, p, st, qkv, B, H):
        w = self.win
        return ops.relpos_attention_stream_la(qkv, st["e"], st["kc"], st["vc"], w.pos, self.reset_flags, w.nvalid, w.ncommit, p["div"], B=B, H=H, L=p["L"], R=p["R"])

    def _dwconv(self, p, st, u, dw, s):
        return ops.glu_dwconv_stream_la(u, dw.weight, dw.bias, st["ss"], st["ctx"], self.win.pos, self.reset_flags, self.win.ncommit, p["div"], s)

    def _begin(self, x):
        if not (x.dtype == torch.float32 and x.is_contiguous()):
            x = x.float().contiguous()
        return ops.stream_window(self.win, x, self._count, self.last_flags, self.reset_flags), self.win.emit

    def _end(self, x):
        ops.stream_window_advance(self.win, x, self.last_flags, self.reset_flags)

    # ---- host side of a push -----------------------------------------------------------------------------------------------------------------------------------------
    def _controls(self, chunk_len, last, reset):
        """-> (reset mask, last mask, host counts or None for a device tensor): checks a host-list push against the contract, changes nothing"""
        B, Tc = self.B, self.Tc
        rmask = self._reset_mask(reset) or [False] * B
        lmask = slot_mask(last, B)
        if torch.is_tensor(chunk_len):
            return rmask, lmask, None
        if chunk_len is not None and len(chunk_len) != B:
            raise ValueError("push: chunk_len %r for %d slots" % (list(chunk_len), B))
        counts = []
        for b in range(B):
            ended = False if rmask[b] else self._ended[b]
            if ended is None:
                raise RuntimeError("push: slot %d was last pushed with device-tensor counts, which the host does not mirror: go on with a tensor, or reset the slot" % b)
            c = (0 if ended else Tc) if chunk_len is None else int(chunk_len[b])
            if c < 0 or c > Tc:
                raise ValueError("push: chunk_len[%d] = %d outside 0 .. %d" % (b, c, Tc))
            if ended and c > 0:
                raise RuntimeError("push: slot %d has ended (last) and was not reset: it takes no frames until reset=[%d] starts the next utterance" % (b, b))
            if not ended and not lmask[b] and c != Tc:
                raise ValueError("push: slot %d is running and takes exactly chunk_frames = %d frames, got %d: fewer only with last (the commit rule keeps whole "
                                 "output frames at every stage)" % (b, Tc, c))
            counts.append(c)
        return rmask, lmask, counts

    def _upload(self, rmask, lmask, counts, dev_counts):
        self._raise_flags(self.reset_flags, rmask)
        self._raise_flags(self.last_flags, lmask)
        if counts is None:
            self._count.copy_(dev_counts.view(self.B), non_blocking=True)
            self._up = None
        elif counts != self._up:
            self._count.copy_(torch.tensor(counts, dtype=torch.int64), non_blocking=True)
            self._up = list(counts)
        self._commit(rmask, lmask, counts)

    def _commit(self, rmask, lmask, counts):
        """the host mirror after a push of these controls: the arithmetic of the two control launches (counts None: device-tensor counts, the caller's contract)"""
        B, LAe, S = self.B, self.lookahead, self.S
        if counts is None:
            self._pend, self._pos, self._ended = [None] * B, [None] * B, [None] * B
            return
        for b in range(B):
            pend, pos, ended = (0, 0, False) if rmask[b] else (self._pend[b], self._pos[b], self._ended[b])
            if not ended:
                n = pend + counts[b]
                c = 0 if lmask[b] else max(0, n - LAe) // S * S
                pend, pos, ended = (0 if lmask[b] else n - c), pos + c, lmask[b]
            self._pend[b], self._pos[b], self._ended[b] = pend, pos, ended

    def _static_input(self, dev):
        D0 = self.stack.conformer_blocks[0].ff_module1.layers[0].normalized_shape[0]
        B = self.B
        return torch.zeros(B, self.Tc, D0, dtype=torch.float32, device=dev), ([True] * B, [False] * B, [self.Tc] * B, None)

    def push(self, x_chunk, chunk_len=None, last=None, reset=None):
        """x_chunk [B, Tc, D] -> (y [B, W / S, D_out] fp32, out_len [B] int64 on the device, inter as offline).  Slot b takes the first chunk_len[b] frames (a Python
        list or an int64 device tensor [B]; default Tc, 0 for an ended slot) and yields out_len[b] rows: those of the frames that became final in this push, which
        trail the input by `lookahead` frames, or every remaining row for a slot in `last`.  last: slots whose utterance ends with these frames; reset: slots to
        restart before them (each a list of indices or a host bool mask [B]); the first push restarts every slot.  With host counts the contract is checked on the
        host, without a synchronisation: a running slot takes exactly Tc frames, a slot in `last` any 0 .. Tc, an ended slot none until it is reset.  With a device
        tensor it is the caller's.  No host synchronisation after the first push; after capture() the results are static tensors that the next push overwrites."""
        self._check_chunk(x_chunk)
        rmask, lmask, counts = self._controls(chunk_len, last, reset)
        return self._push(x_chunk, rmask, lmask, counts, chunk_len)


class _FrontStreamSession(_CapturableSession):
    """A front-end run on input chunks of which slot b takes a count of units (UNIT: samples or frames) per push.  Here, once: the device count and flag vectors,
    their host mirror (`_n` units heard and `_ended` per slot; None: unknown after a push with device-tensor counts), the schedule rules of a host-list push
    (_controls), the upload and the mirror's update (_commit).  A subclass gives UNIT, INPUT (the input's name and rank), `_sched` = (first, chunk) counts, `_caps`
    (the most a slot may take at the start of its utterance, and later), _ready(n) (frames that exist after n units), _frames_at_last(b, n0, c), _zero_input(dev), and its _check,
    _allocate (which calls _allocate_controls) and _run."""

    _cap_note = ""                                 # what the refusal of a count above its cap adds about the schedule

    def __init__(self, enc, batch_size, chunk_frames):
        super().__init__(enc, batch_size)
        self.enc, self.Tc = enc, int(chunk_frames)
        self._check(enc)
        if self.B < 1:
            raise ValueError("stream_front: batch_size %d" % self.B)
        self.Tmax = self.Tc + 2                    # any count up to the first push's, at the end of an utterance too, gives at most Tc + 2 frames
        self._forget()
        self._up = None                            # what self._count holds

    def _allocate_controls(self, dev, bn):
        """the count and flag vectors, and `ss`: the eval-mode scale | shift of the stem's BatchNorm from its running statistics"""
        self._count = torch.zeros(self.B, dtype=torch.int64, device=dev)
        self.reset_flags, self.last_flags = self._flags(dev), self._flags(dev)
        st = ops.BNState(bn.num_features, self._count)
        ops.bn_finalize(bn, st, 1, False)
        self.ss = st.ss

    # ---- host side of a push -----------------------------------------------------------------------------------------------------------------------------------------
    def _controls(self, n_units, last, reset):
        """-> (reset mask, last mask, host counts or None for a device tensor, frames per slot or None): checks a host-list push against the contract, changes nothing"""
        B, unit = self.B, self.UNIT
        first, chunk = self._sched
        rmask = self._reset_mask(reset) or [False] * B
        lmask = slot_mask(last, B)
        if torch.is_tensor(n_units):
            return rmask, lmask, None, None
        if n_units is not None and len(n_units) != B:
            raise ValueError("push: n_%s %r for %d slots" % (unit, list(n_units), B))
        counts, frames = [], []
        (cap0, cap1), ready = self._caps, self._ready      # (a push is partly host-bound: no attribute lookups per slot)
        for b in range(B):
            n0, ended = (0, False) if rmask[b] else (self._n[b], self._ended[b])
            if n0 is None:
                raise RuntimeError("push: slot %d was last pushed with device-tensor counts, which the host does not mirror: go on with a tensor, or reset the slot" % b)
            c = (0 if ended else (first if n0 == 0 else chunk)) if n_units is None else int(n_units[b])
            cap = cap0 if n0 == 0 else cap1
            if c < 0 or c > cap:
                raise ValueError("push: n_%s[%d] = %d outside 0 .. %d%s" % (unit, b, c, cap, self._cap_note))
            if ended:
                if c > 0:
                    raise RuntimeError("push: slot %d has ended (last) and was not reset: it takes no %s until reset=[%d] starts the next utterance" % (b, unit, b))
                frames.append(0)
            elif lmask[b]:
                frames.append(self._frames_at_last(b, n0, c))
            else:
                frames.append(ready(n0 + c) - ready(n0))
            counts.append(c)
        return rmask, lmask, counts, frames

    def _commit(self, rmask, lmask, counts):
        """the host mirror after a push of these controls (counts None: device-tensor counts, whose contract is the caller's)"""
        B = self.B
        if counts is None:
            self._n, self._ended = [None] * B, [None] * B
            return
        for b in range(B):
            n0, ended = (0, False) if rmask[b] else (self._n[b], self._ended[b])
            self._n[b], self._ended[b] = n0 + counts[b], ended or lmask[b]

    def _upload(self, rmask, lmask, counts, dev_counts):
        self._raise_flags(self.reset_flags, rmask)
        self._raise_flags(self.last_flags, lmask)
        if counts is None:
            self._count.copy_(dev_counts.view(self.B), non_blocking=True)
            self._up = None
        elif counts != self._up:
            self._count.copy_(torch.tensor(counts, dtype=torch.int64), non_blocking=True)
            self._up = list(counts)
        self._commit(rmask, lmask, counts)

    def _static_input(self, dev):
        B, first = self.B, self._sched[0]
        return self._zero_input(dev), ([True] * B, [False] * B, [first] * B, None)

    def _forget(self):
        self._n, self._ended = [0] * self.B, [False] * self.B

    def _check_input(self, x):
        """what every push checks of its input before the controls"""
        name, rank = self.INPUT
        if x.dim() != rank or x.shape[0] != self.B or x.shape[1] != self._sched[0]:
            raise ValueError("push: %s %s for a session of %d slots x %d %s" % (name, tuple(x.shape), self.B, self._sched[0], self.UNIT))
        rt.require_gpu(x)
        if self.enc.training:
            raise RuntimeError("push: the encoder went back to training mode; call .eval()")


class AudioFrontStreamSession(_FrontStreamSession):
    """AudioEfficientConformerEncoder.stream_front(): the audio front-end (log-mel -> Conv2d + BatchNorm2d + Swish stem -> Linear) run on waveform chunks.  The frames a
    slot has produced after any sequence of pushes equal the offline front-end's frames on the samples pushed so far (and, once the utterance has ended, on the whole
    utterance: both STFT reflections and both zero paddings of the stem included), up to the DFT GEMM's tile choice.  Mel frame f reads samples [160 f - 200, 160 f + 200),
    stem frame t reads mel frames 2t - 1, 2t, 2t + 1: with n samples heard E(n) = 0 if n < 360 else (n - 40) // 320 frames exist, Ta // 320 + 1 at the end.  Schedule:
    first_samples = 320 Tc + 40 in an utterance's first push, chunk_samples = 320 Tc in every later one; every push but the last then yields exactly Tc frames, the last at
    most Tc + 1.  The carried state is a sample tail of fewer than 720 samples per slot, a counter and an `ended` flag, on the device (ops.audio_stream_state)."""

    UNIT, INPUT = "samples", ("wave", 2)

    def __init__(self, enc, batch_size, chunk_frames):
        super().__init__(enc, batch_size, chunk_frames)
        if self.Tc < 2:
            raise ValueError("stream_front: chunk_frames = %d: a push of %d samples would be shorter than one %d-sample analysis window; at least 2 frames (80 ms) per push"
                             % (self.Tc, 2 * self.hop * self.Tc, self.win))
        self.first_samples, self.chunk_samples = self._sched = 2 * self.hop * self.Tc + (self.win // 2 - self.hop), 2 * self.hop * self.Tc
        self._caps = (self.first_samples, self.first_samples)

    def _check(self, enc):
        if enc.training:
            raise RuntimeError("stream_front: the encoder is in training mode (SpecAugment and BatchNorm batch statistics are not functions of the past): call .eval() first")
        pre = enc.audio_preprocessing
        if pre.normalize:
            raise NotImplementedError("stream_front: AudioPreprocessing(normalize=True) is not streamed: the stem's zero padding would have to become (0 - mean) / std columns")
        conv, bn = enc.subsampling_module.layers[0][0], enc.subsampling_module.layers[0][1]
        if not (bn.track_running_stats and bn.running_mean is not None):
            raise NotImplementedError("stream_front: the stem's BatchNorm keeps no running statistics")
        self.n_fft, self.win, self.hop, self.n_mels = pre.n_fft, pre.win_length, pre.hop_length, pre.n_mels
        if self.win // 2 < self.hop or self.win % 2:
            raise NotImplementedError("stream_front: window %d / hop %d: the schedule needs an even window of at least two hops" % (self.win, self.hop))
        if tuple(conv.weight.shape[1:]) != (1, 3, 3):
            raise NotImplementedError("stream_front: the stem is not a 3x3 convolution of one input channel")

    def _ready(self, n):
        a = self.hop + self.win // 2
        return 0 if n < a else (n - a) // (2 * self.hop) + 1

    def _frames_at_last(self, b, n0, c):
        if n0 + c <= self.n_fft // 2:
            raise ValueError("push: slot %d ends after %d samples: an utterance of at most n_fft / 2 = %d samples cannot be reflect-padded (refused offline as well)"
                             % (b, n0 + c, self.n_fft // 2))
        return (n0 + c) // (2 * self.hop) + 1 - self._ready(n0)

    def _allocate(self, dev):
        self.state = ops.audio_stream_state(self.B, dev)
        self._allocate_controls(dev, self.enc.subsampling_module.layers[0][1])
        self.nsamp = self._count

    def _run(self, wave):
        if not (wave.dtype == torch.float32 and wave.stride(1) == 1):
            wave = wave.float().contiguous()
        enc, pre = self.enc, self.enc.audio_preprocessing
        conv, lin = enc.subsampling_module.layers[0][0], enc.linear
        B, Tmax = self.B, self.Tmax
        kw = dict(n_fft=self.n_fft, win=self.win, hop=self.hop)
        frames, out_len, meta = ops.mel_frames_stream(wave, pre.Spectrogram.window, self.state, self.nsamp, self.reset_flags, self.last_flags, Tmax=Tmax, **kw)
        mel = ops.mel_from_frames(frames, pre._dft_matrix(wave.device), pre.MelScale.fb, B, 2 * Tmax + 1, self.n_mels)
        a = ops.audio_stem_stream(mel, conv.weight, conv.bias, self.ss, out_len, meta, conv.weight.shape[0])
        ops.audio_stream_advance(wave, self.state, self.nsamp, self.reset_flags, self.last_flags, **kw)
        feat = ops.linear_fwd(a.view(B * Tmax, -1), lin.weight, lin.bias, B * Tmax, in_f32=False, out_f32=True)
        return feat.view(B, Tmax, -1), out_len

    def _zero_input(self, dev):
        return torch.zeros(self.B, self.first_samples, dtype=torch.float32, device=dev)

    def push(self, wave, n_samples=None, last=None, reset=None):
        """wave [B, first_samples] fp32 -> (feat [B, Tc + 2, 180] fp32, out_len [B] int64 on the device): slot b takes the first n_samples[b] samples (a Python list
        or an int64 device tensor [B]; default: the schedule's count, first_samples after a restart, chunk_samples later, 0 for an ended slot) and yields out_len[b]
        frames; rows at or past out_len carry no information.  last: slots whose utterance ends with these samples; reset: slots to restart before them (each a list
        of indices or a host bool mask [B]); the first push restarts every slot.  With host counts the contract is checked on the host, without a synchronisation:
        counts within 0 .. first_samples, an utterance longer than n_fft / 2 = 256 samples at `last`, no samples to an ended slot.  With a device tensor it is the
        caller's.  No host synchronisation after the first push; after capture() the results are static tensors that the next push overwrites."""
        self._check_input(wave)
        rmask, lmask, counts, _ = self._controls(n_samples, last, reset)
        return self._push(wave, rmask, lmask, counts, n_samples)


class VisualFrontStreamSession(_FrontStreamSession):
    """VisualEfficientConformerEncoder.stream_front(): the visual front-end (Conv3d stem + BatchNorm3d + ReLU + max pool -> ResNet-18 -> Linear) run on video chunks.
    The frames a slot has produced after any sequence of pushes equal the offline front-end's frames on the frames pushed so far (and, once the utterance has ended, on
    the whole utterance: both temporal zero paddings included).  Everything behind the Conv3d works per frame and eval-mode BatchNorm uses running statistics, so the
    only coupling in time is the five-tap window: output frame t reads input frames t - 2 .. t + 2, with n frames heard E(n) = max(0, n - 2) frames exist, n at the
    end; the look-ahead is 2 frames.  Schedule: first_frames = Tc + 2 in an utterance's first push, chunk_frames = Tc in every later one; every push but the last then
    yields exactly Tc frames, the last at most Tc + 2.  The carried state is a ring of the last 4 input frames per slot, a counter and an `ended` flag, on the device
    (ops.video_stream_state).  The stem launch writes its frames frame-major, so the first Tc * B of them are a plain view: the ResNet and the Linear run on B * Tc
    frames, and on the 2 B tail frames only in a push where some slot can yield more than Tc (`resnet_frames` records what the last push ran)."""

    UNIT, INPUT = "frames", ("video", 4)

    def __init__(self, enc, batch_size, chunk_frames):
        super().__init__(enc, batch_size, chunk_frames)
        if self.Tc < 1:
            raise ValueError("stream_front: chunk_frames = %d: at least 1 frame per push" % self.Tc)
        self.first_frames, self.chunk_frames = self._sched = self._caps = self.Tc + 2, self.Tc
        self._cap_note = " (first_frames = %d at the start of an utterance, chunk_frames = %d later)" % self._sched
        self._frames = self._feat = None           # the stem's frames and the features of the last push (static after capture())
        self.resnet_frames = 0                     # frames the ResNet and the Linear ran on in the last push

    def _check(self, enc):
        if enc.training:
            raise RuntimeError("stream_front: the encoder is in training mode (BatchNorm batch statistics are not functions of the past): call .eval() first")
        stem = enc.front_end[0].layers[0]
        conv, bn = stem[0], stem[1]
        if not (bn.track_running_stats and bn.running_mean is not None):
            raise NotImplementedError("stream_front: the stem's BatchNorm keeps no running statistics")
        if not (tuple(conv.weight.shape) == (64, 1, 5, 7, 7) and tuple(conv.stride) == (1, 2, 2) and getattr(conv, "padding_type", "same") == "same"):
            raise NotImplementedError("stream_front: the stem is not the (5, 7, 7) / stride (1, 2, 2) 'same' convolution of one input channel into 64 (weight %s, stride %s)"
                                      % (tuple(conv.weight.shape), tuple(conv.stride)))

    @staticmethod
    def _ready(n):
        return max(0, n - 2)

    def _frames_at_last(self, b, n0, c):
        return n0 + c - self._ready(n0)

    def _allocate(self, dev):
        stem = self.enc.front_end[0].layers[0]
        self._allocate_controls(dev, stem[1])
        self.nframes = self._count
        self.w8 = ops.video_stem_w8(stem[0].weight)    # once per session, not once per push
        self.state = {"ring": None}                    # the ring's size depends on the frame: allocated by the first _run

    def _resnet(self, frames, f0, f1, feat):
        """frames f0 .. f1 - 1 of the frame-major stem output through the ResNet and the Linear -> feat[:, f0:f1]"""
        nf, B = f1 - f0, self.B
        y = self.enc.front_end[3].forward_nhwc(frames[f0:f1].reshape(nf * B, *frames.shape[2:]))
        feat[:, f0:f1].copy_(y.view(nf, B, -1).transpose(0, 1))

    def _run(self, video):
        if not (video.dtype == torch.float32 and video.is_contiguous()):
            video = video.float().contiguous()
        B, Tc = self.B, self.Tc
        if self.state["ring"] is None:
            self.state["ring"] = ops.video_stream_state(B, video.shape[2], video.shape[3], video.device)
        conv = self.enc.front_end[0].layers[0][0]
        frames, out_len = ops.video_stem_stream(video, self.state["ring"], self.w8, conv.bias, self.ss, self.nframes, self.reset_flags, self.last_flags, Tmax=self.Tmax)
        ops.video_stream_advance(video, self.state["ring"], self.nframes, self.reset_flags, self.last_flags)
        feat = torch.zeros(B, self.Tmax, self.enc.front_end[3].head[1].weight.shape[0], dtype=torch.float32, device=video.device)
        self._resnet(frames, 0, Tc, feat)
        self._frames, self._feat = frames, feat
        return feat, out_len

    def _zero_input(self, dev):
        return torch.zeros(self.B, self.first_frames, *self._capture_frame, dtype=torch.float32, device=dev)

    def capture(self, device=None, frame=(88, 88)):
        """As the other sessions' capture(); `frame` = (H, W) of the video the session will be fed.  The captured push covers the Tc-frame case; a push in which some
        slot can yield more than Tc frames runs the ResNet on the 2 B tail frames eagerly behind the replay."""
        self._capture_frame = (int(frame[0]), int(frame[1]))
        return super().capture(device)

    def push(self, video, n_frames=None, last=None, reset=None):
        """video [B, Tc + 2, H, W] fp32 ([B, 1, Tc + 2, H, W] is viewed) -> (feat [B, Tc + 2, 256] fp32, out_len [B] int64 on the device): slot b takes the first
        n_frames[b] frames (a Python list or an int64 device tensor [B]; default: the schedule's count, first_frames after a restart, chunk_frames later, 0 for an
        ended slot) and yields out_len[b] frames; rows at or past out_len carry no information.  last: slots whose utterance ends with these frames; reset: slots to
        restart before them (each a list of indices or a host bool mask [B]); the first push restarts every slot.  With host counts the contract is checked on the
        host, without a synchronisation: counts within 0 .. chunk_frames (0 .. first_frames for a slot at its start), no frames to an ended slot.  With a device
        tensor it is the caller's.  No host synchronisation after the first push; after capture() the results are static tensors that the next push overwrites."""
        if video.dim() == 5 and video.shape[1] == 1:
            video = video[:, 0]
        self._check_input(video)
        if self._capture is not None and tuple(video.shape[2:]) != self._capture_frame:
            raise ValueError("push: frames of %dx%d for a push captured at %dx%d" % (video.shape[2], video.shape[3], *self._capture_frame))
        rmask, lmask, counts, frames = self._controls(n_frames, last, reset)
        feat, out_len = self._push(video, rmask, lmask, counts, n_frames)
        self.resnet_frames = self.B * self.Tc
        if frames is None or any(f > self.Tc for f in frames):          # (device-tensor counts: the host cannot know, the tail always runs)
            with torch.no_grad():
                self._resnet(self._frames, self.Tc, self.Tmax, self._feat)
            self.resnet_frames = self.B * self.Tmax
        return feat, out_len


def _head(enc, y):
    return y if isinstance(enc.head, nn.Identity) else enc.head(y)


def _push_again(back, enc, first, feed, n):
    """(logits, lengths, inter) of a push of the stack session `back` -> the same with the first n rows of a second push appended, whose (input, chunk lengths)
    feed() gives.  A captured stack's results are static tensors that the second push refills: they are cloned before feed() and the push launch anything."""
    logits, ylen, inter = first[0].clone(), first[1].clone(), {k: [v[0].clone(), v[1].clone()] for k, v in first[2].items()}
    y2, ylen2, inter2 = back.push(*feed(), None)
    for k, v in inter.items():
        inter[k] = [torch.cat([v[0], inter2[k][0][:, :n]], dim=1), v[1] + inter2[k][1]]
    return torch.cat([logits, _head(enc, y2[:, :n].contiguous())], dim=1), ylen + ylen2, inter


class _BranchStreamSession:
    """FRONT(enc, B, Tc) feeds enc.back_end.stream(B, Tc) (a ConformerStreamSession, with its refusals) and the head.  The front's schedule makes every push but an
    utterance's last yield exactly Tc frames, one chunk of the stack; a last push may leave a tail of up to TAIL frames beyond Tc: the stack is then pushed a second
    time with the tail frames of the slots concerned and 0 frames (no change of state) for the others, and the rows that yields are appended."""

    def __init__(self, enc, batch_size, chunk_frames):
        self.enc = enc
        self.front = self.FRONT(enc, batch_size, chunk_frames)
        self.back = enc.back_end.stream(batch_size, chunk_frames)
        self.B, self.Tc, self.S = self.front.B, self.front.Tc, self.back.S
        if self.Tc < self.TAIL:
            raise ValueError("stream: chunk_frames = %d: at least %d, so that a last push's tail of up to %d frames fits one chunk of the stack" % (self.Tc, self.TAIL, self.TAIL))
        self._x2 = None

    def _plan(self, n_units, last, reset):
        """the host side of a push, before anything is launched: the front's controls (reset mask, last mask, counts, frames per slot), checked against the schedule"""
        unit = self.front.UNIT
        if torch.is_tensor(n_units):
            raise TypeError("push: the combined session takes host lists for n_%s (it decides on the host whether the stack needs a second push)" % unit)
        Tc = self.Tc
        rmask, lmask, counts, frames = self.front._controls(n_units, last, reset)
        for b in range(self.B):
            if not (frames[b] == Tc or counts[b] == 0 or (lmask[b] and frames[b] <= Tc + self.TAIL)):
                raise ValueError("push: slot %d would yield %d frames from %s: off the schedule (first_%s = %d in an utterance's first push, chunk_%s = %d later, "
                                 "fewer only with last)" % (b, frames[b], self.FROM % counts[b], unit, self.front._sched[0], unit, self.front._sched[1]))
        return rmask, lmask, counts, frames

    def _tail_input(self, feat, tail):
        """a chunk of the stack whose first TAIL rows are the front's rows behind Tc, and the tail per slot as its chunk lengths"""
        if self._x2 is None:
            self._x2 = torch.zeros(self.B, self.Tc, feat.shape[2], dtype=feat.dtype, device=feat.device)
        self._x2[:, :self.TAIL].copy_(feat[:, self.Tc:self.Tc + self.TAIL])
        return self._x2, torch.tensor(tail, dtype=torch.int64)

    def _push_branch(self, x, n_units, last, reset):
        Tc = self.Tc
        rmask, lmask, counts, frames = self._plan(n_units, last, reset)
        with torch.no_grad():
            feat, _ = self.front.push(x, counts, lmask, rmask)
            tail = [max(0, f - Tc) for f in frames]
            y, ylen, inter = self.back.push(feat[:, :Tc], torch.tensor([min(f, Tc) for f in frames], dtype=torch.int64), rmask)
            if not any(tail):
                return _head(self.enc, y), ylen, inter
            return _push_again(self.back, self.enc, (_head(self.enc, y), ylen, inter), lambda: self._tail_input(feat, tail), -(-max(tail) // self.S))

    def capture(self, device=None, **front_args):
        """capture both halves (the front session's capture with front_args, ConformerStreamSession.capture); call it before the first push"""
        self.front.capture(device, **front_args)
        self.back.capture(device)
        return self


class AudioStreamSession(_BranchStreamSession):
    """AudioEfficientConformerEncoder.stream(): waveform chunks -> logits.  The front session feeds back_end.stream() (a ConformerStreamSession, with its refusals) and
    the head.  The front's schedule makes every push but an utterance's last yield exactly Tc frames, one chunk of the stack; a last push may yield Tc + 1: the stack
    is then pushed a second time with that one frame for the slots concerned and 0 frames (no change of state) for the others, and its first output row is appended."""

    FRONT, TAIL, FROM = AudioFrontStreamSession, 1, "%d samples"

    def __init__(self, enc, batch_size, chunk_frames):
        super().__init__(enc, batch_size, chunk_frames)
        self.first_samples, self.chunk_samples = self.front._sched

    def push(self, wave, n_samples=None, last=None, reset=None):
        """wave [B, first_samples] fp32 -> (logits [B, R, V] fp32, out_len [B] int64 on the device, inter: loss_prefix_i -> [logits chunk, lengths] as offline).
        n_samples / last / reset: host lists as AudioFrontStreamSession.push; counts must follow the schedule (every push of a slot but its last yields exactly
        chunk_frames frames; a slot may idle on 0 samples).  R = Tc / S, or Tc / S + 1 in a push where some slot's last chunk produced Tc + 1 frames."""
        return self._push_branch(wave, n_samples, last, reset)


class VisualStreamSession(_BranchStreamSession):
    """VisualEfficientConformerEncoder.stream(): video chunks -> logits.  The front session feeds back_end.stream() (a ConformerStreamSession, with its refusals) and
    the head.  The front's schedule makes every push but an utterance's last yield exactly Tc frames, one chunk of the stack; a last push may yield Tc + 1 or Tc + 2:
    the stack is then pushed a second time with those tail frames for the slots concerned and 0 frames (no change of state) for the others, and the rows it yields
    are appended."""

    FRONT, TAIL, FROM = VisualFrontStreamSession, 2, "%d"

    def __init__(self, enc, batch_size, chunk_frames):
        super().__init__(enc, batch_size, chunk_frames)
        self.first_frames, self.chunk_frames = self.front._sched

    def push(self, video, n_frames=None, last=None, reset=None):
        """video [B, Tc + 2, H, W] fp32 -> (logits [B, R, V] fp32, out_len [B] int64 on the device, inter: loss_prefix_i -> [logits chunk, lengths] as offline).
        n_frames / last / reset: host lists as VisualFrontStreamSession.push; counts must follow the schedule (every push of a slot but its last yields exactly
        chunk_frames frames; a slot may idle on 0 frames).  R = Tc / S, or Tc / S + ceil(tail / S) in a push where some slot's last chunk left a tail of 1 or 2
        frames beyond Tc (one more row for every S >= 2)."""
        return self._push_branch(video, n_frames, last, reset)

    def capture(self, device=None, frame=(88, 88)):
        """capture both halves (VisualFrontStreamSession.capture, ConformerStreamSession.capture); call it before the first push"""
        return super().capture(device, frame=frame)


class AudioVisualStreamSession(_StreamSession):
    """AudioVisualEfficientConformerEncoder.stream(): video and waveform chunks -> logits.  video_encoder.stream(B, Tv) and audio_encoder.stream(B, 2 Tv) (both built
    without a head: they return their stacks' rows, with their refusals) feed ops.av_fuse_stream, the fusion module's two Linears, audio_visual_encoder.stream(B, R)
    and the head; R = Tv / S_v = 2 Tv / S_a rows per regular push.  An utterance of T video frames has 640 T - 160 samples and both branches yield ceil(T / 2) rows at
    the 80 ms rate, but not in the same pushes: the audio front-end looks 40 samples ahead and the video stem 2 frames, so for T mod Tv in {1, 2} the video branch ends
    one push before the audio branch and is, for one push, one row ahead.  The fuse launch keeps the unpaired rows per slot in two rings of cap = R + 2 rows and emits
    at most R pairs; where some slot still has a pair pending (an utterance's last push can bring R + 1 rows), a second fuse launch without new rows and a second
    stack push follow and their rows are appended, as in the two branch sessions.  The host mirrors the rings' counters (rows pending per branch, rows since the
    restart, `ended` per branch): ring overflow and branches whose row totals differ at the end of an utterance are refused before anything is launched."""

    def __init__(self, enc, batch_size, chunk_frames):
        super().__init__(batch_size)
        self.enc, self.Tv = enc, int(chunk_frames)
        if enc.training:
            raise RuntimeError("stream: the encoder is in training mode (BatchNorm batch statistics, SpecAugment and dropout are not functions of the past): call .eval() first")
        self.video = enc.video_encoder.stream(batch_size, self.Tv)
        self.audio = enc.audio_encoder.stream(batch_size, 2 * self.Tv)
        if self.Tv % self.video.S or 2 * self.Tv % self.audio.S or self.Tv // self.video.S != 2 * self.Tv // self.audio.S:
            raise ValueError("stream: chunk_frames = %d gives %g rows per push behind the video stack (stride %d) and %g behind the audio stack (stride %d, %d stem frames): "
                             "the two branches must yield the same whole number of rows" % (self.Tv, self.Tv / self.video.S, self.video.S, 2 * self.Tv / self.audio.S,
                                                                                                self.audio.S, 2 * self.Tv))
        self.R = self.Tv // self.video.S
        self.cap = self.R + 2
        self.back = enc.audio_visual_encoder.stream(batch_size, self.R)
        self.first_frames, self.chunk_frames = self.video.first_frames, self.video.chunk_frames
        self.first_samples, self.chunk_samples = self.audio.first_samples, self.audio.chunk_samples
        self._forget()

    def _forget(self):
        B = self.B
        self._pend_a, self._pend_v = [0] * B, [0] * B          # host mirrors: rows received and not yet paired, per branch
        self._rows_a, self._rows_v = [0] * B, [0] * B          # rows received since the restart
        self._end_a, self._end_v = [False] * B, [False] * B

    def _commit(self, mirrors):
        """the host mirrors after a push: the last entry of what _plan returned for it"""
        self._first = False
        self._pend_a, self._pend_v, self._rows_a, self._rows_v, self._end_a, self._end_v = mirrors

    def schedule(self, n_video_frames, n_audio_samples):
        """-> per push (n_frames, n_samples, last_video, last_audio) for one utterance on both branch sessions' schedules: first_frames / first_samples in the first
        push, chunk_frames / chunk_samples later, the rest in each branch's last; a branch that has ended idles on 0"""
        T, Ta = int(n_video_frames), int(n_audio_samples)
        if T < 1 or Ta < 1:
            raise ValueError("schedule: an utterance of %d frames and %d samples" % (T, Ta))
        v, a = [], []
        while sum(v) < T:
            v.append(min(T - sum(v), self.chunk_frames if v else self.first_frames))
        while sum(a) < Ta:
            a.append(min(Ta - sum(a), self.chunk_samples if a else self.first_samples))
        return [(v[i] if i < len(v) else 0, a[i] if i < len(a) else 0, i == len(v) - 1, i == len(a) - 1) for i in range(max(len(v), len(a)))]

    @staticmethod
    def _rows(frames, Tc, S):
        """rows a branch session returns for `frames` front-end frames: the chunk of the stack's first push and the tail of its second, each rounded up"""
        return -(-min(frames, Tc) // S) + -(-max(0, frames - Tc) // S)

    def _plan(self, n_frames, n_samples, last_video, last_audio, reset):
        """the host side of a push, before anything is launched: both branches' controls, the mirrors after the push and the pairs of every fuse launch"""
        B, R = self.B, self.R
        rmask = self._reset_mask(reset) or [False] * B
        vplan = self.video._plan(n_frames, last_video, rmask)
        aplan = self.audio._plan(n_samples, last_audio, rmask)
        pend_a, pend_v, rows_a, rows_v, end_a, end_v = [], [], [], [], [], []
        for b in range(B):
            pa, pv, ta, tv, ea, ev = (0, 0, 0, 0, False, False) if rmask[b] else (self._pend_a[b], self._pend_v[b], self._rows_a[b], self._rows_v[b], self._end_a[b], self._end_v[b])
            na, nv = self._rows(aplan[3][b], 2 * self.Tv, self.audio.S), self._rows(vplan[3][b], self.Tv, self.video.S)
            if pa + na > self.cap or pv + nv > self.cap:
                raise RuntimeError("push: slot %d would hold %d audio and %d video rows that are not paired yet: the rings keep %d (one branch ran ahead of the other; "
                                   "both must follow one utterance's schedule)" % (b, pa + na, pv + nv, self.cap))
            ends = (aplan[1][b] and not ea) or (vplan[1][b] and not ev)
            ea, ev = ea or aplan[1][b], ev or vplan[1][b]
            if ends and ea and ev and ta + na != tv + nv:
                raise ValueError("push: slot %d ends its utterance with %d audio rows and %d video rows: the branches must yield the same number (the offline forward fails "
                                 "in cat); T video frames go with 640 T - 160 samples" % (b, ta + na, tv + nv))
            pend_a.append(pa + na), pend_v.append(pv + nv), rows_a.append(ta + na), rows_v.append(tv + nv), end_a.append(ea), end_v.append(ev)
        launches = []                                          # pairs per slot of every fuse launch: the first always runs, further ones while a pair is pending
        while True:
            m = [min(pend_a[b], pend_v[b], R) for b in range(B)]
            if launches and not any(m):
                break
            launches.append(m)
            pend_a, pend_v = [p - k for p, k in zip(pend_a, m)], [p - k for p, k in zip(pend_v, m)]
        return rmask, vplan, aplan, launches, (pend_a, pend_v, rows_a, rows_v, end_a, end_v)

    def _ensure_fuse(self, ya, yv):
        if self.state is None:
            dev = ya.device
            self.state = ops.av_fuse_stream_state(self.B, ya.shape[2], yv.shape[2], self.cap, dev)
            self.reset_flags = self._flags(dev)
            self._no_rows = torch.zeros(self.B, dtype=torch.int64, device=dev)

    def _fuse(self, ya, alen, yv, vlen, flags):
        """the fuse launch -> the fusion module on the pairs (the two Linears of ops.FusionFn.forward on the operand the kernel wrote) -> (x [B, R, F] fp32, pair_len)"""
        l1, l2 = self.enc.fusion_module.layers[0], self.enc.fusion_module.layers[2]
        B, R = self.B, self.R
        xc, plen = ops.av_fuse_stream(ya, alen, yv, vlen, self.state, flags, R)
        h = ops.linear_fwd(xc.view(B * R, -1), l1.weight, l1.bias, B * R, in_f32=False, out_f32=False, act=ops.ACT_SWISH)
        return ops.linear_fwd(h, l2.weight, l2.bias, B * R, in_f32=False, out_f32=True).view(B, R, -1), plen

    def push(self, video, wave, n_frames=None, n_samples=None, last_video=None, last_audio=None, reset=None):
        """video [B, Tv + 2, H, W] fp32, wave [B, first_samples] fp32 -> (logits [B, R or R + n2, V] fp32, out_len [B] int64 on the device, inter: the v_ctc_*, a_ctc_* and
        f_ctc_* entries of the offline forward, [logits chunk, lengths] each with its own lengths).  n_frames / n_samples / last_video / last_audio / reset: host lists
        as in VisualStreamSession.push and AudioStreamSession.push (schedule() gives one utterance's); one reset restarts the slot in both branches, the rings and the
        fusion stack.  n2: the most pairs any slot still had pending behind the first R (at most R).  No host synchronisation after the first push; after capture() the
        entries of inter are static tensors that the next push overwrites."""
        B, R = self.B, self.R
        if video.dim() == 5 and video.shape[1] == 1:
            video = video[:, 0]
        if video.dim() != 4 or video.shape[0] != B or video.shape[1] != self.first_frames:
            raise ValueError("push: video %s for a session of %d slots x %d frames" % (tuple(video.shape), B, self.first_frames))
        if wave.dim() != 2 or wave.shape[0] != B or wave.shape[1] != self.first_samples:
            raise ValueError("push: wave %s for a session of %d slots x %d samples" % (tuple(wave.shape), B, self.first_samples))
        rt.require_gpu(video)
        rt.require_gpu(wave)
        if self.enc.training:
            raise RuntimeError("push: the encoder went back to training mode; call .eval()")
        rmask, vplan, aplan, launches, mirrors = self._plan(n_frames, n_samples, last_video, last_audio, reset)
        with torch.no_grad():
            yv, vlen, inter = self.video.push(video, vplan[2], vplan[1], rmask)
            ya, alen, a_inter = self.audio.push(wave, aplan[2], aplan[1], rmask)
            inter = dict(inter)
            inter.update(a_inter)
            ya, yv = ya.contiguous(), yv.contiguous()
            self._ensure_fuse(ya, yv)
            self._commit(mirrors)
            x, plen = self._fuse(ya, alen, yv, vlen, self._raise_flags(self.reset_flags, rmask))
            y, ylen, f_inter = self.back.push(x, plen, rmask)
            logits = _head(self.enc, y)
            for m in launches[1:]:                             # a fuse launch without new rows, a push of the stack on its pairs
                logits, ylen, f_inter = _push_again(self.back, self.enc, (logits, ylen, f_inter), lambda: self._fuse(ya, self._no_rows, yv, self._no_rows, None),
                                                    -(-max(m) // self.back.S))
            inter.update(f_inter)
            return logits, ylen, inter

    def capture(self, device=None, frame=(88, 88)):
        """capture the three sub-sessions (VisualStreamSession.capture, AudioStreamSession.capture, ConformerStreamSession.capture); the fuse launch, the fusion module
        and the head stay eager launches between the replays.  Call it before the first push"""
        self.video.capture(device, frame)
        self.audio.capture(device)
        self.back.capture(device)
        return self


class CTCBeamStreamSession(_StreamSession):
    """CTCBeamSearchDecoder.stream(): the beam search of avec_amd/csrc/ctc_beam.hip carried across logit chunks (one launch per push, the beam state stays on the
    device).  The search is the offline one bit for bit: after any sequence of pushes the beams are those of beam_search on the frames pushed so far.  One launch
    per push and nothing to replay: it is not capturable."""

    def __init__(self, decoder, batch_size, max_frames):
        super().__init__(batch_size)
        self.dec, self.max_frames = decoder, int(max_frames)
        if self.B < 1 or self.max_frames < 1:
            raise ValueError("stream: batch_size %d, max_frames %d" % (self.B, self.max_frames))
        self._frames = [0] * self.B                      # per slot, an upper bound of the frames it holds (Tc per push): the capacity check needs no sync
        self._emitted = False                            # the state's outputs describe every frame pushed so far

    def _allocate(self, dev):
        self.state = ops.CTCBeamStreamState(self.B, self.dec.beam_size, self.max_frames, dev)
        self.reset_flags = self.state.reset_flags

    def _launch(self, chunk, chunk_len, reset, emit):
        d = self.dec
        out = ops.ctc_beam_stream(self.state, chunk, chunk_len, reset, d.ngram_tmp, d.lm(chunk.shape[-1]), d.ngram_alpha, d.ngram_beta, emit=emit)
        self._emitted = emit
        return out

    def push(self, logits_chunk, chunk_len=None, reset=None, fetch=True):
        """Consume logits_chunk [B, Tc, V]; slot b takes chunk_len[b] frames of it (int64 tensor; default: all Tc).  reset: slots to restart from the empty
        transcript before this chunk, as a list of indices or a host bool mask [B] (a device mask costs a synchronisation); the first push resets every slot.
        A push after which a slot could hold more than max_frames frames raises RuntimeError before anything is launched (each push counts as Tc frames for every
        slot, whatever chunk_len says).
        fetch=True returns one record per slot: {"partial_ids": the best hypothesis so far (the n-gram beam's; neural rescoring happens in finish()),
        "stable_ids": its leading tokens that every live beam shares and no later frame can change}, and with a tokenizer "partial" and "stable", their text.
        "stable" is decode(stable_ids): it is final token by token, not character by character (a later piece can still complete its last word).
        fetch=False skips the traceback and copies nothing to the host."""
        B, Tc, self._V = logits_chunk.shape
        if B != self.B:
            raise ValueError("push: chunk of %d utterances for a session of %d" % (B, self.B))
        mask = self._reset_mask(reset)
        frames = [(0 if mask is not None and mask[b] else n) + Tc for b, n in enumerate(self._frames)]
        if max(frames) > self.max_frames:
            raise RuntimeError("push: %d frames in a slot of a session with max_frames = %d" % (max(frames), self.max_frames))
        self._ensure_state(logits_chunk.device)
        self._first = False
        self._frames = frames
        out = self._launch(logits_chunk, chunk_len, self._raise_flags(self.reset_flags, mask), fetch)
        if not fetch:
            return None
        tokens, out_len, _, _, stable_len = out
        tok0, len0, st = tokens[:, 0].cpu(), out_len[:, 0].cpu().tolist(), stable_len.cpu().tolist()
        tk = self.dec.tokenizer
        recs = []
        for b in range(B):
            rec = {"partial_ids": tok0[b, :len0[b]].tolist(), "stable_ids": tok0[b, :st[b]].tolist()}
            if tk is not None:
                rec["partial"], rec["stable"] = tk.decode(rec["partial_ids"]), tk.decode(rec["stable_ids"])
            recs.append(rec)
        return recs

    def finish(self):
        """What decoder.beam_search returns for the frames pushed: per slot the winning token list (rescored by the neural LM when one is loaded)."""
        if self.state is None:
            raise RuntimeError("finish: nothing was pushed")
        st = self.state
        if not self._emitted:                            # one launch that consumes no frame and emits
            self._launch(torch.zeros(self.B, 1, self._V, device=st.state.device), torch.zeros(self.B, dtype=torch.int64, device=st.state.device), None, True)
        if self.dec.neural_rescorer is not None:
            return self.dec._rescore(st.tokens, st.out_len, st.score, self.B, 1)
        tok0, len0 = st.tokens[:, 0].cpu(), st.out_len[:, 0].cpu().tolist()
        return [tok0[b, :len0[b]].tolist() for b in range(self.B)]


class CTCBeamRingStreamSession(_StreamSession):
    """CTCBeamSearchDecoder.stream(window=N): the window-limited beam search of avec_amd/csrc/ctc_beam.hip (avec_ctc_beam_stream_ring), a stream without a frame
    limit.  The device keeps `window` backpointer rows per slot; whenever a slot holds `window` frames, the older window // 2 of them are committed: the best beam's
    tokens on them become final, go to the device's commit log with the frame that emitted each, and the beams that descend from another hypothesis on those frames are
    dropped.  The commit depends on the frame count alone, so the results do not depend on how the stream is cut into pushes, and up to frame `window` the search is
    the offline one.  What is committed never changes; the final best hypothesis can differ from an unlimited search's when the two disagree on committed frames.
    Host memory: one int per committed token and one per emission frame, per slot, until the slot is reset.
    The commit log holds log_frames entries per slot (default max(4 * window, 256); more than `window` are needed).  Between two reads a slot logs at most the frames
    pushed in between plus `window` tokens, so the session counts, on the host, the frames every slot was pushed since its log was last read, and reads the logs (one
    synchronisation and one device-to-host copy) before any push after which that count plus `window` would pass log_frames, with fetch=False too; a chunk longer than
    log_frames - window frames is consumed in pieces for the same reason.  A fetching push reads the logs anyway.  Not capturable."""

    def __init__(self, decoder, batch_size, window, log_frames=None):
        super().__init__(batch_size)
        self.dec, self.window = decoder, int(window)
        self.log_frames = max(4 * self.window, 256) if log_frames is None else int(log_frames)
        if self.B < 1 or self.window < 2:
            raise ValueError("stream: batch_size %d, window %d (>= 2)" % (self.B, self.window))
        if self.log_frames <= self.window:
            raise ValueError("stream: log_frames %d for window %d: the commit log must hold more than a window" % (self.log_frames, self.window))
        self._since = [0] * self.B                       # per slot, an upper bound of the frames pushed since its log was read (Tc per push): no sync to know it
        self._ids = [[] for _ in range(self.B)]          # committed since the slot's reset
        self._frames = [[] for _ in range(self.B)]
        self._reported = [0] * self.B                    # how many of them a fetch has returned
        self._emitted = False

    def _allocate(self, dev):
        self.state = ops.CTCBeamRingState(self.B, self.dec.beam_size, self.window, self.log_frames, dev)
        self.reset_flags = self.state.reset_flags

    def _launch(self, chunk, chunk_len, reset, emit):
        d = self.dec
        out = ops.ctc_beam_stream_ring(self.state, chunk, chunk_len, reset, d.ngram_tmp, d.lm(chunk.shape[-1]), d.ngram_alpha, d.ngram_beta, emit=emit)
        self._emitted = emit
        return out

    def _drain(self, extra=()):
        """read every slot's new log entries, with `extra` int32 device tensors in the same copy -> the host lists of `extra`"""
        st = self.state
        parts = [st.header()[:, 5].contiguous(), st.log] + list(extra)
        host = torch.cat([p.reshape(-1) for p in parts]).cpu()           # the one synchronisation
        cc, log = host[:self.B].tolist(), host[self.B:self.B + st.log.numel()].view(self.B, self.log_frames, 2).tolist()
        for b in range(self.B):
            for k in range(len(self._ids[b]), cc[b]):
                tok, frame = log[b][k % self.log_frames]
                self._ids[b].append(tok)
                self._frames[b].append(frame)
        self._since = [0] * self.B
        out, at = [], self.B + st.log.numel()
        for p in extra:
            out.append(host[at:at + p.numel()].view(p.shape).tolist())
            at += p.numel()
        return out

    def push(self, logits_chunk, chunk_len=None, reset=None, fetch=True):
        """Consume logits_chunk [B, Tc, V]; slot b takes chunk_len[b] frames of it (int64 tensor; default: all Tc).  reset: slots to restart from the empty
        transcript before this chunk (list of indices or host bool mask [B]); what such a slot had committed and no fetch had returned is dropped with it.  No push is
        refused for its length.  fetch=True returns one record per slot:
            committed_ids, committed_frames   everything committed since the slot's reset with the frame that emitted each token: final, it never changes
            n_new                             how many of them are new since the last fetch
            partial_ids, partial_frames       committed ++ the best beam's tail: the best hypothesis so far
            stable_ids                        its leading tokens that every live beam shares (at least the committed ones)
            dropped                           beams dropped by commits since the slot's reset
        and with a tokenizer "committed", "partial" and "stable", the text of the three id lists (final token by token, not character by character).
        fetch=False skips the traceback and copies nothing, except that the commit log is read first (one synchronisation) when the frames pushed to some slot since
        the last read, plus this chunk, plus `window` would pass log_frames."""
        B, Tc, self._V = logits_chunk.shape
        if B != self.B:
            raise ValueError("push: chunk of %d utterances for a session of %d" % (B, self.B))
        mask = self._reset_mask(reset)
        self._ensure_state(logits_chunk.device)
        piece = self.log_frames - self.window
        for off in range(0, Tc, piece):
            n = min(piece, Tc - off)
            if not self._first and max(self._since) + n + self.window > self.log_frames:
                self._drain()
            if off == 0 and mask is not None:
                for b in range(B):
                    if mask[b]:
                        self._ids[b], self._frames[b], self._reported[b], self._since[b] = [], [], 0, 0
            self._first = False
            self._since = [s + n for s in self._since]
            whole = off == 0 and n == Tc
            part = logits_chunk if whole else logits_chunk[:, off:off + n]
            part_len = chunk_len if whole or chunk_len is None else (chunk_len.to(torch.int64) - off).clamp(0, n)
            self._launch(part, part_len, self._raise_flags(self.reset_flags, mask) if off == 0 else None, fetch and off + n == Tc)
        if not fetch:
            return None
        st = self.state
        tok0, frm0, len0, stable, info = self._drain((st.tokens[:, 0], st.frames[:, 0], st.out_len[:, 0], st.stable_len, st.info))
        tk = self.dec.tokenizer
        recs = []
        for b in range(B):
            ids, frames = list(self._ids[b]), list(self._frames[b])
            rec = {"committed_ids": ids, "committed_frames": frames, "n_new": len(ids) - self._reported[b],
                   "partial_ids": ids + tok0[b][:len0[b]], "partial_frames": frames + frm0[b][:len0[b]], "dropped": info[b][2]}
            rec["stable_ids"] = rec["partial_ids"][:stable[b]]
            self._reported[b] = len(ids)
            if tk is not None:
                rec["committed"], rec["partial"], rec["stable"] = tk.decode(ids), tk.decode(rec["partial_ids"]), tk.decode(rec["stable_ids"])
            recs.append(rec)
        return recs

    def hypotheses(self):
        """after an emitting push: (tokens [B, W, L] int32 and out_len [B, W] int32 on the host: committed ++ tail of every beam, zero past out_len; score [B, W] on
        the device) -- the layout decoder._rescore takes"""
        st = self.state
        tails, lens = self._drain((st.tokens, st.out_len))
        alive = (st.score > float("-inf")).cpu().tolist()
        W = st.W
        hyps = [[(self._ids[b] + tails[b][w][:lens[b][w]]) if alive[b][w] else [] for w in range(W)] for b in range(self.B)]
        L = max(1, max(len(h) for hb in hyps for h in hb))
        tokens, out_len = torch.zeros(self.B, W, L, dtype=torch.int32), torch.zeros(self.B, W, dtype=torch.int32)
        for b in range(self.B):
            for w in range(W):
                out_len[b, w] = len(hyps[b][w])
                tokens[b, w, :len(hyps[b][w])] = torch.tensor(hyps[b][w], dtype=torch.int32)
        return tokens, out_len, st.score

    def finish(self):
        """Per slot the winning token list: committed ++ tail of every beam goes through the decoder's neural rescoring when a neural LM is loaded (the committed part
        is shared, so only the tails compete); otherwise committed ++ the best beam's tail."""
        if self.state is None:
            raise RuntimeError("finish: nothing was pushed")
        dev = self.state.state.device
        if not self._emitted:                            # one launch that consumes no frame and emits
            self._launch(torch.zeros(self.B, 1, self._V, device=dev), torch.zeros(self.B, dtype=torch.int64, device=dev), None, True)
        tokens, out_len, score = self.hypotheses()
        if self.dec.neural_rescorer is not None:
            return self.dec._rescore(tokens, out_len, score, self.B, 1)
        return [tokens[b, 0, :int(out_len[b, 0])].tolist() for b in range(self.B)]
