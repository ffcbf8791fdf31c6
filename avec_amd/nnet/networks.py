"""Encoders (nnet/networks.py): ResNet-18 visual front-end, ConformerInterCTC stack, audio / visual / audio-visual encoders."""
import os

import torch
import torch.nn as nn

from .. import ops
from .. import runtime as rt
from . import attentions, blocks, layers, modules, normalizations, preprocessing, transforms
from .captured import CapturedStep


class ResNet(nn.Module):
    """nnet/networks.py:32-146.  Hot path = ResNet18 without stem; forward_nhwc consumes the stem's channels-last frames."""

    def __init__(self, dim_input=3, dim_output=1000, model="ResNet50", include_stem=True, include_head=True):
        super().__init__()
        assert model in ("ResNet18", "ResNet34") and not include_stem, "hot path: basic-block ResNet fed by the Conv3d stem (nnet/networks.py:472)"
        dim_stem, dim_blocks = 64, [64, 128, 256, 512]
        num_blocks = [2, 2, 2, 2] if model == "ResNet18" else [3, 4, 6, 3]
        self.stem = nn.Identity()
        self.blocks = nn.ModuleList()
        for stage in range(4):
            for b in range(num_blocks[stage]):
                first = b == 0
                cin = (dim_stem if stage == 0 else dim_blocks[stage - 1]) if first else dim_blocks[stage]
                stride = (2, 2) if (first and stage > 0) else (1, 1)
                self.blocks.append(blocks.ResNetBlock(in_features=cin, out_features=dim_blocks[stage], kernel_size=(3, 3), stride=stride,
                                                      act_fun="ReLU", joined_post_act=True))
        self.head = nn.Sequential(layers.GlobalAvgPool2d(),
                                  layers.Linear(dim_blocks[-1], dim_output, weight_init="he_normal", bias_init="zeros")) if include_head else nn.Identity()

    def forward_nhwc(self, x):
        for i, blk in enumerate(self.blocks):
            x = blk.forward_nhwc(x, chain=i + 1 < len(self.blocks))       # every block but the last hands its output to the next block only
        if isinstance(self.head, nn.Identity):
            return x
        x = ops.AvgPoolFn.apply(x)
        lin = self.head[1]
        return ops.linear(x, lin.weight, lin.bias)

    def forward(self, x):
        return self.forward_nhwc(x.permute(0, 2, 3, 1).to(rt.act_dtype()).contiguous())


class Transformer(nn.Module):
    """nnet/networks.py:148-200: positional embedding -> (dropout) -> pre-norm TransformerBlocks -> final nn.LayerNorm (torch default eps 1e-5, unlike the 1e-6 of
    the modules' own norms).  Inference only, causal: `mask` must be attentions.Mask(right_context=0) with no left limit -- it is never materialised, the attention
    kernel computes causality from the indices."""

    def __init__(self, dim_model, num_blocks, att_params={"class": "MultiHeadAttention", "params": {"num_heads": 4, "weight_init": "normal_02", "bias_init": "zeros"}},
                 ff_ratio=4, emb_drop_rate=0.1, drop_rate=0.1, act_fun="GELU", pos_embedding=None, mask=None, inner_dropout=False, weight_init="normal_02",
                 bias_init="zeros", post_norm=False):
        super().__init__()
        assert not post_norm, "post-norm Transformers are not on this path"
        if not (isinstance(mask, attentions.Mask) and mask.right_context == 0 and mask.left_context is None and not mask.mask_start):
            raise NotImplementedError("networks.Transformer on the HIP path is the causal LM stack: mask=attentions.Mask(right_context=0)")
        self.pos_embedding = pos_embedding
        self.dropout = nn.Dropout(p=emb_drop_rate)
        self.mask = mask
        self.blocks = nn.ModuleList([blocks.TransformerBlock(dim_model=dim_model, ff_ratio=ff_ratio, att_params=att_params, drop_rate=drop_rate, inner_dropout=inner_dropout,
                                                             act_fun=act_fun, weight_init=weight_init, bias_init=bias_init, post_norm=post_norm) for _ in range(num_blocks)])
        self.layernorm = nn.LayerNorm(normalized_shape=dim_model)

    def forward_rows(self, x, lengths=None, embedded=False):
        """x (B, T, D) fp32 -> final-LayerNorm rows [B * T, D] in the compute dtype (what the head consumes).  embedded: the positions are already in x."""
        if self.training:
            raise RuntimeError("networks.Transformer is an inference path: call .eval() first (training the LM is out of scope)")
        ops._inference_only("networks.Transformer", x)
        if self.pos_embedding is not None and not embedded:
            x = self.pos_embedding(x)
        B, T, D = x.shape
        mask = attentions.CausalMask(lengths)
        for block in self.blocks:
            x = block(x, mask=mask)
        ln = self.layernorm
        return ops.layernorm_fwd(x.reshape(B * T, D), ln.weight, ln.bias, B * T, D, False, ln.eps)[0]

    def forward(self, x, lengths=None):
        B, T, D = x.shape
        return self.forward_rows(x, lengths).float().view(B, T, D)


class ConformerInterCTC(nn.Module):
    """nnet/networks.py:202-307"""

    def __init__(self, dim_model, num_blocks, interctc_blocks, vocab_size, loss_prefix="ctc", att_params={"class": "MultiHeadAttention", "num_heads": 4},
                 conv_params={"class": "Conv1d", "params": {"padding": "same", "kernel_size": 31}}, ff_ratio=4, drop_rate=0.1, pos_embedding=None,
                 mask=None, conv_stride=1, batch_norm=True):
        super().__init__()
        assert pos_embedding is None
        self.interctc_blocks, self.loss_prefix = interctc_blocks, loss_prefix
        dim_model = [dim_model] if isinstance(dim_model, int) else dim_model
        num_blocks = [num_blocks] if isinstance(num_blocks, int) else num_blocks
        self.pos_embedding = None
        self.dropout = layers.Dropout(p=drop_rate)
        self.mask = mask
        self.conformer_blocks = nn.ModuleList()
        self.interctc_modules = nn.ModuleList()
        i = 1
        for stage, nb in enumerate(num_blocks):
            for b in range(nb):
                down = (b == nb - 1) and (stage < len(num_blocks) - 1)       # last block of every stage but the last: stride + widen
                d_out = dim_model[stage + 1] if down else dim_model[stage]
                stride = (conv_stride[stage] if isinstance(conv_stride, list) else conv_stride) if down else 1
                self.conformer_blocks.append(blocks.ConformerBlock(
                    dim_model=dim_model[stage], dim_expand=d_out, ff_ratio=ff_ratio, drop_rate=drop_rate,
                    att_params=att_params[stage] if isinstance(att_params, list) else att_params, conv_stride=stride,
                    conv_params=conv_params[stage] if isinstance(conv_params, list) else conv_params, batch_norm=batch_norm))
                if i in interctc_blocks:
                    self.interctc_modules.append(modules.InterCTCResModule(dim_model=d_out, vocab_size=vocab_size))
                i += 1

        # the LayerNorm that closes block i is read next by the first pre-norm of block i + 1 (unless an InterCTC module sits between them): one launch for both
        # (ops.LN_PAIR); a plain attribute, not a registered submodule (the state_dict is the reference's)
        for i in range(len(self.conformer_blocks) - 1):
            b0, b1 = self.conformer_blocks[i], self.conformer_blocks[i + 1]
            if (i + 1) not in interctc_blocks and isinstance(b0.norm, nn.LayerNorm) and b0.norm.normalized_shape == b1.ff_module1.layers[0].normalized_shape:
                object.__setattr__(b0, "_next_ln", b1.ff_module1.layers[0])
        # the position projections of the consecutive blocks of a stage share their input (the sinusoid table of the stage's sequence length): one [L D][D] weight in the
        # arena -> one launch per stage and pass instead of one per block (ops._pos_group_entry); state_dict names are unchanged
        i0 = 0
        for nb in num_blocks:
            atts = [getattr(b.self_att_module, "attention", None) for b in self.conformer_blocks[i0:i0 + nb]]
            i0 += nb
            pos = [a.pos_layer for a in atts if a is not None and type(a).__name__ in ("RelPos1dMultiHeadAttention", "RelPosPatch1dMultiHeadAttention") and hasattr(a, "pos_layer")]
            if len(pos) == len(atts) and len(pos) >= 2 and all(p.bias is not None and p.weight.shape == pos[0].weight.shape for p in pos):
                rt.fuse_linears(self, [p.weight for p in pos], [p.bias for p in pos])
        if any(getattr(m, "causal", False) for m in self.modules()):
            # causal relative positions (nnet/attentions.py:234-256): for j <= i the reference reads E[i-j], as the full-context layout does; for j > i its
            # rel_to_abs wraps around into the next query row.  Only a mask that hides every j > i makes that well defined -- required here, not reproduced.
            ok = mask is not None and getattr(mask, "right_context", None) is not None and mask.right_context <= 0 and getattr(mask, "mask_start", 0) <= 1
            assert ok, "causal=True attention needs a causal Mask (right_context <= 0, mask_start <= 1)"

    def forward(self, x, lengths):
        x = self.dropout(x)
        if self.mask is not None and getattr(self.mask, "has_context", False):
            mask = self.mask(x, lengths)              # streaming: dense (B or 1,1,T,T) band mask, strided with the blocks (nnet/networks.py:271-298)
        else:
            mask = modules.LengthMask(lengths) if (self.mask is not None and lengths is not None) else None
        inter, j = {}, 0
        for i, block in enumerate(self.conformer_blocks):
            x = block(x, mask=mask)
            logits = None
            if i + 1 in self.interctc_blocks:
                x, logits = self.interctc_modules[j](x)
                j += 1
            if block.stride > 1:
                same = isinstance(mask, modules.LengthMask) and mask.lengths is lengths      # the length mask carries the very vector that is strided below: computed once
                if lengths is not None:
                    lengths = ops.len_affine(lengths, 1, block.stride, 1)
                if mask is not None:
                    if isinstance(mask, modules.LengthMask):
                        mask = modules.LengthMask(lengths) if same else mask.strided(block.stride)
                    else:
                        mask = mask[:, :, ::block.stride, ::block.stride]
            if logits is not None:
                inter[self.loss_prefix + "_" + str(i)] = [logits, lengths]
        return x, lengths, inter

    def stream(self, batch_size, chunk_frames):
        """A ConformerStreamSession over this (causal, eval-mode) stack: the encoder-side counterpart of CTCBeamSearchDecoder.stream()."""
        return ConformerStreamSession(self, batch_size, chunk_frames)


class ConformerStreamSession:
    """ConformerInterCTC.stream(): a causal stack run chunk by chunk.  After any sequence of push calls the rows a slot has produced equal the rows that
    stack(x, lengths) produces offline (eval mode, the same Mask) on the frames pushed so far for that slot, up to floating-point summation order, for every split
    into chunks.  Everything row-wise (LayerNorm, the feed-forward and pointwise products, the InterCTC modules, the strided k=1 residual) runs through the offline
    eval-path launchers; the depthwise convolution's left context and the attention's keys / values are carried by ops.glu_dwconv_stream / relpos_attention_stream in
    buffers this object owns (nothing is added to the module tree or the state_dict).  Per slot a frame counter lives on the device; a restart only sets a flag that
    the kernels read: whatever the buffers hold from before the restart is older than the counter and counts as absent."""

    def __init__(self, stack, batch_size, chunk_frames):
        self.stack, self.B, self.Tc = stack, int(batch_size), int(chunk_frames)
        self.plan = self._check(stack)
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
        self.state = None                  # per block: E table, key / value rings, conv context, BatchNorm scale | shift -- allocated by the first push (it knows the device)
        self._short = [False] * self.B     # host mirror of "this slot's last chunk was short" (the contract check of host-list chunk lengths: no sync)
        self._first = True
        self._graph = self._static = None

    @staticmethod
    def _check(stack):
        """-> per block {div, stride, L, K}; raises before anything is launched"""
        if stack.training:
            raise RuntimeError("stream: the stack is in training mode (BatchNorm batch statistics and dropout are not functions of the past): call .eval() first")
        m = stack.mask
        if not isinstance(m, attentions.Mask):
            raise NotImplementedError("stream: the stack needs a streaming Mask(left_context=L, right_context=0), got mask=%r" % (m,))
        if m.left_context is None:
            raise NotImplementedError("stream: left_context=None would need an unbounded key/value cache; give the Mask an integer left_context")
        if not isinstance(m.left_context, int) or m.left_context < 0:
            raise NotImplementedError("stream: left_context=%r must be an integer >= 0" % (m.left_context,))
        if m.right_context != 0:
            raise NotImplementedError("stream: right_context=%r needs look-ahead buffering (only right_context=0 is streamed)" % (m.right_context,))
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
            plan.append({"div": div, "stride": blk.stride, "L": m.left_context // div, "K": dw.kernel_size[0]})
            div *= blk.stride
        return plan

    # ---- device state ----------------------------------------------------------------------------------------------------------------------------------------------
    def _allocate(self, dev):
        B, adt = self.B, rt.act_dtype()
        self.pos = torch.zeros(B, dtype=torch.int64, device=dev)
        self.reset_flags = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.clen = torch.full((B,), self.Tc, dtype=torch.int64, device=dev)
        self._clen_full = True
        self.state = []
        for p, blk in zip(self.plan, self.stack.conformer_blocks):
            att, dw, bn = blk.self_att_module.attention, blk.conv_module.layers[3], blk.conv_module.layers[4]
            D, H, L, Tq = att.dim_model, att.num_heads, p["L"], self.Tc // p["div"]
            C = dw.weight.shape[0]
            # E[delta] = pos_layer(PE(delta)), delta = 0 .. L: the offline table's row (T - 1) - delta (ops.rel_pos_table: position p = delta), the same for every T
            pos = torch.arange(0, L + 1, dtype=torch.float32).unsqueeze(1)
            inv = 10000 ** (2 * torch.arange(0, D // 2, dtype=torch.float32).unsqueeze(0) / D)
            pe = torch.zeros(L + 1, D)
            pe[:, 0::2], pe[:, 1::2] = (pos / inv).sin(), (pos / inv).cos()
            pe = pe.to(device=dev, dtype=adt).contiguous()
            e = ops.linear_fwd(pe, att.pos_layer.weight, att.pos_layer.bias, L + 1, in_f32=False, out_f32=False)
            kc, vc = ops.relpos_attention_stream_state(B, H, D // H, L, Tq, dev)
            st = ops.BNState(C, pe)
            ops.bn_finalize(bn, st, 1, False)              # eval mode: scale | shift from the running statistics
            self.state.append({"e": e, "kc": kc, "vc": vc, "ss": st.ss, "ctx": ops.glu_dwconv_stream_state(B, C, p["K"], dev)})

    # ---- one push, eager: a fixed sequence of launches on the current stream ------------------------------------------------------------------------------------
    def _attention(self, p, st, blk, x):
        mod = blk.self_att_module
        att, ln = mod.attention, mod.norm
        B, Tq, D = x.shape
        M, adt = B * Tq, rt.act_dtype()
        x2 = ops._f32c(x.reshape(M, D))
        h, _, _ = ops.layernorm_fwd(x2, ln.weight, ln.bias, M, D, False, ln.eps)
        qkv = ops.empty((M, 3 * D), adt, x2)
        ws = (att.query_layer.weight, att.key_layer.weight, att.value_layer.weight)
        bs = (att.query_layer.bias, att.key_layer.bias, att.value_layer.bias)
        grp = rt.fused_group(ws[0])
        if grp is not None and grp.weights[1] is ws[1] and grp.weights[2] is ws[2] and bs[0] is not None:
            ops.gemm_nt(h, grp.fwd, qkv, M, 3 * D, D, bias=grp.bias)
        else:
            for i in range(3):
                ops.gemm_nt(h, rt.shadow(ws[i]).fwd, qkv[:, i * D:], M, D, D, bias=bs[i], ldo=3 * D)
        o = ops.relpos_attention_stream(qkv, st["e"], st["kc"], st["vc"], self.pos, self.reset_flags, self.clen, p["div"], B=B, H=att.num_heads, L=p["L"])
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
        a = ops.glu_dwconv_stream(u.view(B, Tq, 2 * Dp), dw.weight, dw.bias, st["ss"], st["ctx"], self.pos, self.reset_flags, self.clen, p["div"], s)
        if res_conv is not None:
            rs = res_conv.stride[0]
            R = ops.linear_fwd(x2, res_conv.weight, res_conv.bias, Mo, in_f32=(adt != torch.float32), out_f32=True, rows=ops.rows_plain(D, To, Tq, rs) if rs > 1 else None)
        else:
            R = x2
        return ops.linear_fwd(a.view(Mo, Dp), pw2.weight, pw2.bias, Mo, in_f32=False, out_f32=True, res=R, alpha=1.0).view(B, To, Dp)

    def _run(self, x):
        stack = self.stack
        lengths, inter, j = self.clen, {}, 0
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
        if lengths is self.clen:
            lengths = lengths.clone()
        ops.stream_advance(self.pos, self.reset_flags, self.clen, self.Tc)
        return x, lengths, inter

    # ---- host side of a push -----------------------------------------------------------------------------------------------------------------------------------------
    def _controls(self, chunk_len, reset):
        B = self.B
        if self._first:
            mask = [True] * B
        elif reset is None:
            mask = None
        else:
            r = reset.cpu().tolist() if torch.is_tensor(reset) else list(reset)
            if len(r) == B and all(isinstance(v, bool) for v in r):
                mask = r
            else:
                mask = [False] * B
                for k in r:
                    mask[int(k)] = True
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
        if mask is not None and any(mask):
            self.reset_flags.copy_(torch.tensor(mask, dtype=torch.uint8), non_blocking=True)      # (the push's last launch clears them again: no memset after a restart)
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

    def push(self, x_chunk, chunk_len=None, reset=None):
        """x_chunk [B, Tc, D] (the stack's input features) -> (y [B, Tc / S, D_out] fp32, out_len [B] int64 on the device, inter: the offline forward's dict
        loss_prefix_i -> [logits chunk, lengths]).  Slot b takes the first chunk_len[b] frames (a Python list or an int64 device tensor [B]; default all Tc); fewer
        than Tc is legal only as the slot's last chunk before a reset -- until then the slot may only idle on chunks of 0 frames (checked on the host for a list; the
        caller's contract for a device tensor).  Rows at or past
        chunk_len are computed from whatever was passed and never reach the carried state.  reset: slots to restart before this chunk, a list of indices or a host
        bool mask [B]; the first push restarts every slot.  No host synchronisation after the first push; after capture() the results are static tensors that the
        next push overwrites."""
        if x_chunk.dim() != 3 or x_chunk.shape[0] != self.B or x_chunk.shape[1] != self.Tc:
            raise ValueError("push: chunk %s for a session of %d slots x %d frames" % (tuple(x_chunk.shape), self.B, self.Tc))
        rt.require_gpu(x_chunk)
        if self.stack.training:
            raise RuntimeError("push: the stack went back to training mode; call .eval()")
        mask, host_len = self._controls(chunk_len, reset)
        with torch.no_grad():
            if self.state is None:
                self._allocate(x_chunk.device)
            self._upload(mask, host_len, chunk_len)
            self._first = False
            if self._graph is not None:
                self._static[0].copy_(x_chunk, non_blocking=True)
                self._graph.replay()
                return self._static[1]
            return self._run(x_chunk)

    def capture(self, device=None):
        """Capture one push as a graph on static input / chunk_len / reset buffers; push then copies into them and replays (the device counters make every replay
        advance).  Call it on a fresh session, before the first push; the warm-up pushes it runs are forgotten (the next push restarts every slot)."""
        if self._graph is not None:
            return self
        if not self._first:
            raise RuntimeError("capture: call it before the first push of the session")
        dev = torch.device(device) if device is not None else next(self.stack.parameters()).device
        rt.require_gpu(next(self.stack.parameters()))
        with torch.no_grad():
            if self.state is None:
                with torch.cuda.device(dev):
                    self._allocate(dev)
            D0 = self.stack.conformer_blocks[0].ff_module1.layers[0].normalized_shape[0]
            x = torch.zeros(self.B, self.Tc, D0, dtype=torch.float32, device=dev)
            self._upload([True] * self.B, None, None)
            cap = CapturedStep()
            with torch.cuda.device(dev):
                cap.warm_up(lambda: self._run(x), 2)        # weight shadows, lazy kernel attributes, allocator
                cap.capture(lambda: self._run(x))
        self._graph, self._static = cap.graph, (x, cap.outputs)
        self._first = True
        self._short = [False] * self.B
        return self


def _relpos(num_heads, attn_drop_rate, max_pos, **extra):
    cls = "RelPosPatch1dMultiHeadAttention" if "patch_size" in extra else "RelPos1dMultiHeadAttention"
    return {"class": cls, "params": dict(num_heads=num_heads, attn_drop_rate=attn_drop_rate, num_pos_embeddings=max_pos,
                                         weight_init="default", bias_init="default", **extra)}


class AudioEfficientConformerEncoder(nn.Module):
    """nnet/networks.py:309-440"""

    def __init__(self, include_head=True, vocab_size=256, att_type="patch", interctc_blocks=[3, 6, 10, 13], num_blocks=[5, 6, 5], loss_prefix="ctc"):
        super().__init__()
        assert att_type in ("regular", "grouped", "patch")
        filters, n_mels, dim_model, H = 180, 80, [180, 256, 360], 4
        self.audio_preprocessing = preprocessing.AudioPreprocessing(16000, 512, 25, 10, n_mels, False, -5.6501, 4.2280)
        self.spec_augment = preprocessing.SpecAugment(mF=2, F=27, mT=5, pS=0.05)
        self.unsqueeze = layers.Unsqueeze(dim=1)
        self.subsampling_module = modules.ConvNeuralNetwork(dim_input=1, dim_layers=filters, kernel_size=3, strides=2, norm="BatchNorm2d", act_fun="Swish",
                                                            drop_rate=0.0, dim=2)
        self.reshape = layers.Reshape(shape=(filters * n_mels // 2, -1), include_batch=False)
        self.transpose = layers.Transpose(1, 2)
        self.linear = layers.Linear(filters * n_mels // 2, dim_model[0])
        if att_type == "grouped":             # nnet/networks.py:389-392: Transformer-XL biases everywhere, 3-frame groups in the first stage
            grouped = lambda G: {"class": "GroupedRelPosMultiHeadSelfAttention", "params": {"num_heads": H, "group_size": G, "attn_drop_rate": 0.0, "max_pos_encoding": 10000, "causal": False}}
            att = [grouped(3), grouped(1), grouped(1)]
        else:
            att = [_relpos(H, 0.0, 10000, patch_size=3) if att_type == "patch" else _relpos(H, 0.0, 10000), _relpos(H, 0.0, 10000), _relpos(H, 0.0, 10000)]
        self.back_end = ConformerInterCTC(dim_model=dim_model, num_blocks=num_blocks, interctc_blocks=interctc_blocks, vocab_size=vocab_size,
                                          att_params=att,
                                          conv_params={"class": "Conv1d", "params": {"padding": "same", "kernel_size": 15}}, ff_ratio=4, drop_rate=0.1,
                                          pos_embedding=None, mask=attentions.Mask(), conv_stride=2, batch_norm=True, loss_prefix=loss_prefix)
        self.head = layers.Linear(dim_model[-1], vocab_size) if include_head else nn.Identity()

    def forward(self, x, lengths):
        mel, lengths = self.audio_preprocessing(x, lengths)
        mel = self.spec_augment(mel, lengths)
        stem = self.subsampling_module.layers[0]
        a = ops.AudioStemFn.apply(mel, stem[0].weight, stem[0], stem[1], stem[1].training and not stem[1].frozen)     # (B, T', 7200) act
        lengths = ops.len_affine(lengths, 1, 2, 1)
        x = ops.linear(a, self.linear.weight, self.linear.bias)
        x, lengths, inter = self.back_end(x, lengths)
        if not isinstance(self.head, nn.Identity):
            x = self.head(x)
        return x, lengths, inter

    def stream_front(self, batch_size, chunk_frames):
        """An AudioFrontStreamSession: waveform chunks -> the 180-wide features the back-end consumes, with the offline front-end's arithmetic."""
        return AudioFrontStreamSession(self, batch_size, chunk_frames)

    def stream(self, batch_size, chunk_frames):
        """An AudioStreamSession: waveform chunks -> logits, the front session + back_end.stream() + head (the back-end's refusals are ConformerInterCTC.stream()'s)."""
        return AudioStreamSession(self, batch_size, chunk_frames)


def _flag_mask(flags, B):
    """reset / last as passed to a push (None, a list of slot indices, or a host bool mask [B]) -> a bool list [B]"""
    if flags is None:
        return [False] * B
    r = flags.cpu().tolist() if torch.is_tensor(flags) else list(flags)
    if len(r) == B and all(isinstance(v, bool) for v in r):
        return r
    mask = [False] * B
    for k in r:
        mask[int(k)] = True
    return mask


class AudioFrontStreamSession:
    """AudioEfficientConformerEncoder.stream_front(): the audio front-end (log-mel -> Conv2d + BatchNorm2d + Swish stem -> Linear) run on waveform chunks.  The frames a
    slot has produced after any sequence of pushes equal the offline front-end's frames on the samples pushed so far (and, once the utterance has ended, on the whole
    utterance: both STFT reflections and both zero paddings of the stem included), up to the DFT GEMM's tile choice.  Mel frame f reads samples [160 f - 200, 160 f + 200),
    stem frame t reads mel frames 2t - 1, 2t, 2t + 1: with n samples heard E(n) = 0 if n < 360 else (n - 40) // 320 frames exist, Ta // 320 + 1 at the end.  Schedule:
    first_samples = 320 Tc + 40 in an utterance's first push, chunk_samples = 320 Tc in every later one; every push but the last then yields exactly Tc frames, the last at
    most Tc + 1.  The carried state is a sample tail of fewer than 720 samples per slot, a counter and an `ended` flag, on the device (ops.audio_stream_state); nothing
    is added to the module tree or the state_dict."""

    def __init__(self, enc, batch_size, chunk_frames):
        self.enc, self.B, self.Tc = enc, int(batch_size), int(chunk_frames)
        self._check(enc)
        if self.B < 1:
            raise ValueError("stream_front: batch_size %d" % self.B)
        if self.Tc < 2:
            raise ValueError("stream_front: chunk_frames = %d: a push of %d samples would be shorter than one %d-sample analysis window; at least 2 frames (80 ms) per push"
                             % (self.Tc, 2 * self.hop * self.Tc, self.win))
        self.first_samples, self.chunk_samples = 2 * self.hop * self.Tc + (self.win // 2 - self.hop), 2 * self.hop * self.Tc
        self.Tmax = self.Tc + 2                    # any count up to first_samples, at the end of an utterance too, gives at most Tc + 2 frames
        self.state = None
        self._n = [0] * self.B                     # host mirror of the device counters (None: unknown after a push with device-tensor counts)
        self._ended = [False] * self.B
        self._first = True
        self._ns_up = None                         # what self.nsamp holds
        self._graph = self._static = None

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

    def _allocate(self, dev):
        B = self.B
        bn = self.enc.subsampling_module.layers[0][1]
        self.state = ops.audio_stream_state(B, dev)
        self.nsamp = torch.zeros(B, dtype=torch.int64, device=dev)
        self.reset_flags = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.last_flags = torch.zeros(B, dtype=torch.uint8, device=dev)
        st = ops.BNState(bn.num_features, self.state)
        ops.bn_finalize(bn, st, 1, False)              # eval mode: scale | shift from the running statistics
        self.ss = st.ss

    def _run(self, wave):
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

    # ---- host side of a push -----------------------------------------------------------------------------------------------------------------------------------------
    def _controls(self, n_samples, last, reset):
        """-> (reset mask, last mask, host counts or None for a device tensor, frames per slot or None): checks a host-list push against the contract, changes nothing"""
        B = self.B
        rmask = [True] * B if self._first else _flag_mask(reset, B)
        lmask = _flag_mask(last, B)
        if torch.is_tensor(n_samples):
            return rmask, lmask, None, None
        if n_samples is not None and len(n_samples) != B:
            raise ValueError("push: n_samples %r for %d slots" % (list(n_samples), B))
        counts, frames = [], []
        for b in range(B):
            n0, ended = (0, False) if rmask[b] else (self._n[b], self._ended[b])
            if n0 is None:
                raise RuntimeError("push: slot %d was last pushed with device-tensor counts, which the host does not mirror: go on with a tensor, or reset the slot" % b)
            c = (0 if ended else (self.first_samples if n0 == 0 else self.chunk_samples)) if n_samples is None else int(n_samples[b])
            if c < 0 or c > self.first_samples:
                raise ValueError("push: n_samples[%d] = %d outside 0 .. %d" % (b, c, self.first_samples))
            if ended:
                if c > 0:
                    raise RuntimeError("push: slot %d has ended (last) and was not reset: it takes no samples until reset=[%d] starts the next utterance" % (b, b))
                frames.append(0)
            elif lmask[b]:
                if n0 + c <= self.n_fft // 2:
                    raise ValueError("push: slot %d ends after %d samples: an utterance of at most n_fft / 2 = %d samples cannot be reflect-padded (refused offline as well)"
                                     % (b, n0 + c, self.n_fft // 2))
                frames.append((n0 + c) // (2 * self.hop) + 1 - self._ready(n0))
            else:
                frames.append(self._ready(n0 + c) - self._ready(n0))
            counts.append(c)
        return rmask, lmask, counts, frames

    def _upload(self, rmask, lmask, counts, n_samples):
        B = self.B
        if any(rmask):
            self.reset_flags.copy_(torch.tensor(rmask, dtype=torch.uint8), non_blocking=True)        # (the push's last launch clears both flag vectors again)
        if any(lmask):
            self.last_flags.copy_(torch.tensor(lmask, dtype=torch.uint8), non_blocking=True)
        if counts is None:
            self.nsamp.copy_(n_samples.view(B), non_blocking=True)
            self._ns_up = None
            self._n, self._ended = [None] * B, [None] * B                 # a device tensor's contract is the caller's
            return
        if counts != self._ns_up:
            self.nsamp.copy_(torch.tensor(counts, dtype=torch.int64), non_blocking=True)
            self._ns_up = list(counts)
        for b in range(B):
            n0, ended = (0, False) if rmask[b] else (self._n[b], self._ended[b])
            self._n[b], self._ended[b] = n0 + counts[b], ended or lmask[b]

    def push(self, wave, n_samples=None, last=None, reset=None):
        """wave [B, first_samples] fp32 -> (feat [B, Tc + 2, 180] fp32, out_len [B] int64 on the device): slot b takes the first n_samples[b] samples (a Python list
        or an int64 device tensor [B]; default: the schedule's count, first_samples after a restart, chunk_samples later, 0 for an ended slot) and yields out_len[b]
        frames; rows at or past out_len carry no information.  last: slots whose utterance ends with these samples; reset: slots to restart before them (each a list
        of indices or a host bool mask [B]); the first push restarts every slot.  With host counts the contract is checked on the host, without a synchronisation:
        counts within 0 .. first_samples, an utterance longer than n_fft / 2 = 256 samples at `last`, no samples to an ended slot.  With a device tensor it is the
        caller's.  No host synchronisation after the first push; after capture() the results are static tensors that the next push overwrites."""
        if wave.dim() != 2 or wave.shape[0] != self.B or wave.shape[1] != self.first_samples:
            raise ValueError("push: wave %s for a session of %d slots x %d samples" % (tuple(wave.shape), self.B, self.first_samples))
        rt.require_gpu(wave)
        if self.enc.training:
            raise RuntimeError("push: the encoder went back to training mode; call .eval()")
        rmask, lmask, counts, _ = self._controls(n_samples, last, reset)
        with torch.no_grad():
            if self.state is None:
                self._allocate(wave.device)
            self._upload(rmask, lmask, counts, n_samples)
            self._first = False
            if self._graph is not None:
                self._static[0].copy_(wave, non_blocking=True)
                self._graph.replay()
                return self._static[1]
            return self._run(wave if (wave.dtype == torch.float32 and wave.stride(1) == 1) else wave.float().contiguous())

    def capture(self, device=None):
        """Capture one push as a graph on static wave / count / flag buffers, as ConformerStreamSession.capture(): call it on a fresh session; the device counters
        make every replay advance; the warm-up pushes are forgotten (the next push restarts every slot)."""
        if self._graph is not None:
            return self
        if not self._first:
            raise RuntimeError("capture: call it before the first push of the session")
        dev = torch.device(device) if device is not None else next(self.enc.parameters()).device
        rt.require_gpu(next(self.enc.parameters()))
        with torch.no_grad():
            with torch.cuda.device(dev):
                if self.state is None:
                    self._allocate(dev)
                x = torch.zeros(self.B, self.first_samples, dtype=torch.float32, device=dev)
                self._upload([True] * self.B, [False] * self.B, [self.first_samples] * self.B, None)
                cap = CapturedStep()
                cap.warm_up(lambda: self._run(x), 2)
                cap.capture(lambda: self._run(x))
        self._graph, self._static = cap.graph, (x, cap.outputs)
        self._first, self._n, self._ended = True, [0] * self.B, [False] * self.B
        return self


class AudioStreamSession:
    """AudioEfficientConformerEncoder.stream(): waveform chunks -> logits.  The front session feeds back_end.stream() (a ConformerStreamSession, with its refusals) and
    the head.  The front's schedule makes every push but an utterance's last yield exactly Tc frames, one chunk of the stack; a last push may yield Tc + 1: the stack
    is then pushed a second time with that one frame for the slots concerned and 0 frames (no change of state) for the others, and its first output row is appended."""

    def __init__(self, enc, batch_size, chunk_frames):
        self.enc = enc
        self.front = AudioFrontStreamSession(enc, batch_size, chunk_frames)
        self.back = enc.back_end.stream(batch_size, chunk_frames)
        self.B, self.Tc, self.S = self.front.B, self.front.Tc, self.back.S
        self.first_samples, self.chunk_samples = self.front.first_samples, self.front.chunk_samples
        self._x2 = None

    def _head(self, y):
        return y if isinstance(self.enc.head, nn.Identity) else self.enc.head(y)

    def push(self, wave, n_samples=None, last=None, reset=None):
        """wave [B, first_samples] fp32 -> (logits [B, R, V] fp32, out_len [B] int64 on the device, inter: loss_prefix_i -> [logits chunk, lengths] as offline).
        n_samples / last / reset: host lists as AudioFrontStreamSession.push; counts must follow the schedule (every push of a slot but its last yields exactly
        chunk_frames frames; a slot may idle on 0 samples).  R = Tc / S, or Tc / S + 1 in a push where some slot's last chunk produced Tc + 1 frames."""
        if torch.is_tensor(n_samples):
            raise TypeError("push: the combined session takes host lists for n_samples (it decides on the host whether the stack needs a second push)")
        B, Tc = self.B, self.Tc
        rmask, lmask, counts, frames = self.front._controls(n_samples, last, reset)
        for b in range(B):
            if not (frames[b] == Tc or counts[b] == 0 or (lmask[b] and frames[b] <= Tc + 1)):
                raise ValueError("push: slot %d would yield %d frames from %d samples: off the schedule (first_samples = %d in an utterance's first push, chunk_samples = %d "
                                 "later, fewer only with last)" % (b, frames[b], counts[b], self.first_samples, self.chunk_samples))
        with torch.no_grad():
            feat, _ = self.front.push(wave, counts, lmask, rmask)
            tail = [f > Tc for f in frames]
            y, ylen, inter = self.back.push(feat[:, :Tc], torch.tensor([min(f, Tc) for f in frames], dtype=torch.int64), rmask)
            if not any(tail):
                return self._head(y), ylen, inter
            # (a captured stack's results are static: keep this push's before the second one refills them)
            logits, ylen, inter = self._head(y).clone(), ylen.clone(), {k: [v[0].clone(), v[1].clone()] for k, v in inter.items()}
            if self._x2 is None:
                self._x2 = torch.zeros(B, Tc, feat.shape[2], dtype=feat.dtype, device=feat.device)
            self._x2[:, 0].copy_(feat[:, Tc])
            y2, ylen2, inter2 = self.back.push(self._x2, torch.tensor([1 if t else 0 for t in tail], dtype=torch.int64), None)
            for k, v in inter.items():
                inter[k] = [torch.cat([v[0], inter2[k][0][:, :1]], dim=1), v[1] + inter2[k][1]]
            return torch.cat([logits, self._head(y2[:, :1].contiguous())], dim=1), ylen + ylen2, inter

    def capture(self, device=None):
        """capture both halves (AudioFrontStreamSession.capture, ConformerStreamSession.capture); call it before the first push"""
        self.front.capture(device)
        self.back.capture(device)
        return self


class VisualEfficientConformerEncoder(nn.Module):
    """nnet/networks.py:442-512"""

    def __init__(self, include_head=True, vocab_size=256, interctc_blocks=[3, 6, 9], num_blocks=[6, 6], loss_prefix="ctc"):
        super().__init__()
        dim_model, H = [256, 360], 4
        self.front_end = nn.Sequential(
            modules.ConvNeuralNetwork(dim_input=1, dim_layers=64, kernel_size=(5, 7, 7), strides=(1, 2, 2), norm="BatchNorm3d", act_fun="ReLU", drop_rate=0.0, dim=3),
            layers.MaxPool3d(kernel_size=(1, 3, 3), stride=(1, 2, 2), padding="same"),
            transforms.VideoToImages(),
            ResNet(include_stem=False, dim_output=dim_model[0], model="ResNet18"))
        self.expand_time = transforms.ImagesToVideos()
        self.back_end = ConformerInterCTC(dim_model=dim_model, num_blocks=num_blocks, interctc_blocks=interctc_blocks, vocab_size=vocab_size,
                                          att_params=_relpos(H, 0.0, 10000), conv_params={"class": "Conv1d", "params": {"padding": "same", "kernel_size": 15}},
                                          ff_ratio=4, drop_rate=0.1, pos_embedding=None, mask=attentions.Mask(), conv_stride=2, batch_norm=True,
                                          loss_prefix=loss_prefix)
        self.head = layers.Linear(dim_model[-1], vocab_size) if include_head else nn.Identity()

    def forward_front(self, x):
        """x: (B, 1, T, H, W) -> per-frame features (B, T, 256) fp32: Conv3d stem + max-pool + ResNet-18 (nnet/networks.py:497-504)"""
        B, C, T, H, W = x.shape
        assert C == 1
        stem = self.front_end[0].layers[0]
        bn = stem[1]
        frames = ops.VideoStemFn.apply(x.reshape(B, T, H, W), stem[0].weight, stem[0], bn, bn.training and not bn.frozen)     # (B*T, H/4, W/4, 64) act, channels-last
        frames = ops.mark(frames, "v_stem")
        feats = self.front_end[3].forward_nhwc(frames)                                                          # (B*T, 256) fp32
        return feats.view(B, T, -1)

    def forward_back(self, x, lengths):
        x, lengths, inter = self.back_end(x, lengths)
        if not isinstance(self.head, nn.Identity):
            x = self.head(x)
        return x, lengths, inter

    def forward(self, x, lengths):
        """x: (B, 1, T, H, W)"""
        return self.forward_back(self.forward_front(x), lengths)


def audio_first_env():
    return os.environ.get("AVEC_AUDIO_FIRST", "0") == "1"


class AudioVisualEfficientConformerEncoder(nn.Module):
    """nnet/networks.py:514-579"""

    def __init__(self, include_head=True, vocab_size=256, v_interctc_blocks=[3, 6], a_interctc_blocks=[8, 11], f_interctc_blocks=[2]):
        super().__init__()
        dim_model = 360
        self.video_encoder = VisualEfficientConformerEncoder(include_head=False, vocab_size=vocab_size, interctc_blocks=v_interctc_blocks,
                                                             num_blocks=[6, 1], loss_prefix="v_ctc")
        self.audio_encoder = AudioEfficientConformerEncoder(include_head=False, vocab_size=vocab_size, interctc_blocks=a_interctc_blocks,
                                                            num_blocks=[5, 6, 1], loss_prefix="a_ctc")
        self.fusion_module = modules.FusionModule(a_dim_model=dim_model, v_dim_model=dim_model, f_dim_model=dim_model)
        self.audio_visual_encoder = ConformerInterCTC(dim_model=dim_model, num_blocks=5, interctc_blocks=f_interctc_blocks, vocab_size=vocab_size,
                                                      att_params=_relpos(4, 0.0, 10000),
                                                      conv_params={"class": "Conv1d", "params": {"padding": "same", "kernel_size": 15}}, ff_ratio=4,
                                                      drop_rate=0.1, pos_embedding=None, mask=attentions.Mask(), conv_stride=2, batch_norm=True, loss_prefix="f_ctc")
        self.head = layers.Linear(dim_model, vocab_size) if include_head else nn.Identity()

    def forward(self, video, video_len, audio, audio_len):
        side = rt.branch_stream() if (video.is_cuda and audio.is_cuda) else None
        if side is None:
            video, video_len, v_inter = self.video_encoder(video, video_len)
            audio, audio_len, a_inter = self.audio_encoder(audio, audio_len)
        else:
            # the two encoders are independent: the audio branch runs on a second stream beside the visual one (runtime.branch_stream)
            main = torch.cuda.current_stream()
            rt.stream()                                   # default reduction workspace registered before the fork
            # weight shadows: the visual front-end's on this stream (the stem starts at once), the other 80 % on the audio stream beside the stem's forward
            # pass (a persistent kernel that leaves the HBM idle); this stream waits for them in front of the visual back-end.
            arena = rt.arena_of(self)
            sh_ev = None
            split = arena is not None and not audio_first_env()
            if split:
                side.wait_stream(main)
                sh_ev = arena.ensure_fresh_split(arena.prefix_blocks(self.video_encoder.front_end), side)
            else:
                rt.ensure_shadows_fresh(self)
                side.wait_stream(main)
            for t in (audio, audio_len):
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(side)
            # Host launch order = order in which a captured graph's kernels reach the GPU.  Forward: the visual front-end (few long kernels, the critical
            # path) goes first, the ~400 short audio kernels are submitted while it runs, the visual conformer stack follows.  The autograd engine replays
            # nodes newest-first, so the backward order is: visual conformer stack, audio encoder, ResNet / stem -- the audio submissions again hide
            # behind running work instead of delaying the critical branch.  AVEC_AUDIO_FIRST=1 restores the old order (audio encoder first).
            audio_first = audio_first_env()
            if audio_first:
                with torch.cuda.stream(side):
                    audio, audio_len, a_inter = self.audio_encoder(audio, audio_len)
                video, video_len, v_inter = self.video_encoder(video, video_len)
            else:
                ops.stamp("step_start:f")
                feats = ops.mark(self.video_encoder.forward_front(video), "v_front")
                with torch.cuda.stream(side):
                    ops.stamp("a_start:f")
                    audio, audio_len, a_inter = self.audio_encoder(audio, audio_len)
                    audio = ops.mark(audio, "a_enc")
                if sh_ev is not None:
                    main.wait_event(sh_ev)
                video, video_len, v_inter = self.video_encoder.forward_back(feats, video_len)
                video = ops.mark(video, "v_back")
            main.wait_stream(side)
            for t in [audio, audio_len] + [u for v in a_inter.values() for u in (v if isinstance(v, (list, tuple)) else [v])]:
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(main)
        arena = rt.arena_of(self.fusion_module) if audio.is_cuda else None
        if arena is not None and arena._early_armed:
            # distributed training: when the gradient reaches these two tensors, the fusion module / audio-visual encoder / head gradients are final ->
            # their all-reduce starts while the two encoders are still back-propagating; the audio encoder's follows when its own backward ends
            r_f, r_h = arena.range_of(self.fusion_module), arena.range_of(self.head) if not isinstance(self.head, nn.Identity) else arena.range_of(self.audio_visual_encoder)
            r_a = arena.range_of(self.audio_encoder)
            arena._boundary_fired = False
            arena._audio_range = r_a
            if r_f is not None and r_h is not None and r_h[1] >= r_f[0]:
                audio, video = rt.grad_boundary(audio, arena, r_f[0], r_h[1]), rt.grad_boundary(video, arena, r_f[0], r_h[1])
        x = ops.mark(self.fusion_module(audio, video), "fusion")
        x, lengths, inter = self.audio_visual_encoder(x, audio_len)
        x = ops.mark(x, "av_enc")
        inter.update(v_inter)
        inter.update(a_inter)
        if not isinstance(self.head, nn.Identity):
            x = self.head(x)
        return x, lengths, inter
