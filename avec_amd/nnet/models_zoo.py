"""Model definitions (nnet/models_zoo.py): audio-only, visual-only and audio-visual Efficient Conformer InterCTC models."""
import torch
import torch.nn as nn

from .. import ops
from . import attentions, embeddings, layers
from . import losses as L
from . import networks, optimizers, schedulers
from .model import Model
from .models import Classifier


def _default_adam(model):
    """Adam(b=(0.9,0.98), eps=1e-9, wd=1e-6) + Noam(warmup 10k, dim 360, factor 2)  (nnet/models_zoo.py:172-174)"""
    lr = schedulers.NoamDecayScheduler(warmup_steps=10000, dim_decay=360, val_factor=2)
    return optimizers.Adam(params=model.parameters(), lr=lr, betas=(0.9, 0.98), eps=1e-9, weight_decay=1e-6)


class VisualEfficientConformerCE(Model):
    """nnet/models_zoo.py:33-62: the LRW word classifier -- visual encoder without InterCTC, head to `vocab_size` classes, logits averaged over time."""

    def __init__(self, vocab_size=500):
        super().__init__(name="Visual Efficient Conformer CE")
        self.encoder = networks.VisualEfficientConformerEncoder(vocab_size=vocab_size, interctc_blocks=[])

    def forward(self, inputs):
        from .. import ops
        x = self.encoder(inputs, lengths=None)[0]
        return ops.TimeMeanFn.apply(x) if x.is_cuda else x.mean(dim=1)

    def compile(self, losses=None, loss_weights=None, optimizer="Adam", metrics="default", decoders=None):
        from . import metrics as M
        if losses is None:
            losses = L.SoftmaxCrossEntropy()
        if metrics == "default":
            metrics = M.CategoricalAccuracy()
        if optimizer == "Adam":
            optimizer = _default_adam(self)
        super().compile(losses=losses, loss_weights=loss_weights, optimizer=optimizer, metrics=metrics, decoders=decoders)


_DEFAULT = object()                                        # "argument omitted": an explicit None must stay None (nnet/models_zoo.py:128-147)


def is_native_flip(augment):
    """True for the augment the HIP clip-batch kernel covers: a `RandomHorizontalFlip` (torchvision's or avec_amd.compat.torchvision_fallback's, told by the class
    name) that always flips (p >= 1.0)"""
    p = getattr(augment, "p", None)
    return type(augment).__name__ == "RandomHorizontalFlip" and isinstance(p, (int, float)) and p >= 1.0


class _InterCTCModel(Model):
    default_loss_weights = None

    def compile(self, losses=_DEFAULT, loss_weights="default", optimizer="Adam", metrics=None, decoders=None):
        """losses omitted: CTCLoss() as the reference's default argument; an explicit None: no losses (compiled_losses == [], the test-time-augmentation configs)"""
        if losses is _DEFAULT:
            losses = L.CTCLoss()
        if loss_weights == "default":
            lw = self.default_loss_weights
            loss_weights = dict(lw) if isinstance(lw, dict) else list(lw)
        if optimizer == "Adam":
            optimizer = _default_adam(self)
        super().compile(losses=losses, loss_weights=loss_weights, optimizer=optimizer, metrics=metrics, decoders=decoders)


class AudioEfficientConformerInterCTC(_InterCTCModel):
    """nnet/models_zoo.py:64-97"""
    default_loss_weights = [0.5 / 4, 0.5 / 4, 0.5 / 4, 0.5 / 4, 0.5]

    def __init__(self, vocab_size=256, att_type="patch", interctc_blocks=[3, 6, 10, 13]):
        super().__init__(name="Audio Efficient Conformer Inter CTC")
        self.encoder = networks.AudioEfficientConformerEncoder(vocab_size=vocab_size, att_type=att_type, interctc_blocks=interctc_blocks)

    def forward(self, inputs):
        x, lengths = inputs
        x, lengths, inter = self.encoder(x, lengths)
        out = {"outputs": [x, lengths]}
        out.update(inter)
        return out


class VisualEfficientConformerInterCTC(_InterCTCModel):
    """nnet/models_zoo.py:99-147.  test_augments (None, a callable or a list of callables on clips (B, 1, T, H, W)): test-time augmentation.  In eval mode with A
    augments "outputs" is [logits [B, 1 + A, T', V], lengths [B, 1 + A]] (index 0: the clips as given, then the augments in list order) and the InterCTC entries
    are those of the clips as given, as in the reference (nnet/models_zoo.py:113-122).  The reference runs the encoder 1 + A times; here it runs ONCE over
    (1 + A) * B clips laid out utterance-major (row b * (1 + A) + k), so the logits are a plain view and CTCBeamSearchDecoder's flatten(0, 1) costs no copy.
    That is the same function: eval-mode BatchNorm uses its running statistics and every other layer works per utterance."""
    default_loss_weights = [0.5 / 3, 0.5 / 3, 0.5 / 3, 0.5]

    def __init__(self, vocab_size=256, interctc_blocks=[3, 6, 9], test_augments=None):
        super().__init__(name="Visual Efficient Conformer Inter CTC")
        self.encoder = networks.VisualEfficientConformerEncoder(vocab_size=vocab_size, interctc_blocks=interctc_blocks)
        # (a plain list, as in the reference: an augment that is an nn.Module is not registered, so the state_dict keys do not change)
        self.test_augments = test_augments if isinstance(test_augments, list) else [test_augments] if test_augments is not None else test_augments

    def tta_clips(self, video, native=None):
        """video (B, T, H, W, 1) -> the (B * (1 + A), T, H, W, 1) clip batch of one augmented pass.  native (default: when every augment is the always-on horizontal
        flip): one HIP launch (ops.video_tta_batch); otherwise every augment is applied as the reference does, to video.permute(0, 4, 1, 2, 3), and the results are
        interleaved with PyTorch ops."""
        augs = self.test_augments
        n = 1 + len(augs)
        if native is None:
            native = n <= 32 and all(is_native_flip(a) for a in augs)
        if native:
            return ops.video_tta_batch(video, n, (1 << n) - 2)
        clips = video.permute(0, 4, 1, 2, 3)
        both = torch.stack([clips] + [a(clips) for a in augs], dim=1)          # (B, n, 1, T, H, W)
        return both.flatten(0, 1).permute(0, 2, 3, 4, 1).contiguous()

    def forward(self, inputs):
        video, video_lengths = inputs
        assert not (self.training and self.test_augments is not None), "Training requires setting test_time_aug to False / test_augments to None"
        if self.test_augments is None:
            x, lengths, inter = self.encoder(video.permute(0, 4, 1, 2, 3), video_lengths)
        else:
            B, n = video.shape[0], 1 + len(self.test_augments)
            x, lengths, inter = self.encoder(self.tta_clips(video).permute(0, 4, 1, 2, 3), video_lengths.repeat_interleave(n))
            x, lengths = x.unflatten(0, (B, n)), lengths.unflatten(0, (B, n))          # views
            inter = {k: [lg.unflatten(0, (B, n))[:, 0], ln.unflatten(0, (B, n))[:, 0]] for k, (lg, ln) in inter.items()}
        out = {"outputs": [x, lengths]}
        out.update(inter)
        return out


class AudioVisualEfficientConformerInterCTC(_InterCTCModel):
    """nnet/models_zoo.py:149-182"""
    default_loss_weights = {"v_ctc_2": 0.5 / 3, "v_ctc_5": 0.5 / 3, "a_ctc_7": 0.5 / 3, "a_ctc_10": 0.5 / 3, "f_ctc_1": 0.5 / 3, "outputs": 0.5}

    def __init__(self, vocab_size=256, v_interctc_blocks=[3, 6], a_interctc_blocks=[8, 11], f_interctc_blocks=[2]):
        super().__init__(name="Audio-Visual Efficient Conformer Inter CTC")
        self.encoder = networks.AudioVisualEfficientConformerEncoder(vocab_size=vocab_size, v_interctc_blocks=v_interctc_blocks,
                                                                     a_interctc_blocks=a_interctc_blocks, f_interctc_blocks=f_interctc_blocks)

    def forward(self, inputs):
        video, video_len, audio, audio_len = inputs
        x, lengths, inter = self.encoder(video.permute(0, 4, 1, 2, 3), video_len, audio, audio_len)
        out = {"outputs": [x, lengths]}
        out.update(inter)
        return out


class TransformerLM(Classifier):
    """Causal Transformer language model of any size: nn.Embedding -> networks.Transformer (pre-norm, GELU, plain causal attention) -> Linear head; sub-module
    names `embedding` / `transformer` / `head` and state_dict keys as nnet.GPT in the reference (nnet/models_zoo.py:239-261).  GPT below only adds the named size
    table; tests and the synthetic configs run small models through this very class.  Inference only (the rescorer of CTCBeamSearchDecoder): head width
    dim_model / num_heads must be 64 (ops.causal_attention).
      forward(ids) -> logits [N, L, V] fp32                  (the unfused path: the logits are materialised; parity tests)
      score(ids, lengths) -> nll sums [N] fp32                (the fused path: head + log_softmax + gather in one kernel, logits never written)"""

    def __init__(self, vocab_size, dim_model, num_blocks, num_heads, padding_idx=None, max_pos_encoding=2048, pos_embedding=embeddings.PosEmbedding1d, drop_rate=0.1,
                 ff_ratio=4, name="TransformerLM"):
        super().__init__(name=name)
        self.embedding = nn.Embedding(num_embeddings=vocab_size, embedding_dim=dim_model, padding_idx=padding_idx)
        self.transformer = networks.Transformer(
            dim_model=dim_model, num_blocks=num_blocks,
            att_params={"class": "MultiHeadAttention", "params": {"num_heads": num_heads, "attn_drop_rate": drop_rate}}, ff_ratio=ff_ratio, emb_drop_rate=drop_rate,
            drop_rate=drop_rate, act_fun="GELU", pos_embedding=pos_embedding(num_embeddings=max_pos_encoding, dim_emb=dim_model), inner_dropout=False,
            mask=attentions.Mask(right_context=0))
        self.head = layers.Linear(in_features=dim_model, out_features=vocab_size)

        def init_weights(m):                                   # nnet/models_zoo.py:263-273
            if isinstance(m, (nn.Linear, nn.Embedding)):
                torch.nn.init.normal_(m.weight, mean=0.0, std=0.02)
                if isinstance(m, nn.Linear) and m.bias is not None:
                    torch.nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                torch.nn.init.zeros_(m.bias)
                torch.nn.init.ones_(m.weight)
        self.apply(init_weights)

    def compile(self, losses=None, loss_weights=None, optimizer="AdamW", metrics=None, decoders=None):
        """Holds what the reference's LM configs pass (nnet/models_zoo.py:275-317) so that they import; there is no LM training loop here."""
        if optimizer == "AdamW":
            optimizer = optimizers.AdamW(params=optimizers.get_decay_param_groups(self, weight_decay=0.1), lr=6e-4, betas=(0.9, 0.95), eps=1e-8)
        Model.compile(self, losses=L.SoftmaxCrossEntropy() if losses is None else losses, loss_weights=loss_weights, optimizer=optimizer, metrics=metrics,
                      decoders=decoders)

    def _rows(self, ids, lengths=None):
        """ids [N, L] -> final-LayerNorm rows [N * L, D] (compute dtype): embedding + positions in one launch, then the block stack"""
        if self.training:
            raise RuntimeError("%s is an inference model here: call .eval() first (training the LM is out of scope)" % type(self).__name__)
        ids = ids.to(self.embedding.weight.device)
        x = ops.embed_pos(ids, self.embedding.weight, self.transformer.pos_embedding.table(), out_f32=True)
        return self.transformer.forward_rows(x, lengths, embedded=True)

    def forward(self, ids):
        N, Lq = ids.shape
        with torch.no_grad():
            h = self._rows(ids)
            return ops.linear_fwd(h, self.head.weight, self.head.bias, N * Lq, in_f32=False, out_f32=True).view(N, Lq, -1)

    def token_nll(self, ids, lengths):
        """nll [N, L]: row (n, t) = -log p(ids[n, t + 1] | ids[n, :t + 1]) for t < lengths[n] - 1, 0 elsewhere"""
        N, Lq = ids.shape
        with torch.no_grad():
            ids = ids.to(self.embedding.weight.device)
            lengths = lengths.to(device=ids.device, dtype=torch.int64)
            tgt = torch.full_like(ids, -1, dtype=torch.int64)
            tgt[:, :-1] = ids[:, 1:]
            tgt = torch.where(torch.arange(Lq, device=ids.device)[None, :] < (lengths[:, None] - 1), tgt, torch.full_like(tgt, -1))
            h = self._rows(ids, lengths)
            return ops.lm_head_nll(h, self.head.weight, self.head.bias, tgt).view(N, Lq)

    def score(self, ids, lengths):
        """sum over t < lengths - 1 of the target nll (nnet/decoders.py:226-231; lengths count <sos> and <eos>), one pass for all sequences"""
        return ops.lm_segment_sum(self.token_nll(ids, lengths), lengths)


class GPT(TransformerLM):
    """nnet/models_zoo.py:184-327: the named GPT-3 sizes.  `GPT(vocab_size=1025, padding_idx=0, model="GPT-Small", pos_embedding=SinPosEmbedding)` has the reference's
    state_dict keys and shapes, so a released LM checkpoint loads with strict=True."""
    sizes = {"GPT-Small": (768, 12, 12), "GPT-Medium": (1024, 24, 16), "GPT-Large": (1536, 24, 16), "GPT-XL": (2048, 24, 24), "GPT-2.7B": (2560, 32, 32),
             "GPT-6.7B": (4096, 32, 32), "GPT-13.0B": (5140, 40, 40), "GPT-175.0B": (12288, 96, 96)}        # dim_model, num_blocks, num_heads
    lr_max = {"GPT-Small": 6e-4, "GPT-Medium": 3e-4, "GPT-Large": 2.5e-4, "GPT-XL": 2e-4, "GPT-2.7B": 1.6e-4, "GPT-6.7B": 1.2e-4, "GPT-13.0B": 1e-4, "GPT-175.0B": 0.6e-4}

    def __init__(self, vocab_size=25000, padding_idx=None, max_pos_encoding=2048, model="GPT-Small", pos_embedding=embeddings.PosEmbedding1d, drop_rate=0.1):
        assert model in self.sizes, model
        dim_model, num_blocks, num_heads = self.sizes[model]
        super().__init__(vocab_size=vocab_size, dim_model=dim_model, num_blocks=num_blocks, num_heads=num_heads, padding_idx=padding_idx,
                         max_pos_encoding=max_pos_encoding, pos_embedding=pos_embedding, drop_rate=drop_rate, name=model)

    def compile(self, losses=None, loss_weights=None, optimizer="AdamW", metrics=None, decoders=None):
        if optimizer == "AdamW":
            optimizer = optimizers.AdamW(params=optimizers.get_decay_param_groups(self, weight_decay=0.1), lr=self.lr_max[self.name], betas=(0.9, 0.95), eps=1e-8)
        super().compile(losses=losses, loss_weights=loss_weights, optimizer=optimizer, metrics=metrics, decoders=decoders)
