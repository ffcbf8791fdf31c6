"""Decoders (nnet/decoders.py).  Greedy CTC: device argmax (HIP) + exact integer collapse.  Beam search: the CTC prefix beam search with n-gram LM
fusion of avec_amd/csrc/ctc_beam.hip (in place of `ctcdecode` + KenLM), then the Transformer-LM (GPT) rescoring of the beams (avec_amd/csrc/lm.hip): all
hypotheses of a batch in one scoring pass.  Timestamps: the CTC forced alignment of avec_amd/csrc/ctc_align.hip.  Test-time augmentation
([B, Naug, T, V] logits): beam_search picks the winner on the host; decode_augmented picks it on the device (avec_amd/csrc/tta.hip), says which augmentation won and
aligns the winner to that augmentation's logits."""
import importlib.util
import os
import sys
import warnings

import torch
import torch.nn as nn

from .. import ops
from .streaming import CTCBeamRingStreamSession, CTCBeamStreamSession


def ctc_collapse(tokens, length, blank=0):
    """unique_consecutive then drop blanks (nnet/decoders.py:105-113) -- bit-exact index work"""
    out, prev = [], None
    for t in tokens[:length]:
        if t != prev and t != blank:
            out.append(t)
        prev = t
    return out


def words_from_pieces(pieces, spans, logps):
    """Word records from aligned sentencepiece pieces (host): a word begins at the first piece and before every piece that starts with "\u2581"; its text is the
    pieces joined with "\u2581" removed, start = the first piece's start, end = the last piece's end, logp = the sum over its pieces.  Words whose text is empty
    (a lone "\u2581") are dropped.  spans: (start, end) per piece, in any unit.  Returns [(text, start, end, logp)]."""
    groups = []
    for piece, (start, end), lp in zip(pieces, spans, logps):
        if not groups or piece.startswith("\u2581"):
            groups.append([piece, start, end, lp])
        else:
            g = groups[-1]
            g[0], g[2], g[3] = g[0] + piece, end, g[3] + lp
    return [(g[0].replace("\u2581", ""), g[1], g[2], g[3]) for g in groups if g[0].replace("\u2581", "")]


class CTCGreedySearchDecoder(nn.Module):
    def __init__(self, tokenizer_path=None, blank_token=0):
        super().__init__()
        self.blank_token = blank_token
        self.tokenizer = None
        if tokenizer_path is not None:
            import os
            if os.path.exists(tokenizer_path):
                import sentencepiece as spm
                self.tokenizer = spm.SentencePieceProcessor(tokenizer_path)

    def token_ids(self, logits, logits_len):
        am = ops.argmax_rows(logits).cpu().tolist()
        lens = logits_len.cpu().tolist()
        return [ctc_collapse(seq, int(n), self.blank_token) for seq, n in zip(am, lens)]

    def forward(self, outputs, from_logits=True):
        if from_logits:
            ids = self.token_ids(outputs[0], outputs[1])
        else:
            tokens, lens = outputs
            ids = [t[:int(n)].tolist() for t, n in zip(tokens.cpu(), lens.cpu())]
        return self.tokenizer.decode(ids) if self.tokenizer is not None else ids

    def align(self, outputs, ids, frame_seconds=0.04):
        """Token (and word) timestamps of known transcripts: the CTC forced alignment of avec_amd/csrc/ctc_align.hip, one launch for the batch.
        outputs = (logits [B, T, V], lengths [B]); ids = a list of token lists, or (tokens [B, Lmax], lens [B]) tensors.  One record per utterance:
        {"score": log-probability of the best path (-inf: the transcript cannot be aligned, e.g. more tokens than frames; "tokens" is then empty),
         "tokens": [(id, start_frame, end_frame, logp)], "token_seconds": [(start, end)] = frames * frame_seconds (0.04 s = one frame of the 25 fps
         output of the AV model), and with a tokenizer "words": [(text, start_frame, end_frame, logp)] and "word_seconds": [(start, end)]}.
        end_frame is exclusive; the blank frames between two tokens belong to neither."""
        logits, lengths = outputs[0], outputs[1]
        if isinstance(ids, (tuple, list)) and len(ids) == 2 and torch.is_tensor(ids[0]):
            tokens, lens = ids[0], ids[1]
        else:
            lens = torch.tensor([len(h) for h in ids], dtype=torch.int64)
            tokens = torch.full((len(ids), max(1, int(lens.max()) if len(ids) else 1)), -1, dtype=torch.int64)
            for b, h in enumerate(ids):
                if len(h):
                    tokens[b, :len(h)] = torch.tensor(list(h), dtype=torch.int64)
        _, spans, score, logp = ops.ctc_align(logits, lengths, tokens, lens, blank=self.blank_token)
        return self._align_records(tokens.cpu().tolist(), lens.cpu().tolist(), spans.cpu().tolist(), score.cpu().tolist(), logp.cpu().tolist(), frame_seconds)

    def _align_records(self, tok, n, spans, score, logp, frame_seconds):
        """the records of align() from host lists: tok [B][Lmax], n [B], spans [B][Lmax][2], score [B], logp [B][Lmax]"""
        records = []
        for b in range(len(tok)):
            k = int(n[b]) if score[b] > float("-inf") else 0
            rec = {"score": score[b], "tokens": [(tok[b][i], spans[b][i][0], spans[b][i][1], logp[b][i]) for i in range(k)]}
            rec["token_seconds"] = [(s * frame_seconds, e * frame_seconds) for _, s, e, _ in rec["tokens"]]
            if self.tokenizer is not None:
                pieces = [self.tokenizer.id_to_piece(t) for t, _, _, _ in rec["tokens"]]
                rec["words"] = words_from_pieces(pieces, [(s, e) for _, s, e, _ in rec["tokens"]], [lp for _, _, _, lp in rec["tokens"]])
                rec["word_seconds"] = [(s * frame_seconds, e * frame_seconds) for _, s, e, _ in rec["words"]]
            records.append(rec)
        return records

    def _decode_ids(self, logits, logits_len):
        return self.token_ids(logits, logits_len)

    def decode_with_timestamps(self, outputs, frame_seconds=0.04):
        """forward(outputs) plus the alignment of the winning hypothesis: (ids, or text with a tokenizer; records as align() returns them)"""
        if getattr(self, "test_time_aug", False):
            raise NotImplementedError("decode_with_timestamps with test_time_aug=True: it takes [B, T, V] logits; CTCBeamSearchDecoder.decode_augmented(outputs, "
                                      "timestamps=True) aligns the winning hypothesis to the logits of the augmentation that won")
        ids = self._decode_ids(outputs[0], outputs[1])
        records = self.align(outputs, ids, frame_seconds)
        return (self.tokenizer.decode(ids) if self.tokenizer is not None else ids), records


class CTCBeamSearchDecoder(CTCGreedySearchDecoder):
    """nnet/decoders.py:122-257: CTC prefix beam search (beam_size, blank 0) over log_softmax(logits / ngram_tmp), fused with the n-gram LM at
    `ngram_path` (ARPA; token k = word chr(k + ngram_offset); ngram_alpha * ln P + ngram_beta per emitted token), one device launch per batch.
    The ranking score is ln P_ctc(prefix) + the summed LM terms (higher is better), and a token that is not an LM word costs ln P = -1000.  ctcdecode's
    own score convention and OOV constant cannot be checked against here (ctcdecode and kenlm are not available), so they are not claimed.
    A missing or empty ARPA file means beam search without an LM (warned).  test_time_aug: logits [B, Naug, T, V], lengths [B, Naug]; per utterance
    the augmentation whose best beam scores highest (ties: the lower index); decode_augmented returns the same hypotheses together with the winning augmentation
    and beam and, on request, the timestamps against that augmentation's logits.
    Neural rescoring (nnet/decoders.py:156-162,208-242): when `neural_config_path` names an existing config file and `os.path.join(config.callback_path,
    neural_checkpoint)` exists, the config is imported, its `model` (anything with `score(ids, lengths)` and `load(path)`; nnet.GPT in the shipped configs) loads the
    checkpoint and is put in eval mode.  Every non-empty beam slot then becomes [sos] + retokenise(tokens) + [eos] (retokenise = neural tokenizer over the decoder
    tokenizer's text; the identity when both are the same file or the decoder has no tokenizer), all B * Naug * W of them are scored in ONE pass, and per utterance
        total = beam_score - neural_alpha * nll_sum + neural_beta * neural_beta * (tokens + 1)
    is maximised over the Naug * W slots (first maximum; empty slots never win).  This is the reference's `beam_scores + alpha * nll - beta * (beta * len)` under argmin
    with the sign of the beam score flipped to this repository's higher-is-better convention; beta enters SQUARED there (neural_lengths is already beta * len when it is
    multiplied by beta again) and that is kept.  Otherwise (no such file, no checkpoint) one UserWarning says that there is no neural rescoring, nothing is imported,
    and the n-gram winner is returned as before."""

    _warned_neural = False

    def __init__(self, tokenizer_path=None, beam_size=16, ngram_path=None, ngram_tmp=1.0, ngram_alpha=0.6, ngram_beta=1.0, ngram_offset=100,
                 neural_config_path=None, neural_checkpoint=None, neural_alpha=0.6, neural_beta=1.0, num_processes=8, test_time_aug=False):
        super().__init__(tokenizer_path=tokenizer_path)
        self.beam_size, self.test_time_aug = beam_size, test_time_aug
        self.ngram_path, self.ngram_tmp, self.ngram_alpha, self.ngram_beta, self.ngram_offset = ngram_path, ngram_tmp, ngram_alpha, ngram_beta, ngram_offset
        self._lm = {}                                   # vocabulary size -> NGramLM or None (parsed on first use, on the host)
        if not ngram_path or not os.path.exists(ngram_path):
            warnings.warn("CTCBeamSearchDecoder: n-gram LM %r not found: beam search without an LM" % (ngram_path,))
            self.ngram_path = None
        self.neural_alpha, self.neural_beta = neural_alpha, neural_beta
        object.__setattr__(self, "neural_rescorer", None)      # (kept out of the module tree: not a state_dict entry of whatever owns the decoder)
        self.neural_tokenizer, self.last_totals = None, None
        if neural_config_path is not None and not self._load_neural(neural_config_path, neural_checkpoint, tokenizer_path) and not CTCBeamSearchDecoder._warned_neural:
            CTCBeamSearchDecoder._warned_neural = True
            warnings.warn("CTCBeamSearchDecoder: no neural rescoring: config %s or its checkpoint %r not found: n-gram beam search only" % (neural_config_path, neural_checkpoint))

    def _load_neural(self, config_path, checkpoint, tokenizer_path):
        """import the LM config as the reference does (nnet/decoders.py:156-162) and load its checkpoint; False when either file is missing (nothing imported then)"""
        if not os.path.isfile(config_path) or checkpoint is None:
            return False
        name = config_path.replace(".py", "").replace("/", ".").strip(".")
        spec = importlib.util.spec_from_file_location(name, config_path)
        cfg = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(cfg)
        ckpt = os.path.join(cfg.callback_path, checkpoint)
        if not os.path.isfile(ckpt):
            return False
        sys.modules[name] = cfg
        model = cfg.model
        if not (hasattr(model, "score") and hasattr(model, "load")):
            raise TypeError("CTCBeamSearchDecoder: the neural config's `model` (%s) needs score(ids, lengths) and load(path)" % type(model).__name__)
        model.load(ckpt, load_optimizer=False)
        model.requires_grad_(False)
        model.eval()
        object.__setattr__(self, "neural_rescorer", model)
        self.neural_pad_token, self.neural_sos_token, self.neural_eos_token = int(cfg.pad_token), int(cfg.sos_token), int(cfg.eos_token)
        lm_tok = getattr(cfg, "tokenizer_path", None)
        same = self.tokenizer is None or lm_tok is None or (tokenizer_path is not None and os.path.exists(lm_tok) and os.path.samefile(lm_tok, tokenizer_path))
        if not same:
            import sentencepiece as spm
            self.neural_tokenizer = spm.SentencePieceProcessor(lm_tok)
        return True

    def _neural_ids(self, hyps):
        """token lists of the decoder -> token lists of the LM, for the whole batch at once (host work on short strings)"""
        if self.neural_tokenizer is None:
            return hyps
        return self.neural_tokenizer.encode(self.tokenizer.decode(hyps))

    def _rescore_best(self, tokens, out_len, score, B, naug):
        """tokens [S, W, T], out_len [S, W], score [S, W] of ops.ctc_beam_search (S = B * naug) -> (best [B] int64 on the device: the winning slot in [0, naug * W),
        the host copies of tokens and out_len)"""
        S, W, T = tokens.shape
        tok, ol, alive = tokens.cpu(), out_len.cpu().tolist(), (score > float("-inf")).cpu().tolist()
        slots = [(s, w) for s in range(S) for w in range(W) if alive[s][w]]
        hyps = self._neural_ids([tok[s, w, :ol[s][w]].tolist() for s, w in slots])
        Lmax = 2 + max((len(h) for h in hyps), default=0)
        ids = torch.full((S * W, Lmax), self.neural_pad_token, dtype=torch.int64)
        lens = torch.zeros(S * W, dtype=torch.int64)                         # 0 = empty slot
        for (s, w), h in zip(slots, hyps):
            row = [self.neural_sos_token] + list(h) + [self.neural_eos_token]
            ids[s * W + w, :len(row)] = torch.tensor(row, dtype=torch.int64)
            lens[s * W + w] = len(row)
        lm = self.neural_rescorer
        dev = score.device
        if next(lm.parameters()).device != dev:
            lm.to(dev)
        best, total, _ = ops.lm_rescore(lm, ids.to(dev), lens.to(dev), score.reshape(-1), self.neural_alpha, self.neural_beta, B)
        self.last_totals = total                                             # [B, naug * W], stays on the device (tests read it)
        return best, tok, ol

    def _rescore(self, tokens, out_len, score, B, naug):
        """... -> per utterance the winning token list"""
        W = tokens.shape[1]
        best, tok, ol = self._rescore_best(tokens, out_len, score, B, naug)
        out = []
        for b, k in enumerate(best.cpu().tolist()):
            s, w = b * naug + k // W, k % W
            out.append(tok[s, w, :ol[s][w]].tolist())
        return out

    def lm(self, vocab_size):
        if vocab_size not in self._lm:
            from .. import ngram
            self._lm[vocab_size] = ngram.load(self.ngram_path, vocab_size, self.ngram_offset) if self.ngram_path else None
        return self._lm[vocab_size]

    def beam_search(self, logits, logits_len):
        if self.test_time_aug:
            B, naug = logits.shape[:2]
            logits, logits_len = logits.flatten(0, 1), logits_len.flatten(0, 1)
        else:
            B, naug = logits.shape[0], 1
        tokens, out_len, score, _ = ops.ctc_beam_search(logits, logits_len, self.beam_size, self.ngram_tmp, self.lm(logits.shape[-1]), self.ngram_alpha,
                                                        self.ngram_beta)
        if self.neural_rescorer is not None:
            return self._rescore(tokens, out_len, score, B, naug)
        T = tokens.shape[-1]
        tok0, len0 = tokens[:, 0].reshape(B, naug, T).cpu(), out_len[:, 0].reshape(B, naug).cpu()
        best = score[:, 0].reshape(B, naug).cpu().argmax(dim=1)        # the first maximum: ties go to the lower augmentation index
        return [tok0[b, best[b], :len0[b, best[b]]].tolist() for b in range(B)]

    def decode_augmented(self, outputs, timestamps=False, frame_seconds=0.04):
        """Decode test-time-augmented logits and say which augmentation won: outputs = (logits [B, n, T, V], lengths [B, n]) as VisualEfficientConformerInterCTC
        gives them with test_augments (n = 1 is valid).  Returns (ids per utterance, or text with a tokenizer; records), one record per utterance:
        {"ids": the winning token list (what beam_search returns), "augmentation": the index along n it came from (0 = the clip as given), "beam": its beam slot,
         "score": its ranking score (-inf: every slot of the utterance is empty)}.  The winner is beam_search's: without a neural rescorer the augmentation whose best
        beam scores highest (first maximum) and beam 0; with one, the first maximum of the rescored totals over the n * W slots.
        timestamps=True adds every field of align() for the winning hypothesis against the logits of the augmentation that won ("tokens", "token_seconds", with a
        tokenizer "words" and "word_seconds"); align()'s "score", the log-probability of the best path, is stored as "align_score".
        The beam search, the choice (ops.ctc_tta_pick), the gather of the winners' logits and the alignment stay on the device; the results come back in ONE
        device-to-host copy at the end.  (A neural rescorer fetches the beams before that to retokenise them, as in beam_search.)"""
        logits, lengths = outputs[0], outputs[1]
        if logits.dim() != 4 or tuple(lengths.shape) != tuple(logits.shape[:2]):
            raise ValueError("decode_augmented: logits %s, lengths %s; expected [B, n, T, V] and [B, n]" % (tuple(logits.shape), tuple(lengths.shape)))
        B, n, T, V = logits.shape
        flat, flat_len = logits.flatten(0, 1), lengths.flatten(0, 1).to(device=logits.device, dtype=torch.int64)
        tokens, out_len, score, _ = ops.ctc_beam_search(flat, flat_len, self.beam_size, self.ngram_tmp, self.lm(V), self.ngram_alpha, self.ngram_beta)
        best_slot = self._rescore_best(tokens, out_len, score, B, n)[0] if self.neural_rescorer is not None else None
        aug, beam, ids, ids_len, best_score = ops.ctc_tta_pick(tokens, out_len, score, n, best_slot)
        parts = [aug, beam, ids_len, best_score, ids.reshape(-1)]
        if timestamps:
            rows = torch.arange(B, device=aug.device) * n + aug                  # the winners' rows of the flattened batch
            _, spans, a_score, logp = ops.ctc_align(flat.index_select(0, rows), flat_len.index_select(0, rows), ids, ids_len, blank=self.blank_token)
            parts += [a_score, spans.reshape(-1), logp.reshape(-1)]
        host = torch.cat([p.to(torch.float64) for p in parts]).cpu().tolist()   # (every value is an int32-range integer or an fp32: exact in fp64) the one fetch

        def take(k, integer):
            out = host[take.at:take.at + k]
            take.at += k
            return [int(v) for v in out] if integer else out
        take.at = 0
        aug, beam, ids_len, best_score = take(B, True), take(B, True), take(B, True), take(B, False)
        ids = take(B * T, True)
        tok = [ids[b * T:(b + 1) * T] for b in range(B)]
        records = [{"ids": tok[b][:ids_len[b]], "augmentation": aug[b], "beam": beam[b], "score": best_score[b]} for b in range(B)]
        if timestamps:
            a_score, spans, logp = take(B, False), take(B * T * 2, True), take(B * T, False)
            spans = [[spans[(b * T + i) * 2:(b * T + i) * 2 + 2] for i in range(T)] for b in range(B)]
            logp = [logp[b * T:(b + 1) * T] for b in range(B)]
            for rec, al in zip(records, self._align_records(tok, ids_len, spans, a_score, logp, frame_seconds)):
                al["align_score"] = al.pop("score")
                rec.update(al)
        hyps = [r["ids"] for r in records]
        return (self.tokenizer.decode(hyps) if self.tokenizer is not None else hyps), records

    def stream(self, batch_size, max_frames=None, window=None, log_frames=None):
        """A streaming session over batch_size utterance slots: push logits chunk by chunk as the encoder emits them, read the partial and the final part of the
        transcript after every chunk, finish() for the winning hypotheses.
        window=None: a CTCBeamStreamSession of at most max_frames frames per slot, whose finish() is what beam_search gives on the whole.
        window=N (>= 2, max_frames must be None): a CTCBeamRingStreamSession without a frame limit: history older than N frames is committed N // 2 frames at a time
        (the beams that disagree with the best beam on it are dropped) and reported as final; log_frames (default max(4 N, 256)) sizes the device's commit log."""
        if self.test_time_aug:
            raise NotImplementedError("CTCBeamSearchDecoder.stream with test_time_aug=True: the augmentations of an utterance would have to be pushed in step, at "
                                      "twice the encoder cost per chunk; decode_augmented covers whole utterances")
        if window is None:
            if max_frames is None:
                raise ValueError("CTCBeamSearchDecoder.stream: max_frames is needed (or window=N for a session without a frame limit)")
            if log_frames is not None:
                raise ValueError("CTCBeamSearchDecoder.stream: log_frames belongs to window=N")
            return CTCBeamStreamSession(self, batch_size, max_frames)
        if max_frames is not None:
            raise ValueError("CTCBeamSearchDecoder.stream: window=%r together with max_frames=%r: a ring session has no frame limit" % (window, max_frames))
        return CTCBeamRingStreamSession(self, batch_size, window, log_frames)

    def _decode_ids(self, logits, logits_len):
        return self.beam_search(logits, logits_len)

    def forward(self, outputs, from_logits=True):
        if from_logits:
            ids = self.beam_search(outputs[0], outputs[1])
        else:
            tokens, lens = outputs
            ids = [t[:int(n)].tolist() for t, n in zip(tokens.cpu(), lens.cpu())]
        return self.tokenizer.decode(ids) if self.tokenizer is not None else ids


decoder_dict = {"CTCGreedySearchDecoder": CTCGreedySearchDecoder, "CTCBeamSearchDecoder": CTCBeamSearchDecoder, "CTCBeamSearch": CTCBeamSearchDecoder}
