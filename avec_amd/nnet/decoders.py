"""Decoders (nnet/decoders.py).  Greedy CTC: device argmax (HIP) + exact integer collapse.  Beam search: the CTC prefix beam search with n-gram LM
fusion of avec_amd/csrc/ctc_beam.hip (in place of `ctcdecode` + KenLM); the GPT rescoring pass stays out of scope."""
import os
import warnings

import torch
import torch.nn as nn

from .. import ops


def ctc_collapse(tokens, length, blank=0):
    """unique_consecutive then drop blanks (nnet/decoders.py:105-113) -- bit-exact index work"""
    out, prev = [], None
    for t in tokens[:length]:
        if t != prev and t != blank:
            out.append(t)
        prev = t
    return out


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


class CTCBeamSearchDecoder(CTCGreedySearchDecoder):
    """nnet/decoders.py:122-257: CTC prefix beam search (beam_size, blank 0) over log_softmax(logits / ngram_tmp), fused with the n-gram LM at
    `ngram_path` (ARPA; token k = word chr(k + ngram_offset); ngram_alpha * ln P + ngram_beta per emitted token), one device launch per batch.
    The ranking score is ln P_ctc(prefix) + the summed LM terms (higher is better), and a token that is not an LM word costs ln P = -1000.  ctcdecode's
    own score convention and OOV constant cannot be checked against here (ctcdecode and kenlm are not available), so they are not claimed.
    A missing or empty ARPA file means beam search without an LM (warned).  test_time_aug: logits [B, Naug, T, V], lengths [B, Naug]; per utterance
    the augmentation whose best beam scores highest (ties: the lower index).  neural_config_path (GPT rescoring) is not imported: out of scope."""

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
        if neural_config_path is not None and not CTCBeamSearchDecoder._warned_neural:
            CTCBeamSearchDecoder._warned_neural = True
            warnings.warn("CTCBeamSearchDecoder: neural rescoring (%s) is out of scope: n-gram beam search only" % neural_config_path)

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
        T = tokens.shape[-1]
        tok0, len0 = tokens[:, 0].reshape(B, naug, T).cpu(), out_len[:, 0].reshape(B, naug).cpu()
        best = score[:, 0].reshape(B, naug).cpu().argmax(dim=1)        # the first maximum: ties go to the lower augmentation index
        return [tok0[b, best[b], :len0[b, best[b]]].tolist() for b in range(B)]

    def forward(self, outputs, from_logits=True):
        if from_logits:
            ids = self.beam_search(outputs[0], outputs[1])
        else:
            tokens, lens = outputs
            ids = [t[:int(n)].tolist() for t, n in zip(tokens.cpu(), lens.cpu())]
        return self.tokenizer.decode(ids) if self.tokenizer is not None else ids


decoder_dict = {"CTCGreedySearchDecoder": CTCGreedySearchDecoder, "CTCBeamSearchDecoder": CTCBeamSearchDecoder, "CTCBeamSearch": CTCBeamSearchDecoder}
