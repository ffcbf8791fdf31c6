"""CTC prefix beam search with n-gram LM fusion, host side: the ARPA parser, the device table layout (through its numpy mirror), the fp64 oracle
against brute force, and the decoder's CPU-only construction."""
import itertools
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctc_beam_oracle as O  # noqa: E402
from avec_amd import ngram  # noqa: E402

STUB = "\\data\\\nngram 1=0\n\n\\1-grams:\n\n\\end\\\n"          # what tools/make_synthetic_assets.py writes as the 6-gram file


def test_arpa_parser_entries_and_dropped_lines(tmp_path):
    p = str(tmp_path / "lm3.arpa")
    want, dropped = O.write_random_arpa(p, V=40, order=3, n_per_order=150, seed=3)
    arpa = ngram.parse_arpa(p, 40, offset=100)
    assert arpa.order == 3 and arpa.counts[1] == sum(1 for k in want if len(k) == 1) + 4
    assert arpa.entries() == want
    assert arpa.dropped == dropped
    assert any(b is None for k, (_, b) in want.items() if len(k) < 3) and (-1,) in want      # missing backoffs and <s> are exercised
    # blank lines / spaces instead of tabs parse the same
    txt = open(p).read().replace("\t", " ").replace("\n\\2-grams:", "\n\n\n\\2-grams:")
    p2 = str(tmp_path / "lm3b.arpa")
    open(p2, "w").write(txt)
    assert ngram.parse_arpa(p2, 40, offset=100).entries() == want


def test_empty_stub_is_no_lm(tmp_path):
    p = str(tmp_path / "6gram.arpa")
    open(p, "w").write(STUB)
    assert not ngram.NGramLM(p, 256).usable
    with pytest.warns(UserWarning, match="no unigram"):
        assert ngram.load(p, 256) is None
    with pytest.warns(UserWarning, match="not found"):
        assert ngram.load(str(tmp_path / "missing.arpa"), 256) is None


@pytest.mark.parametrize("order", [1, 3, 6])
def test_host_table_rows_equal_backoff_definition(tmp_path, order):
    V = 40
    p = str(tmp_path / "lm.arpa")
    want, _ = O.write_random_arpa(p, V=V, order=order, n_per_order=300, seed=order)
    lm = ngram.NGramLM(p, V, offset=100)
    assert lm.usable and lm.order == order and (lm.ctx_cap == 0 or lm.n_contexts <= lm.ctx_cap // 2)
    oov = [k for k in range(V) if (k,) not in want]
    assert oov, "the generated LM leaves some tokens out"
    rnd = np.random.default_rng(order)
    ctxs = [k[:-1] for k in want if len(k) >= 2][:60]                           # contexts that exist (long chains)
    ctxs += [tuple(int(x) for x in rnd.integers(0, V, size=rnd.integers(0, 9))) for _ in range(60)]      # random ones: back off, some to the unigram
    ctxs += [(-1,) + c for c in ctxs[:40]] + [(oov[0],), (-1, oov[0]), (3, oov[-1], 5)]
    dl = O.DictLM(want, order, V)
    for ctx in ctxs:
        hist = ctx if (ctx and ctx[0] == -1) else (-1,) + ctx
        row = lm.row(hist)
        ref = np.array([O.lm_logprob(want, order, hist, c) for c in range(V)])
        np.testing.assert_allclose(row, ref, rtol=0, atol=2e-5, err_msg=str(ctx))
        np.testing.assert_allclose(dl.row(hist), ref, rtol=0, atol=1e-9)
        assert (row[oov] == -1000.0).all()


def _brute_force(logp, V):
    """{label tuple: ln sum over all alignments that collapse to it}"""
    T = logp.shape[0]
    acc = {}
    for path in itertools.product(range(V), repeat=T):
        lab, prev = [], None
        for k in path:
            if k != prev and k != 0:
                lab.append(k)
            prev = k
        acc.setdefault(tuple(lab), []).append(sum(logp[t, k] for t, k in enumerate(path)))
    return {k: float(np.logaddexp.reduce(v)) for k, v in acc.items()}


@pytest.mark.parametrize("with_lm", [False, True])
def test_oracle_without_pruning_equals_brute_force(tmp_path, with_lm):
    T, V, W = 4, 3, 32
    g = np.random.default_rng(7)
    logits = g.standard_normal((T, V)).astype(np.float32)
    logp = O.log_softmax64(logits, 1.5)
    lm = None
    if with_lm:
        p = str(tmp_path / "lm.arpa")
        want, _ = O.write_random_arpa(p, V=V, order=3, n_per_order=6, seed=1, extras=False)
        lm = O.DictLM(want, 3, V)
    beams, _ = O.beam_search(logp, T, W, lm=lm, alpha=0.6, beta=1.0)
    ref = _brute_force(logp, V)
    assert len(beams) == len(ref) <= W                                         # nothing pruned
    for toks, score, ctc in beams:
        assert abs(ctc - ref[tuple(toks)]) < 1e-9
        nll = torch.nn.functional.ctc_loss(torch.tensor(logp, dtype=torch.float64)[:, None], torch.tensor([toks or [1]], dtype=torch.long)[:, :len(toks)],
                                           torch.tensor([T]), torch.tensor([len(toks)]), blank=0, reduction="none")
        assert abs(-float(nll[0]) - ctc) < 1e-9
        lmsum = 0.0
        if with_lm:
            for k, c in enumerate(toks):
                lmsum += 0.6 * O.lm_logprob(want, 3, (-1,) + tuple(toks[:k]), c) + 1.0
        assert abs((score - ctc) - lmsum) < 1e-9


def test_beam_decoder_constructs_cpu_only_from_the_av_config_kwargs(tmp_path):
    """the reference AV config's decoder (configs/LRS23/AV/EffConfInterCTC.py:39-46,64), with its ARPA missing and its GPT config named"""
    code = r'''
import sys, warnings
sys.path.insert(0, %r)
import torch
import nnet
with warnings.catch_warnings(record=True) as w:
    warnings.simplefilter("always")
    d = nnet.CTCBeamSearchDecoder(tokenizer_path="datasets/LRS3/tokenizerbpe256.model", beam_size=16, ngram_path="datasets/LRS3/6gram_lrs23.arpa",
                                  ngram_tmp=1.0, ngram_alpha=0.6, ngram_beta=1.0, ngram_offset=100, neural_config_path="configs/LRS23/LM/GPT-Small.py",
                                  neural_checkpoint="checkpoints_epoch_10_step_2860.ckpt", neural_alpha=0.6, neural_beta=1.0)
msgs = [str(x.message) for x in w]
assert any("not found" in m for m in msgs), msgs
assert any("neural rescoring" in m for m in msgs), msgs
assert not any(k.startswith("configs") for k in sys.modules), [k for k in sys.modules if k.startswith("configs")]
assert not torch.cuda.is_initialized()
assert d.beam_size == 16 and d.ngram_path is None
from avec_amd.nnet.decoders import decoder_dict
assert decoder_dict["CTCBeamSearch"] is decoder_dict["CTCBeamSearchDecoder"]
print("OK")
''' % ROOT
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
