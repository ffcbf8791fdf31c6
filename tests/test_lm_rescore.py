"""Transformer-LM rescoring, the parts that need no GPU: the fp64 oracle (tests/lm_oracle.py) pinned to fixtures made by the reference
(tests/golden/make_golden_lm.py), state_dict compatibility of nnet.GPT, the decoder's construction and host-side bookkeeping, the thin LM-config API."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lm_oracle as O  # noqa: E402
from tests.helpers import GOLDEN, rel_err  # noqa: E402

TOL = 1e-5          # fp64 oracle against the reference's fp32 output: the tolerance of tests/test_oracle_golden.py
REF_LM_CFG = "/root/reference/configs/LRS23/LM/GPT-Small.py"


@pytest.mark.parametrize("name,base,H", [("lm_d128_sin", None, 2), ("lm_d128_pos", "lm_d128_sin", 2), ("lm_d64_2blk", None, 1)])
def test_oracle_matches_the_reference_fixtures(name, base, H):
    sd, ids, lens, logits, nll = O.load_fixture(os.path.join(GOLDEN, name + ".npz"), None if base is None else os.path.join(GOLDEN, base + ".npz"))
    assert set([2, 3, 17, 64]) <= set(lens.tolist())
    mine = O.logits(sd, ids, H)
    assert rel_err(mine, logits) < TOL
    assert rel_err(O.nll_sums(mine, ids, lens), nll) < TOL
    # the bf16-operand variant is a different (coarser) function, not a no-op
    assert 1e-4 < rel_err(O.logits(sd, ids, H, q=O.bf16_round), logits) < 1e-1
    for f in os.listdir(GOLDEN):
        if f.startswith("lm_"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) <= 1048576, f


def test_gpt_small_state_dict_equals_the_reference():
    import nnet
    want = json.load(open(os.path.join(GOLDEN, "lm_gpt_small_keys.json")))
    m = nnet.GPT(vocab_size=1025, padding_idx=0, model="GPT-Small", pos_embedding=nnet.SinPosEmbedding)
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert isinstance(m, nnet.TransformerLM) and isinstance(m, nnet.Classifier) and isinstance(m, nnet.Model)
    with pytest.raises(AssertionError):
        nnet.GPT(model="GPT-Tiny")
    # learned positions add exactly one key
    mp = nnet.TransformerLM(65, 128, 1, 2, padding_idx=0, max_pos_encoding=64, pos_embedding=nnet.PosEmbedding1d)
    assert "transformer.pos_embedding.pos_encoding" in mp.state_dict() and mp.state_dict()["transformer.pos_embedding.pos_encoding"].shape == (64, 128)
    # registries
    from avec_amd.nnet import activations, attentions, blocks, optimizers
    assert attentions.att_dict["MultiHeadAttention"] is nnet.MultiHeadAttention and blocks.block_dict["TransformerBlock"] is nnet.TransformerBlock
    assert activations.act_dict["GELU"] is nnet.GELU and optimizers.optim_dict["AdamW"] is nnet.AdamW
    # the conformer classes keep their guards
    with pytest.raises(AssertionError):
        nnet.RelPos1dMultiHeadAttention(64, 1, 10, attn_drop_rate=0.1)
    with pytest.raises(AssertionError):
        nnet.FeedForwardModule(64, 256, 0.1, "ReLU", False)


def test_sin_pos_embedding_table_and_thin_lm_api():
    import nnet
    e = nnet.SinPosEmbedding(50, 64)
    assert e.pos_encoding.shape == (1, 50, 64) and "pos_encoding" not in e.state_dict()
    assert torch.equal(e.table().double(), O.sin_table(50, 64))
    x = torch.randn(2, 7, 64)
    assert torch.equal(e(x), x + e.table()[:7])
    m = nnet.TransformerLM(65, 64, 1, 1)
    groups = nnet.get_decay_param_groups(m, weight_decay=0.1)
    assert [g["weight_decay"] for g in groups] == [0.1, 0.0] and sum(len(g["params"]) for g in groups) == len(list(m.parameters()))
    assert all(p.dim() == 2 for p in groups[0]["params"]) and not any(p is m.embedding.weight for p in groups[0]["params"])
    opt = nnet.AdamW(params=groups, lr=6e-5, betas=(0.9, 0.95), eps=1e-8)
    m.compile(optimizer=opt)
    assert m.optimizer is opt and opt.scheduler.get_val() == 6e-5 and opt.defaults["betas"] == (0.9, 0.95)
    with pytest.raises(NotImplementedError):
        opt.step()
    ds = nnet.datasets.CorpusLM(collate_fn=None, batch_size=128, tokenizer_path="t.model", max_length=100, corpus_path="c.txt")
    assert (ds.batch_size, ds.tokenizer_path, ds.corpus_path, ds.max_length, len(ds)) == (128, "t.model", "c.txt", 100, 0)
    # inference only: a training-mode LM says so instead of returning a graph-less tensor
    with pytest.raises(RuntimeError, match="inference"):
        m.train()(torch.zeros(1, 4, dtype=torch.long))


def test_head_workspace_does_not_scale_with_rows_or_vocabulary():
    from avec_amd import ops
    sizes = {ops.lm_head_workspace_bytes(R, V, 768) for R in (1, 512 * 66, 10 ** 7) for V in (65, 1025, 50000)}
    assert len(sizes) == 1 and sizes.pop() <= 1 << 20


def test_decoder_with_a_complete_lm_directory_constructs_on_the_cpu(tmp_path):
    code = r'''
import os, sys, warnings
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tools"))
import torch
import nnet
import make_synthetic_lm_assets as A
cfg_path = os.path.join(%r, "tests", "configs", "lm_synthetic.py")
A.write_checkpoint(A.draw_weights(A.load_config(cfg_path).model, seed=1), os.path.join(os.environ["AVEC_TEST_LM_DIR"], "lm.ckpt"))
with warnings.catch_warnings(record=True) as w:
    warnings.simplefilter("always")
    d = nnet.CTCBeamSearchDecoder(beam_size=16, ngram_path=None, neural_config_path=cfg_path, neural_checkpoint="lm.ckpt", neural_alpha=0.6, neural_beta=1.0)
    missing = nnet.CTCBeamSearchDecoder(beam_size=16, ngram_path=None, neural_config_path=cfg_path, neural_checkpoint="absent.ckpt")
msgs = [str(x.message) for x in w]
assert isinstance(d.neural_rescorer, nnet.TransformerLM) and not d.neural_rescorer.training, type(d.neural_rescorer)
assert not any(p.requires_grad for p in d.neural_rescorer.parameters())
assert (d.neural_pad_token, d.neural_sos_token, d.neural_eos_token) == (0, 256, 256) and d.neural_tokenizer is None
assert len(list(d.parameters())) == 0 and len(d.state_dict()) == 0          # the LM is not part of the decoder's module tree
ck = torch.load(os.path.join(os.environ["AVEC_TEST_LM_DIR"], "lm.ckpt"))["model_state_dict"]
assert all(torch.equal(v, ck[k]) for k, v in d.neural_rescorer.state_dict().items())
assert missing.neural_rescorer is None and sum("neural rescoring" in m for m in msgs) == 1, msgs
assert not torch.cuda.is_initialized()
print("OK")
''' % (ROOT, ROOT, ROOT)
    env = dict(os.environ, AVEC_TEST_LM_DIR=str(tmp_path))
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_rescoring_arithmetic_on_hand_made_scores():
    inf = float("inf")
    beam = torch.tensor([[-1.0, -2.0, -3.0, -inf], [-5.0, -5.0, -inf, -inf]])
    nll = torch.tensor([[10.0, 5.0, 1.0, 0.0], [2.0, 2.0, 0.0, 0.0]])
    lens = torch.tensor([[4, 4, 3, 0], [3, 3, 0, 0]])
    total, best = O.rescore(beam, nll, lens, alpha=0.5, beta=2.0)
    # beta enters squared: + 4 per scored token (len - 1)
    assert total[0].tolist() == [-1.0 - 5.0 + 12.0, -2.0 - 2.5 + 12.0, -3.0 - 0.5 + 8.0, -inf]
    assert best.tolist() == [1, 0]                       # row 1: an exact tie, the first maximum wins; empty slots never win
    assert O.rescore(torch.full((1, 3), -inf), torch.zeros(1, 3), torch.zeros(1, 3, dtype=torch.long), 0.6, 1.0)[1].tolist() == [0]


def test_decoder_host_bookkeeping_with_test_time_augmentation(monkeypatch):
    """sequence framing ([sos] + ids + [eos], pad), empty slots, ONE score call per batch and the (augmentation, beam) slot of the winner -- with the device launches
    replaced by stand-ins that do the same arithmetic on the host"""
    import nnet
    from avec_amd import ops
    B, naug, W, T = 2, 2, 3, 5
    inf = float("inf")
    tokens = torch.zeros(B * naug, W, T, dtype=torch.int32)
    out_len = torch.zeros(B * naug, W, dtype=torch.int32)
    score = torch.full((B * naug, W), -inf)
    hyp = {(0, 0): [5, 6], (0, 1): [7], (1, 0): [5, 6, 9], (2, 0): [], (3, 0): [4], (3, 1): [4, 4], (3, 2): [8]}
    for (s, w), h in hyp.items():
        tokens[s, w, :len(h)], out_len[s, w], score[s, w] = torch.tensor(h, dtype=torch.int32), len(h), -1.0 - w - 0.25 * s
    monkeypatch.setattr(ops, "ctc_beam_search", lambda *a, **k: (tokens, out_len, score, score))
    seen = []

    class FakeLM(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def score(self, ids, lengths):
            seen.append((ids.clone(), lengths.clone()))
            return torch.where(lengths > 0, 10.0 - ids.sum(1).float() / 5.0, torch.zeros(len(ids)))        # likes long hypotheses with large ids

    def rescore(model, ids, lens, beam, alpha, beta, Bn):
        neural = model.score(ids, lens)
        total, best = O.rescore(beam.view(Bn, -1), neural.view(Bn, -1), lens.view(Bn, -1), alpha, beta)
        return best, total, neural.view(Bn, -1)
    monkeypatch.setattr(ops, "lm_rescore", rescore)
    dec = nnet.CTCBeamSearchDecoder(beam_size=W, ngram_path=None, test_time_aug=True, neural_alpha=1.0, neural_beta=0.5)
    object.__setattr__(dec, "neural_rescorer", FakeLM())
    dec.neural_pad_token, dec.neural_sos_token, dec.neural_eos_token = 0, 100, 101
    got = dec.beam_search(torch.zeros(B, naug, T, 16), torch.full((B, naug), T))
    assert len(seen) == 1
    ids, lens = seen[0]
    assert ids.shape == (B * naug * W, 5) and lens.view(B * naug, W).tolist() == [[4, 3, 0], [5, 0, 0], [2, 0, 0], [3, 4, 3]]
    assert ids[0].tolist() == [100, 5, 6, 101, 0] and ids[3].tolist() == [100, 5, 6, 9, 101] and ids[6].tolist() == [100, 101, 0, 0, 0] and ids[2].tolist() == [0] * 5
    want_total, want_best = O.rescore(score.view(B, naug * W), FakeLM().score(ids, lens).view(B, naug * W), lens.view(B, naug * W), 1.0, 0.5)
    assert torch.equal(dec.last_totals, want_total)
    assert got == [[5, 6, 9], [4, 4]] and want_best.tolist() == [3, 4]       # utterance 0: augmentation 1 beam 0; utterance 1: augmentation 1 beam 1


@pytest.mark.skipif(not os.path.exists(REF_LM_CFG), reason="needs the reference tree (build container only)")
def test_reference_lm_config_imports_in_place(tmp_path):
    """the reference's own configs/LRS23/LM/GPT-Small.py, imported unchanged from a scratch directory that holds a synthetic pretrained checkpoint (~0.5 GB, temporary)"""
    run = tmp_path / "run"
    sub = os.path.join("callbacks", "LibriSpeechCorpus", "GPT-Small")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_lm_assets.py"), "--gpt-small", "--out", str(run / sub), "--name",
                    "checkpoints_epoch_13_step_512924.ckpt"], check=True, capture_output=True, timeout=900)
    code = r'''
import json, os, sys
sys.path.insert(0, %r)
import main as entry
import torch
cfg = entry.load_config(%r)
import nnet
assert type(cfg.model) is nnet.GPT and cfg.model.name == "GPT-Small", type(cfg.model)
want = json.load(open(%r))
assert {k: list(v.shape) for k, v in cfg.model.state_dict().items()} == want
ck = torch.load(cfg.pretrained_checkpoint, map_location="cpu")["model_state_dict"]
assert torch.equal(cfg.model.head.weight, ck["head.weight"])                       # the pretrained weights were loaded with strict=True
assert isinstance(cfg.model.optimizer, nnet.AdamW) and isinstance(cfg.training_dataset, nnet.datasets.CorpusLM) and len(cfg.evaluation_dataset) == 2
assert (cfg.pad_token, cfg.sos_token, cfg.eos_token, cfg.callback_path) == (0, 1024, 1024, "callbacks/LRS23/LM/GPT-Small")
print("OK")
''' % (ROOT, REF_LM_CFG, os.path.join(GOLDEN, "lm_gpt_small_keys.json"))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-B", "-c", code], cwd=str(run), capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
