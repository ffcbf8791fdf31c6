"""Transformer-LM (GPT) rescoring of the CTC beam on the device (avec_amd/csrc/lm.hip) through the C ABI: every kernel in fp32 against the reference's fixtures
(tests/golden/lm_*.npz) or an fp64 restatement, the fused head against the unfused path, GPT-Small dimensions in fp32 and bf16 against the fp64 oracle
(tests/lm_oracle.py), the decoder end to end against oracle beam search + oracle rescoring, the guard-page allocator, and main.py -m evaluation.

Tolerances: fp32 results within 1e-3 relative (the project's rule for logits and losses, README).  bf16 (test_gpt_small_dimensions[bf16]): the fp64 oracle evaluated
with every matrix-product operand rounded to bf16 (weights, activations, attention probabilities) is the error floor of ANY bf16-operand / fp32-accumulate
implementation of this model; the device result must stay within 4 x that floor -- the margin the project gives an implementation over its reference's own
error (tests/golden/check_oracle_fullsize.py), here for what the floor does not model: the order of the fp32 accumulations, the hardware exp, and bf16 storage of
the activations between kernels where the oracle rounds the same values once.  Measured values: see DESIGN.md section 25."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctc_beam_oracle as CO  # noqa: E402
import lm_oracle as O  # noqa: E402
import make_synthetic_lm_assets as A  # noqa: E402
import avec_amd  # noqa: E402
from avec_amd import ngram, ops  # noqa: E402
from avec_amd import runtime as rt  # noqa: E402
from tests.helpers import GOLDEN, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-3
FIXTURES = [("lm_d128_sin", None, 2), ("lm_d128_pos", "lm_d128_sin", 2), ("lm_d64_2blk", None, 1)]


@pytest.fixture(autouse=True)
def _f32():
    avec_amd.set_compute_dtype("f32")
    yield
    avec_amd.set_compute_dtype("f32")


def _fixture(name, base):
    return O.load_fixture(os.path.join(GOLDEN, name + ".npz"), None if base is None else os.path.join(GOLDEN, base + ".npz"))


def _model(sd, H, maxpos=64):
    import nnet
    V, D = sd["embedding.weight"].shape
    pos = nnet.PosEmbedding1d if "transformer.pos_embedding.pos_encoding" in sd else nnet.SinPosEmbedding
    m = nnet.TransformerLM(V, D, O.num_blocks(sd), H, padding_idx=0, max_pos_encoding=maxpos, pos_embedding=pos)
    m.load_state_dict(sd, strict=True)
    return m.eval().requires_grad_(False).cuda()


def test_embed_pos_is_bit_exact():
    g = torch.Generator().manual_seed(0)
    for N, L, V, D in ((3, 17, 65, 128), (2, 64, 1025, 768)):
        E, P = torch.randn(V, D, generator=g), torch.randn(L + 5, D, generator=g)
        ids = torch.randint(0, V, (N, L), generator=g)
        ids[0, 0], ids[-1, -1] = 0, V - 1
        got = ops.embed_pos(ids.cuda(), E.cuda(), P.cuda())
        assert got.dtype == torch.float32 and torch.equal(got.cpu(), E[ids] + P[:L])
        avec_amd.set_compute_dtype("bf16")
        got16 = ops.embed_pos(ids.cuda(), E.cuda(), P.cuda(), out_f32=False)
        avec_amd.set_compute_dtype("f32")
        assert got16.dtype == torch.bfloat16 and torch.equal(got16.cpu(), (E[ids] + P[:L]).to(torch.bfloat16))


@pytest.mark.parametrize("L", [1, 17, 32, 33, 64, 130])
def test_causal_attention_fp32(L):
    N, H, d = 3, 2, 64
    g = torch.Generator().manual_seed(L)
    qkv = torch.randn(N * L, 3 * H * d, generator=g)
    lens = torch.tensor([L, max(1, L // 2), 1])
    got = ops.causal_attention(qkv.cuda(), N, H, L, lens.cuda()).cpu().view(N, L, H, d)
    q, k, v = (t.double().view(N, L, H, d).transpose(1, 2) for t in qkv.split(H * d, dim=1))
    s = (q @ k.transpose(2, 3)) / d ** 0.5
    s = s.masked_fill(~torch.tril(torch.ones(L, L, dtype=torch.bool)), float("-inf"))
    ref = (s.softmax(-1) @ v).transpose(1, 2)
    for n in range(N):
        ln = int(lens[n])
        assert rel_err(got[n, :ln], ref[n, :ln]) < TOL, (n, rel_err(got[n, :ln], ref[n, :ln]))
    assert torch.isfinite(got).all()                       # rows past a length are defined (zeros or the padded rows' own attention), never garbage
    with pytest.raises(NotImplementedError, match="d = 64"):
        ops.causal_attention(torch.randn(4, 3 * 2 * 32).cuda(), 1, 2, 4)


def test_gelu_feed_forward_module_fp32():
    import nnet
    sd, _, _, _, _ = _fixture("lm_d128_sin", None)
    pre = "transformer.blocks.0.ff_module."
    ff = nnet.FeedForwardModule(128, 512, 0.1, "GELU", False)
    ff.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)
    ff = ff.eval().requires_grad_(False).cuda()
    x = torch.randn(5, 13, 128, generator=torch.Generator().manual_seed(3))
    got = ff.residual_forward(x.cuda(), 1.0).cpu()
    w = {k[len(pre) + 7:]: v.double() for k, v in sd.items() if k.startswith(pre)}
    h = O._ln(x.double(), w["0.weight"], w["0.bias"], 1e-6)
    ref = x.double() + O._gelu(h @ w["1.weight"].T + w["1.bias"]) @ w["4.weight"].T + w["4.bias"]
    print("gelu ffn rel err", rel_err(got, ref))
    assert rel_err(got, ref) < TOL
    assert rel_err(ff(x.cuda()).cpu(), ref - x.double()) < TOL
    with pytest.raises(RuntimeError, match="inference"):
        ff.train()(x.cuda())


def test_transformer_block_on_its_own_fp32():
    """a TransformerBlock outside a Model (no parameter arena: the Q, K, V projections are three launches into one buffer) with plain MultiHeadAttention"""
    import nnet
    from avec_amd.nnet.attentions import CausalMask
    sd, _, _, _, _ = _fixture("lm_d128_sin", None)
    pre = "transformer.blocks.0."
    blk = nnet.TransformerBlock(128, {"class": "MultiHeadAttention", "params": {"num_heads": 2, "attn_drop_rate": 0.1}})
    blk.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)
    blk = blk.eval().requires_grad_(False).cuda()
    x = torch.randn(3, 37, 128, generator=torch.Generator().manual_seed(4))
    got = blk(x.cuda(), mask=CausalMask(torch.tensor([37, 5, 20]).cuda())).cpu()
    ref = O.block({k: v.double() for k, v in sd.items()}, pre, x.double(), 2)
    for n, ln in enumerate((37, 5, 20)):
        assert rel_err(got[n, :ln], ref[n, :ln]) < TOL, (n, rel_err(got[n, :ln], ref[n, :ln]))
    with pytest.raises(NotImplementedError, match="CausalMask"):
        blk(x.cuda(), mask=None)
    with pytest.raises(RuntimeError, match="inference"):
        blk.train()(x.cuda(), mask=CausalMask())


@pytest.mark.parametrize("name,base,H", FIXTURES)
def test_forward_and_score_match_the_reference_fixtures(name, base, H):
    sd, ids, lens, logits, nll = _fixture(name, base)
    m = _model(sd, H)
    got = m(ids.cuda()).cpu()
    e = max(rel_err(got[n, :int(lens[n])], logits[n, :int(lens[n])]) for n in range(len(lens)))
    print(name, "logits rel err", e, "(whole tensor incl. pad rows: %g)" % rel_err(got, logits))
    assert e < TOL and rel_err(got, logits) < TOL
    sc = m.score(ids.cuda(), lens.cuda()).cpu()
    es = ((sc.double() - nll.double()).abs() / nll.double().abs()).max().item()
    print(name, "nll sums rel err", es)
    assert es < TOL
    # fused == unfused: forward -> host log-softmax -> gather
    assert torch.allclose(sc.double(), O.nll_sums(got.double(), ids, lens), rtol=1e-4, atol=1e-4)
    with pytest.raises(RuntimeError, match="inference"):
        m.train()(ids.cuda())
    m.eval()


@pytest.mark.parametrize("V", [65, 1024, 1025])
def test_lm_head_nll_tail_columns_and_targets(V):
    import nnet
    R, D = 77, 128
    g = torch.Generator().manual_seed(V)
    head = nnet.layers.Linear(D, V)
    with torch.no_grad():
        head.weight.copy_(torch.randn(V, D, generator=g) / D ** 0.5 * 2.0)
        head.bias.copy_(torch.randn(V, generator=g))
    head = head.requires_grad_(False).cuda()
    h = torch.randn(R, D, generator=g)
    tgt = torch.randint(0, V, (R,), generator=g)
    tgt[0], tgt[1], tgt[2], tgt[R - 1], tgt[R - 2] = 0, V - 1, -1, V - 1, 0
    got = ops.lm_head_nll(h.cuda(), head.weight, head.bias, tgt.cuda()).cpu()
    lg = h.double() @ head.weight.cpu().double().T + head.bias.cpu().double()
    ref = -lg.log_softmax(-1).gather(1, tgt.clamp_min(0)[:, None])[:, 0]
    ref[tgt < 0] = 0.0
    print("V", V, "nll rel err", rel_err(got, ref))
    assert got[2] == 0.0 and rel_err(got, ref) < TOL
    assert ops.lm_head_workspace_bytes(R, V, D) == ops.lm_head_workspace_bytes(1000 * R, V, D) == ops.lm_head_workspace_bytes(R, 65, D)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_gpt_small_dimensions(dtype):
    """N = 512 hypotheses, L <= 66, 12 x 768, V = 1025 against the fp64 oracle (evaluated on the device in fp64).  fp32: 1e-3 relative.  bf16: 4 x the floor the
    oracle gives with bf16-rounded product operands (module docstring)."""
    import nnet
    N, L, V = 512, 66, 1025
    m = A.draw_weights(nnet.GPT(vocab_size=V, padding_idx=0, model="GPT-Small", pos_embedding=nnet.SinPosEmbedding, max_pos_encoding=128), seed=5)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    lens = torch.randint(2, L + 1, (N,), generator=g)
    lens[0], lens[1] = L, 2
    ids = torch.randint(1, V - 1, (N, L), generator=g)
    ids[:, 0] = V - 1
    for n in range(N):
        ids[n, int(lens[n]) - 1] = V - 1
        ids[n, int(lens[n]):] = 0
    with torch.no_grad():
        cids = ids.cuda()
        ref = O.nll_sums(O.logits(sd, cids, 12), cids, lens).cpu()
        floor = rel_err(O.nll_sums(O.logits(sd, cids, 12, q=O.bf16_round), cids, lens).cpu(), ref) if dtype == "bf16" else 0.0
    torch.cuda.empty_cache()
    avec_amd.set_compute_dtype(dtype)
    m = m.eval().requires_grad_(False).cuda()
    got = m.score(ids.cuda(), lens.cuda()).cpu()
    err = rel_err(got, ref)
    bound = TOL if dtype == "f32" else 4.0 * floor
    print("GPT-Small %s: nll-sum rel err %.3e, bf16-operand floor %.3e, bound %.3e" % (dtype, err, floor, bound))
    assert torch.isfinite(got).all() and err < bound


def _ragged(B, T, seed):
    g = np.random.default_rng(seed)
    lens = g.integers(T // 2, T + 1, size=B)
    lens[0], lens[1 % B], lens[-1] = T, 0, 1
    return lens


E2E = dict(B=16, T=40, V=64, W=8, tmp=1.2, alpha=0.6, beta=1.0, head_std=3.0)


def _lm_dir(tmp_path, head_std):
    cfg = A.load_config(os.path.join(ROOT, "tests", "configs", "lm_synthetic.py"))
    A.write_checkpoint(A.draw_weights(cfg.model, seed=11, head_std=head_std), str(tmp_path / "lm.ckpt"))
    return cfg, {k: v.detach().clone() for k, v in cfg.model.state_dict().items()}


@pytest.mark.parametrize("with_ngram", [False, True])
@pytest.mark.parametrize("naug", [1, 2])
def test_decoder_rescoring_equals_oracle(tmp_path, monkeypatch, with_ngram, naug):
    """chosen token lists == oracle beam search + oracle rescoring on every utterance whose two best oracle totals are decidable (>= 75 % must be), and rescoring
    changes the winner at least once (otherwise the test could not tell rescoring from its absence)"""
    import nnet
    c = E2E
    monkeypatch.setenv("AVEC_TEST_LM_DIR", str(tmp_path))
    cfg, sd = _lm_dir(tmp_path, c["head_std"])
    arpa, dlm = None, None
    if with_ngram:
        arpa = str(tmp_path / "lm.arpa")
        want, _ = CO.write_random_arpa(arpa, V=c["V"], order=3, n_per_order=500, seed=2)
        dlm = CO.DictLM(want, 3, c["V"])
    dec = nnet.CTCBeamSearchDecoder(beam_size=c["W"], ngram_path=arpa, ngram_tmp=c["tmp"], ngram_alpha=0.6, ngram_beta=1.0, test_time_aug=naug > 1,
                                    neural_config_path=os.path.join(ROOT, "tests", "configs", "lm_synthetic.py"), neural_checkpoint="lm.ckpt",
                                    neural_alpha=c["alpha"], neural_beta=c["beta"])
    assert dec.neural_rescorer is not None
    calls = []
    score = dec.neural_rescorer.score
    dec.neural_rescorer.score = lambda ids, lens: (calls.append(tuple(ids.shape)), score(ids, lens))[1]
    logits = np.stack([CO.ctc_like_logits(c["B"], c["T"], c["V"], seed=70 + a) for a in range(naug)], 1)
    lens = np.stack([_ragged(c["B"], c["T"], seed=80 + a) for a in range(naug)], 1)
    tl, tn = torch.from_numpy(logits).cuda(), torch.from_numpy(lens).cuda()
    got = dec.beam_search(tl if naug > 1 else tl[:, 0], tn if naug > 1 else tn[:, 0])
    assert len(calls) == 1 and calls[0][0] == c["B"] * naug * c["W"]        # ONE scoring pass for the whole batch
    want = O.oracle_decode(logits, lens, c["W"], c["tmp"], dlm, 0.6, 1.0, sd, cfg.num_heads, c["alpha"], c["beta"], cfg.sos_token, cfg.eos_token)
    totals = dec.last_totals.cpu()
    compared = changed = 0
    for b, (toks, t1, decidable, moved) in enumerate(want):
        if not decidable:
            continue
        compared += 1
        changed += moved
        assert got[b] == toks, (b, got[b], toks)
        assert O.close(float(totals[b].max()), t1), (b, float(totals[b].max()), t1)
    print("compared %d of %d, rescoring changed the winner in %d" % (compared, c["B"], changed))
    assert compared >= 0.75 * c["B"] and changed >= 1


def test_kernels_on_the_guard_page_allocator():
    """the fused head (V = 1025: tail tile, clamped rows of W and h) and the attention kernel with the tensors' ends against unmapped pages (tools/guard)"""
    for mode in ("tail", "head"):
        env = dict(os.environ, GUARD_MODE=mode, PYTHONPATH=ROOT)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "guard", "guard_lm.py")], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "GUARD LM OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_main_evaluation_with_beam_search_and_lm_config(tmp_path):
    env = dict(os.environ, AVEC_TEST_CALLBACKS=str(tmp_path), AVEC_TEST_ARPA=str(tmp_path / "6gram.arpa"), AVEC_TEST_LM_DIR=str(tmp_path / "lm"), PYTHONPATH=ROOT)
    cfg = os.path.join("tests", "configs", "av_synthetic_beam_lm.py")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "-c", cfg, "-m", "evaluation", "--eval_steps", "2"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Evaluation:" in r.stdout and "'wer'" in r.stdout
    assert "no neural rescoring" not in r.stdout + r.stderr
