"""fp64 oracle of the Transformer-LM rescorer (plain torch, test infrastructure only): token embedding + positions, the causal pre-norm block stack, final
LayerNorm, head, per-sequence nll sums and the rescoring arithmetic of CTCBeamSearchDecoder.  State dicts use the key names of nnet.TransformerLM / nnet.GPT.
`q` (optional) is applied to every operand of a matrix product (weights, activations, probabilities): with q = round-to-bf16 the oracle gives the error floor of a
bf16-operand / fp32-accumulate implementation."""
import math

import torch

EPS_MODULE, EPS_FINAL = 1e-6, 1e-5        # LayerNorm eps of the attention / feed-forward modules and of the Transformer's final norm


def sin_table(n, dim, dtype=torch.float64):
    """absolute sinusoid positions: channel 2i = sin(pos / 10000^(2i / dim)), channel 2i + 1 = cos(same); evaluated in fp32 like the model's host table"""
    pos = torch.arange(n, dtype=torch.float32)[:, None]
    i = torch.arange(dim // 2, dtype=torch.float32)[None, :]
    ang = pos / 10000 ** (2 * i / dim)
    tab = torch.zeros(n, dim)
    tab[:, 0::2], tab[:, 1::2] = ang.sin(), ang.cos()
    return tab.to(dtype)


def bf16_round(t):
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _lin(x, w, b, q):
    return q(x) @ q(w).T + b


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def num_blocks(sd):
    return 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.blocks."))


def block(sd, prefix, x, num_heads, q=None):
    """one pre-norm block: x += MHSA(LN(x)) under the causal mask; x += W2 gelu(W1 LN(x)).  sd holds tensors of x's dtype / device under `prefix`"""
    q = q or (lambda t: t)
    N, L, D = x.shape
    d = D // num_heads
    keep = torch.tril(torch.ones(L, L, dtype=torch.bool, device=x.device))
    a, f = prefix + "self_att_module.", prefix + "ff_module.layers."
    h = _ln(x, sd[a + "norm.weight"], sd[a + "norm.bias"], EPS_MODULE)
    Q, K, Vv = (_lin(h, sd[a + "attention.%s_layer.weight" % n], sd[a + "attention.%s_layer.bias" % n], q).view(N, L, num_heads, d).transpose(1, 2)
                for n in ("query", "key", "value"))
    s = (q(Q) @ q(K).transpose(2, 3)) / math.sqrt(d)
    s = s.masked_fill(~keep, float("-inf"))
    o = (q(s.softmax(-1)) @ q(Vv)).transpose(1, 2).reshape(N, L, D)
    x = x + _lin(o, sd[a + "attention.output_layer.weight"], sd[a + "attention.output_layer.bias"], q)
    h = _ln(x, sd[f + "0.weight"], sd[f + "0.bias"], EPS_MODULE)
    u = _gelu(_lin(h, sd[f + "1.weight"], sd[f + "1.bias"], q))
    return x + _lin(u, sd[f + "4.weight"], sd[f + "4.bias"], q)


def hidden(sd, ids, num_heads, q=None, dtype=torch.float64):
    """rows after the final LayerNorm, [N, L, D]"""
    q = q or (lambda t: t)
    sd = {k: v.to(device=ids.device, dtype=dtype) for k, v in sd.items()}
    N, L = ids.shape
    E = sd["embedding.weight"]
    D = E.shape[1]
    pos = sd.get("transformer.pos_embedding.pos_encoding")
    if pos is None:
        pos = sin_table(L, D, dtype).to(ids.device)
    x = E[ids] + pos[:L]
    for i in range(num_blocks(sd)):
        x = block(sd, "transformer.blocks.%d." % i, x, num_heads, q)
    return _ln(x, sd["transformer.layernorm.weight"], sd["transformer.layernorm.bias"], EPS_FINAL)


def logits(sd, ids, num_heads, q=None, dtype=torch.float64):
    qq = q or (lambda t: t)
    return _lin(hidden(sd, ids, num_heads, q, dtype), sd["head.weight"].to(device=ids.device, dtype=dtype), sd["head.bias"].to(device=ids.device, dtype=dtype), qq)


def token_nll(lg, ids, lengths):
    """[N, L]: -log softmax(lg[n, t])[ids[n, t + 1]] for t < lengths[n] - 1, else 0"""
    N, L = ids.shape
    ids, lengths = ids.to(lg.device), lengths.to(lg.device)
    nxt = torch.cat([ids[:, 1:], torch.zeros(N, 1, dtype=ids.dtype, device=ids.device)], 1)
    picked = -lg.log_softmax(-1).gather(2, nxt[:, :, None])[:, :, 0]
    scored = torch.arange(L, device=lg.device)[None, :] < (lengths[:, None] - 1)
    return torch.where(scored, picked, torch.zeros_like(picked))


def nll_sums(lg, ids, lengths):
    return token_nll(lg, ids, lengths).sum(1)


def rescore(beam_score, neural, lens, alpha, beta):
    """[B, K] beam scores (higher is better, -inf = empty slot), nll sums and hypothesis lengths incl. <sos> / <eos> (0 = empty) ->
    total = beam - alpha * nll + beta^2 * (len - 1) and the FIRST maximum per row; empty slots get -inf"""
    beam_score, neural = beam_score.to(torch.float64), neural.to(torch.float64)
    total = beam_score - alpha * neural + beta * beta * (lens.to(torch.float64) - 1)
    total = torch.where((beam_score > float("-inf")) & (lens >= 1), total, torch.full_like(total, float("-inf")))
    best = []
    for row in total:
        b, bv = 0, float("-inf")
        for k, v in enumerate(row.tolist()):
            if v > bv:
                b, bv = k, v
        best.append(b)
    return total, torch.tensor(best)


def load_fixture(path, base=None):
    """-> (state_dict, ids, lengths, logits, nll sums); `base`: the fixture whose weights this one shares (lm_d128_pos.npz stores the position parameter only)"""
    import numpy as np
    z = np.load(path)
    sd = {}
    if base is not None:
        zb = np.load(base)
        sd.update({k[3:]: torch.from_numpy(zb[k]) for k in zb.files if k.startswith("sd/")})
    sd.update({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")})
    return sd, torch.from_numpy(z["ids"]), torch.from_numpy(z["lengths"]), torch.from_numpy(z["logits"]), torch.from_numpy(z["nll"])


def close(a, b):
    """the closeness rule for scores of tests/test_gpu_ctc_beam.py"""
    return abs(a - b) <= 1e-4 * abs(b) + 1e-5


def oracle_decode(logits, lens, W, tmp, dlm, ngram_alpha, ngram_beta, sd, num_heads, alpha, beta, sos, eos, pad=0, gap_min=1e-4):
    """Oracle beam search (tests/ctc_beam_oracle.py) + oracle rescoring for logits [B, naug, T, V] (numpy), lens [B, naug].
    -> per utterance (winning token list, best total, decidable, rescoring changed the winner): `decidable` is False when the two best totals are within gap_min
    or within the closeness rule of each other (a device implementation may then legitimately pick either)."""
    import ctc_beam_oracle as CO
    B, naug = logits.shape[:2]
    slots = []                                             # per utterance: naug * W entries (tokens, beam score) or None
    for b in range(B):
        row = []
        for a in range(naug):
            beams, _ = CO.beam_search(CO.log_softmax64(logits[b, a], tmp), lens[b, a], W, lm=dlm, alpha=ngram_alpha, beta=ngram_beta)
            row += [(list(t), float(s)) for t, s, _ in beams] + [None] * (W - len(beams))
        slots.append(row)
    K = naug * W
    Lmax = 2 + max(len(s[0]) for row in slots for s in row if s is not None)
    ids = torch.full((B * K, Lmax), pad, dtype=torch.long)
    ln = torch.zeros(B * K, dtype=torch.long)
    beam = torch.full((B * K,), float("-inf"), dtype=torch.float64)
    for b, row in enumerate(slots):
        for k, s in enumerate(row):
            if s is not None:
                seq = [sos] + s[0] + [eos]
                ids[b * K + k, :len(seq)] = torch.tensor(seq)
                ln[b * K + k], beam[b * K + k] = len(seq), s[1]
    neural = nll_sums(logits_fn(sd, ids, num_heads), ids, ln)
    total, best = rescore(beam.view(B, K), neural.view(B, K), ln.view(B, K), alpha, beta)
    out = []
    for b in range(B):
        t = sorted(total[b].tolist(), reverse=True)
        t1, t2 = t[0], (t[1] if K > 1 else float("-inf"))
        decidable = t2 == float("-inf") or (t1 - t2 > gap_min and not close(t2, t1))
        k = int(best[b])
        ngram_best = max(range(K), key=lambda j: (slots[b][j][1] if slots[b][j] is not None and j % W == 0 else float("-inf"), -j))
        out.append((slots[b][k][0], t1, decidable, slots[b][k][0] != slots[b][ngram_best][0]))
    return out


logits_fn = logits
