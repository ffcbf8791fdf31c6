"""Generate the Transformer-LM fixtures by running THE REFERENCE (imported via ref_shims) in the build container.  Output (data only: weights, ids, numbers, key names):
  lm_d128_sin.npz   nn.Embedding + networks.Transformer (dim 128, 2 heads of 64, 1 block, GELU, SinPosEmbedding, Mask(right_context=0)) + layers.Linear head, V = 65:
                    state_dict ("sd/<key>"), ragged ids / lengths, logits, nll sums by the literal loop of the reference decoder (nnet/decoders.py:221-231)
  lm_d128_pos.npz   the same weights under PosEmbedding1d: only the position parameter, logits and nll sums are stored (the rest is lm_d128_sin.npz)
  lm_d64_2blk.npz   dim 64, 1 head, 2 blocks (block chaining)
  lm_gpt_small_keys.json   names and shapes of the reference GPT-Small state_dict (no weights)
Run on the build machine only:  python tests/golden/make_golden_lm.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np
import torch
import ref_shims

nnet = ref_shims.import_reference()
MAXPOS, V, PAD = 64, 65, 0
LENGTHS = [2, 3, 17, 64, 40, 9]


class RefLM(torch.nn.Module):
    def __init__(self, dim_model, num_heads, num_blocks, pos_embedding):
        super().__init__()
        self.embedding = torch.nn.Embedding(V, dim_model, padding_idx=PAD)
        self.transformer = nnet.networks.Transformer(
            dim_model=dim_model, num_blocks=num_blocks, att_params={"class": "MultiHeadAttention", "params": {"num_heads": num_heads, "attn_drop_rate": 0.1}},
            ff_ratio=4, emb_drop_rate=0.1, drop_rate=0.1, act_fun="GELU", pos_embedding=pos_embedding(num_embeddings=MAXPOS, dim_emb=dim_model), inner_dropout=False,
            mask=nnet.attentions.Mask(right_context=0))
        self.head = nnet.layers.Linear(dim_model, V)

    def forward(self, ids):
        return self.head(self.transformer(self.embedding(ids)))


def draw(model, seed):
    """seeded weights with opinions: unit-variance projections, non-zero biases, LayerNorm scales away from 1 (the std-0.02 init of GPT gives a nearly uniform LM)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("pos_encoding"):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif p.dim() == 2 and name.startswith("embedding"):
                p.copy_(0.7 * torch.randn(p.shape, generator=g))
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))


def make_ids(seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(LENGTHS), max(LENGTHS)), PAD, dtype=torch.long)
    for n, ln in enumerate(LENGTHS):
        ids[n, :ln] = torch.randint(1, V, (ln,), generator=g)
    return ids


def nll_sums(logits, ids):
    neural = -logits.log_softmax(dim=-1)                                  # nnet/decoders.py:221
    out = torch.zeros(len(LENGTHS))
    for b in range(len(LENGTHS)):                                          # :226-231
        length_pred = LENGTHS[b] - 1
        for t in range(length_pred):
            out[b] += neural[b][t][ids[b][t + 1]]
    return out


def run(model, ids):
    model.eval()
    with torch.no_grad():
        logits = model(ids)
    return logits, nll_sums(logits, ids)


def save(name, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()})
    print(name, os.path.getsize(path), "bytes")


def main():
    ids = make_ids(7)
    common = {"ids": ids, "lengths": torch.tensor(LENGTHS)}
    m = RefLM(128, 2, 1, nnet.embeddings.SinPosEmbedding)
    draw(m, 1)
    logits, nll = run(m, ids)
    save("lm_d128_sin", logits=logits, nll=nll, **common, **{"sd/" + k: v for k, v in m.state_dict().items()})
    mp = RefLM(128, 2, 1, nnet.embeddings.PosEmbedding1d)
    mp.load_state_dict(m.state_dict(), strict=False)
    with torch.no_grad():
        mp.transformer.pos_embedding.pos_encoding.copy_(0.3 * torch.randn(MAXPOS, 128, generator=torch.Generator().manual_seed(2)))
    logits, nll = run(mp, ids)
    save("lm_d128_pos", logits=logits, nll=nll, **common, **{"sd/transformer.pos_embedding.pos_encoding": mp.transformer.pos_embedding.pos_encoding})
    m2 = RefLM(64, 1, 2, nnet.embeddings.SinPosEmbedding)
    draw(m2, 3)
    logits, nll = run(m2, ids)
    save("lm_d64_2blk", logits=logits, nll=nll, **common, **{"sd/" + k: v for k, v in m2.state_dict().items()})
    gpt = nnet.GPT(vocab_size=1025, padding_idx=0, model="GPT-Small", pos_embedding=nnet.SinPosEmbedding)
    with open(os.path.join(HERE, "lm_gpt_small_keys.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in gpt.state_dict().items()}, f, indent=0)


if __name__ == "__main__":
    main()
