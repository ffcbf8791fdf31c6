"""Synthetic assets for the Transformer-LM rescorer (beside make_synthetic_assets.py): a seeded checkpoint in the format Model.load reads, for any model of an LM
config.  The released LM checkpoints and tokenizers are not available offline; nothing is downloaded.

    python tools/make_synthetic_lm_assets.py --config tests/configs/lm_synthetic.py --out DIR [--name lm_synthetic.ckpt] [--seed 0] [--head-std 1.0]
    python tools/make_synthetic_lm_assets.py --gpt-small --out DIR          (nnet.GPT GPT-Small, vocabulary 1025: a ~500 MB file, for a scratch directory only)

No tokenizer is written: a 1024-piece sentencepiece model cannot be trained from the synthetic label ids (they are random integers, not text); configs that need
one keep the decoder without a tokenizer, where the LM scores the decoder's own ids."""
import argparse
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def draw_weights(model, seed=0, head_std=1.0):
    """Seeded weights that give the LM opinions (GPT's own std-0.02 init is a nearly uniform LM): fan-in-scaled projections, the head at `head_std` times that,
    non-zero biases, LayerNorm scales away from 1."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            r = torch.randn(p.shape, generator=g)
            if name.endswith("pos_encoding"):
                p.copy_(0.3 * r)
            elif name.startswith("embedding"):
                p.copy_(0.7 * r)
            elif name == "head.weight":
                p.copy_(head_std * r / p.shape[1] ** 0.5)
            elif p.dim() == 2:
                p.copy_(r / p.shape[1] ** 0.5)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * r)
            else:
                p.copy_(0.1 * r)
    return model


def write_checkpoint(model, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save({"model_state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, "optimizer_state_dict": None, "model_step": 0,
                "is_distributed": False, "ema_model_state_dict": None, "grad_scaler_state_dict": None}, path)
    return path


def load_config(path):
    spec = importlib.util.spec_from_file_location("avec_lm_config", path)
    cfg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cfg)
    return cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config")
    ap.add_argument("--gpt-small", action="store_true")
    ap.add_argument("--out", required=True)
    ap.add_argument("--name", default="lm_synthetic.ckpt")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--head-std", type=float, default=1.0)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import nnet
    if args.gpt_small:
        model = nnet.GPT(vocab_size=1025, padding_idx=0, model="GPT-Small", pos_embedding=nnet.SinPosEmbedding)
    else:
        model = load_config(args.config).model
    print(write_checkpoint(draw_weights(model, args.seed, args.head_std), os.path.join(args.out, args.name)))


if __name__ == "__main__":
    main()
