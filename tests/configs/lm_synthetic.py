"""A small Transformer LM in the format of the reference's LM configs (configs/LRS23/LM/GPT-Small.py): what CTCBeamSearchDecoder imports through
`neural_config_path`.  Its vocabulary covers the 256 CTC tokens of tests/configs/av_synthetic_beam.py (the decoder there returns ids, so the LM scores the very
same ids) plus one <sos>/<eos> id; the checkpoint is looked up in $AVEC_TEST_LM_DIR (tools/make_synthetic_lm_assets.py writes one)."""
import os
import tempfile

import nnet

vocab_size = 256
pad_token = 0
sos_token = vocab_size
eos_token = vocab_size
dim_model, num_blocks, num_heads, max_pos_encoding = 128, 2, 2, 256
tokenizer_path = None
callback_path = os.environ.get("AVEC_TEST_LM_DIR") or os.path.join(tempfile.gettempdir(), "avec_callbacks", "lm_synthetic")

model = nnet.TransformerLM(vocab_size=vocab_size + 1, dim_model=dim_model, num_blocks=num_blocks, num_heads=num_heads, padding_idx=pad_token,
                           max_pos_encoding=max_pos_encoding, pos_embedding=nnet.SinPosEmbedding)
model.compile(optimizer=nnet.AdamW(params=nnet.get_decay_param_groups(model, weight_decay=0.1), lr=6e-5, betas=(0.9, 0.95), eps=1e-8))
