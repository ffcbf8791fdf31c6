"""tests/configs/av_synthetic_beam.py with the decoder's second half switched on: the beams are rescored by the small Transformer LM of
tests/configs/lm_synthetic.py, as the reference's LRS2/3 configs do with GPT-Small (configs/LRS23/AV/EffConfInterCTC.py:39-46).  The LM directory comes from
$AVEC_TEST_LM_DIR (a seeded checkpoint is written there when it is missing).  Used by tests/test_gpu_lm_rescore.py through main.py -m evaluation."""
import os
import sys
import tempfile

import nnet
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tools"))
import ctc_beam_oracle  # noqa: E402
import make_synthetic_lm_assets  # noqa: E402

ngram_path = os.environ.get("AVEC_TEST_ARPA") or os.path.join(tempfile.mkdtemp(), "6gram_synthetic.arpa")
if not os.path.exists(ngram_path):
    ctc_beam_oracle.write_random_arpa(ngram_path, V=256, order=6, n_per_order=2000, seed=6, extras=False)
lm_dir = os.environ.setdefault("AVEC_TEST_LM_DIR", os.path.join(tempfile.gettempdir(), "avec_callbacks", "lm_synthetic"))
lm_config = os.path.join(HERE, "lm_synthetic.py")
lm_checkpoint = "lm_synthetic.ckpt"
if not os.path.exists(os.path.join(lm_dir, lm_checkpoint)):
    make_synthetic_lm_assets.write_checkpoint(make_synthetic_lm_assets.draw_weights(make_synthetic_lm_assets.load_config(lm_config).model, seed=0),
                                              os.path.join(lm_dir, lm_checkpoint))

vocab_size = 256
loss_weights = {"v_ctc_2": 0.5 / 3, "v_ctc_5": 0.5 / 3, "a_ctc_7": 0.5 / 3, "a_ctc_10": 0.5 / 3, "f_ctc_1": 0.5 / 3, "outputs": 0.5}

batch_size = 4
accumulated_steps = 1
eval_training = False
precision = torch.bfloat16
epochs = 1
recompute_metrics = True
callback_path = os.environ.get("AVEC_TEST_CALLBACKS", os.path.join(tempfile.gettempdir(), "avec_callbacks", "av_synthetic_beam_lm"))

model = nnet.AudioVisualEfficientConformerInterCTC(vocab_size=vocab_size, v_interctc_blocks=[3, 6], a_interctc_blocks=[8, 11], f_interctc_blocks=[2])
model.compile(losses=nnet.CTCLoss(zero_infinity=True, assert_shorter=False),
              decoders={"outputs": nnet.CTCBeamSearchDecoder(beam_size=16, ngram_path=ngram_path, ngram_alpha=0.6, ngram_beta=1.0, ngram_offset=100,
                                                             neural_config_path=lm_config, neural_checkpoint=lm_checkpoint, neural_alpha=0.6, neural_beta=1.0)},
              metrics={"outputs": nnet.WordErrorRate()}, loss_weights=loss_weights)

collate_fn = nnet.CollateFn(inputs_params=[{"axis": 0, "padding": True}, {"axis": 3}, {"axis": 1, "padding": True}, {"axis": 4}],
                            targets_params=({"axis": 2, "padding": True}, {"axis": 5}))
training_dataset = nnet.datasets.LRS(batch_size=batch_size, collate_fn=collate_fn, version="LRS2", mode="pretrain+train+val", video_max_length=100,
                                     align=True, num_synthetic=12, seed=0)
evaluation_dataset = [nnet.datasets.LRS(batch_size=batch_size, collate_fn=collate_fn, version="LRS2", mode="test", num_synthetic=8, seed=1)]
