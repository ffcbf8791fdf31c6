"""Test-time augmentation, the parts that need no GPU: the two entry points are declared and exported, their argument checks (reported before any HIP call: the
pointers below are never dereferenced), the model's constructor / compile / training refusal, the rule that tells the native flip, and the pick oracle
(tests/tta_oracle.py) on hand-written cases."""
import os
import re
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tta_oracle as O  # noqa: E402
from avec_amd.lib import HEADER, declared_functions, lib  # noqa: E402

P = 4096                                                    # a non-null, 16-byte aligned "pointer"
NEG = float("-inf")


def _batch(x=P, y=P, B=2, rows=15, W=88, n=2, mask=0b10):
    lib.video_tta_batch(x, y, B, rows, W, n, mask, None)


def _pick(tokens=P, out_len=P, score=P, best_slot=None, B=3, n=2, W=4, T=9, best_aug=P, best_beam=P, ids=P, ids_len=P, best_score=P):
    lib.ctc_tta_pick(tokens, out_len, score, best_slot, B, n, W, T, best_aug, best_beam, ids, ids_len, best_score, None)


def test_header_declares_and_library_exports_the_entry_points():
    fns = declared_functions()
    assert len(fns["avec_video_tta_batch"][1]) == 8 and len(fns["avec_ctc_tta_pick"][1]) == 14
    for name in ("avec_video_tta_batch", "avec_ctc_tta_pick"):
        assert callable(lib.raw(name))
    assert int(re.search(r"#define AVEC_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 4        # no struct changed


def test_video_tta_batch_argument_errors_before_any_hip_call():
    for ptr in ("x", "y"):
        with pytest.raises(RuntimeError, match="null pointer"):
            _batch(**{ptr: None})
    for bad, msg in ((dict(B=0), "B=0"), (dict(rows=0), "rows=0"), (dict(W=0), "W=0"), (dict(n=0, mask=0), "n=0"), (dict(n=33, mask=0), "n=33"), (dict(B=65536), "B=65536")):
        with pytest.raises(RuntimeError, match=msg):
            _batch(**bad)
    with pytest.raises(RuntimeError, match="bits at or above n=2"):
        _batch(mask=0b100)
    for ptr in ("x", "y"):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            _batch(**{ptr: P + 4})


def test_ctc_tta_pick_argument_errors_before_any_hip_call():
    for ptr in ("tokens", "out_len", "score", "best_aug", "best_beam", "ids", "ids_len", "best_score"):
        with pytest.raises(RuntimeError, match="null pointer"):
            _pick(**{ptr: None})
    for dim in ("B", "n", "W", "T"):
        with pytest.raises(RuntimeError, match="%s=0" % dim):
            _pick(**{dim: 0})
    with pytest.raises(RuntimeError, match="beyond 2\\^31"):
        _pick(B=1 << 20, n=1 << 10, W=64)
    for ptr in ("tokens", "out_len", "score", "best_score"):
        with pytest.raises(RuntimeError, match="4-byte aligned"):
            _pick(**{ptr: P + 2})
    for ptr in ("best_slot", "best_aug", "best_beam", "ids", "ids_len"):
        with pytest.raises(RuntimeError, match="8-byte aligned"):
            _pick(**{ptr: P + 4})


def test_ops_refuse_bad_arguments_on_the_host():
    from avec_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.video_tta_batch(torch.zeros(1, 2, 4, 8, 1), 2, 0b10)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ctc_tta_pick(torch.zeros(4, 2, 3, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, 2), 2)


def test_flip_recognition_rule():
    from avec_amd.compat import torchvision_fallback as tv
    from avec_amd.nnet.models_zoo import is_native_flip
    assert is_native_flip(tv.RandomHorizontalFlip(p=1.0)) and is_native_flip(tv.RandomHorizontalFlip(p=1))
    assert not is_native_flip(tv.RandomHorizontalFlip(p=0.5)) and not is_native_flip(tv.RandomHorizontalFlip())
    assert not is_native_flip(lambda v: v.flip(-1))
    assert not is_native_flip(tv.CenterCrop((88, 88)))

    class RandomHorizontalFlip:                             # any class of that name with p >= 1.0 (torchvision's own, when it is installed)
        p = 1.0
    assert is_native_flip(RandomHorizontalFlip())


def test_model_constructs_compiles_and_refuses_training():
    import nnet
    from avec_amd.compat import torchvision_fallback as tv
    flip, other = tv.RandomHorizontalFlip(p=1.0), (lambda v: v.flip(-1))
    plain = nnet.VisualEfficientConformerInterCTC()
    one = nnet.VisualEfficientConformerInterCTC(test_augments=flip)
    two = nnet.VisualEfficientConformerInterCTC(test_augments=[flip, other])
    assert plain.test_augments is None and one.test_augments == [flip] and two.test_augments == [flip, other]
    assert list(one.state_dict().keys()) == list(plain.state_dict().keys()) == list(two.state_dict().keys())
    # an explicit None means no losses; an omitted argument means CTCLoss (nnet/models_zoo.py:128-147 of the reference)
    one.compile(losses=None)
    assert one.compiled_losses == []
    plain.compile()
    assert isinstance(plain.compiled_losses, nnet.CTCLoss)
    av = nnet.AudioEfficientConformerInterCTC()
    av.compile(losses=None)
    assert av.compiled_losses == []
    # training with augments: the reference's assertion, before any device work (CPU tensors: the HIP path would refuse them with a RuntimeError)
    one.train()
    with pytest.raises(AssertionError, match="Training requires setting test_time_aug to False / test_augments to None"):
        one.forward([torch.zeros(1, 2, 88, 88, 1), torch.tensor([2])])


def test_refusals_name_decode_augmented():
    import nnet
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dec = nnet.CTCBeamSearchDecoder(beam_size=4, test_time_aug=True)
    with pytest.raises(NotImplementedError, match="test_time_aug.*decode_augmented"):
        dec.decode_with_timestamps((torch.zeros(1, 2, 3, 4), torch.ones(1, 2)))
    with pytest.raises(NotImplementedError, match="test_time_aug.*decode_augmented"):
        dec.stream(1, 8)
    with pytest.raises(ValueError, match=r"expected \[B, n, T, V\]"):
        dec.decode_augmented((torch.zeros(2, 3, 4), torch.ones(2)))


# ---- the pick oracle on hand-written cases: B = 2 utterances, n = 2 augmentations, W = 2 beams, T = 3 ----
TOK = [[[1, 2, 3], [4, 0, 0]], [[5, 6, 0], [7, 7, 7]],      # utterance 0: augmentation 0, augmentation 1
       [[9, 9, 9], [9, 9, 9]], [[8, 8, 8], [8, 8, 8]]]      # utterance 1: every slot empty (stale rows)
LEN = [[3, 1], [2, 3], [0, 0], [0, 0]]
SCO = [[-1.5, -2.0], [-1.5, -1.75], [NEG, NEG], [NEG, NEG]]


def test_oracle_tie_goes_to_the_lower_augmentation():
    aug, beam, ids, n, sc = O.pick(TOK, LEN, SCO, 2)
    assert (aug[0], beam[0], ids[0], n[0], sc[0]) == (0, 0, [1, 2, 3], 3, -1.5)
    higher = [[-1.5, -2.0], [-1.25, -1.75]] + SCO[2:]
    aug, beam, ids, n, sc = O.pick(TOK, LEN, higher, 2)
    assert (aug[0], beam[0], ids[0], n[0], sc[0]) == (1, 0, [5, 6, 0], 2, -1.25)


def test_oracle_all_empty_utterance():
    aug, beam, ids, n, sc = O.pick(TOK, LEN, SCO, 2)
    assert (aug[1], beam[1], ids[1], n[1], sc[1]) == (0, 0, [0, 0, 0], 0, NEG)


def test_oracle_best_slot_given_and_clamped():
    aug, beam, ids, n, sc = O.pick(TOK, LEN, SCO, 2, best_slot=[3, 0])
    assert (aug[0], beam[0], ids[0], n[0], sc[0]) == (1, 1, [7, 7, 7], 3, -1.75)
    aug, beam, ids, n, sc = O.pick(TOK, LEN, SCO, 2, best_slot=[1, 2])
    assert (aug[0], beam[0], ids[0], n[0]) == (0, 1, [4, 0, 0], 1)
    assert (aug[1], beam[1], ids[1], n[1], sc[1]) == (1, 0, [0, 0, 0], 0, NEG)          # an empty slot has no tokens, whatever its row holds
    aug, beam, _, _, _ = O.pick(TOK, LEN, SCO, 2, best_slot=[99, -7])
    assert (aug, beam) == ([1, 0], [1, 0])
    # out_len outside [0, T] is clamped
    _, _, ids, n, _ = O.pick(TOK, [[7, 1], [2, 3], [0, 0], [0, 0]], SCO, 2)
    assert (ids[0], n[0]) == ([1, 2, 3], 3)
