"""Test-time augmentation on the device: the clip-batch kernel (avec_video_tta_batch) and the pick kernel (avec_ctc_tta_pick) bit for bit against torch / the
oracle of tests/tta_oracle.py, the augmented VisualEfficientConformerInterCTC against plain eval forwards of the same model, CTCBeamSearchDecoder.decode_augmented
against beam_search / separate beam searches / align(), and one forward_model of the visual-only config's setup.

Tolerances.  The two kernels move bytes and compare fp32 values: torch.equal.  The augmented forward is the plain forward at another batch size: every layer works
per utterance and eval-mode BatchNorm uses its running statistics, so only the GEMM tiling may differ; the bound is the project's logit bound, 1e-3 relative
(max-norm, tests.helpers.rel_err).  decode_augmented's alignment is the same kernel on the same bytes as align(): equality."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctc_beam_oracle as CO  # noqa: E402
import tta_oracle as TO  # noqa: E402
import avec_amd  # noqa: E402
from avec_amd import ops  # noqa: E402
from avec_amd import runtime as rt  # noqa: E402
from avec_amd.lib import lib  # noqa: E402
from tests.helpers import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.fixture(autouse=True)
def _f32():
    avec_amd.set_compute_dtype("f32")
    yield
    avec_amd.set_compute_dtype("f32")


def _flip():
    from avec_amd.compat import torchvision_fallback as tv
    return tv.RandomHorizontalFlip(p=1.0)


# ---- the clip-batch kernel ----
def _clips_ref(video, n, mask):
    return torch.stack([video.flip(3) if (mask >> k) & 1 else video for k in range(n)], dim=1).flatten(0, 1)


@pytest.mark.parametrize("shape,n,mask", [((2, 3, 5, 88), 2, 0b10),        # the model's width: 16-byte path
                                          ((1, 1, 7, 7), 3, 0b110),         # odd width: scalar path, the middle column maps to itself
                                          ((3, 2, 4, 6), 1, 0),             # n = 1: a copy
                                          ((2, 1, 3, 90), 2, 0b10)])        # W % 4 == 2: scalar path
def test_video_tta_batch_equals_flip_and_interleave(shape, n, mask):
    B, T, H, W = shape
    video = torch.randn(B, T, H, W, 1, generator=torch.Generator().manual_seed(W)).cuda()
    want = _clips_ref(video, n, mask)
    if mask == 0:
        assert torch.equal(want, video.repeat_interleave(n, dim=0))
    y = torch.full((B * n, T, H, W, 1), float("nan"), device="cuda")
    lib.video_tta_batch(video.data_ptr(), y.data_ptr(), B, T * H, W, n, mask, rt.stream())
    assert torch.equal(y, want)
    assert torch.equal(ops.video_tta_batch(video, n, mask), want)


def test_video_tta_batch_more_than_one_block_and_unaligned_input():
    """(2, 9, 88, 88): 17 424 chunks per clip = 69 workgroups of 256 with a partial last one; a view 4 bytes into its storage is copied by ops, not refused"""
    B, T, H, W = 2, 9, 88, 88
    store = torch.randn(B * T * H * W + 1, generator=torch.Generator().manual_seed(3)).cuda()
    video = store[1:].view(B, T, H, W, 1)
    assert video.data_ptr() % 16 == 4
    assert torch.equal(ops.video_tta_batch(video, 2, 0b10), _clips_ref(video, 2, 0b10))


# ---- the pick kernel ----
def _pick_raw(tokens, out_len, score, n, best_slot=None):
    """avec_ctc_tta_pick on outputs pre-filled with garbage"""
    S, W, T = tokens.shape
    B = S // n
    aug, beam, ids_len = (torch.full((B,), -77, dtype=torch.int64, device="cuda") for _ in range(3))
    ids = torch.full((B, T), -77, dtype=torch.int64, device="cuda")
    sc = torch.full((B,), float("nan"), device="cuda")
    lib.ctc_tta_pick(tokens.data_ptr(), out_len.data_ptr(), score.data_ptr(), None if best_slot is None else best_slot.data_ptr(), B, n, W, T, aug.data_ptr(),
                     beam.data_ptr(), ids.data_ptr(), ids_len.data_ptr(), sc.data_ptr(), rt.stream())
    return aug, beam, ids, ids_len, sc


def _check_pick(tokens, out_len, score, n, best_slot=None):
    want = TO.pick(tokens.cpu().tolist(), out_len.cpu().tolist(), score.cpu().tolist(), n, None if best_slot is None else best_slot.cpu().tolist())
    dtypes = (torch.int64, torch.int64, torch.int64, torch.int64, torch.float32)
    for got in (_pick_raw(tokens, out_len, score, n, best_slot), ops.ctc_tta_pick(tokens, out_len, score, n, best_slot)):
        for g, w, dt in zip(got, want, dtypes):
            assert g.dtype == dt and torch.equal(g.cpu(), torch.tensor(w, dtype=dt)), (g, w)
    return want


@functools.lru_cache(maxsize=None)
def _beams(B, n, W, T, V, seed):
    """ops.ctc_beam_search on [B, n, T, V] ctc-like logits whose last augmentation (n >= 3) is a copy of augmentation 0; utterance 1 has length 0"""
    logits = np.stack([CO.ctc_like_logits(B, T, V, seed=seed + a) for a in range(n)], 1)
    lens = np.random.default_rng(seed).integers(T // 2, T + 1, size=(B, n))
    if n >= 3:
        logits[:, n - 1], lens[:, n - 1] = logits[:, 0], lens[:, 0]
    if B > 1:
        lens[1] = 0
    tokens, out_len, score, _ = ops.ctc_beam_search(torch.from_numpy(logits).cuda().flatten(0, 1), torch.from_numpy(lens).cuda().flatten(0, 1), W)
    return tokens, out_len, score


def test_ctc_tta_pick_first_maximum():
    tokens, out_len, score = _beams(3, 3, 4, 9, 16, seed=40)
    aug, beam, _, ids_len, _ = _check_pick(tokens, out_len, score, 3)
    top = score[:, 0].view(3, 3).cpu()
    assert torch.equal(top[:, 2], top[:, 0])                   # the copy ties with augmentation 0 ...
    assert all(a != 2 for a in aug) and beam == [0, 0, 0]       # ... and never wins
    assert aug == [int(np.argmax(top[b].numpy())) for b in range(3)]          # (np.argmax: the first maximum)
    assert ids_len[1] == 0 and ids_len[0] > 0                  # the utterance without frames decodes to nothing


def test_ctc_tta_pick_with_best_slot():
    tokens, out_len, score = _beams(3, 3, 4, 9, 16, seed=40)
    for slots in ([5, 11, 2], [0, 7, 9], [12, -1, 1 << 40]):     # the last: out of range on both sides, clamped
        _check_pick(tokens, out_len, score, 3, torch.tensor(slots, dtype=torch.int64).cuda())


def test_ctc_tta_pick_full_beam_single_augmentation():
    tokens, out_len, score = _beams(2, 1, 64, 12, 80, seed=50)
    _check_pick(tokens, out_len, score, 1)
    _check_pick(tokens, out_len, score, 1, torch.tensor([63, 17], dtype=torch.int64).cuda())


def test_ctc_tta_pick_all_empty_utterance():
    tokens, out_len, score = (t.clone() for t in _beams(3, 3, 4, 9, 16, seed=40))
    score[3:6] = float("-inf")                                  # utterance 1: every slot empty, stale tokens and lengths left in place
    out_len[3:6] = 5
    aug, beam, ids, ids_len, sc = _check_pick(tokens, out_len, score, 3)
    assert (aug[1], beam[1], ids_len[1], sc[1]) == (0, 0, 0, float("-inf")) and not any(ids[1])


# ---- the model ----
@functools.lru_cache(maxsize=None)
def _model_run():
    """seed-0 visual-only model in eval mode, fp32: plain forwards of the clips and of the mirrored clips (computed once, shared), then the augmented forwards"""
    import nnet
    avec_amd.set_compute_dtype("f32")
    torch.manual_seed(0)
    flip = _flip()
    model = nnet.VisualEfficientConformerInterCTC(test_augments=flip)
    model.compile(losses=None)
    model = model.to(torch.device("cuda")).eval()
    torch.manual_seed(1)
    video, vlen = torch.randn(2, 40, 88, 88, 1).cuda(), torch.tensor([40, 27]).cuda()
    out = {}
    with torch.no_grad():
        model.test_augments = None
        out["plain"], out["mirrored"] = model([video, vlen]), model([video.flip(3), vlen])
        model.test_augments = [flip]
        out["one"] = model([video, vlen])
        model.test_augments = [flip, lambda v: v.flip(-1)]
        out["two"] = model([video, vlen])
        out["clips_generic"], out["clips_native"] = model.tta_clips(video, native=False), ops.video_tta_batch(video, 3, 0b110)
        model.test_augments = [flip]
    return model, video, vlen, out


def test_model_single_flip_matches_plain_forwards():
    _, _, _, out = _model_run()
    (lg, ln), (p_lg, p_ln), (m_lg, m_ln) = out["one"]["outputs"], out["plain"]["outputs"], out["mirrored"]["outputs"]
    Tp = p_lg.shape[1]
    assert tuple(lg.shape) == (2, 2, Tp, 256) and tuple(ln.shape) == (2, 2)
    assert torch.equal(ln[:, 0], p_ln) and torch.equal(ln[:, 1], p_ln) and ln.dtype == p_ln.dtype
    e0, e1 = rel_err(lg[:, 0].float().cpu(), p_lg.float().cpu()), rel_err(lg[:, 1].float().cpu(), m_lg.float().cpu())
    print("augmented vs plain forward: unaugmented %.3g, mirrored %.3g (max-norm relative)" % (e0, e1))
    assert e0 < TOL and e1 < TOL
    print("mirrored vs plain forward: %.3g" % rel_err(m_lg.float().cpu(), p_lg.float().cpu()))
    assert not torch.equal(m_lg, p_lg)                                         # the mirrored clip is a different input
    assert lg.flatten(0, 1).data_ptr() == lg.data_ptr()                        # beam_search's flatten costs no copy
    keys = [k for k in out["plain"] if k != "outputs"]
    assert keys and sorted(out["one"]) == sorted(out["plain"])
    for k in keys:
        (i_lg, i_ln), (q_lg, q_ln) = out["one"][k], out["plain"][k]
        assert tuple(i_lg.shape) == tuple(q_lg.shape) and torch.equal(i_ln, q_ln)
        assert rel_err(i_lg.float().cpu(), q_lg.float().cpu()) < TOL, k


def test_model_two_augments_through_the_generic_path():
    _, _, _, out = _model_run()
    (lg, ln), (p_lg, p_ln), (m_lg, _) = out["two"]["outputs"], out["plain"]["outputs"], out["mirrored"]["outputs"]
    assert tuple(lg.shape) == (2, 3, p_lg.shape[1], 256) and tuple(ln.shape) == (2, 3)
    assert all(torch.equal(ln[:, k], p_ln) for k in range(3))
    assert rel_err(lg[:, 0].float().cpu(), p_lg.float().cpu()) < TOL
    for k in (1, 2):
        assert rel_err(lg[:, k].float().cpu(), m_lg.float().cpu()) < TOL, k
    assert tuple(out["clips_generic"].shape) == (6, 40, 88, 88, 1) and torch.equal(out["clips_generic"], out["clips_native"])
    for k in (k for k in out["plain"] if k != "outputs"):
        assert rel_err(out["two"][k][0].float().cpu(), out["plain"][k][0].float().cpu()) < TOL, k


def test_forward_model_of_the_visual_only_config_setup():
    """the augmented model compiled with losses=None, the beam decoder with test_time_aug=True and WordErrorRate: one evaluation forward gives a WER and a zero loss"""
    import nnet
    model, video, vlen, _ = _model_run()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dec = nnet.CTCBeamSearchDecoder(beam_size=4, test_time_aug=True)
    model.compile(losses=None, decoders={"outputs": dec}, metrics={"outputs": nnet.WordErrorRate()})
    model.built = False
    labels, llen = torch.randint(1, 256, (2, 6)).cuda(), torch.tensor([6, 4]).cuda()
    with torch.no_grad():
        losses, metrics, truths, preds = model.forward_model([video, vlen], (labels, llen))
    assert list(losses) == ["loss"] and float(losses["loss"]) == 0.0
    assert 0.0 <= metrics["wer"] and len(preds["wer"]) == 2 and truths["wer"] == [labels[0].tolist(), labels[1, :4].tolist()]


# ---- the decoder ----
DEC = dict(B=3, n=3, T=30, V=32, W=8)


@functools.lru_cache(maxsize=None)
def _dec_inputs():
    c = DEC
    logits = np.stack([CO.ctc_like_logits(c["B"], c["T"], c["V"], seed=90 + a) for a in range(c["n"])], 1)
    lens = np.random.default_rng(9).integers(c["T"] // 2, c["T"] + 1, size=(c["B"], c["n"]))
    lens[0, 0] = c["T"]
    return torch.from_numpy(logits).cuda(), torch.from_numpy(lens).cuda()


def _decoders(arpa=None, **kw):
    import nnet
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        args = dict(beam_size=DEC["W"], ngram_path=arpa, ngram_alpha=0.6, ngram_beta=1.0)
        return nnet.CTCBeamSearchDecoder(test_time_aug=True, **args, **kw), nnet.CTCBeamSearchDecoder(**args)


@pytest.mark.parametrize("with_ngram", [False, True])
def test_decode_augmented_equals_beam_search_and_names_the_winner(tmp_path, with_ngram):
    c = DEC
    arpa = None
    if with_ngram:
        arpa = str(tmp_path / "lm.arpa")
        CO.write_random_arpa(arpa, V=c["V"], order=3, n_per_order=300, seed=2)
    tta, plain = _decoders(arpa)
    logits, lens = _dec_inputs()
    ids, recs = tta.decode_augmented((logits, lens))
    assert ids == tta.beam_search(logits, lens) == [r["ids"] for r in recs]
    # the winner against three separate beam searches, one per augmentation
    tops = torch.stack([ops.ctc_beam_search(logits[:, k].contiguous(), lens[:, k], c["W"], 1.0, plain.lm(c["V"]), 0.6, 1.0)[2][:, 0] for k in range(c["n"])], 1).cpu()
    assert with_ngram == (plain.lm(c["V"]) is not None)
    assert [r["augmentation"] for r in recs] == [int(np.argmax(tops[b].numpy())) for b in range(c["B"])]          # (np.argmax: the first maximum)
    assert [r["beam"] for r in recs] == [0] * c["B"] and [r["score"] for r in recs] == [float(tops[b].max()) for b in range(c["B"])]
    assert set(recs[0]) == {"ids", "augmentation", "beam", "score"}
    # timestamps: align() of a plain decoder on the winner's augmentation, field for field (align()'s "score" is "align_score" here)
    ids_t, recs_t = tta.decode_augmented((logits, lens), timestamps=True, frame_seconds=0.04)
    assert ids_t == ids
    for b, rec in enumerate(recs_t):
        k = rec["augmentation"]
        ref = plain.align((logits[:, k].contiguous(), lens[:, k]), ids, frame_seconds=0.04)[b]
        assert {f: rec[f] for f in ("ids", "augmentation", "beam", "score")} == recs[b]
        assert rec["align_score"] == ref["score"] and ref["score"] > float("-inf") and len(rec["tokens"]) == len(ids[b])
        assert set(rec) == {"ids", "augmentation", "beam", "score", "align_score"} | (set(ref) - {"score"})
        for f in set(ref) - {"score"}:
            assert rec[f] == ref[f], (b, f)
    # n = 1 is valid
    ids1, recs1 = tta.decode_augmented((logits[:, 1:2], lens[:, 1:2]))
    assert ids1 == plain.beam_search(logits[:, 1].contiguous(), lens[:, 1]) and [r["augmentation"] for r in recs1] == [0] * c["B"]


def test_decode_augmented_with_the_neural_rescorer(tmp_path, monkeypatch):
    """the winner is the rescorer's: (augmentation, beam) = divmod(argmax of the rescored totals, W), ids = beam_search's"""
    import make_synthetic_lm_assets as A
    c = DEC
    monkeypatch.setenv("AVEC_TEST_LM_DIR", str(tmp_path))
    cfg_path = os.path.join(ROOT, "tests", "configs", "lm_synthetic.py")
    cfg = A.load_config(cfg_path)
    A.write_checkpoint(A.draw_weights(cfg.model, seed=11, head_std=3.0), str(tmp_path / "lm.ckpt"))
    tta, _ = _decoders(neural_config_path=cfg_path, neural_checkpoint="lm.ckpt", neural_alpha=0.6, neural_beta=1.0)
    assert tta.neural_rescorer is not None
    logits, lens = _dec_inputs()
    ids, recs = tta.decode_augmented((logits, lens), timestamps=True)
    best = tta.last_totals.cpu().argmax(1).tolist()
    assert [(r["augmentation"], r["beam"]) for r in recs] == [divmod(k, c["W"]) for k in best]
    assert ids == tta.beam_search(logits, lens)
    assert all(len(r["tokens"]) == len(r["ids"]) and r["align_score"] > float("-inf") for r in recs)


def test_pinned_refusals_still_raise():
    tta, _ = _decoders()
    logits, lens = _dec_inputs()
    with pytest.raises(NotImplementedError, match="test_time_aug"):
        tta.decode_with_timestamps((logits, lens))
    with pytest.raises(NotImplementedError, match="test_time_aug"):
        tta.stream(DEC["B"], DEC["T"])
