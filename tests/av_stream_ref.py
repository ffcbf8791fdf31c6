"""Host-side pieces of the audio-visual streaming tests (tests/test_av_stream_ref.py, tests/test_gpu_stream_av_fuse_kernel.py, tests/test_gpu_stream_av.py): a FIFO
reference of what avec_av_fuse_stream (avec_amd/csrc/av_stream.hip) computes, written from its semantics alone (Python lists, no ring, no project code), the joint
push schedule of the two branches with the rows each push yields, its simulation through the pairing, and the small causal audio-visual encoder the session tests run.

Arithmetic: an utterance of T video frames has 640 T - 160 samples.  The video branch (chunk Tv, stack stride S_v) and the audio branch (chunk 2 Tv stem frames, stack
stride S_a = 2 S_v) both yield R = Tv / S_v rows per regular push and ceil(T / S_v) in all, but the audio front-end looks 40 samples ahead and the video stem 2 frames.
"""
import torch

from tests import stream_front_ref as SF
from tests import video_stream_ref as VR


class FuseRef:
    """B slots; per slot two FIFOs of rows already cast to `dtype` (what the kernel's rings hold) -- push(a, a_len, v, v_len, reset, max_emit) -> (xc, pair_len)"""

    def __init__(self, B, cap, dtype):
        self.B, self.cap, self.dtype = B, cap, dtype
        self.fa, self.fv = [[] for _ in range(B)], [[] for _ in range(B)]

    def push(self, a, a_len, v, v_len, reset=(), max_emit=1):
        B, D = self.B, a.shape[2] + v.shape[2]
        xc, plen = torch.zeros(B, max_emit, D, dtype=self.dtype), []
        for b in range(B):
            if b in reset:
                self.fa[b], self.fv[b] = [], []                          # pending rows vanish
            self.fa[b] += [a[b, i].to(self.dtype) for i in range(a_len[b])]
            self.fv[b] += [v[b, i].to(self.dtype) for i in range(v_len[b])]
            assert len(self.fa[b]) <= self.cap and len(self.fv[b]) <= self.cap, "overflow: the caller's contract"
            m = min(len(self.fa[b]), len(self.fv[b]), max_emit)
            for i in range(m):
                xc[b, i] = torch.cat([self.fa[b][i], self.fv[b][i]])
            self.fa[b], self.fv[b] = self.fa[b][m:], self.fv[b][m:]
            plen.append(m)
        return xc, plen


def rows_of(frames, Tc, S):
    """rows a branch session returns for `frames` front-end frames of one push: ceil(chunk / S) from the stack's first push, ceil(tail / S) from its second"""
    return -(-min(frames, Tc) // S) + -(-max(0, frames - Tc) // S)


def audio_yields(sizes):
    """stem frames every push of an audio plan yields (the last one ends the utterance)"""
    out, n = [], 0
    for i, c in enumerate(sizes):
        out.append((((n + c) // 320 + 1) if i + 1 == len(sizes) else SF.ready(n + c)) - SF.ready(n))
        n += c
    return out


def joint_schedule(T, Ta, Tv):
    """-> per push (n_frames, n_samples, last_video, last_audio): what AudioVisualStreamSession.schedule must return"""
    v, a = VR.schedule_sizes(T, Tv), SF.schedule_sizes(Ta, 2 * Tv)
    return [(v[i] if i < len(v) else 0, a[i] if i < len(a) else 0, i == len(v) - 1, i == len(a) - 1) for i in range(max(len(v), len(a)))]


def branch_rows(T, Ta, Tv, Sv=2, Sa=4):
    """-> per push (audio rows, video rows) on the joint schedule"""
    v, a = VR.schedule_sizes(T, Tv), SF.schedule_sizes(Ta, 2 * Tv)
    rv = [rows_of(f, Tv, Sv) for f in VR.yields(v)]
    ra = [rows_of(f, 2 * Tv, Sa) for f in audio_yields(a)]
    n = max(len(rv), len(ra))
    return [(ra[i] if i < len(ra) else 0, rv[i] if i < len(rv) else 0) for i in range(n)], len(ra), len(rv)


def simulate(T, Ta, Tv, Sv=2, Sa=4):
    """one utterance through the pairing with max_emit = R and as many fuse launches per push as pairs are pending -> a record of what the session relies on"""
    R = Tv // Sv
    rows, na, nv = branch_rows(T, Ta, Tv, Sv, Sa)
    pa = pv = 0
    peak, chunks = 0, []                      # most unpaired rows a branch held; the chunk lengths the fusion stack receives, in order
    for ra, rv in rows:
        pa, pv = pa + ra, pv + rv
        peak = max(peak, pa, pv)
        first = True
        while first or min(pa, pv) > 0:
            m = min(pa, pv, R)
            pa, pv = pa - m, pv - m
            chunks.append(m)
            first = False
    fed = [m for m in chunks if m > 0]
    return {"total_a": sum(r[0] for r in rows), "total_v": sum(r[1] for r in rows), "left": (pa, pv), "peak": peak,
            "short_then_more": any(m < R for m in fed[:-1]), "pairs": sum(chunks), "pushes": (na, nv), "R": R}


ATT = lambda cls, **kw: {"class": cls, "params": dict(num_heads=4, attn_drop_rate=0.0, num_pos_embeddings=64, weight_init="default", bias_init="default", **kw)}
V_BLOCKS, A_BLOCKS, F_BLOCKS = ([1, 1], [1]), ([1, 1, 1], [2]), ([2], [1])          # (num_blocks, interctc_blocks) of the three small stacks
KEYS = ("v_ctc_0", "a_ctc_1", "f_ctc_0")


def make_av_enc(causal=True):
    """AudioVisualEfficientConformerEncoder(vocab_size=16); causal: both back-ends, the fusion module, the fusion stack and the head replaced by small causal ones at
    width 48 (Mask(left_context=6, right_context=0), K = 15 causal, one InterCTC module per stack; video stride 2, audio stride 4, fusion stride 1); seeded weights,
    running statistics that are not the identity, eval mode"""
    import nnet
    torch.manual_seed(1234)
    enc = nnet.AudioVisualEfficientConformerEncoder(vocab_size=16, v_interctc_blocks=[], a_interctc_blocks=[], f_interctc_blocks=[])
    if causal:
        conv = {"class": "Conv1d", "params": {"padding": "causal", "kernel_size": 15}}
        kw = dict(vocab_size=16, conv_params=conv, ff_ratio=4, drop_rate=0.1, conv_stride=2)
        rel, relc = ATT("RelPos1dMultiHeadAttention"), ATT("RelPos1dMultiHeadAttention", causal=True)
        enc.video_encoder.back_end = nnet.ConformerInterCTC(dim_model=[256, 48], num_blocks=V_BLOCKS[0], interctc_blocks=V_BLOCKS[1], loss_prefix="v_ctc",
                                                            att_params=[rel, relc], mask=nnet.Mask(left_context=6, right_context=0), **kw)
        enc.audio_encoder.back_end = nnet.ConformerInterCTC(dim_model=[180, 64, 48], num_blocks=A_BLOCKS[0], interctc_blocks=A_BLOCKS[1], loss_prefix="a_ctc",
                                                            att_params=[rel, relc, relc], mask=nnet.Mask(left_context=6, right_context=0), **kw)
        enc.fusion_module = nnet.FusionModule(a_dim_model=48, v_dim_model=48, f_dim_model=48)
        enc.audio_visual_encoder = nnet.ConformerInterCTC(dim_model=48, num_blocks=F_BLOCKS[0][0], interctc_blocks=F_BLOCKS[1], loss_prefix="f_ctc", att_params=relc,
                                                          mask=nnet.Mask(left_context=6, right_context=0), **kw)
        enc.head = nnet.Linear(48, 16)
    g = torch.Generator().manual_seed(99)
    for m in enc.modules():
        if hasattr(m, "running_mean") and m.running_mean is not None:
            m.running_mean.copy_(0.3 * torch.randn(m.running_mean.shape[0], generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.running_var.shape[0], generator=g))
    return enc.eval()


def host_push(ses, row, reset=None):
    """what a push does to the session's host mirrors, without a device: plan it (every refusal of a push comes from here) and commit the plan"""
    nf, ns, lv, la = [list(c) for c in zip(*row)]
    lv, la = [b for b, f in enumerate(lv) if f], [b for b, f in enumerate(la) if f]
    rmask, vplan, aplan, launches, mirrors = ses._plan(nf, ns, lv, la, reset)
    for front, plan in ((ses.video.front, vplan), (ses.audio.front, aplan)):
        front._commit(rmask, plan[1], plan[2])
        front._first = False
    ses._commit(mirrors)
    return launches
