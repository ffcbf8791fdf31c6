"""Chunked float64 reference of the streamed visual stem (avec_amd/csrc/video_stream.hip, nnet.VisualFrontStreamSession) and the offline stem it must equal.
Torch on the CPU only; no project code is called.

The stem: Conv3d(1 -> 64, (5,7,7), stride (1,2,2), zero pad (2,3,3), bias) -> y * scale + shift (eval-mode BatchNorm) -> ReLU -> max pool 3x3 / stride 2 / pad 1 per
frame.  Output frame t reads input frames t - 2 .. t + 2; a frame index < 0 is zero, and one >= n is zero once the utterance has ended.  With n frames heard
E(n) = max(0, n - 2) output frames exist, n at the end.  VideoFrontStream carries what the kernels carry: per slot a ring of the last 4 input frames indexed by
frame & 3 (never shifted, never cleared: it starts as NaN), a frame counter and an `ended` flag.

Layouts: video [T][H][W]; w [64][245], k = (kd * 7 + kh) * 7 + kw; stem output [frames][PH][PW][64].
"""
import torch
import torch.nn.functional as F

F64 = torch.float64
UNEVEN = (3, 0, 1, 2, 4, 1, 0, 2, 3)      # a plan of counts that includes 0, 1, 2 and 3: the ring wraps partially (for Tc = 4: every count <= Tc)
LENGTHS = (1, 2, 3, 4, 5, 6, 7, 11, 23)


def ready(n):
    """E(n): output frames that exist after n input frames of an utterance that has not ended"""
    return max(0, n - 2)


def schedule_sizes(T, Tc):
    """the session's schedule for an utterance of T frames: first_frames = Tc + 2 in the first push, chunk_frames = Tc later; the last push takes what is left"""
    sizes, at = [], 0
    while at < T:
        c = min(T - at, Tc + 2 if at == 0 else Tc)
        sizes.append(c)
        at += c
    return sizes


def uneven_sizes(T, start=0):
    """UNEVEN, cycled from `start` and cut at T frames"""
    sizes, at, i = [], 0, start
    while at < T:
        c = min(T - at, UNEVEN[i % len(UNEVEN)])
        sizes.append(c)
        at += c
        i += 1
    return sizes


def yields(sizes):
    """frames every push of a plan yields (the last one ends the utterance)"""
    out, n = [], 0
    for i, c in enumerate(sizes):
        out.append((n + c if i + 1 == len(sizes) else ready(n + c)) - ready(n))
        n += c
    return out


def stem_windows(win, w, bias, scale, shift):
    """win [n][5][H][W] (the five input frames of n output frames) -> [n][PH][PW][64]"""
    n = win.shape[0]
    if n == 0:
        H, W = win.shape[2], win.shape[3]
        return torch.zeros(0, ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1, 64, dtype=F64)
    z = F.conv3d(win[:, None].to(F64), w.to(F64).view(64, 1, 5, 7, 7), bias.to(F64), stride=(1, 2, 2), padding=(0, 3, 3))[:, :, 0]      # [n][64][OH][OW]
    y = torch.relu(z * scale.to(F64).view(1, 64, 1, 1) + shift.to(F64).view(1, 64, 1, 1))
    return F.max_pool2d(y, 3, 2, 1).permute(0, 2, 3, 1).contiguous()


def offline_stem(video, w, bias, scale, shift):
    """the whole utterance at once: video [T][H][W] -> [T][PH][PW][64], two zero frames on either side"""
    T, H, W = video.shape
    vp = torch.zeros(T + 4, H, W, dtype=F64)
    vp[2:2 + T] = video
    return stem_windows(torch.stack([vp[t:t + 5] for t in range(T)]), w, bias, scale, shift)


class VideoFrontStream:
    """B slots; push(chunks, last, reset) -> per slot the [frames][PH][PW][64] it yields.  chunks[b]: [c][H][W] (c may be 0) or None"""

    def __init__(self, B, H, W, w, bias, scale, shift):
        self.B, self.H, self.W = B, H, W
        self.k = (w, bias, scale, shift)
        self.ring = torch.full((B, 4, H, W), float("nan"), dtype=F64)
        self.n = [0] * B
        self.ended = [False] * B

    def push(self, chunks, last=(), reset=()):
        outs = []
        for b in range(self.B):
            if b in reset:
                self.n[b], self.ended[b] = 0, False                      # the ring keeps what it held: older than the counter, it counts as absent
            x = chunks[b]
            c = 0 if (x is None or self.ended[b]) else x.shape[0]
            n0 = self.n[b]
            E0 = ready(n0)
            E1 = E0 if self.ended[b] else (n0 + c if b in last else ready(n0 + c))
            zero = torch.zeros(self.H, self.W, dtype=F64)

            def frame(f):
                if f < 0:
                    return zero
                if f < n0:
                    assert f >= n0 - 4
                    return self.ring[b, f & 3]
                return x[f - n0].to(F64) if f < n0 + c else zero
            win = [torch.stack([frame(t + k - 2) for k in range(5)]) for t in range(E0, E1)]
            outs.append(stem_windows(torch.stack(win) if win else torch.zeros(0, 5, self.H, self.W, dtype=F64), *self.k))
            for i in range(max(0, c - 4), c):
                self.ring[b, (n0 + i) & 3] = x[i].to(F64)
            self.n[b] = n0 + c
            self.ended[b] = self.ended[b] or (b in last)
        return outs


def run_plan(video, sizes, k, late_last=False):
    """one utterance through a one-slot stream on the plan `sizes` -> the concatenated output; late_last: the end is announced by one more push of 0 frames"""
    T, H, W = video.shape
    s = VideoFrontStream(1, H, W, *k)
    plan = list(sizes) + ([0] if late_last else [])
    outs, at = [], 0
    for i, c in enumerate(plan):
        outs.append(s.push([video[at:at + c]], last=(0,) if i + 1 == len(plan) else ())[0])
        at += c
    assert at == T
    return torch.cat(outs)
