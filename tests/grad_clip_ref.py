"""Host references of the gradient-norm / clip-factor pair (csrc/loss_optim.hip: avec_grad_norm) and of the clipped Adam launch (avec_adam_step_clipped), for
tests/test_grad_clip_ref.py (which pins them to torch.nn.utils.clip_grad_norm_ and torch.optim.Adam in fp64) and tests/test_gpu_grad_clip.py."""
import math

import numpy as np
import torch

from tests import loss_optim_ref as R

EPS_CLIP = float(np.float32(1e-6))          # the 1e-6 of clip_grad_norm_, as the fp32 constant the kernel adds


def norm_ref(g, grad_scale):
    """fp64: sqrt(sum g^2) * fp32(grad_scale), every element widened before it is squared"""
    g = g.double()
    return float(torch.sqrt((g * g).sum())) * R.f32(grad_scale)


def coef_ref(norm, max_norm):
    """fp64: min(1, max_norm / (norm + 1e-6)); 1 for max_norm <= 0 or infinite (the norm-only mode) and for a norm that is not finite"""
    if not (max_norm > 0) or math.isinf(max_norm) or not math.isfinite(norm):
        return 1.0
    return min(1.0, R.f32(max_norm) / (norm + EPS_CLIP))


def coef_f32(norm32, max_norm):
    """the kernel's formula in fp32, on the norm the kernel itself produced: every operation one np.float32 operation"""
    if not (max_norm > 0) or math.isinf(max_norm) or not math.isfinite(float(norm32)):
        return np.float32(1.0)
    return np.minimum(np.float32(1.0), np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6)))


def ulp32(x):
    """spacing of fp32 at |x|"""
    return float(np.spacing(np.float32(abs(float(x)))))


def gscale_eff(grad_scale, coef32):
    """what adam_kernel multiplies the gradient by: fp32(grad_scale * coef)"""
    return float(np.float32(grad_scale) * np.float32(coef32))
