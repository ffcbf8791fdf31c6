"""The three modes of avec_weight_average (include/avec_hip.h) restated with torch fp32 tensor operations, one correctly rounded operation per line, on whatever
device the operands live; and the reference's own lines they stand for (nnet/model.py:403-405, 950).  Shared by tests/test_weight_average.py and
tests/test_gpu_weight_average.py."""
import numpy as np
import torch


def f32(x):
    """the float32 nearest to the Python float x, as a Python float (what a C `float` argument receives)"""
    return float(np.float32(x))


def restate(avg, p, mode, wa=0.0, wp=0.0):
    """-> the new average (a new tensor; `avg` and `p` are left alone).  wa / wp are rounded to fp32 first, then every product, difference and sum is its own tensor
    operation, so nothing can be contracted into an FMA."""
    if mode == 0:
        return p.clone()
    assert avg.dtype == p.dtype == torch.float32
    wa_t, wp_t = torch.tensor(f32(wa), dtype=torch.float32, device=avg.device), torch.tensor(f32(wp), dtype=torch.float32, device=avg.device)
    if mode == 1:
        d = p - avg
        d = wp_t * d
        return avg + d
    a = wa_t * avg
    b = wp_t * p
    return a + b


def reference_exp_fn(swa_decay):
    """an avg_fn for torch's AveragedModel with the arithmetic of the reference's swa_type="exp" (nnet/model.py:950): Python-float weights, the decay
    complement formed in double precision, two scalar-tensor products and their sum"""
    return lambda avg, p, n: (1 - swa_decay) * avg + swa_decay * p


def reference_ema_update(ema, p, tau):
    """the arithmetic of the reference's EMA update (nnet/model.py:404-405), in place on `ema`: scale by tau, then add (1 - tau) * p"""
    ema.mul_(tau)
    ema.add_((1 - tau) * p)
    return ema
