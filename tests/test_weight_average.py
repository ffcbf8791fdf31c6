"""Checkpoint averaging (Model.average_checkpoints / Model.swa, main.py -m swa) and the EMA recursion, the parts that need no GPU.

A model without a parameter arena takes the three formulas of avec_weight_average as separate torch fp32 operations (tests/weight_average_ref.py restates them):
* swa_type="exp" is bit-identical to torch.optim.swa_utils.AveragedModel driven with the reference's avg_fn over the same checkpoints;
* swa_type="equal" is bit-identical to the mode-1 restatement, and within  4 * N * 2^-24 * max|input|  of the fp64 mean and of AveragedModel's own result (torch's
  "equal" average is a lerp whose rounding differs).  The bound: each of the N updates makes at most three roundings (difference, product, sum) of values no larger
  than the inputs, i.e. at most 3 * 2^-24 * max|input| of new error, and the errors carried from earlier updates are damped by 1 - w; N * 4 * 2^-24 * max|input|
  covers their sum.  For these inputs (N = 10, max|input| about 15) the bound is 3.6e-5 and both torch's own result and the restatement sit near 4e-7;
* buffers and model_step end as the last checkpoint's; a missing epoch raises before anything changed.
Also: the argument checks of the C entry point (made before any HIP call: the pointers below are never dereferenced), the EMA recursion (mode 2 with wa = tau,
wp = 1 - tau) against the reference's mul_ / add_ lines, Model.set_ema on a CPU model, and main.py's parser."""
import os
import sys

import pytest
import torch

from tests import weight_average_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_CKPT = 10


def _model():
    import nnet

    class Tiny(nnet.Model):
        def __init__(self):
            super().__init__(name="tiny")
            self.lin = torch.nn.Linear(37, 53)
            self.bn = torch.nn.BatchNorm1d(53)

        def forward(self, x):
            raise AssertionError("these tests never run a forward pass")

    m = Tiny()
    m.compile(losses=None, optimizer="Adam")
    return m


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    """ten checkpoints written with Model.save: parameters randn * (1 + 3 * i % 4), running_mean = i, model_step = 100 + i; -> (dir, paths, [parameter lists])"""
    d = tmp_path_factory.mktemp("swa")
    m = _model()
    g = torch.Generator().manual_seed(1234)
    paths, params = [], []
    for i in range(N_CKPT):
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (1 + 3 * i % 4))
            m.bn.running_mean.fill_(float(i))
            m.bn.num_batches_tracked.fill_(7 * i)
            m.model_step.fill_(100 + i)
        path = str(d / "checkpoints_epoch_{}_step_{}.ckpt".format(i + 1, 100 + i))
        m.save(path)
        paths.append(path)
        params.append([p.detach().clone() for p in m.parameters()])
    return str(d), paths, params


def _averaged_model(paths, **kw):
    """torch's AveragedModel over the checkpoints, loaded one by one as the reference's swa does -> its parameters"""
    from torch.optim.swa_utils import AveragedModel
    m = _model()
    swa = AveragedModel(m, **kw)
    for path in paths:
        m.load(path)
        swa.update_parameters(m)
    return [p.detach().clone() for p in swa.module.parameters()], swa


def test_exp_average_is_bit_identical_to_averaged_model_with_the_reference_lambda(ckpts):
    _, paths, _ = ckpts
    m = _model()
    m.average_checkpoints(paths, swa_type="exp", swa_decay=0.9)
    ref, _ = _averaged_model(paths, avg_fn=R.reference_exp_fn(0.9))
    for got, want in zip(m.parameters(), ref):
        assert torch.equal(got.detach(), want)


def test_equal_average_restatement_bound_buffers_and_step(ckpts):
    _, paths, params = ckpts
    m = _model()
    m.average_checkpoints(paths, swa_type="equal")
    torch_avg, swa = _averaged_model(paths)
    amax = max(float(p.abs().max()) for ps in params for p in ps)
    bound = 4 * N_CKPT * 2.0 ** -24 * amax
    worst = {"fp64": 0.0, "torch": 0.0, "torch_vs_fp64": 0.0}
    for k, got in enumerate(m.parameters()):
        got = got.detach()
        avg = None
        for i in range(N_CKPT):
            avg = R.restate(avg, params[i][k], 0) if i == 0 else R.restate(avg, params[i][k], 1, wp=1.0 / (i + 1))
        assert torch.equal(got, avg), k
        mean64 = torch.stack([params[i][k].double() for i in range(N_CKPT)]).mean(0)
        worst["fp64"] = max(worst["fp64"], float((got.double() - mean64).abs().max()))
        worst["torch"] = max(worst["torch"], float((got.double() - torch_avg[k].double()).abs().max()))
        worst["torch_vs_fp64"] = max(worst["torch_vs_fp64"], float((torch_avg[k].double() - mean64).abs().max()))
    print("equal average: max|input| %.3f bound %.3e, |got - fp64| %.3e, |got - AveragedModel| %.3e, |AveragedModel - fp64| %.3e"
          % (amax, bound, worst["fp64"], worst["torch"], worst["torch_vs_fp64"]))
    assert worst["torch_vs_fp64"] <= bound          # the reference alone is inside the bound
    assert worst["fp64"] <= bound and worst["torch"] <= bound
    # parameters only are averaged: the buffers are the last checkpoint's -- as AveragedModel(use_buffers=False) of this torch leaves them -- and so is the step
    assert torch.equal(m.bn.running_mean, torch.full((53,), float(N_CKPT - 1))) and int(m.bn.num_batches_tracked) == 7 * (N_CKPT - 1)
    assert torch.equal(swa.module.bn.running_mean, m.bn.running_mean) and int(swa.module.bn.num_batches_tracked) == int(m.bn.num_batches_tracked)
    assert int(m.model_step) == 100 + N_CKPT - 1


def test_single_checkpoint_is_copied_and_bad_type_is_refused(ckpts):
    _, paths, params = ckpts
    m = _model()
    m.average_checkpoints(paths[3:4], swa_type="exp")
    assert all(torch.equal(p.detach(), q) for p, q in zip(m.parameters(), params[3]))
    with pytest.raises(AssertionError):
        m.average_checkpoints(paths[:2], swa_type="linear")


def test_swa_missing_epoch_raises_before_the_model_changed(ckpts):
    d, _, _ = ckpts
    m = _model()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(FileNotFoundError, match="checkpoints_epoch_11_step_"):
        m.swa(None, callback_path=d, start_epoch="9", end_epoch="11")           # (the epochs arrive from argparse as strings)
    with pytest.raises(FileNotFoundError, match="checkpoints_epoch_12_step_"):
        m.swa(None, callback_path=d, start_epoch=None, end_epoch=None, epochs_list=["2", "12", "3"])
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before) and int(m.model_step) == 0
    assert not [f for f in os.listdir(d) if "swa" in f]


def test_ema_recursion_is_bit_identical_to_the_reference_lines():
    g = torch.Generator().manual_seed(7)
    for tau in (0.9, 0.999, 0.5, 0.9999):
        ema = torch.randn(4099, generator=g)
        ref = ema.clone()
        for _ in range(5):
            p = torch.randn(4099, generator=g) * 3
            ema = R.restate(ema, p, 2, wa=tau, wp=1 - tau)
            R.reference_ema_update(ref, p, tau)
            assert torch.equal(ema, ref), tau
    # and the "exp" weights the same way
    a, p = torch.randn(1000, generator=g), torch.randn(1000, generator=g)
    assert torch.equal(R.restate(a, p, 2, wa=1 - 0.9, wp=0.9), R.reference_exp_fn(0.9)(a, p, 3))


def test_set_ema_on_a_cpu_model_and_checkpoint_key(tmp_path):
    m = _model()
    keys = list(m.state_dict())
    path = str(tmp_path / "a.ckpt")
    m.save(path)
    assert torch.load(path, weights_only=False)["ema_model_state_dict"] is None                  # without set_ema: None, as before
    m.set_ema(0.9)
    ema = m.ema_model
    assert list(m.state_dict()) == keys and ema is not m and ema.arena is None and m.ema_tau == 0.9      # outside the module tree; no arena on the CPU
    assert not ema.training and not any(p.requires_grad for p in ema.parameters()) and all(p.requires_grad for p in m.parameters())
    assert ema.ema_model is None and ema.__dict__.get("optimizer") is None                       # the copy carries neither an optimizer nor an EMA model of its own
    assert all(torch.equal(p, q) and p.data_ptr() != q.data_ptr() for p, q in zip(m.parameters(), ema.parameters()))
    with torch.no_grad():
        m.bn.running_mean.fill_(3.0)
        m.lin.weight.add_(1.0)
    assert float(ema.bn.running_mean.abs().max()) == 0.0
    m.save(path)                                                                                 # save syncs the buffers, then writes the EMA state
    sd = torch.load(path, weights_only=False)["ema_model_state_dict"]
    assert list(sd) == keys and torch.equal(sd["bn.running_mean"], m.bn.running_mean) and not torch.equal(sd["lin.weight"], m.lin.weight.detach())
    m2 = _model()
    m2.set_ema(0.5)
    m2.load(path)
    assert all(torch.equal(a, b) for a, b in zip(m2.ema_model.state_dict().values(), ema.state_dict().values()))
    with pytest.raises(RuntimeError, match="Model.to"):
        m._update_ema()                                                                          # the update itself is a HIP launch over the arenas: no CPU stand-in


def test_set_ema_leaves_no_captured_step_in_either_model():
    """a captured step replays launches on the model's own buffers: the EMA copy must not get one (nor a copy of one), and the model's own whole-step graphs
    hold no EMA launch, so they go as well"""
    class Entry:
        copies = 0

        def __deepcopy__(self, memo):
            Entry.copies += 1
            return Entry()

    m = _model()
    entry, made = m.captured_steps.get_or_make(("micro", ((2, 3), "torch.float32"), "torch.float32", 2), Entry, 8, "test")
    assert made and m.captured_steps.count() == m.captured_steps.count("micro") == 1
    m.set_ema(0.9)
    assert Entry.copies == 0, "set_ema deep-copied a captured step"
    assert m.ema_model.captured_steps is not m.captured_steps
    assert m.ema_model.captured_steps.count() == 0 and m.ema_model.captured_steps.evictions == 0
    assert m.captured_steps.count() == 0
    assert m.ema_model.eager_fallback is None


def test_weight_average_argument_errors_before_any_hip_call():
    from avec_amd.lib import declared_functions, lib
    assert len(declared_functions()["avec_weight_average"][1]) == 7
    P, Q = 4096, 4096 + 4 * 1024                # non-null "pointers", 1024 floats apart
    for n in (0, -4, 1, 1022, 1023):
        with pytest.raises(RuntimeError, match="multiple of 4"):
            lib.weight_average(P, Q, 0, 0.0, 0.0, n, None)
    for a, b in ((None, Q), (P, None)):
        with pytest.raises(RuntimeError, match="weight_average"):
            lib.weight_average(a, b, 0, 0.0, 0.0, 1024, None)
    for a, b, n in ((P, P, 1024), (P, Q, 1028), (Q, P, 1028), (P, P + 16, 8)):
        with pytest.raises(RuntimeError, match="overlap"):
            lib.weight_average(a, b, 2, 0.5, 0.5, n, None)
    for mode in (-1, 3):
        with pytest.raises(RuntimeError, match="mode"):
            lib.weight_average(P, Q, mode, 0.5, 0.5, 1024, None)


def test_main_parser_accepts_swa_mode():
    sys.path.insert(0, ROOT)
    import main
    args = main.build_parser().parse_args(["-m", "swa", "--swa_epochs", "1", "3", "--swa_type", "exp"])
    assert args.mode == "swa" and args.swa_epochs == ["1", "3"] and args.swa_epochs_list is None and args.swa_type == "exp"
    args = main.build_parser().parse_args(["-m", "swa", "--swa_epochs_list", "2", "5", "9"])
    assert args.swa_epochs_list == ["2", "5", "9"] and args.swa_epochs is None and args.swa_type == "equal"
    assert "swa" in main.__doc__
