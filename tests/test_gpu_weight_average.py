"""GPU (-m gpu): weight averaging on the flat fp32 arenas -- the avec_weight_average kernel through the C ABI, Model.average_checkpoints / Model.swa on a model with an
arena, and the EMA model of Model.set_ema in eager and captured steps.

Kernel.  The three modes are defined by their exact sequence of correctly rounded fp32 operations, so the reference is the same three lines evaluated with torch fp32
tensors ON THE DEVICE, one tensor operation per rounding (tests/weight_average_ref.py; tests/test_weight_average.py pins mode 2 to the reference's own lines on the
host), and the comparison is torch.equal.  `avg` and `p` are carved out of one allocation filled with a NaN pattern (tests/test_gpu_rowwise.py: Carve): the gaps must
stay intact and no NaN may reach the result.  Sizes: one element group, one short of / exactly / one past a 256-thread block's 1024 elements, and one element group
past the 8192-block cap (the grid-stride loop's second trip).

Model.  No model the GPU tests build has a parameter whose element count is not a multiple of 4 (every arena offset would be a multiple of 4 without any padding), so
the smallest one with BatchNorm layers -- the audio-only Efficient Conformer without InterCTC heads, as tests/test_gpu_round2.py builds it -- gets two unused
parameters of 7 and 15 elements in front of all others: every later offset moves by the padding.  The checkpoints are written once per module from CPU models, and the
CPU result of average_checkpoints (the plain torch path, itself pinned to torch's AveragedModel by tests/test_weight_average.py) is computed once and shared."""
import os

import pytest
import torch

from tests import weight_average_ref as R
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

N_CKPT = 4
TAU = 0.9


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_mode():
    import avec_amd
    avec_amd.set_compute_dtype("f32")
    yield
    avec_amd.set_compute_dtype("f32")


# ----------------------------------------------------------------------------------------------
# the kernel, through the C ABI
# ----------------------------------------------------------------------------------------------
SIZES = [4, 1020, 1024, 1028, 8192 * 1024 + 4]
MODES = [(0, 0.0, 0.0), (1, 0.0, 1.0 / 3), (1, 123.0, 1.0 / 10), (2, TAU, 1 - TAU), (2, 1 - 0.9, 0.9), (2, 0.9999, 1 - 0.9999)]       # (mode, wa, wp); mode 1 ignores wa


@pytest.mark.parametrize("n", SIZES)
def test_kernel_is_bit_identical_to_the_fp32_restatement(n):
    from avec_amd import runtime as rt
    from avec_amd.lib import lib
    from tests.test_gpu_rowwise import Carve
    g = torch.Generator().manual_seed(n)
    a0 = (torch.randn(n, generator=g) * torch.logspace(-3, 3, 7)[torch.randint(0, 7, (n,), generator=g)]).to(dev())
    p0 = (torch.randn(n, generator=g) * torch.logspace(-3, 3, 7)[torch.randint(0, 7, (n,), generator=g)]).to(dev())
    for mode, wa, wp in MODES:
        c = Carve([(n, "f32"), (n, "f32")])
        avg, p = c.views
        if mode != 0:
            avg.copy_(a0)                        # (mode 0 must overwrite every element of the NaN pattern)
        p.copy_(p0)
        lib.weight_average(avg.data_ptr(), p.data_ptr(), mode, wa, wp, n, rt.stream())
        want = R.restate(a0, p0, mode, wa, wp)
        assert not bool(torch.isnan(avg).any()), (n, mode)
        assert torch.equal(avg, want), (n, mode, wa, wp, float((avg - want).abs().max()))
        assert torch.equal(p, p0) and c.intact(), (n, mode)
    # these inputs tell the two-rounding form from a contracted one: fma(wa, avg, round(wp * p)), evaluated in fp64 (the product of two fp32 values is exact there)
    if n >= 1020:
        fused = (R.f32(TAU) * a0.double() + (R.f32(1 - TAU) * p0.double()).float().double()).float()
        assert not torch.equal(fused, R.restate(a0, p0, 2, TAU, 1 - TAU))


def test_ops_wrapper_and_rejections_before_any_launch():
    from avec_amd import ops, runtime as rt
    from avec_amd.lib import lib
    from tests.test_gpu_rowwise import Carve
    c = Carve([(1024, "f32"), (1024, "f32")])
    avg, p = c.views
    st = rt.stream()
    for n in (1023, 1022, 1, 0, -4):
        with pytest.raises(RuntimeError, match="multiple of 4"):
            lib.weight_average(avg.data_ptr(), p.data_ptr(), 2, 0.5, 0.5, n, st)
    for a, b in ((None, p.data_ptr()), (avg.data_ptr(), None)):
        with pytest.raises(RuntimeError, match="weight_average"):
            lib.weight_average(a, b, 2, 0.5, 0.5, 1024, st)
    for a, b, n in ((avg.data_ptr(), avg.data_ptr(), 1024), (avg.data_ptr(), avg.data_ptr() + 16, 8), (avg.data_ptr() + 16, avg.data_ptr(), 8)):
        with pytest.raises(RuntimeError, match="overlap"):
            lib.weight_average(a, b, 2, 0.5, 0.5, n, st)
    with pytest.raises(RuntimeError, match="mode"):
        lib.weight_average(avg.data_ptr(), p.data_ptr(), 3, 0.5, 0.5, 1024, st)
    with pytest.raises(RuntimeError):
        ops.weight_average(avg, p[:1020], 2, 0.5, 0.5)
    with pytest.raises(RuntimeError):
        ops.weight_average(avg, p.cpu(), 2, 0.5, 0.5)
    torch.cuda.synchronize()
    assert c.untouched()                         # nothing was launched
    a0, p0 = torch.randn(1024).to(dev()), torch.randn(1024).to(dev())
    avg.copy_(a0)
    p.copy_(p0)
    assert ops.weight_average(avg, p, 2, TAU, 1 - TAU) is avg
    assert torch.equal(avg, R.restate(a0, p0, 2, TAU, 1 - TAU)) and c.intact()


# ----------------------------------------------------------------------------------------------
# models
# ----------------------------------------------------------------------------------------------
class _NoAugment(torch.nn.Module):
    """stands in for SpecAugment (no parameters, no buffers: the state_dict is unchanged) where a test replays training-mode passes"""

    def forward(self, samples, lengths):
        return samples


def _ao_model(seed, device=None, augment=False):
    """the audio-only model of tests/test_gpu_round2.py (dropout off) with two unused parameters of 7 and 15 elements at the head of the arena"""
    import nnet

    class PaddedAO(nnet.AudioEfficientConformerInterCTC):
        def __init__(self):
            super().__init__(vocab_size=256, att_type="patch", interctc_blocks=[])
            self.odd_a = torch.nn.Parameter(torch.randn(7))
            self.odd_b = torch.nn.Parameter(torch.randn(3, 5))

    torch.manual_seed(seed)
    model = PaddedAO()
    for x in model.modules():
        if isinstance(x, torch.nn.Dropout):
            x.p = 0.0
        if hasattr(x, "drop_rate"):
            x.drop_rate = 0.0
    if not augment:
        model.encoder.spec_augment = _NoAugment()
    model.compile(losses=nnet.CTCLoss(zero_infinity=True, assert_shorter=False))
    return model if device is None else model.to(device)


def _ao_batch(seed=3):
    g = torch.Generator().manual_seed(seed)
    audio, alen = 0.1 * torch.randn(2, 16000, generator=g), torch.tensor([16000, 12000])
    labels, llen = torch.randint(1, 256, (2, 5), generator=g), torch.tensor([5, 3])
    return [audio.to(dev()), alen.to(dev())], (labels.to(dev()), llen.to(dev()))


class _Loader:
    """a data loader as Model.evaluate / Model.swa see one: iterable, with a length (a plain list would be read as a list of evaluation sets)"""

    def __init__(self, batches):
        self.batches = batches

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def _pad_mask(arena):
    """True at the arena elements that belong to no parameter"""
    mask = torch.ones(arena.numel, dtype=torch.bool, device=arena.master.device)
    for p, o in zip(arena.params, arena.offsets):
        mask[o:o + p.numel()] = False
    return mask


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    """four checkpoints of differently seeded models (running statistics and counters set apart as well), written from the CPU; and the CPU averages of both types.
    -> (directory, paths, {swa_type: {name: tensor}}, last checkpoint's state_dict)"""
    d = tmp_path_factory.mktemp("swa_gpu")
    paths, last = [], None
    for i in range(N_CKPT):
        m = _ao_model(seed=20 + i)
        g = torch.Generator().manual_seed(100 + i)
        with torch.no_grad():
            for k, b in m.named_buffers():
                if k.endswith("running_mean"):
                    b.copy_(0.1 * torch.randn(b.shape, generator=g))
                elif k.endswith("running_var"):
                    b.copy_(1.0 + 0.2 * torch.rand(b.shape, generator=g))
                elif k.endswith("num_batches_tracked"):
                    b.fill_(10 + i)
            m.model_step.fill_(50 * (i + 1))
        paths.append(str(d / "checkpoints_epoch_{}_step_{}.ckpt".format(i + 1, 50 * (i + 1))))
        m.save(paths[-1])
        last = {k: v.clone() for k, v in m.state_dict().items()}
    cpu = {}
    m = _ao_model(seed=1)
    for swa_type in ("equal", "exp"):
        m.average_checkpoints(paths, swa_type=swa_type, swa_decay=0.9)
        cpu[swa_type] = {k: v.detach().clone() for k, v in m.named_parameters()}
    return str(d), paths, cpu, last


def test_padded_model_has_arena_padding():
    m = _ao_model(seed=0, device=dev())
    odd = [p.numel() for p in m.arena.params if p.numel() % 4]
    assert len(odd) >= 2 and m.arena.offsets[:3] == [0, 8, 24] and int(_pad_mask(m.arena).sum()) == 2
    assert sum(k.endswith("running_mean") for k, _ in m.named_buffers()) > 10           # BatchNorm layers


@pytest.mark.parametrize("swa_type", ["equal", "exp"])
def test_average_checkpoints_matches_the_cpu_result_and_reaches_the_forward_pass(ckpts, swa_type):
    d, paths, cpu, last = ckpts
    inputs, _ = _ao_batch()
    m = _ao_model(seed=2, device=dev()).eval()
    m.load(paths[-1])
    with torch.no_grad():
        y_last = m(inputs)["outputs"][0].float().clone()
    m.average_checkpoints(paths, swa_type=swa_type, swa_decay=0.9)
    for k, p in m.named_parameters():
        assert torch.equal(p.detach().cpu(), cpu[swa_type][k]), k
    assert float(m.arena.master[_pad_mask(m.arena)].abs().max()) == 0.0            # the padding elements are still zero
    assert int(m.model_step) == 50 * N_CKPT
    for k, b in m.named_buffers():
        assert torch.equal(b.cpu(), last[k]), k                                    # buffers: the last checkpoint's
    with torch.no_grad():
        y_avg = m(inputs)["outputs"][0].float().clone()                            # (the weight shadows must have been refreshed from the averaged masters)
    assert torch.isfinite(y_avg).all() and rel_err(y_avg, y_last) > 1e-2
    path = os.path.join(d, "checkpoints_swa-{}-1-{}.ckpt".format(swa_type, N_CKPT))
    m.save(path, save_optimizer=False)
    f = _ao_model(seed=3, device=dev()).eval()
    f.load(path)
    assert torch.equal(f.arena.master, m.arena.master)
    with torch.no_grad():
        y_file = f(inputs)["outputs"][0].float()
    assert rel_err(y_file, y_avg) <= 1e-5         # same weights, statistics, input and kernels: only the order of fp32 atomic sums may differ
    os.remove(path)


def _refresh_pass(model, inputs):
    """one BatchNorm-refresh step as Model.swa makes it"""
    import nnet
    from avec_amd import runtime as rt
    rt.set_compute_dtype(torch.float32)
    rt.reset_zero_pool(model.device)
    nnet.Model._pre_forward(model, None)
    with torch.no_grad():
        model.forward(inputs)
    rt.advance_rng(model.device)


def test_swa_end_to_end(ckpts):
    from avec_amd import runtime as rt
    d, paths, cpu, last = ckpts
    batches = [{"inputs": _ao_batch(seed=s)[0]} for s in (3, 4)]                   # two batches, three steps: the loop wraps around as the reference's while loop
    m = _ao_model(seed=4, device=dev())
    rng0 = int(rt.rng_state(dev())[1])
    m.swa(_Loader(batches), callback_path=d, start_epoch="1", end_epoch=str(N_CKPT), update_steps=3, swa_type="equal", precision=torch.float32)
    assert m.training and int(rt.rng_state(dev())[1]) == rng0 + 3                   # the step counter of the RNG moved: other masks on every pass
    for k, p in m.named_parameters():
        assert torch.equal(p.detach().cpu(), cpu["equal"][k]), k                   # the refresh changed no parameter
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    changed = 0
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(last[k]) + 3 == 10 + N_CKPT - 1 + 3, k
        elif k.endswith(("running_mean", "running_var")):
            changed += int(not torch.equal(v.cpu(), last[k]))
            assert torch.isfinite(v).all(), k
    assert changed == sum(k.endswith(("running_mean", "running_var")) for k in sd) > 0
    # manual replay: the average (parameters) and the last checkpoint's buffers in a fresh model, three training-mode passes on the same batches
    f = _ao_model(seed=5, device=dev())
    f.load_state_dict(dict(last, **cpu["equal"]))
    f.train()
    for i in range(3):
        _refresh_pass(f, batches[i % 2]["inputs"])
    worst = 0.0
    for k, v in f.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            worst = max(worst, rel_err(sd[k], v))
    print("swa: running statistics against the manual replay, worst max-norm relative error %.3e" % worst)
    assert worst <= 1e-3
    path = os.path.join(d, "checkpoints_swa-equal-1-{}.ckpt".format(N_CKPT))
    assert os.path.exists(path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["optimizer_state_dict"] is None and ck["ema_model_state_dict"] is None and int(ck["model_step"]) == 50 * N_CKPT
    f.load(path, strict=True)
    for k, v in f.state_dict().items():
        assert torch.equal(v, sd[k]), k
    os.remove(path)


# ----------------------------------------------------------------------------------------------
# the EMA model
# ----------------------------------------------------------------------------------------------
def _recursion(e0, snaps, tau):
    want = e0
    for s in snaps:
        want = R.restate(want, s, 2, wa=tau, wp=1 - tau)
    return want


def test_ema_eager_steps_accumulation_buffers_evaluate_and_checkpoint(tmp_path, capsys):
    inputs, targets = _ao_batch()
    m = _ao_model(seed=6, device=dev()).train()
    keys = list(m.state_dict())
    plain = str(tmp_path / "plain.ckpt")
    m.save(plain)
    assert torch.load(plain, map_location="cpu", weights_only=False)["ema_model_state_dict"] is None           # without set_ema the file holds None, as before
    m.set_ema(TAU)
    ema = m.ema_model
    assert list(m.state_dict()) == keys and list(ema.state_dict()) == keys
    assert ema.arena is not m.arena and ema.arena.offsets == m.arena.offsets and torch.equal(ema.arena.master, m.arena.master)
    assert ema.arena.master.data_ptr() != m.arena.master.data_ptr() and not ema.training and not any(p.requires_grad for p in ema.parameters())
    assert all(p.data_ptr() == ema.arena.master.data_ptr() + 4 * o for p, o in zip(ema.arena.params, ema.arena.offsets))
    # three optimizer steps
    e0, snaps = ema.arena.master.clone(), []
    for _ in range(3):
        m.train_step(inputs, targets, precision=torch.float32)
        snaps.append(m.arena.master.clone())
    assert not torch.equal(snaps[0], e0) and not torch.equal(snaps[2], snaps[1])
    assert torch.equal(ema.arena.master, _recursion(e0, snaps, TAU))
    assert float(ema.arena.master[_pad_mask(ema.arena)].abs().max()) == 0.0
    # accumulated_steps = 2 over four micro-steps: exactly two updates, after the second and the fourth
    e1, snaps, acc = ema.arena.master.clone(), [], 0
    for i in range(4):
        before = ema.arena.master.clone()
        _, _, acc = m.train_step(inputs, targets, precision=torch.float32, accumulated_steps=2, acc_step=acc)
        if i % 2 == 0:
            assert acc == 1 and torch.equal(ema.arena.master, before)
        else:
            assert acc == 0 and not torch.equal(ema.arena.master, before)
            snaps.append(m.arena.master.clone())
    assert int(m.model_step) == 5 and torch.equal(ema.arena.master, _recursion(e1, snaps, TAU))
    # buffers: the model's, from sync_ema_buffers() on
    stale = sum(int(not torch.equal(a, b)) for a, b in zip(ema.buffers(), m.buffers()))
    assert stale > 0
    assert m.sync_ema_buffers() is ema and all(torch.equal(a, b) for a, b in zip(ema.buffers(), m.buffers()))
    # evaluation of the EMA model: its own weights (through its own refreshed shadows), hence another loss
    data = _Loader([{"inputs": inputs, "targets": targets}])
    l_ema, l_model = ema.evaluate(data)["loss"], m.evaluate(data)["loss"]
    m.train()
    assert l_ema == l_ema and l_model == l_model and abs(l_ema - l_model) > 1e-6 * abs(l_model), (l_ema, l_model)
    # checkpoint round trip
    path = str(tmp_path / "ema.ckpt")
    m.train_step(inputs, targets, precision=torch.float32)                         # (the buffers move once more: save() must sync them itself)
    m.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=False)["ema_model_state_dict"]
    assert list(sd) == keys
    m2 = _ao_model(seed=7, device=dev())
    m2.set_ema(0.5)
    m2.load(path)
    assert torch.equal(m2.ema_model.arena.master, ema.arena.master) and torch.equal(m2.arena.master, m.arena.master)
    assert all(torch.equal(a, b) for a, b in zip(m2.ema_model.buffers(), m.buffers()))
    with torch.no_grad():
        y_a, y_b = ema(inputs)["outputs"][0].float(), m2.ema_model(inputs)["outputs"][0].float()              # the loaded EMA weights reach its forward pass
    assert rel_err(y_b, y_a) <= 1e-5
    m3 = _ao_model(seed=8, device=dev())
    m3.load(path)                                                                  # a model without EMA ignores the entry
    assert m3.ema_model is None and torch.equal(m3.arena.master, m.arena.master)
    # fit: where the model is evaluated, the EMA model is evaluated after it (buffers synced first) and its results are printed
    capsys.readouterr()
    m.fit(data, epochs=1, dataset_eval=data, eval_steps=1, steps_per_epoch=1, precision=torch.float32, eval_training=False)
    assert "epoch 1 ema eval: {'loss': " in capsys.readouterr().out
    assert all(torch.equal(a, b) for a, b in zip(ema.buffers(), m.buffers()))


def test_ema_inside_the_captured_step():
    """the EMA launch follows the optimizer launch INSIDE the hipGraph: three replays against the mode-2 recursion over the masters each replay leaves.  The model,
    precision and batch are those of the captured-step test of tests/test_gpu_round3.py; the process keeps the hardware-queue count it was started with."""
    import nnet
    from tests.test_gpu_round3 import _small_av_batch
    inputs, targets = _small_av_batch(2, (0.9, 0.7), 1)
    torch.manual_seed(0)
    model = nnet.AudioVisualEfficientConformerInterCTC()
    for x in model.modules():
        if isinstance(x, torch.nn.Dropout):
            x.p = 0.0
        if hasattr(x, "drop_rate"):
            x.drop_rate = 0.0
    model.compile(losses=nnet.CTCLoss(zero_infinity=True, assert_shorter=False))
    model = model.to(dev()).train()
    model.encoder.audio_encoder.spec_augment.eval()
    model.set_ema(TAU)
    ema = model.ema_model
    assert ema.arena.offsets == model.arena.offsets
    init = model.arena.master.clone()
    step = model.make_graphed_train_step(inputs, targets, precision=torch.float32, warmup=1)          # one eager step (with its EMA update), then the capture
    warm = model.arena.master.clone()
    assert torch.equal(ema.arena.master, _recursion(init, [warm], TAU))
    e0, snaps = ema.arena.master.clone(), []
    for _ in range(3):
        step()
        snaps.append(model.arena.master.clone())
    torch.cuda.synchronize()
    assert int(model.model_step) == 4 and not torch.equal(snaps[2], snaps[1]) and not torch.equal(snaps[0], warm)
    assert torch.equal(ema.arena.master, _recursion(e0, snaps, TAU))
    assert ema.arena.dirty                      # whatever evaluates the EMA model next refreshes its weight shadows first


def test_set_ema_before_and_after_placement_and_compile():
    import nnet
    a = _ao_model(seed=9)                       # compiled, on the CPU
    a.set_ema(TAU)
    assert a.ema_model.arena is None
    a = a.to(dev())                             # Model.to carries the EMA model along
    b = _ao_model(seed=9, device=dev())
    b.set_ema(TAU)
    torch.manual_seed(9)
    c = nnet.AudioEfficientConformerInterCTC(vocab_size=256, att_type="patch", interctc_blocks=[])
    c.set_ema(TAU)                              # before compile
    c.compile(losses=nnet.CTCLoss(zero_infinity=True, assert_shorter=False))
    c = c.to(dev())
    for m in (a, b, c):
        e = m.ema_model
        assert e.arena is not None and e.arena is not m.arena and e.arena.offsets == m.arena.offsets and e.arena.numel == m.arena.numel
        assert e.device == m.device and torch.equal(e.arena.master, m.arena.master) and e.arena.master.data_ptr() != m.arena.master.data_ptr()
        assert [tuple(p.shape) for p in e.arena.params] == [tuple(p.shape) for p in m.arena.params]
    assert a.ema_model.arena.offsets == b.ema_model.arena.offsets and torch.equal(a.ema_model.arena.master, b.ema_model.arena.master)
    inputs, targets = _ao_batch()
    for m in (a, c):                            # and the update runs on each of them
        e0 = m.ema_model.arena.master.clone()
        m.train().train_step(inputs, targets, precision=torch.float32)
        assert torch.equal(m.ema_model.arena.master, _recursion(e0, [m.arena.master], TAU)) and not torch.equal(m.arena.master, e0)
