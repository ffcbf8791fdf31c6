"""Optimizers (nnet/optimizers.py).  Adam keeps torch.optim.Adam's state_dict format (+ "model_step") but steps the whole model with ONE
HIP launch over the flat fp32 arenas (the reference's single-tensor path issues ~15k ATen ops per step)."""
import torch
import torch.optim as optim

from .. import ops
from .. import runtime as rt
from ..lib import lib
from . import schedulers


class Adam(optim.Adam):
    """nnet/optimizers.py:61-93: lr read from the scheduler before every update (model_step incremented first), coupled L2 weight decay."""

    def __init__(self, params, lr=0.001, betas=(0.9, 0.999), eps=1e-08, weight_decay=0, amsgrad=False):
        assert not amsgrad
        super().__init__(params=params, lr=0.0, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False)
        self.scheduler = lr if isinstance(lr, schedulers.Scheduler) else schedulers.ConstantScheduler(val=lr)
        self.arena = None
        self.grad_scale = 1.0
        self._flat = None

    # -- flat state -------------------------------------------------------------------------
    def attach_arena(self, arena):
        """Bind to the model's ParamArena: moments become two flat fp32 buffers laid out like the master arena."""
        self.arena = arena
        dev = arena.master.device
        self._flat = {"exp_avg": torch.zeros_like(arena.master), "exp_avg_sq": torch.zeros_like(arena.master),
                      "state": torch.zeros(2, dtype=torch.float32, device=dev),
                      # ops.grad_norm's outputs (clipping and the non-finite guard): {norm, coef}, {skip this step, steps skipped so far}, and its fp64 partial sums
                      "clip_stats": torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev), "clip_flag": torch.zeros(2, dtype=torch.int32, device=dev),
                      "clip_ws": ops.grad_norm_workspace(arena.numel, dev)}
        self._step_t = torch.tensor(0.0)
        for p, o in zip(arena.params, arena.offsets):
            st = self.state[p]
            n = p.numel()
            st["step"] = self._step_t
            st["exp_avg"] = self._flat["exp_avg"][o:o + n].as_strided(p.shape, p.stride())
            st["exp_avg_sq"] = self._flat["exp_avg_sq"][o:o + n].as_strided(p.shape, p.stride())

    def prepare_step(self):
        """host half of step(), never inside a graph: advance the scheduler, publish {step, lr} to the device scalar pair the kernel reads"""
        lr = self.scheduler.step()
        for group in self.param_groups:
            group["lr"] = lr
        if self.arena is None:
            raise RuntimeError("nnet.Adam steps a model's flat parameter arena on the GPU: move the model with Model.to('cuda') first "
                               "(there is no per-tensor / CPU optimizer path)")
        # ring of pinned {step, lr} slots: the H2D copy of step N is asynchronous, so the host may already be preparing step N+1 (graph replays,
        # eager steps never sync) -- it then writes a DIFFERENT slot; a slot is reused only after its copy's event completed
        if "host_ring" not in self._flat:
            self._flat["host_ring"] = [(torch.zeros(2, dtype=torch.float32).pin_memory(), torch.cuda.Event()) for _ in range(8)]
            self._flat["host_pos"] = 0
        slot, ev = self._flat["host_ring"][self._flat["host_pos"] % 8]
        if self._flat["host_pos"] >= 8:
            ev.synchronize()
        self._flat["host_pos"] += 1
        slot[0] = float(self.scheduler.model_step)
        slot[1] = float(lr)
        self._flat["state"].copy_(slot, non_blocking=True)
        ev.record()
        self._step_t.fill_(float(self.scheduler.model_step))     # one shared CPU scalar stands for every per-parameter "step" (state_dict)

    def launch_grad_norm(self, max_norm=None, skip_nonfinite=False):
        """Global gradient norm (times grad_scale) and clip factor on the device, two launches (ops.grad_norm); the next launch_step(clip=True) applies the factor
        and skips the update when the flag is raised (a non-finite norm under `skip_nonfinite`, or the peer exchange's error flag).  Returns the {norm, coef} pair."""
        from .. import peer
        px = peer.active()
        f = self._flat
        return ops.grad_norm(self.arena.grad, f["clip_ws"], f["clip_stats"], f["clip_flag"], self.grad_scale, max_norm, skip_nonfinite,
                             px.err if px is not None else None)

    @property
    def grad_norm_stats(self):
        """device fp32 pair {norm, coef} of the last launch_grad_norm"""
        return self._flat["clip_stats"]

    @property
    def skipped_steps(self):
        """device int32 scalar: optimizer steps skipped by the guard so far (reading it synchronises).  It lives beside the clip pair in the flat state that
        attach_arena allocates: it is not part of state_dict, so a checkpoint does not hold it and load_state_dict (which attaches the arena again) starts it at 0"""
        return self._flat["clip_flag"][1]

    def launch_step(self, clip=False):
        """device half: ONE kernel over the flat arenas (graph-capturable).  clip: read the clip factor and the skip flag launch_grad_norm left on the device"""
        g = self.param_groups[0]
        self._launch(g, clip)
        self.arena.mark_dirty()

    @torch.no_grad()
    def step(self, closure=None, clip=False):
        self.prepare_step()
        self.launch_step(clip)
        return None

    def _launch(self, g, clip=False):
        from .. import peer
        if clip:                      # (the peer exchange's error flag arrived in clip_flag through the norm launch's skip_in)
            lib.adam_step_clipped(self.arena.master.data_ptr(), self.arena.grad.data_ptr(), self._flat["exp_avg"].data_ptr(), self._flat["exp_avg_sq"].data_ptr(),
                                  self._flat["state"].data_ptr(), g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self.grad_scale, 1,
                                  self.arena.numel, self._flat["clip_flag"].data_ptr(), self._flat["clip_stats"].data_ptr(), rt.stream())
            return
        px = peer.active()            # data parallel with the peer exchange: its device error flag guards the update (a lost rank -> NaN sums -> skipped step)
        lib.adam_step_guarded(self.arena.master.data_ptr(), self.arena.grad.data_ptr(), self._flat["exp_avg"].data_ptr(), self._flat["exp_avg_sq"].data_ptr(),
                              self._flat["state"].data_ptr(), g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self.grad_scale, 1,
                              self.arena.numel, px.err.data_ptr() if px is not None else None, rt.stream())

    def zero_grad(self, set_to_none=False):
        if self.arena is not None:
            return            # the Adam kernel clears the gradient arena in the same pass
        super().zero_grad(set_to_none=False)

    def state_dict(self):
        sd = super().state_dict()
        sd["model_step"] = self.scheduler.model_step
        return sd

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        self.scheduler.model_step.fill_(state_dict.pop("model_step"))
        super().load_state_dict(state_dict)
        if self.arena is not None:      # re-home the loaded moments into the flat buffers
            loaded = {p: dict(self.state[p]) for p in self.arena.params if p in self.state}
            self.attach_arena(self.arena)
            for p, st in loaded.items():
                if "exp_avg" in st:
                    self.state[p]["exp_avg"].copy_(st["exp_avg"])
                    self.state[p]["exp_avg_sq"].copy_(st["exp_avg_sq"])


class AdamW(optim.AdamW):
    """nnet/optimizers.py AdamW as far as an LM config needs it to import: holds its arguments (parameter groups, betas, eps, the lr or its scheduler) and nothing
    more -- there is no HIP AdamW step and no LM training loop here; step() says so."""

    def __init__(self, params, lr=0.001, betas=(0.9, 0.999), eps=1e-08, weight_decay=0.01, amsgrad=False):
        super().__init__(params=params, lr=0.0, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        self.scheduler = lr if isinstance(lr, schedulers.Scheduler) else schedulers.ConstantScheduler(val=lr)

    def step(self, closure=None):
        raise NotImplementedError("nnet.AdamW holds its arguments only: training the Transformer LM is out of scope on this path")


def get_decay_param_groups(model, weight_decay=0.1):
    """nnet/optimizers.py: weights of Linear layers decay, everything else (biases, norms, embeddings) does not.  Holds the split; nothing steps it here."""
    decay, no_decay = [], []
    for m in model.modules():
        for name, p in m.named_parameters(recurse=False):
            (decay if isinstance(m, torch.nn.Linear) and name == "weight" else no_decay).append(p)
    return [{"params": decay, "weight_decay": weight_decay}, {"params": no_decay, "weight_decay": 0.0}]


optim_dict = {"Adam": Adam, "AdamW": AdamW}
