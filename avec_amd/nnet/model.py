"""Training / evaluation harness (API of nnet/model.py).  Host-side Python like the reference; what differs is what a step launches:
the forward/backward are fused HIP sequences, the optimizer is one launch over the flat arena, and data parallelism is one process per
GPU exchanging the flat gradient buffer (and BatchNorm statistics) over RCCL -- no DistributedDataParallel wrapper, no per-step buffer
broadcast."""
import copy
import glob
import os
import time

import torch
import torch.nn as nn

from .. import ops
from .. import runtime as rt
from .captured import CapturedStep, StepCache
from .decoders import decoder_dict
from .losses import loss_dict
from .metrics import metric_dict
from .module import Module
from .normalizations import SyncBatchNorm
from .optimizers import optim_dict
from .schedulers import ConstantScheduler, Scheduler


class Model(Module):
    def __init__(self, name="model"):
        super().__init__()
        self.is_distributed, self.rank, self.is_parallel = False, 0, False
        self.compiled, self.built = False, False
        self.name = name
        self.ema_model, self.ema_tau, self.grad_max_norm = None, 0.0, None
        self.skip_nonfinite_steps = False      # skip an optimizer step whose global gradient norm is NaN or infinite (what the reference's GradScaler does under fp16)
        self.arena = None
        self.world_size = 1
        self.captured_steps = StepCache()      # graphed_train_step / graphed_micro_step: captured steps per batch shape
        self.eager_fallback, self._eager_fallback_said = None, False       # why graphed_micro_step ran train_step instead (fit says so once)

    @staticmethod
    def _pre_forward(model, _args):
        """before every forward pass: in-place weight edits -> stale shadows; fp8 operands -> fresh activation amax slots"""
        if model.arena is None:
            return None
        model.arena.check_versions()
        if getattr(model.arena, "_fp8", None) is not None:
            model.arena._fp8.begin_pass()
        return None

    # -- placement ------------------------------------------------------------------------------
    def to(self, device):
        out = super().to(device)
        if self.device.type == "cuda":
            self.arena = rt.ParamArena(self)
            if not getattr(self, "_avec_version_hook", False):       # every forward (training, evaluation, a bare model(x)): weights edited in place since the last pass -> refresh the shadows
                self._avec_version_hook = True
                self.register_forward_pre_hook(Model._pre_forward)
            if self.compiled and hasattr(self.optimizer, "attach_arena"):
                self.optimizer.attach_arena(self.arena)
        if self.ema_model is not None:
            self.ema_model.to(device)
            self._check_ema_layout()
        return out

    def cuda(self, device=None):
        return self.to(torch.device("cuda", torch.cuda.current_device() if device is None else (device.index if isinstance(device, torch.device) else device)))

    def load_state_dict(self, state_dict, strict=True):
        out = super().load_state_dict(state_dict, strict=strict)
        if self.arena is not None:
            self.arena.mark_dirty()
        return out

    def distribute_strategy(self, rank, sync_batch_norm=True):
        """nnet/model.py:59-65.  Parameters/buffers are broadcast once from rank 0; afterwards each step all-reduces the flat gradient
        arena (and, with sync_batch_norm, the BatchNorm statistic vectors)."""
        import torch.distributed as dist
        if sync_batch_norm:
            SyncBatchNorm.convert_sync_batchnorm(self)
        self.rank, self.is_distributed = rank, True
        self.world_size = dist.get_world_size()
        rt.ensure_branch_group()          # second communicator for the collectives of the audio branch's stream (runtime.collective_group)
        if sync_batch_norm and self.device.type == "cuda":
            from .. import peer
            peer.setup(self.device)       # SyncBatchNorm statistics by peer writes over xGMI (one small kernel per exchange, no host work); None -> torch.distributed collectives
        if self.arena is not None:
            dist.broadcast(self.arena.master, 0)
            self.arena.mark_dirty()
        else:
            for p in self.parameters():
                dist.broadcast(p.data, 0)
        for b in self.buffers():
            if b.is_floating_point() or b.dtype == torch.int64:
                dist.broadcast(b, 0)

    def parallel_strategy(self):
        raise RuntimeError("single-process DataParallel is a legacy path of the reference (nnet/model.py:67-69); use one process per GPU")

    # -- exponential moving average of the weights (nnet/model.py:71-78, 401-407) --------------------
    def set_ema(self, ema_tau):
        """Keep an evaluation copy of the model whose parameters follow  ema = tau * ema + (1 - tau) * model  after every optimizer step (one
        ops.weight_average launch over the two flat arenas, inside the captured step when there is one).  Works before and after .to('cuda') / compile().
        The copy lives outside the module tree (no state_dict keys), has its OWN ParamArena laid out like the model's, and no optimizer.  Its buffers are
        the model's as of the last sync_ema_buffers() (save, fit's evaluation and this call do it); the reference copies them after every step, which is
        the same observable state."""
        # what must not be cloned: the arena (the copy gets its own), the optimizer and its moments, an earlier EMA model, captured steps (a StepCache copies as an
        # empty one).  What is shared, as the reference's build() shares it: losses, loss weights, decoders, metrics, and the step counter the loss-weight schedules read
        memo = {}
        for name in ("arena", "optimizer", "ema_model"):
            if self.__dict__.get(name) is not None:
                memo[id(self.__dict__[name])] = None
        for name in ("compiled_losses", "compiled_loss_weights", "compiled_metrics", "compiled_decoders", "losses", "loss_weights", "decoders", "metrics", "model_step"):
            if self.__dict__.get(name) is not None:
                memo[id(self.__dict__[name])] = self.__dict__[name]
        ema = copy.deepcopy(self, memo)
        src = dict(self.named_parameters())
        for name, q in ema.named_parameters():
            # a copied Parameter is a dense tensor of its own (not a view into this model's arena) without the attributes of the original: the GEMM weights
            # need their shadow descriptors again before an arena can be built over them
            sh = getattr(src[name], "_avec_shadow", None)
            if sh is not None:
                rt.register_weight(q, sh.A, sh.Tm, sh.C, sh.need_bwd, sh.Cp)
        for m in ema.modules():
            m._load_state_dict_post_hooks.clear()       # (the copied hooks mark THIS model's arena stale; the copy's arena registers its own)
        ema.requires_grad_(False)
        ema.eval()
        if self.arena is not None:
            ema.to(self.device)
        object.__setattr__(self, "ema_model", ema)
        self.ema_tau = float(ema_tau)
        self.captured_steps.clear()                      # whole steps captured so far have no EMA launch in them
        self._check_ema_layout()

    def _check_ema_layout(self):
        a, b = self.arena, self.ema_model.arena
        assert (a is None) == (b is None), "the EMA model must live where the model lives"
        if a is None:
            return
        assert b is not a and b.master.data_ptr() != a.master.data_ptr(), "the EMA model needs a parameter arena of its own"
        na, nb = {id(p): k for k, p in self.named_parameters()}, {id(p): k for k, p in self.ema_model.named_parameters()}
        assert a.numel == b.numel and a.offsets == b.offsets and len(a.params) == len(b.params) and \
            all(na[id(p)] == nb[id(q)] and p.shape == q.shape and p.stride() == q.stride() for p, q in zip(a.params, b.params)), \
            "the EMA model's arena is not laid out like the model's"

    def _update_ema(self):
        """after the optimizer launch: ema = tau * ema + (1 - tau) * model over the flat arenas -- one launch, no host synchronisation, graph-capturable"""
        ema = self.ema_model
        if ema is None:
            return
        if self.arena is None:
            raise RuntimeError("the EMA update runs on the flat parameter arenas on the GPU: move the model with Model.to('cuda') first")
        ops.weight_average(ema.arena.master, self.arena.master, 2, self.ema_tau, 1.0 - self.ema_tau)
        ema.arena.mark_dirty()

    @torch.no_grad()
    def sync_ema_buffers(self):
        """the EMA model's buffers (BatchNorm running statistics, num_batches_tracked) become the model's.  The reference copies them after every step
        (nnet/model.py:406-407); the copy is idempotent, so it is made where its result can be observed: before the EMA model is evaluated, saved or used."""
        if self.ema_model is not None:
            for target, buf in zip(self.ema_model.buffers(), self.buffers()):
                target.copy_(buf)
        return self.ema_model

    # -- compile / build (nnet/model.py:80-225) --------------------------------------------------
    def compile(self, losses, loss_weights=None, optimizer="Adam", metrics=None, decoders=None):
        self.optimizer = optim_dict[optimizer](params=self.parameters()) if isinstance(optimizer, str) else optimizer
        self.model_step = self.optimizer.scheduler.model_step
        self.compiled_losses = loss_dict[losses]() if isinstance(losses, str) else ([] if losses is None else losses)
        if loss_weights is None:
            self.compiled_loss_weights = ConstantScheduler(1.0)
        elif isinstance(loss_weights, float):
            self.compiled_loss_weights = ConstantScheduler(loss_weights)
        else:
            assert isinstance(loss_weights, (dict, list))
            it = loss_weights.items() if isinstance(loss_weights, dict) else enumerate(loss_weights)
            for k, v in list(it):
                if not isinstance(v, Scheduler):
                    loss_weights[k] = ConstantScheduler(v)
            self.compiled_loss_weights = loss_weights
        self.compiled_metrics = metric_dict[metrics]() if isinstance(metrics, str) else ([] if metrics is None else metrics)
        self.compiled_decoders = decoder_dict[decoders]() if isinstance(decoders, str) else ([] if decoders is None else decoders)
        self.compiled = True
        if self.arena is not None and hasattr(self.optimizer, "attach_arena"):
            self.optimizer.attach_arena(self.arena)

    def build(self, outputs):
        self.losses = self.map_to_outputs(outputs, self.compiled_losses)
        self.loss_weights = self.map_to_outputs(outputs, self.compiled_loss_weights)
        self.decoders = self.map_to_outputs(outputs, self.compiled_decoders)
        self.metrics = self.map_to_outputs(outputs, self.compiled_metrics)
        self.built = True
        if self.ema_model is not None:          # nnet/model.py:158-164
            ema = self.ema_model
            ema.losses, ema.loss_weights, ema.decoders, ema.metrics, ema.built = self.losses, self.loss_weights, self.decoders, self.metrics, True

    def map_to_outputs(self, outputs, struct):
        """dict -> fill missing keys with None; list -> positional over the output order; single item -> every output."""
        if struct is None:
            return struct
        if isinstance(struct, dict):
            for key in struct:
                if key not in outputs:
                    raise Exception("Found unexpected dict key: {}. Valid output names are: {}".format(key, outputs.keys()))
            for key in outputs:
                struct.setdefault(key, None)
            return struct
        if isinstance(struct, list):
            return {key: (struct[i] if i < len(struct) else None) for i, key in enumerate(outputs)}
        return {key: struct for key in outputs}

    def _fused_ctc_losses(self, outputs, targets):
        """The CTC heads of an InterCTC model share the batch and the labels: when they all fit the LDS-resident kernel they are evaluated by ONE launch
        (ops.CTCLossMultiFn) instead of one 32-workgroup launch per head.  Returns ({key: loss} for the heads it covered (same values as losses.CTCLoss; for logging), their weighted sum (differentiable)) or ({}, None)."""
        from .losses import CTCLoss
        keys = [k for k in outputs if isinstance(self.losses.get(k), CTCLoss) and isinstance(outputs[k], (list, tuple)) and len(outputs[k]) == 2
                and torch.is_tensor(outputs[k][0]) and outputs[k][0].is_cuda and outputs[k][0].dim() == 3]
        if len(keys) < 2 or len(keys) > 8:
            return {}, None
        l0, t0 = self.losses[keys[0]], targets[keys[0]]
        same = all(self.losses[k].blank == l0.blank and self.losses[k].zero_infinity == l0.zero_infinity and self.losses[k].reduction == "mean" and not self.losses[k].assert_shorter
                   and targets[k][0] is t0[0] and targets[k][1] is t0[1] and outputs[k][0].shape[0] == outputs[keys[0]][0].shape[0]
                   and outputs[k][0].shape[2] == outputs[keys[0]][0].shape[2] for k in keys)
        y, y_len = t0
        Lmax = y.shape[1] if y.dim() == 2 else y.numel() // outputs[keys[0]][0].shape[0]
        if not same or not all(ops.ctc_multi_fits(outputs[k][0].shape[1], outputs[k][0].shape[2], Lmax) for k in keys):
            return {}, None
        flat = []
        for k in keys:
            flat += [outputs[k][0], outputs[k][1]]
        weights = tuple(self.loss_weights[k].get_val_step(self.model_step + 1) for k in keys)
        res = ops.CTCLossMultiFn.apply(l0.blank, l0.zero_infinity, y, y_len, weights, *flat)
        return dict(zip(keys, res[1:])), res[0]

    # -- one forward + losses (nnet/model.py:227-344) ---------------------------------------------
    def forward_model(self, inputs, targets, compute_metrics=True, verbose=0):
        batch_losses, batch_metrics, batch_truths, batch_preds = {}, {}, {}, {}
        total_loss = None                        # (no zero-filled accumulator: with the fused CTC heads the weighted total comes out of their launch as is)
        Model._pre_forward(self, None)       # self.forward() is called directly (no __call__): the pre-forward hook would not fire on the training / evaluation paths
        outputs = self.forward(inputs)
        if isinstance(outputs, list):
            outputs = {"output_" + str(k): v for k, v in enumerate(outputs)}
        elif not isinstance(outputs, dict):
            outputs = {"output": outputs}
        targets = self.map_to_outputs(outputs, targets)
        if not self.built:
            self.build(outputs)
        fused, fused_total = self._fused_ctc_losses(outputs, targets)
        if fused_total is not None:
            total_loss = fused_total
        for key in outputs:
            if self.losses[key] is not None:
                if key in fused:                     # already inside fused_total with its weight
                    batch_losses["loss_" + key] = fused[key]
                else:
                    l = self.losses[key](targets[key], outputs[key])
                    batch_losses["loss_" + key] = l
                    wl = l * self.loss_weights[key].get_val_step(self.model_step + 1)
                    total_loss = wl if total_loss is None else total_loss + wl
            if compute_metrics and self.metrics and self.metrics[key] is not None:
                metric, decoder = self.metrics[key], (self.decoders[key] if self.decoders else None)
                name = metric.name if metric.name not in batch_metrics else metric.name + "_" + key
                if decoder is not None:
                    batch_truths[name] = decoder(targets[key], from_logits=False) if targets[key] is not None else None
                    batch_preds[name] = decoder(outputs[key])
                else:
                    batch_truths[name], batch_preds[name] = targets[key], outputs[key]
                batch_metrics[name] = metric(batch_truths[name], batch_preds[name])
        for module in self.modules():
            if getattr(module, "added_losses", None):
                for key, value in module.added_losses.items():
                    batch_losses["loss_" + key] = value["loss"]
                    wl = value["loss"] * value["weight"]
                    total_loss = wl if total_loss is None else total_loss + wl
                module.reset_losses()
        if total_loss is None:
            total_loss = torch.zeros((), device=self.device)
        batch_losses = dict({"loss": total_loss}, **batch_losses) if len(batch_losses) > 1 else {"loss": total_loss}
        return batch_losses, batch_metrics, batch_truths, batch_preds

    # -- one optimisation micro-step (nnet/model.py:346-409) ---------------------------------------
    def train_step(self, inputs, targets, precision=torch.float32, grad_scaler=None, accumulated_steps=1, acc_step=0, eval_training=False):
        rt.set_compute_dtype(precision)
        rt.reset_zero_pool(self.device)
        if self.is_distributed and self.arena is not None:       # overlap part of the gradient exchange with the backward pass of the last micro-step
            self.arena.arm_early_all_reduce(acc_step + 1 >= accumulated_steps and rt.early_all_reduce_enabled())
        batch_losses, batch_metrics, _, _ = self.forward_model(inputs, targets, compute_metrics=eval_training)
        (batch_losses["loss"] / accumulated_steps).backward()
        rt.advance_rng(self.device)
        batch_losses = self._own_losses(batch_losses)
        acc_step += 1
        if acc_step < accumulated_steps:
            return batch_losses, batch_metrics, acc_step
        self._finish_optimizer_step()
        return batch_losses, batch_metrics, 0

    def _finish_optimizer_step(self):
        """what follows the last micro-step's backward pass, as eager launches without host synchronisation: the optimizer's host half (scheduler, {step, lr} to the
        device), the device half (_launch_optimizer_tail, with the global norm and clip factor under grad_max_norm / skip_nonfinite_steps), the infos.
        The host never reads the guard's flag, so on a skipped step everything but the optimizer launch still happens: the scheduler and model_step advance, and
        the EMA model takes one more step toward parameters that did not change.  infos["skipped_steps"] counts since the optimizer's flat state was allocated: it
        is not saved in checkpoints and starts at 0 again after Adam.load_state_dict."""
        guard = bool(self.skip_nonfinite_steps)
        clip = self.grad_max_norm is not None or guard
        if clip and (self.arena is None or not hasattr(self.optimizer, "launch_grad_norm")):
            raise RuntimeError("gradient clipping and the non-finite guard run on the flat gradient arena on the GPU with nnet.Adam: move the model with Model.to('cuda') first")
        self.optimizer.prepare_step()
        stats = self._launch_optimizer_tail(clip)
        if clip:
            self.add_info("grad_norm", stats[0])              # device scalars: turned into numbers only where fit prints
            if guard:
                self.add_info("skipped_steps", self.optimizer.skipped_steps)
        self.optimizer.zero_grad()
        self.add_info("lr", float(self.optimizer.param_groups[0]["lr"]))
        self.add_info("step", int(self.model_step))

    def _launch_optimizer_tail(self, clip=False):
        """device half of an optimizer step, graph-capturable (no host synchronisation, no host state but the arenas' dirty marks): gradient all-reduce (data parallel;
        the 1 / world factor goes into the optimizer launch), the global norm and clip factor on the device when `clip` (ops.grad_norm, read by the optimizer launch),
        the optimizer launch, the EMA launch.  optimizer.prepare_step() must have run since the last one.  Returns the norm launch's {norm, coef} pair or None."""
        if self.is_distributed:
            # the reference all-reduces on every micro-batch (no no_sync); summing once per optimizer step is numerically the same
            self.arena.all_reduce_grads()
            self.optimizer.grad_scale = 1.0 / self.world_size
        stats = self.optimizer.launch_grad_norm(self.grad_max_norm, bool(self.skip_nonfinite_steps)) if clip else None
        self.optimizer.launch_step(clip)
        self._update_ema()
        return stats

    def clip_gradients(self, max_norm):
        """global-norm clipping of the flat gradient arena (torch.nn.utils.clip_grad_norm_ semantics, nnet/model.py:381-383); returns the norm before clipping"""
        norm = self.arena.grad.norm() * getattr(self.optimizer, "grad_scale", 1.0)
        self.arena.grad.mul_((max_norm / (norm + 1e-6)).clamp(max=1.0))
        return norm

    def make_graphed_train_step(self, inputs, targets, precision=torch.bfloat16, warmup=2):
        """Capture ONE optimisation step into a hipGraph: ~1600 launches replay from a single submission, removing the host-side launch overhead.
        Static shapes: later batches are copied into the captured buffers.  Returns step(inputs, targets) -> losses dict (device scalars).
        * single process: shadow refresh, forward, 6 losses, backward and Adam are all inside the graph;
        * data parallel (one process per GPU): the graph holds shadow refresh + forward + losses + backward -- the SyncBatchNorm statistic exchanges are
          peer-write kernels (avec_amd/peer.py), so no host-driven collective interrupts it; the gradient all-reduce (RCCL) and the Adam launch follow the
          replay.  Requires the peer exchange (otherwise every BatchNorm layer needs a host-issued collective: use train_step)."""
        from .. import peer
        dist_mode = self.is_distributed
        nccl = dist_mode and torch.distributed.get_backend() == "nccl"
        # RCCL collectives are capturable: over the nccl backend the WHOLE data-parallel step -- SyncBatchNorm exchanges (peer writes, or RCCL when the peer exchange is
        # off / refused), the range-wise gradient all-reduce (fusion + audio-visual ranges when the gradient crosses the fusion inputs, the audio encoder's from the audio
        # branch's stream beside the visual backward, the visual encoder's at the end) and the Adam launch -- is ONE hipGraph, unless rt.graph_all_reduce_enabled() says no.
        in_graph = nccl and rt.graph_all_reduce_enabled()
        assert not dist_mode or in_graph or peer.active() is not None, "graph capture of a data-parallel step needs capturable SyncBatchNorm exchanges (RCCL, or the peer exchange); use train_step"
        rt.set_compute_dtype(precision)
        cap = CapturedStep(inputs, targets)
        if dist_mode:
            self.arena.arm_early_all_reduce(False)          # (armed per pass inside body() when the collectives are captured)
        tail_in_graph = [not dist_mode or in_graph]         # else (data parallel without captured collectives) the optimizer tail follows the replay

        def body():
            rt.reset_zero_pool(self.device)
            if dist_mode and tail_in_graph[0]:
                self.arena.arm_early_all_reduce(rt.early_all_reduce_enabled(), sync=True)     # sync holds until the tail's all_reduce_grads: every collective is captured
            losses, _, _, _ = self.forward_model(cap.inputs, cap.targets, compute_metrics=False)
            ops.stamp("loss_done:f")
            losses["loss"].backward()
            ops.stamp("bwd_done:b")
            rt.advance_rng(self.device)
            if tail_in_graph[0]:
                self._launch_optimizer_tail()
            return losses

        def run(inner):                                     # one optimisation step around the eager body (warm-up) or the replay
            self.optimizer.prepare_step()                   # (the optimizer's device-side {step, lr} pair is written OUTSIDE the graph, before every pass)
            losses = inner()
            if not tail_in_graph[0]:
                self._launch_optimizer_tail()
            return losses

        # lazily created constants (DFT matrix, sinusoid tables, loss weights) must exist before the capture: at least one eager pass
        warm = cap.warm_up(lambda: run(body), max(int(warmup), 1))
        cap_err = None
        try:
            cap.capture(body, drain=nccl)
        except Exception as e:
            if not in_graph:
                raise
            cap_err = e
        if in_graph:
            # the fallback must be the SAME on every rank: a rank that keeps captured collectives beside one that issues them eagerly is a collective mismatch
            flag = torch.tensor([0.0 if cap_err is None else 1.0], device=self.device)
            torch.cuda.synchronize()
            torch.distributed.all_reduce(flag)
            torch.cuda.synchronize()
            if cap_err is None and float(flag.item()) > 0:
                cap_err = RuntimeError("another rank could not capture the collectives")
                ops.reset_backward_state()                  # (as the ranks whose capture was aborted)
        if cap_err is not None:
            # the collectives could not be captured on this stack: capture forward + backward only (peer-write SyncBatchNorm), all-reduce + Adam after each replay
            print("[avec_amd] rank %d: capture with in-graph RCCL collectives failed (%s: %s); capturing forward + backward only"
                  % (self.rank, type(cap_err).__name__, cap_err), flush=True)
            tail_in_graph[0] = False
            self.arena.arm_early_all_reduce(False)
            cap.capture(body, drain=True)

        replays = [0]

        def step(new_inputs=None, new_targets=None):
            replays[0] += 1
            px = peer.active() if dist_mode else None       # None: SyncBatchNorm over RCCL (peer exchange off / refused / more than one node)
            if px is not None and replays[0] % 100 == 0:
                px.check()                          # (synchronises) a lost rank: the guarded Adam launch skipped those steps, say so instead of training on
            if new_inputs is not None:
                cap.load(new_inputs, new_targets)
            losses = run(cap.replay)
            if self.ema_model is not None:
                self.ema_model.arena.mark_dirty()   # (the captured EMA launch rewrote its masters as well)
            if tail_in_graph[0]:
                self.arena.mark_dirty()             # host-side view of what the replay's closing Adam launch left behind: whatever runs next OUTSIDE the graph
            return losses                           # (evaluation, an eager step) must refresh the weight shadows first -- the captured refresh sits at the START of a replay

        if dist_mode:
            self.arena.arm_early_all_reduce(rt.early_all_reduce_enabled())      # later eager train_steps keep their overlapped exchange
        step.graph = cap.graph
        step.collectives_in_graph = bool(dist_mode and tail_in_graph[0])
        step.warm_losses = {k: v.detach().clone() for k, v in warm.items()}
        return step

    # -- hipGraph replay for ragged training batches: one captured step per batch SHAPE --------------------------------------------------------------------
    @staticmethod
    def pad_av_batch(inputs, targets, bucket_frames):
        """zero-pad an audio-visual batch [video (B,Tv,H,W,C), video_len, audio (B,Ta), audio_len], (labels (B,L), label_len) to the next multiple of
        `bucket_frames` video frames (audio to the longest clip with that many frames: 640 * Tv' - 1 samples, labels to a multiple of 8): the true lengths stay, so
        attention masks and CTC are unchanged; like the reference's own padding to the batch maximum (nnet/collate_fn.py:143-146) the zero frames do enter the
        BatchNorm batch statistics -- a coarser bucket is a (slightly) different batch composition, which is why bucketing is opt-in."""
        video, vlen, audio, alen = inputs
        labels, llen = targets
        Tv = video.shape[1]
        Tvp = (Tv + bucket_frames - 1) // bucket_frames * bucket_frames
        Tap = 640 * Tvp - 1
        if Tvp > Tv:
            video = torch.nn.functional.pad(video, (0, 0, 0, 0, 0, 0, 0, Tvp - Tv))
        if Tap > audio.shape[1]:
            audio = torch.nn.functional.pad(audio, (0, Tap - audio.shape[1]))
        Lp = (labels.shape[1] + 7) // 8 * 8
        if Lp > labels.shape[1]:
            labels = torch.nn.functional.pad(labels, (0, Lp - labels.shape[1]))
        return [video, vlen, audio, alen], (labels, llen)

    def _graph_capturable(self):
        """a step can be captured as is: constant loss weights (scheduled ones change a launch argument from step to step), and in data parallel capturable
        SyncBatchNorm exchanges (the peer exchange, or RCCL over the nccl backend)"""
        from .. import peer
        lw = self.compiled_loss_weights
        const_w = isinstance(lw, ConstantScheduler) or (isinstance(lw, dict) and all(isinstance(v, ConstantScheduler) for v in lw.values())) \
            or (isinstance(lw, list) and all(isinstance(v, ConstantScheduler) for v in lw))
        capturable = (not self.is_distributed) or peer.active() is not None or (torch.distributed.get_backend() == "nccl" and rt.graph_all_reduce_enabled())
        return const_w and capturable

    def _cached_step(self, kind, make, inputs, targets, precision, cache_size, bucket_frames, *extra):
        """the captured step of `kind` ("step" / "micro") for this batch's shape from self.captured_steps, captured by make(inputs, targets) when the shape is new
        -> (inputs, targets as the captured step takes them: bucketed when `bucket_frames`, see pad_av_batch; the step; whether it was made just now)"""
        if bucket_frames and len(inputs) == 4 and inputs[0].dim() == 5 and isinstance(targets, (tuple, list)) and len(targets) == 2:
            inputs, targets = self.pad_av_batch(inputs, targets, bucket_frames)
        key = (kind,) + tuple((tuple(t.shape), str(t.dtype)) for t in list(inputs) + list(targets)) + (str(precision),) + extra
        who = {"step": "graphed_train_step", "micro": "graphed_micro_step"}[kind]
        step, made = self.captured_steps.get_or_make(key, lambda: make(inputs, targets), cache_size, who)
        return inputs, targets, step, made

    def graphed_train_step(self, inputs, targets, precision=torch.bfloat16, cache_size=8, bucket_frames=None):
        """train_step through the cache of captured steps keyed by the batch shape (self.captured_steps: LRU, `cache_size` graphs, each with its own activation pool).
        Ragged LRS batches (nnet/collate_fn.py pads to the batch maximum) repeat a small set of shapes once they are bucketed (`bucket_frames`, see pad_av_batch) or
        come from a length-bucketed sampler.  Falls back to train_step when a step cannot be captured as is (scheduled loss weights, data parallel without capturable
        SyncBatchNorm exchanges).  With gradient clipping or the non-finite guard the step is graphed_micro_step's: forward + backward replayed, norm and optimizer
        launches behind the replay."""
        if not self._graph_capturable():
            return self.train_step(inputs, targets, precision=precision)[0]
        if self.grad_max_norm is not None or self.skip_nonfinite_steps:
            return self.graphed_micro_step(inputs, targets, precision, 1, 0, cache_size=cache_size, bucket_frames=bucket_frames)[0]
        make = lambda i, t: self.make_graphed_train_step(i, t, precision=precision, warmup=1)      # (the warm-up pass is a real optimisation step on this batch)
        inputs, targets, step, made = self._cached_step("step", make, inputs, targets, precision, cache_size, bucket_frames)
        return step.warm_losses if made else step(inputs, targets)

    # -- hipGraph replay of ONE micro-step (forward + backward): gradient accumulation, clipping and the non-finite guard keep the optimizer tail eager ---------
    def make_graphed_micro_step(self, inputs, targets, precision, accumulated_steps):
        """Run ONE real micro-step eagerly on this batch (it accumulates into the gradient arena like train_step's), then capture the same body into a hipGraph:
        reset_zero_pool, forward, losses, (loss / accumulated_steps).backward(), advance_rng.  No optimizer, no EMA, no gradient all-reduce and no shadow refresh are
        inside: the weight shadows are made fresh before the capture and before every replay (one eager launch after an optimizer step, nothing on the other
        micro-steps).  Capturing executes nothing, so the arena is not touched twice.  Like every captured step it holds the modules' training / evaluation
        modes as they were at the capture.  Returns micro(inputs, targets) -> losses (static device scalars) with .warm_losses, the eager pass's."""
        dist_mode = self.is_distributed
        cap = CapturedStep(inputs, targets)

        def body():
            rt.reset_zero_pool(self.device)
            losses, _, _, _ = self.forward_model(cap.inputs, cap.targets, compute_metrics=False)
            (losses["loss"] / accumulated_steps).backward()
            rt.advance_rng(self.device)
            return losses

        def settle(fresh=True):                             # before every pass
            if dist_mode:
                self.arena.arm_early_all_reduce(False)      # the gradient exchange follows the LAST replay (amortised over the micro-steps), never from inside the backward pass
            rt.set_compute_dtype(precision)
            if fresh:                                       # no refresh inside the graph (the eager pass brings its own)
                self.arena.check_versions()                 # (weights edited in place since the last pass: the forward pre-hook's check does not run inside a replay)
                self.arena.ensure_fresh()

        def before_capture():
            settle()
            ops.invalidate_pos_cache()                      # the position projections, cached per refresh, are computed INSIDE the graph: every replay follows the weights

        settle(fresh=False)
        warm = cap.warm_up(lambda: self._own_losses(body()))
        cap.capture(body, drain=dist_mode and torch.distributed.get_backend() == "nccl", before=before_capture)
        assert not self.arena.dirty, "the captured micro-step must not hold a shadow refresh"

        def micro(new_inputs, new_targets):
            cap.load(new_inputs, new_targets)
            settle()
            return cap.replay()

        micro.graph = cap.graph
        micro.warm_losses = warm
        return micro

    def _micro_fallback_reason(self, eval_training=False):
        """why graphed_micro_step runs train_step instead of a captured micro-step, or None"""
        from .. import fp8
        if self.device.type != "cuda":
            return "the model is not on a GPU"
        if eval_training and self.compiled_metrics:
            return "eval_training with compiled metrics needs the host on every step (pass eval_training=False / --no_eval_training)"
        if fp8.enabled():
            return "AVEC_FP8=1"
        if not self._graph_capturable():
            return "scheduled loss weights, or data parallel without capturable SyncBatchNorm exchanges"
        return None

    def graphed_micro_step(self, inputs, targets, precision=torch.bfloat16, accumulated_steps=1, acc_step=0, cache_size=8, bucket_frames=None, eval_training=False):
        """One micro-step of train_step(accumulated_steps=k) from a cache of captured forward + backward passes keyed by batch shape, precision and k (LRU,
        `cache_size` graphs, each with its own activation pool); returns (losses, acc_step) with acc_step = 0 after the optimizer step.  The first time a shape
        appears the micro-step runs eagerly (a real micro-step) and is captured afterwards.  Behind the last micro-step's replay follow, as eager launches without
        host synchronisation: the gradient all-reduce (data parallel), the norm / clip-factor launches (grad_max_norm, skip_nonfinite_steps), the optimizer and EMA
        launches.  Falls back to train_step when the step cannot be captured as is: scheduled loss weights, eval_training with compiled metrics (they need the
        host), AVEC_FP8=1, data parallel without capturable SyncBatchNorm exchanges."""
        why = self._micro_fallback_reason(eval_training)
        if why is not None:
            self.eager_fallback = why                        # (fit says so once: nobody should believe they are on the replay path)
            losses, _, acc_step = self.train_step(inputs, targets, precision, None, accumulated_steps, acc_step, eval_training)
            return losses, acc_step
        make = lambda i, t: self.make_graphed_micro_step(i, t, precision, accumulated_steps)
        inputs, targets, micro, made = self._cached_step("micro", make, inputs, targets, precision, cache_size, bucket_frames, int(accumulated_steps))
        losses = micro.warm_losses if made else self._own_losses(micro(inputs, targets))      # copies: the next replay refills the static outputs
        acc_step += 1
        if acc_step < accumulated_steps:
            return losses, acc_step
        self._finish_optimizer_step()
        return losses, 0

    @staticmethod
    def _own_losses(batch_losses):
        """the fused CTC launch leaves its means and the weighted total in the step's pre-zeroed scratch pool, which the next step (or graph replay) overwrites: hand
        the caller values it can keep (ONE stacked copy; a captured step returns the pool views themselves -- static outputs refilled by every replay)"""
        keys = list(batch_losses)
        vals = torch.stack([batch_losses[k].detach().reshape(()).float() for k in keys]).unbind(0)
        return dict(zip(keys, vals))

    def eval_step(self, inputs, targets, verbose=0):
        with torch.no_grad():
            rt.reset_zero_pool(self.device, create=False)      # (the scratch pool hands out PRE-ZEROED accumulators: whatever earlier steps or replays of other shapes left there must go; an evaluation-only process never allocates it)
            batch_losses, batch_metrics, batch_truths, batch_preds = self.forward_model(inputs, targets, verbose=verbose)
            return self._own_losses(batch_losses), batch_metrics, batch_truths, batch_preds

    # -- checkpoints (nnet/model.py:499-544) -------------------------------------------------------
    def save(self, path, save_optimizer=True):
        if self.is_distributed:
            from .. import peer
            if peer.active() is not None:
                peer.active().check()            # (synchronises) a SyncBatchNorm exchange that lost a rank since the last check: raise instead of writing a checkpoint of skipped steps
        torch.save({"model_state_dict": self.state_dict(), "optimizer_state_dict": self.optimizer.state_dict() if save_optimizer else None,
                    "model_step": self.model_step, "is_distributed": self.is_distributed or self.is_parallel,
                    "ema_model_state_dict": None if self.ema_model is None else self.sync_ema_buffers().state_dict(), "grad_scaler_state_dict": None}, path)

    def load(self, path, load_optimizer=True, verbose=True, strict=True):
        ckpt = torch.load(path, map_location=self.device, weights_only=False)
        sd = ckpt["model_state_dict"]
        if ckpt.get("is_distributed", False):
            sd = {k.replace(".module.", ".").replace("module.", "", 1) if k.startswith("module.") else k.replace(".module.", "."): v for k, v in sd.items()}
        self.load_state_dict({k: v for k, v in sd.items()}, strict=strict)
        if load_optimizer and ckpt.get("optimizer_state_dict") is not None:
            # the step counter (Noam schedule, loss-weight schedules, Adam bias correction) travels with the optimizer state (nnet/model.py:527-536):
            # fine-tuning from a checkpoint without its optimizer restarts the schedule at step 0 on zero moments
            self.optimizer.load_state_dict(ckpt["optimizer_state_dict"])
            self.model_step.fill_(ckpt["model_step"])
        if ckpt.get("ema_model_state_dict") is not None and self.ema_model is not None:      # nnet/model.py:538-540
            self.ema_model.load_state_dict(ckpt["ema_model_state_dict"])

    # -- checkpoint averaging (nnet/model.py:944-1015) ------------------------------------------------
    def average_checkpoints(self, paths, swa_type="equal", swa_decay=0.9):
        """Load the checkpoints of `paths` in order (optimizer included, as the reference's swa does: model_step ends as the last one's) and leave their
        average in the model: swa_type "equal" is the running mean  avg += (p - avg) / (k + 1), "exp" is  avg = (1 - swa_decay) * avg + swa_decay * p;  the
        first checkpoint is copied.  On the GPU each checkpoint is ONE ops.weight_average launch from the flat master arena into a second flat buffer; a
        model without an arena (CPU) takes the same formulas as separate torch fp32 operations, which give the same bits.
        Parameters only are averaged.  Buffers (BatchNorm running statistics, num_batches_tracked) end as the LAST checkpoint's: that is what
        torch.optim.swa_utils.AveragedModel(use_buffers=False), which the reference uses, leaves -- update_parameters copies the buffers on every call --
        and why swa() refreshes the statistics afterwards."""
        assert swa_type in ("equal", "exp"), "swa_type: equal or exp"
        assert len(paths) > 0, "no checkpoint to average"
        avg = None
        with torch.no_grad():
            for k, path in enumerate(paths):
                self.load(path)
                mode = 0 if k == 0 else (1 if swa_type == "equal" else 2)
                wa, wp = (0.0, 1.0 / (k + 1)) if swa_type == "equal" else (1.0 - swa_decay, swa_decay)
                if self.arena is not None:
                    if avg is None:
                        avg = torch.empty_like(self.arena.master)
                    ops.weight_average(avg, self.arena.master, mode, wa, wp)
                elif mode == 0:
                    avg = [p.detach().clone() for p in self.parameters()]
                else:
                    for a, p in zip(avg, self.parameters()):
                        if mode == 1:
                            a.add_((p.detach() - a).mul_(wp))                     # three roundings, as the kernel's mode 1
                        else:
                            a.copy_(a.mul(wa).add_(p.detach().mul(wp)))           # alpha = 1: a plain sum of the two rounded products
            if self.arena is not None:
                self.arena.master.copy_(avg)
                self.arena.mark_dirty()
            else:
                for a, p in zip(avg, self.parameters()):
                    p.copy_(a)

    def swa(self, dataset, callback_path, start_epoch, end_epoch, epochs_list=None, update_steps=None, swa_type="equal", swa_decay=0.9, precision=torch.float32):
        """main.py -m swa: average checkpoints_epoch_{e}_step_*.ckpt of `callback_path` for e in epochs_list (or start_epoch .. end_epoch), refresh the BatchNorm
        statistics with `update_steps` training-mode forward passes over `dataset` (no loss, no backward, no optimizer: the parameters do not move), and write
        checkpoints_swa-{swa_type}-{first}-{last}.ckpt without the optimizer state."""
        if not epochs_list:
            epochs_list = list(range(int(start_epoch), int(end_epoch) + 1))
        if self.rank == 0:
            print("Stochastic Weight Averaging on checkpoints : {}".format(list(epochs_list)))
        paths = []
        for epoch in epochs_list:
            pattern = os.path.join(callback_path, "checkpoints_epoch_{}_step_*.ckpt".format(epoch))
            found = glob.glob(pattern)
            if not found:
                raise FileNotFoundError("no checkpoint matches " + pattern)
            paths.append(found[0])
        self.average_checkpoints(paths, swa_type=swa_type, swa_decay=swa_decay)
        if self.rank == 0:
            print("Updating Batch Normalization Statistics")
        if update_steps is None:
            update_steps = len(dataset)
        self.train()
        steps = 0
        while steps < update_steps:
            seen = steps
            for batch in dataset:
                inputs = self.transfer_to_device(batch["inputs"])
                rt.set_compute_dtype(precision)
                rt.reset_zero_pool(self.device)
                Model._pre_forward(self, None)
                with torch.no_grad():
                    self.forward(inputs)
                rt.advance_rng(self.device)        # dropout and SpecAugment are active, as in the reference: the next step draws other masks
                steps += 1
                if steps == update_steps:
                    break
            assert steps > seen, "swa: the dataset is empty"
        if self.rank == 0:
            self.save(os.path.join(callback_path, "checkpoints_swa-{}-{}-{}.ckpt".format(swa_type, epochs_list[0], epochs_list[-1])), save_optimizer=False)
        if self.is_distributed:
            torch.distributed.barrier()

    # -- loops (compact counterparts of nnet/model.py:668-942, 1047-1077) ----------------------------
    def fit(self, dataset_train, epochs, dataset_eval=None, eval_steps=None, verbose_eval=0, initial_epoch=0, callback_path=None, steps_per_epoch=None,
            precision=torch.float32, accumulated_steps=1, eval_period_step=None, eval_period_epoch=1, saving_period_epoch=1, log_figure_period_step=None,
            log_figure_period_epoch=1, step_log_period=100, eval_training=True, grad_init_scale=65536.0, detect_anomaly=False, recompute_metrics=False,
            wandb_logging=False, verbose_progress_bar=1, keep_last_k=None, use_graphs=False, graph_bucket_frames=None, graph_cache_size=8):
        """use_graphs: replay captured steps per batch shape instead of eager launches -- the whole step (graphed_train_step) when accumulated_steps == 1 without
        clipping or the non-finite guard, else forward + backward per micro-step with the optimizer tail behind the last one (graphed_micro_step; with eval_training
        and compiled metrics it runs eagerly: metrics need the host); graph_bucket_frames: additionally zero-pad AV batches to multiples of that many video frames so
        that few shapes occur (opt-in: changes the padding the BatchNorm statistics see)."""
        if callback_path is not None and self.rank == 0:
            os.makedirs(callback_path, exist_ok=True)
        for epoch in range(initial_epoch, epochs):
            self.train()
            sampler = getattr(dataset_train, "sampler", None)
            if self.is_distributed and hasattr(sampler, "set_epoch"):
                sampler.set_epoch(epoch)          # reshuffle + re-shard per epoch (nnet/model.py:709-710)
            bsamp = getattr(dataset_train, "batch_sampler", None)
            if hasattr(bsamp, "set_epoch"):
                bsamp.set_epoch(epoch)            # length-bucketed batches: new windows every epoch (nnet/samplers.py)
            acc_step, t0, n = 0, time.time(), 0
            for step, batch in enumerate(dataset_train):
                inputs = self.transfer_to_device(batch["inputs"])
                targets = self.transfer_to_device(batch["targets"])
                micro = accumulated_steps > 1 or self.grad_max_norm is not None or self.skip_nonfinite_steps
                if use_graphs and micro and self.device.type == "cuda":
                    losses, acc_step = self.graphed_micro_step(inputs, targets, precision, accumulated_steps, acc_step, cache_size=graph_cache_size,
                                                               bucket_frames=graph_bucket_frames, eval_training=eval_training)
                    if self.eager_fallback is not None and not self._eager_fallback_said:
                        self._eager_fallback_said = True
                        if self.rank == 0:
                            print("use_graphs: training with eager launches, not replayed graphs -- " + self.eager_fallback)
                elif use_graphs and self.device.type == "cuda":
                    losses = self.graphed_train_step(inputs, targets, precision=precision, cache_size=graph_cache_size, bucket_frames=graph_bucket_frames)
                else:
                    losses, _, acc_step = self.train_step(inputs, targets, precision, None, accumulated_steps, acc_step, eval_training)
                n += 1
                if self.is_distributed and step % step_log_period == 0:
                    from .. import peer
                    if peer.active() is not None:
                        peer.active().check()            # a SyncBatchNorm peer exchange that lost a rank raises here (its sums were NaN from that step on)
                if self.rank == 0 and step % step_log_period == 0:
                    extra = ""
                    if torch.is_tensor(self.infos.get("grad_norm")):       # device scalars of the last optimizer step: read (one synchronisation) only here
                        extra += " grad_norm %.4f" % float(self.infos["grad_norm"])
                    if torch.is_tensor(self.infos.get("skipped_steps")):
                        extra += " skipped_steps %d" % int(self.infos["skipped_steps"])
                    print("epoch %d step %d model_step %d loss %.4f%s" % (epoch + 1, step, int(self.model_step), float(losses["loss"].detach()), extra))
                if steps_per_epoch is not None and step + 1 >= steps_per_epoch:
                    break
            if self.rank == 0:
                print("epoch %d: %d steps in %.1fs" % (epoch + 1, n, time.time() - t0))
                if callback_path is not None and (epoch + 1) % saving_period_epoch == 0:
                    self.save(os.path.join(callback_path, "checkpoints_epoch_{}_step_{}.ckpt".format(epoch + 1, int(self.model_step))))
            if dataset_eval is not None and (epoch + 1) % eval_period_epoch == 0:
                self.evaluate(dataset_eval, eval_steps)
                if self.ema_model is not None:    # nnet/model.py:853-861
                    res = self.sync_ema_buffers().evaluate(dataset_eval, eval_steps)
                    if self.rank == 0:
                        for r in (res if isinstance(res, list) else [res]):
                            print("epoch %d ema eval:" % (epoch + 1), {k: round(v, 4) for k, v in r.items()})
            if self.is_distributed:
                torch.distributed.barrier()       # ranks leave the epoch together (rank 0 wrote the checkpoint)

    def evaluate(self, dataset_eval, eval_steps=None, verbose=0, eval_loss=True, recompute_metrics=False):
        if isinstance(dataset_eval, (list, tuple)):          # several evaluation sets (the reference configs list LRS2 and LRS3 test sets)
            res = [self.evaluate(d, eval_steps, verbose, eval_loss, recompute_metrics) for d in dataset_eval]
            return res[0] if len(res) == 1 else res
        self.eval()
        sums, count = {}, 0
        metric_keys, truths, preds = [], {}, {}
        for step, batch in enumerate(dataset_eval):
            inputs = self.transfer_to_device(batch["inputs"])
            targets = self.transfer_to_device(batch["targets"])
            losses, metrics, batch_truths, batch_preds = self.eval_step(inputs, targets, verbose)
            for k, v in list(losses.items()) + list(metrics.items()):
                sums[k] = sums.get(k, 0.0) + float(v)
            metric_keys = list(metrics.keys())
            if recompute_metrics:                           # keep the decoded references / hypotheses: corpus-level metrics (nnet/model.py:899-903, 928-931)
                for k in metric_keys:
                    if isinstance(batch_truths.get(k), (list, tuple)) and isinstance(batch_preds.get(k), (list, tuple)):
                        truths.setdefault(k, []).extend(batch_truths[k])
                        preds.setdefault(k, []).extend(batch_preds[k])
            count += 1
            if eval_steps is not None and step + 1 >= eval_steps:
                break
        if self.is_distributed:                             # sum over ranks (nnet/model.py:912-918: reduce_losses_metrics / gather_truths_preds)
            import torch.distributed as dist
            # every collective below must be issued by every rank with the same shapes, whatever this rank saw (zero batches, no list-type hypotheses):
            # agree on the key sets first
            all_keys = [None] * dist.get_world_size()
            dist.all_gather_object(all_keys, (sorted(sums), bool(truths)))
            keys = sorted(set(k for ks, _ in all_keys for k in ks))
            for k in keys:
                sums.setdefault(k, 0.0)
            any_truths = any(t for _, t in all_keys)
            vec = torch.tensor([sums[k] for k in keys] + [float(count)], dtype=torch.float64, device=self.device if dist.get_backend() != "gloo" else "cpu")
            dist.all_reduce(vec)
            sums, count = {k: float(v) for k, v in zip(keys, vec[:-1].tolist())}, int(vec[-1].item())
            if any_truths:
                gathered = [None] * dist.get_world_size()
                dist.all_gather_object(gathered, (truths, preds))
                truths, preds = {}, {}
                for t, p in gathered:
                    for k in t:
                        truths.setdefault(k, []).extend(t[k])
                        preds.setdefault(k, []).extend(p[k])
        res = {k: v / max(count, 1) for k, v in sums.items()}
        for k in truths:                                    # metric of the whole evaluation set, not the mean of per-batch values
            cands = [mt for mt in (self.metrics.values() if isinstance(self.metrics, dict) else [self.metrics]) if mt is not None]
            metric = next((mt for mt in cands if mt.name == k), None) or next((mt for mt in cands if k.startswith(mt.name + "_")), None)
            if metric is not None:
                res[k] = float(metric(truths[k], preds[k]))
        return res

    def eval_time(self, dataset_eval, eval_steps=None, **kwargs):
        if isinstance(dataset_eval, (list, tuple)):
            return sum(self.eval_time(d, eval_steps, **kwargs) for d in dataset_eval)
        self.eval()
        torch.cuda.synchronize()
        t0 = time.time()
        for step, batch in enumerate(dataset_eval):
            with torch.no_grad():
                self.forward(self.transfer_to_device(batch["inputs"]))
            if eval_steps is not None and step + 1 >= eval_steps:
                break
        torch.cuda.synchronize()
        return time.time() - t0

    def summary(self, show_dict=False):
        print(self.name, "Parameters:", sum(p.numel() for p in self.parameters()))
