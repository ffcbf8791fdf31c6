"""One data-parallel rank on one GPU (a one-rank nccl group, AVEC_DIST_SINGLE=1): two optimizer steps of the AV model with accumulated_steps = 2, eagerly
(Model.train_step) or through the captured micro-step (Model.graphed_micro_step: forward + backward with the SyncBatchNorm exchanges inside the graph, the gradient
all-reduce and the optimizer launch behind the last replay) -- launched by tests/test_gpu_graph_accum.py.

Both optimizer steps start from the initial weights with Adam's moments at zero (the state is put back in between), so that after the second one
exp_avg / (1 - beta1) - wd * p0 IS the accumulated gradient: in graph mode both of its micro-steps are replays.  Writes {grads, losses, step, cached, peer} to --out."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def small_av_batch(B, secs, seed, dev):
    g = torch.Generator().manual_seed(seed)
    alen = torch.tensor([int(16000 * s) for s in secs])
    vlen = alen // 640 + 1
    Ta, Tv = int(alen.max()), int(vlen.max())
    audio, video = torch.zeros(B, Ta), torch.zeros(B, Tv, 88, 88, 1)
    for b in range(B):
        audio[b, :alen[b]] = 0.1 * torch.randn(int(alen[b]), generator=g)
        video[b, :vlen[b]] = torch.randn(int(vlen[b]), 88, 88, 1, generator=g)
    labels = torch.randint(1, 256, (B, 3), generator=g)
    return [video.to(dev), vlen.to(dev), audio.to(dev), alen.to(dev)], (labels.to(dev), torch.full((B,), 3).to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--mode", default="eager", choices=["eager", "graph"])
    args = ap.parse_args()
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    torch.distributed.init_process_group(backend="nccl", init_method="env://", device_id=dev)
    import avec_amd
    import nnet
    from avec_amd import peer
    avec_amd.set_compute_dtype("f32")
    avec_amd.manual_seed(7)
    torch.manual_seed(0)
    model = nnet.AudioVisualEfficientConformerInterCTC()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if hasattr(m, "drop_rate"):
            m.drop_rate = 0.0
    model.compile(losses=nnet.CTCLoss(zero_infinity=True, assert_shorter=False))
    model = model.to(dev).train()
    model.encoder.audio_encoder.spec_augment.eval()
    model.distribute_strategy(int(os.environ.get("RANK", "0")))
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    master0 = model.arena.master.detach().clone()
    batches = [small_av_batch(2, (0.9, 0.7), 1, dev), small_av_batch(2, (1.0, 0.8), 2, dev)]
    k, losses = 2, []
    for step in range(2):
        model.load_state_dict(sd0)
        model.optimizer._flat["exp_avg"].zero_()
        model.optimizer._flat["exp_avg_sq"].zero_()
        acc = 0
        for i in range(k):
            inp, tgt = batches[i]
            if args.mode == "eager":
                l, _, acc = model.train_step(inp, tgt, torch.float32, None, k, acc)
            else:
                l, acc = model.graphed_micro_step(inp, tgt, torch.float32, k, acc)
            losses.append(float(l["loss"].detach()))
        assert acc == 0
    torch.cuda.synchronize()
    if peer.active() is not None:
        peer.active().check()
    grp = model.optimizer.param_groups[0]
    beta1, wd = grp["betas"][0], grp["weight_decay"]
    grads = (model.optimizer._flat["exp_avg"].detach().float() / (1.0 - beta1) - wd * master0).cpu()      # flat, laid out like the parameter arena
    names = {id(p): name for name, p in model.named_parameters()}
    layout = [[names[id(p)], int(o), p.numel()] for p, o in zip(model.arena.params, model.arena.offsets)]
    torch.save({"grads": grads, "layout": layout, "losses": losses, "step": int(model.model_step), "cached": model.captured_steps.count("micro"),
                "peer": peer.active() is not None, "world": model.world_size}, args.out)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
