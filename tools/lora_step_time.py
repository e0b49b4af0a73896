"""Time and memory of the LoRA optimisation step against the full one at the shipped training shape (DiT-S/2 on latents, batch 16 x 5 frames x 144 tokens): the
full step (every parameter trained) and DiT(train_lora_rank=16) / (train_lora_rank=64), three models in ONE process on one GPU, `--reps` steps per reading
between device events, the three alternating for `--rounds` rounds after a warm-up; the median reading of each is reported.  Memory: what building the handle
took from the device (hipMemGetInfo before / after: masters, images, moments, saved activations, workspaces) and torch's own peak (the gradient arena is a
torch tensor).  Per-launch times: the in-situ profiler (gtav_dit_profile) books inference forwards only, so those of the training step come from a kernel
trace of this tool (rocprofv3 --kernel-trace --stats -- python tools/lora_step_time.py --rounds 1), in a run of its own.
    python tools/lora_step_time.py [--out profiles/lora/lora_step_time.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtav_amd import lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16")
    ap.add_argument("--ranks", type=int, nargs="*", default=[16, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    L.load()
    import gtav_amd.weights as W
    from gtav_amd.model.dit import DiT
    from gtav_amd.train import training_step
    dev = torch.device("cuda", 0)
    B, F, C_, LH, LW = args.batch, 5, 16, 18, 32
    sd = W.synth_state_dict(W.dit_param_shapes(depth=16), seed=0)
    g = torch.Generator().manual_seed(7)
    lat = (torch.randn(B, F, C_, LH, LW, generator=g) * 0.5).to(dev)
    actions = torch.zeros(B, F, 25, device=dev)
    actions[:, :, 3] = 1
    tgt, ctx = torch.randint(1, 51, (B,), generator=g), torch.randint(1, 41, (B,), generator=g)
    ctx_noise, noise = torch.randn(B, F - 1, C_, LH, LW, generator=g).to(dev), torch.randn(B, 1, C_, LH, LW, generator=g).to(dev)

    models, mem = {}, {}
    for name, rank in [("full", None)] + [(f"lora r{r}", r) for r in args.ranks]:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        torch_before, free_before = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
        m = DiT(input_h=LH, input_w=LW, patch_size=2, in_channels=C_, hidden_size=1024, depth=16, num_heads=16, max_frames=F, init_weights=False, max_batch=B,
                trainable=True, train_dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float16, train_lora_rank=rank)
        m.load_state_dict(sd)
        if rank:                                       # live adapters: B = 0 would make half of the gradient work trivially zero-valued (not cheaper, but unrepresentative)
            ad = m.lora_state_dict()
            m.load_lora_state_dict({k: (torch.randn(v.shape, generator=g) * 0.02 if ".lora_B." in k else v) for k, v in ad.items()})
        saved = m.train_saved_bytes()                   # builds the handle
        training_step(m, lat, actions, tgt, ctx, ctx_noise, noise, lr=1e-5, weight_decay=0.01, max_grad_norm=1.0, n_prompt_frames=F - 1)
        torch.cuda.synchronize()
        mem[name] = dict(params=m.grad_arena.numel(), saved=saved, device=free_before - torch.cuda.mem_get_info()[0],
                         torch_peak=torch.cuda.max_memory_allocated() - torch_before)
        models[name] = m

    def timed(m):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            training_step(m, lat, actions, tgt, ctx, ctx_noise, noise, lr=1e-5, weight_decay=0.01, max_grad_norm=1.0, n_prompt_frames=F - 1)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    for m in models.values():                           # warm-up of every shape the timed window uses
        timed(m)
    res = {k: [] for k in models}
    for _ in range(args.rounds):
        for k, m in models.items():
            res[k].append(timed(m))
    lines = [f"optimisation step of DiT-S/2 on latents, batch {B} x {F} frames x 144 tokens, {args.dtype} operands, {args.reps} steps per reading, {args.rounds} "
             f"alternating rounds, device events, {torch.cuda.get_device_name(0)}",
             "ms per step (median, min .. max) | trainable parameters | device memory of the model (handle + torch) | torch peak | saved activations"]
    for k, v in res.items():
        applied, skipped, _ = models[k].train_stats()
        q = mem[k]
        lines.append(f"  {k:9s} {statistics.median(v):7.2f}  ({min(v):.2f} .. {max(v):.2f}) | {q['params']:>11,d} | {q['device'] / 2**30:6.2f} GiB | "
                     f"{q['torch_peak'] / 2**30:5.2f} GiB | {q['saved'] / 2**30:5.2f} GiB | skipped steps {skipped}")
    full = statistics.median(res["full"])
    for k, v in res.items():
        if k != "full":
            lines.append(f"  {k}: {statistics.median(v) / full:.3f} of the full step's time, {(mem['full']['device'] - mem[k]['device']) / 2**30:.2f} GiB less device memory")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
