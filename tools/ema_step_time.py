"""Time and memory of the optimisation step with averaged (EMA) weights against the step without, at the shipped training shape (DiT-S/2 on latents, batch
16 x 5 frames x 144 tokens): DiT(trainable=True) / (train_ema_decay=0.9999) / (train_ema_decay=0.9999, train_ema_warmup=True), three models in ONE process on
one GPU, `--reps` steps per reading between device events, the three alternating for `--rounds` rounds after a warm-up; median and spread of each are reported.
Also: the optimizer call alone (gtav_dit_adamw_step: norm, coefficient and the AdamW launch) timed the same way, with the bytes per second its 32 / 40 bytes per
parameter come to; device memory before / after building each model; the time of one swap (gtav_dit_train_swap_ema).
The AdamW launch's own time comes from a kernel trace of this tool in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/ema_step_time.py --rounds 1).
`--root DIR --models plain` times the model without a shadow of ANOTHER checkout of this project (the parent commit, built in DIR) with the same script, for the
before / after comparison on one GPU in one job.
    python tools/ema_step_time.py [--out profiles/ema/ema_step_time.txt]"""
import argparse
import os
import statistics
import sys

import torch

MODELS = {"plain": None, "ema": dict(train_ema_decay=0.9999), "ema+warmup": dict(train_ema_decay=0.9999, train_ema_warmup=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16")
    ap.add_argument("--models", nargs="*", default=list(MODELS), choices=list(MODELS))
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose gtav_amd is measured (default: this one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    sys.path.insert(0, os.path.abspath(args.root))
    from gtav_amd import lib as L
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

    def step(m):
        training_step(m, lat, actions, tgt, ctx, ctx_noise, noise, lr=1e-5, weight_decay=0.01, max_grad_norm=1.0, n_prompt_frames=F - 1)

    models, mem = {}, {}
    for name in args.models:
        torch.cuda.synchronize()
        torch_before, free_before = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
        m = DiT(input_h=LH, input_w=LW, patch_size=2, in_channels=C_, hidden_size=1024, depth=16, num_heads=16, max_frames=F, init_weights=False, max_batch=B,
                trainable=True, train_dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float16, **(MODELS[name] or {}))
        m.load_state_dict(sd)
        m.train_saved_bytes()                           # builds the handle
        step(m)
        torch.cuda.synchronize()
        free_after = torch.cuda.mem_get_info()[0]
        mem[name] = dict(params=m.grad_arena.numel(), before=free_before, after=free_after, torch=torch.cuda.memory_allocated() - torch_before)
        models[name] = m

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for m in models.values():                           # warm-up of every launch the timed windows use
        timed(lambda: step(m), args.reps)
        timed(lambda: m.adamw_step(1e-5, weight_decay=0.01, max_grad_norm=1.0), args.reps)
    res, opt = {k: [] for k in models}, {k: [] for k in models}
    for _ in range(args.rounds):
        for k, m in models.items():
            res[k].append(timed(lambda: step(m), args.reps))
        for k, m in models.items():                     # (the arena holds the last step's gradients: an applied step every time)
            opt[k].append(timed(lambda: m.adamw_step(1e-5, weight_decay=0.01, max_grad_norm=1.0), args.reps))
    lines = [f"optimisation step of DiT-S/2 on latents, batch {B} x {F} frames x 144 tokens, {args.dtype} operands, {args.reps} steps per reading, {args.rounds} "
             f"alternating rounds, device events, {torch.cuda.get_device_name(0)}, checkout {os.path.basename(os.path.abspath(args.root))}",
             "whole step, ms (median, min .. max, spread = max - min) | optimizer call alone, ms (median, min .. max) | bytes per parameter it moves, achieved TB/s | "
             "device memory free before -> after building the model | taken"]
    for k in models:
        v, o, q = res[k], opt[k], mem[k]
        applied, skipped, _ = models[k].train_stats()
        bpp = 32 if MODELS[k] is None else 40            # g, m, v, w read + m, v, w and the two 2-byte images written (+ the shadow read and written)
        # (the optimizer call also reads the gradients once more for the norm: 4 bytes per parameter that the figure leaves out, as the kernel's own time would)
        lines.append(f"  {k:10s} {statistics.median(v):7.2f}  ({min(v):.2f} .. {max(v):.2f}, spread {max(v) - min(v):.2f}) | {statistics.median(o):6.3f}  ({min(o):.3f} .. "
                     f"{max(o):.3f}) | {bpp} B, {bpp * q['params'] / (statistics.median(o) * 1e-3) / 1e12:.2f} TB/s | {q['before'] / 2**30:7.2f} -> "
                     f"{q['after'] / 2**30:7.2f} GiB | {(q['before'] - q['after']) / 2**30:6.2f} GiB | parameters {q['params']:,d} | skipped steps {skipped}")
    if "plain" in models:
        base, base_o, base_m = statistics.median(res["plain"]), statistics.median(opt["plain"]), mem["plain"]["before"] - mem["plain"]["after"]
        for k in models:
            if k != "plain":
                lines.append(f"  {k}: whole step {statistics.median(res[k]) - base:+.2f} ms ({statistics.median(res[k]) / base:.4f} x), optimizer call "
                             f"{statistics.median(opt[k]) - base_o:+.3f} ms ({statistics.median(opt[k]) / base_o:.3f} x), "
                             f"{(mem[k]['before'] - mem[k]['after'] - base_m) / 2**30:+.2f} GiB device memory")
    for k, m in models.items():
        if MODELS[k] is None:
            continue
        swap = lambda: L.check(L.load().gtav_dit_train_swap_ema(m._handle, L.current_stream()))  # noqa: E731  (an even number of calls: the model ends as it was)
        timed(swap, 2)
        t = [timed(swap, 2) for _ in range(args.rounds)]
        lines.append(f"  {k}: one swap (masters <-> shadow, both 2-byte images remade) {statistics.median(t):.3f} ms  ({min(t):.3f} .. {max(t):.3f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
