"""Time of the guided sampler step (gtav_dit_set_guidance: one forward over 2 B internal samples) against the unguided step of the same build on the same
GPU: DiT-S/2 on 18 x 32 latents (144 tokens per frame), a 5-frame window, hoisted conditioning, captured steps (hipGraph replay), at batch 1 and batch 8.
Four variants per batch — window step and context-cached step, each unguided and guided — alternate for `--rounds` rounds of `--steps` replayed steps between
device events after an eager step, the capture and a first replay; the median reading of each is reported, and guided / unguided per kind of step.
Two unguided steps would cost 2.00; the claim under test is that the guided step, which stays one launch chain, costs well under that.
    python tools/guidance_step_time.py [--out profiles/guidance/guidance_step_time.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtav_amd import lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    L.load()
    import gtav_amd.weights as W
    from gtav_amd.model.dit import DiT
    from gtav_amd.utils import alphas_cumprod
    dev = torch.device("cuda", 0)
    T, C_, LH, LW = 5, 16, 18, 32
    sd = W.synth_state_dict(W.dit_param_shapes(depth=16), seed=0)
    ts = [999 - 7 * k for k in range(args.steps + 3)]
    lines = [f"fused sampler step of DiT-S/2 on latents, {T}-frame window x 144 tokens, hoisted conditioning, captured steps, guidance scale {args.scale}, "
             f"{args.steps} replays per reading, {args.rounds} alternating rounds, device events, {torch.cuda.get_device_name(0)}",
             "ms per step: median (min .. max)"]
    # one handle for every batch (sized once for the largest doubled batch and table: no variant rebuilds it; the kernels see token counts, not capacities)
    m = DiT(input_h=LH, input_w=LW, patch_size=2, in_channels=C_, hidden_size=1024, depth=16, num_heads=16, max_frames=T, init_weights=False,
            max_batch=2 * max(args.batches))
    m.load_state_dict(sd)
    m.set_schedule(alphas_cumprod(1e-4))
    m.set_guidance(args.scale)
    m.reserve(max(args.batches), T, noise_steps=len(ts))
    for B in args.batches:
        x0 = (torch.randn(B, T, C_, LH, LW, generator=torch.Generator().manual_seed(11)) * 0.5).to(dev)
        act = torch.zeros(B, T, 25, device=dev)
        act[:, :, 3] = 1
        xs = {v: x0.clone() for v in ((False, False), (True, False), (False, True), (True, True))}   # one buffer per variant: its captured step is found again

        def timed(guided, cached):
            x = xs[(guided, cached)]
            x.copy_(x0)
            m.set_guidance(args.scale if guided else None)
            m.prepare_frame_(B, T, 0, T - 1, 15, ts, act)
            m.denoise_step_(x, 0, T - 1, 15, ts[0], ts[1], False, act, cond_step=0)              # full window: the context K/V a cached step needs
            for k in range(1, 3):                                                              # this variant's eager step and capture (first round), replays after
                m.denoise_step_(x, 0, T - 1, 15, ts[k], ts[k + 1], False, act, cached=cached, cond_step=k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            for k in range(3, args.steps + 3):
                m.denoise_step_(x, 0, T - 1, 15, ts[k], ts[min(k + 1, args.steps + 2)], False, act, cached=cached, cond_step=k)
            e1.record()
            torch.cuda.synchronize(dev)
            return e0.elapsed_time(e1) / args.steps

        for v in xs:                                    # warm-up: every variant captured
            timed(*v)
            timed(*v)
        res = {v: [] for v in xs}
        for _ in range(args.rounds):
            for v in xs:
                res[v].append(timed(*v))
        m.check()
        med = {v: statistics.median(r) for v, r in res.items()}
        for cached in (False, True):
            kind = "context-cached step" if cached else "window step"
            u, g = (False, cached), (True, cached)
            lines.append(f"  batch {B} {kind:20s} unguided {med[u]:7.3f} ({min(res[u]):.3f} .. {max(res[u]):.3f}) | guided {med[g]:7.3f} ({min(res[g]):.3f} .. {max(res[g]):.3f}) | "
                         f"guided / unguided {med[g] / med[u]:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
