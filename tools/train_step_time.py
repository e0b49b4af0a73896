"""Times the DiT optimisation step (forward + loss, backward, AdamW) at batch 16 on latents through the EXPERIMENTS library, so that the GTAV_* overrides apply
(e.g. GTAV_DW_TN=0: transposed operand copies in front of the grouped weight-gradient launch; GTAV_DW_GROUPED=0).  One configuration per process: run it
twice in one job for an A/B on one box.   Usage (GPU box): GTAV_DW_TN=0 python tools/train_step_time.py [--steps 8] [--batch 16]
--dtype fp16 | bf16: the operand type of the training step (DiT(train_dtype=...)) on the PRODUCT library instead (no GTAV_* overrides there): the fp16 / bf16
A/B of profiles/round7/train_step_bf16_ab.txt.
--frames N: clips of N frames whose one target frame sees a window of N frames (default 5); above 8 the model is constructed with train_max_frames=N
(profiles/long_window_train/: batch 8 x 8, 4 x 16 and 2 x 32 frames, 9 216 tokens each).
--recompute: DiT(train_recompute=True), the activation recomputation of DESIGN.md 7 (product library: give --dtype).  Every run reports the handle's saved-activation
bytes (train_saved_bytes) and the device's free memory before and after the training handle was built.  --forward-only times gtav_dit_train_forward alone on the
same inputs (the yardstick of the recompute mode's extra time: it re-runs L - 1 of the L blocks' forwards).
--mixed none | one | alternating: DiT(train_range_policy="auto"), the mixed operand types of DESIGN.md 7 (product library: give --dtype, the type every group starts
on) with no group switched, with group 1 on the other type, or with every even group on it (profiles/train_mixed/).
--in-channels C --patch-size p: another patch geometry than (2, 16) (profiles/geometry/)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gtav_amd import lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--latent-hw", type=int, nargs=2, default=[18, 32], help="latent height and width (36 64: 576 tokens per frame)")
    ap.add_argument("--frames", type=int, default=5, help="frames per clip = the window of the step (above 8: DiT(train_max_frames=frames))")
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default=None, help="operand type of the training step, on the product library")
    ap.add_argument("--recompute", action="store_true", help="DiT(train_recompute=True): recompute each block's activations in the backward pass")
    ap.add_argument("--forward-only", action="store_true", help="time the training forward (forward_train) alone instead of the optimisation step")
    ap.add_argument("--mixed", choices=("none", "one", "alternating"), default=None, help="DiT(train_range_policy='auto') and which groups run on the other type")
    ap.add_argument("--in-channels", type=int, default=16, help="latent channels (profiles/geometry/: 4 at patch 2 = 16 features per patch, padded to 64)")
    ap.add_argument("--patch-size", type=int, default=2)
    a = ap.parse_args()
    if (a.recompute or a.mixed) and a.dtype is None:
        ap.error("--recompute / --mixed run on the product library: give --dtype fp16 or bf16")
    if a.dtype is None:
        L.load_experiments()
    else:
        L.load()
    import gtav_amd.weights as W
    from gtav_amd.model.dit import DiT_models
    from gtav_amd.train import training_step
    dev = torch.device("cuda", 0)
    B = a.batch
    train_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    LH, LW = a.latent_hw
    F = a.frames
    C_ = a.in_channels
    from gtav_amd.model.dit import DiT
    dit = DiT(input_h=LH, input_w=LW, patch_size=a.patch_size, in_channels=C_, hidden_size=1024, depth=16, num_heads=16, max_frames=F, init_weights=False, max_batch=B, trainable=True,
              train_dtype=train_dtype, train_max_frames=F if F > 8 else None, train_recompute=a.recompute,
              **({"train_range_policy": "auto"} if a.mixed else {}))   # DiT-S/2 at the given latent size
    dit.load_state_dict(W.synth_state_dict(W.dit_param_shapes(depth=16, input_h=LH, input_w=LW, patch_size=a.patch_size, in_channels=C_), seed=0))
    with torch.cuda.device(dev):
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        saved = dit.train_saved_bytes()               # builds the handle: gtav_dit_create + train_enable
        torch.cuda.synchronize()
        free_after = torch.cuda.mem_get_info()[0]
    if a.mixed in ("one", "alternating"):
        other = torch.float16 if a.dtype == "bf16" else torch.bfloat16
        dit.train_set_group_dtype(other, [1] if a.mixed == "one" else range(0, dit.n_operand_groups, 2))
    g = torch.Generator().manual_seed(7)
    lat = (torch.randn(B, F, C_, LH, LW, generator=g) * 0.5).to(dev)
    actions = torch.zeros(B, F, 25, device=dev)
    actions[:, :, 3] = 1
    tgt = torch.randint(1, 51, (B,), generator=g)
    ctx = torch.randint(1, 41, (B,), generator=g)
    ctx_noise = torch.randn(B, F - 1, C_, LH, LW, generator=g).to(dev)
    noise = torch.randn(B, 1, C_, LH, LW, generator=g).to(dev)

    def step():
        return training_step(dit, lat, actions, tgt, ctx, ctx_noise, noise, lr=1e-5, weight_decay=0.01, max_grad_norm=1.0, world_size=1, n_prompt_frames=F - 1)

    if a.forward_only:
        x = lat.clone()
        tt = torch.randint(0, 1000, (B, F), generator=g)

        def step():                                   # noqa: F811
            dit.forward_train(x, tt, actions)
            return torch.zeros(1)

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    applied, skipped, gnorm = dit.train_stats()
    print(json.dumps({"batch": B, "frames": F, "latent_hw": [LH, LW], "in_channels": C_, "patch_size": a.patch_size, "dtype": a.dtype or "fp16 (experiments library)", "recompute": a.recompute, "mixed": a.mixed,
                      "bf16_groups": [i for i, d in enumerate(dit.operand_dtypes()) if d == torch.bfloat16],
                      "what": "train_forward" if a.forward_only else "optimisation step", "ms_per_step": round(ms, 3), "loss": float(loss), "grad_norm": gnorm, "skipped": skipped,
                      "saved_bytes": saved, "free_before_enable": free_before, "free_after_enable": free_after, "handle_bytes": free_before - free_after,
                      "env": {k: v for k, v in os.environ.items() if k.startswith("GTAV_")}}))


if __name__ == "__main__":
    main()
