"""Training forward + loss (reference train_dit.py:329-351 `encode_frames`, :554-682 `_shared_step`, forward part):
noise the context and target frames, run the DiT once over the window, MSE against the v-target of the
last frame.  Random draws are arguments so that parity runs can inject them; with `rng=` (a gtav_amd.rng.NoiseSource) the step makes them itself:
the noise indices on the host, the Gaussian noise inside the launch that consumes it (DESIGN.md "Noise streams")."""
from __future__ import annotations

from typing import Optional

import torch

from . import lib as _lib
from . import rng as _rng
from .generate import vae_encode
from .utils import alphas_cumprod as _alphas_cumprod


@torch.inference_mode()
def encode_frames(vae, frames: torch.Tensor) -> torch.Tensor:
    """train_dit.py:329-351."""
    return vae_encode(frames, vae, frames.shape[1])


def _frame_step(dit, latents, actions, i, target_noise_idx, ctx_noise_idx, ctx_noise, noise, nr, ac, noise_abs_max, keep_activations, rng=None,
                noise_steps=None, ctx_max_noise_idx=None, action_keep=None):
    """One iteration of the frame loop of `_shared_step` (train_dit.py:590-650) for target frame i: returns (loss (1,), v_pred, v_target).
    With `rng` the frame takes one draw number: the two noise indices of every sample come from the host stream (train_dit.py:574-587) and the window's noise
    (slots 0 .. W - 1 of sample rng.sample0 + b) is drawn inside the one launch that noises the window and makes the v-target."""
    dev = dit.device
    L = _lib.load()
    B = latents.shape[0]
    if rng is not None:
        draw = rng.next_draw()
        target_noise_idx = rng.randint(1, noise_steps + 1, B, _rng.SLOT_TARGET_IDX, draw).tolist()
        ctx_noise_idx = rng.randint(1, ctx_max_noise_idx + 1, B, _rng.SLOT_CTX_IDX, draw).tolist()
    tgt = [int(v) for v in target_noise_idx]
    ctx = [min(int(c), t_) for c, t_ in zip(ctx_noise_idx, tgt)]                       # train_dit.py:587 torch.minimum
    start = max(0, i + 1 - dit.max_frames)
    t = torch.zeros((B, i + 1), dtype=torch.long)
    t[:, :-1] = nr[torch.tensor(ctx)].unsqueeze(1)
    t[:, -1] = nr[torch.tensor(tgt)]
    t = t[:, start:]
    W = t.shape[1]
    x_curr = latents[:, start: i + 1].to(dev, torch.float32).contiguous()
    a = actions[:, start: i + 1].to(dev, torch.float32).contiguous() if actions is not None else None
    n = x_curr[0, 0].numel()
    alpha = ac[t].to(dev).contiguous()                                                  # (B, W)
    x_noisy = torch.empty_like(x_curr)
    stream = _lib.current_stream()
    if rng is not None:
        v_target = torch.empty((B, *x_curr.shape[2:]), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(L.gtav_noise_window_rng(x_curr.data_ptr(), alpha.data_ptr(), x_noisy.data_ptr(), v_target.data_ptr(), B, W, n, rng.seed, draw,
                                               rng.sample0 & 0xFFFFFFFF, noise_abs_max, stream))
    else:
        all_noise = torch.empty_like(x_curr)                                            # copies only: torch is storage here
        all_noise[:, :-1] = ctx_noise.to(dev, torch.float32)
        all_noise[:, -1:] = noise.to(dev, torch.float32)
        with torch.cuda.device(dev):
            _lib.check(L.gtav_add_noise(x_curr.data_ptr(), all_noise.data_ptr(), alpha.data_ptr(), x_noisy.data_ptr(), B * W, n,
                                        noise_abs_max, stream))
            x_last = x_curr[:, -1].contiguous()
            nz_last = all_noise[:, -1].contiguous()
            a_last = alpha[:, -1].contiguous()
            v_target = torch.empty_like(x_last)
            _lib.check(L.gtav_vtarget(x_last.data_ptr(), nz_last.data_ptr(), a_last.data_ptr(), v_target.data_ptr(), B, n,
                                      noise_abs_max, stream))
    if action_keep is not None:
        v_pred = dit.forward_train(x_noisy, t, a, action_keep=action_keep)             # (forward_loss: the mask needs the training forward)
    else:
        v_pred = dit.forward_train(x_noisy, t, a) if keep_activations else dit(x_noisy, t, a)
    out = torch.empty(1 + B, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        vp_last = v_pred[:, -1]
        _lib.check(L.gtav_mse(vp_last.data_ptr(), v_pred.stride(0), v_target.data_ptr(), n, B, n, out.data_ptr(), stream))
    return out[:1], v_pred, v_target.reshape(B, 1, *x_curr.shape[2:])


def _per_frame(arg, n_iter, what):
    """A per-iteration argument of the frame loop: a list / tuple of n_iter entries, or (one target frame) the entry itself."""
    if isinstance(arg, (list, tuple)):
        assert len(arg) == n_iter, f"{what}: {len(arg)} entries for {n_iter} target frames"
        return list(arg)
    if torch.is_tensor(arg) and what.endswith("idx") and arg.dim() == 2:
        assert arg.shape[0] == n_iter, f"{what}: {arg.shape[0]} rows for {n_iter} target frames"
        return [arg[k] for k in range(n_iter)]
    assert n_iter == 1, f"{what}: clips with {n_iter} target frames need one entry per target frame"
    return [arg]


@torch.inference_mode()
def forward_loss(dit, latents: torch.Tensor, actions: Optional[torch.Tensor], target_noise_idx=None, ctx_noise_idx=None, ctx_noise=None, noise=None,
                 noise_steps: int = 50, n_prompt_frames: int = 4, noise_abs_max: float = 20.0, clamp_min: float = 1e-6,
                 keep_activations: bool = False, on_frame=None, rng=None, ctx_max_noise_idx: Optional[int] = None, action_keep=None):
    """train_dit.py:590-682 `_shared_step`: for every target frame i in [n_prompt_frames, total_frames) noise the window that ends at i,
    run the DiT over it, MSE against the v-target of frame i; returns (mean loss over the target frames (1,), v_pred, v_target) of the LAST
    target frame.  The shipped dataset has ONE target frame (5-frame clips): then the draws are plain tensors — target_noise_idx /
    ctx_noise_idx (B,), ctx_noise (B, W - 1, C, h, w), noise (B, 1, C, h, w).  Longer clips pass one entry per target frame (lists, or
    (n, B) index tensors); the window of target frame i holds min(i + 1, max_frames) frames.
    keep_activations: run the DiT through forward_train so that dit.backward_(v_pred, v_target) can follow; on_frame(k, v_pred, v_target)
    is called after target frame k's forward (the trainer differentiates each frame's loss right there, train_dit.py:679-680).
    rng (a gtav_amd.rng.NoiseSource) in place of the four draws, which must then be None: every target frame takes one draw number of it, target index in
    [1, noise_steps], context index in [1, ctx_max_noise_idx] (required; config.ctx_max_noise_idx of the reference) capped by the target index, the window's
    noise from slots 0 .. W - 1 of that draw (DESIGN.md "Noise streams").
    action_keep (B,) of 0 / 1, or None: per-sample action dropout (draw_action_keep; the reference's commented-out train_dit.py:704-705) — a sample with 0 is
    conditioned as external_cond=None in every target frame's forward.  It lives in the training forward: needs keep_activations=True and actions."""
    if action_keep is not None and not (keep_activations and actions is not None):
        raise ValueError("forward_loss: action_keep needs keep_activations=True (the training forward) and actions")
    _rng.check_exclusive(rng, "forward_loss", target_noise_idx=target_noise_idx, ctx_noise_idx=ctx_noise_idx, ctx_noise=ctx_noise, noise=noise)
    if rng is not None and ctx_max_noise_idx is None:
        raise ValueError("forward_loss: rng= needs ctx_max_noise_idx (the upper end of the context noise index, config.ctx_max_noise_idx)")
    B, total = latents.shape[:2]
    n_iter = total - n_prompt_frames
    assert n_iter >= 1, "forward_loss: no target frame behind the prompt frames"
    if rng is None:
        tgts, ctxs = _per_frame(target_noise_idx, n_iter, "target_noise_idx"), _per_frame(ctx_noise_idx, n_iter, "ctx_noise_idx")
        cns, nzs = _per_frame(ctx_noise, n_iter, "ctx_noise"), _per_frame(noise, n_iter, "noise")
    nr = torch.linspace(0, 999, noise_steps + 1).long()                                 # train_dit.py:309-315
    ac = _alphas_cumprod(clamp_min)
    total_loss = None
    for k, i in enumerate(range(n_prompt_frames, total)):
        if rng is None:
            loss, v_pred, v_target = _frame_step(dit, latents, actions, i, tgts[k].cpu().tolist(), ctxs[k].cpu().tolist(), cns[k], nzs[k], nr, ac,
                                                 noise_abs_max, keep_activations, action_keep=action_keep)
        else:
            loss, v_pred, v_target = _frame_step(dit, latents, actions, i, None, None, None, None, nr, ac, noise_abs_max, keep_activations, rng,
                                                 int(noise_steps), int(ctx_max_noise_idx), action_keep=action_keep)
        if on_frame is not None:
            on_frame(k, v_pred, v_target)
        if total_loss is None:
            total_loss = loss
        else:
            with torch.cuda.device(dit.device):                                         # total_loss += loss (train_dit.py:676), as a HIP kernel
                _lib.check(_lib.load().gtav_axpy_f32(total_loss.data_ptr(), loss.data_ptr(), 1.0, 1, _lib.current_stream()))
    if n_iter > 1:
        with torch.cuda.device(dit.device):                                             # / (total_frames - n_prompt_frames) (train_dit.py:682)
            _lib.check(_lib.load().gtav_axpy_f32(total_loss.data_ptr(), total_loss.data_ptr(), 1.0 / n_iter - 1.0, 1, _lib.current_stream()))
    return total_loss, v_pred, v_target


# ------------------------------------------------------------------------------------------------------------------------
# Inference helpers of the trainer (reference train_dit.py:352-552): decode_frames, predict, predict_noise.  Same kernels as the
# generation harness; the trainer's constants differ from generate.py's: schedule clamp_min 1e-6, the
# stabilisation level is noise_range[1] of the TRAINING range (19 for ddim_noise_steps = 50), inference range as .long().
# Random draws are arguments (the reference draws them from the global RNG), so parity runs inject identical noise.
# ------------------------------------------------------------------------------------------------------------------------
def stabilization_level(ddim_noise_steps: int = 50) -> int:
    """train_dit.py:309-327: noise_range = linspace(0, 999, steps + 1).long(); stabilization_level = noise_range[1]."""
    return int(torch.linspace(0, 999, ddim_noise_steps + 1).long()[1])


@torch.inference_mode()
def decode_frames(vae, latents: torch.Tensor) -> torch.Tensor:
    """train_dit.py:352-368: latents (B, t, C, h, w) -> uint8 video (B, t, H, W, 3)."""
    from .generate import vae_decode_frames
    return vae_decode_frames(latents, vae, to_uint8=True)


@torch.inference_mode()
def predict(dit, vae, frames: torch.Tensor, actions: Optional[torch.Tensor], new_frame_noise: Optional[torch.Tensor] = None, num_frames: int = 32,
            n_prompt_frames: int = 4, ddim_noise_steps: int = 50, ddim_noise_steps_inference: int = 50, noise_abs_max: float = 20.0,
            decode: bool = True, rng=None, guidance_scale: Optional[float] = None):
    """train_dit.py:370-466 `predict`: first sample of the batch, prompt = its first n_prompt_frames, actions padded with "W"
    (index 3) up to num_frames, autoregressive generation with the trainer's constants.  new_frame_noise (1, num_frames -
    n_prompt_frames, C, h, w): the standard-normal draw of every generated frame, or rng= (a NoiseSource: one draw number, made on the device
    as in generate_latents) in its place.  guidance_scale: classifier-free guidance on the actions, as in generate_latents (needs actions and a model with
    max_batch >= 2).  Returns (latents (1, num_frames, C, h, w), uint8 video (1, num_frames, H, W, 3) or None)."""
    from .generate import generate_latents
    _rng.check_exclusive(rng, "predict", new_frame_noise=new_frame_noise)
    frames = frames[:1, :n_prompt_frames]
    act = None
    if actions is not None:
        act = actions[:1].to(torch.float32)
        if act.shape[1] < num_frames:
            pad = torch.zeros((1, num_frames - act.shape[1], act.shape[2]), dtype=act.dtype, device=act.device)
            pad[:, :, 3] = 1                                                  # drive straight (train_dit.py:386-390)
            act = torch.cat([act, pad], dim=1)
    x = encode_frames(vae, frames.to(vae.device))
    lat = generate_latents(dit, x, num_frames, ddim_noise_steps_inference, new_frame_noise, act,
                           stabilization_level=stabilization_level(ddim_noise_steps), noise_abs_max=noise_abs_max, clamp_min=1e-6, rng=rng, guidance_scale=guidance_scale)
    return lat, (decode_frames(vae, lat) if decode else None)


@torch.inference_mode()
def predict_noise(dit, vae, frames: torch.Tensor, actions: Optional[torch.Tensor], ctx_noise: Optional[torch.Tensor] = None,
                  new_frame_noise: Optional[torch.Tensor] = None, ddim_noise_steps: int = 50, ddim_noise_steps_inference: int = 50,
                  noise_abs_max: float = 20.0, rng=None):
    """train_dit.py:468-552 `predict_noise`: encode every frame of the first clip, noise the context frames at level
    stabilization_level - 1 (train_dit.py:498), replace the last frame by clamped noise and denoise it.
    ctx_noise (1, n - 1, C, h, w), new_frame_noise (1, 1, C, h, w), or rng= (a NoiseSource) in their place: one draw number for the clip, frame f is
    slot f.  Returns (latents, x_noisy before denoising, x after)."""
    from .generate import generate_latents
    _rng.check_exclusive(rng, "predict_noise", ctx_noise=ctx_noise, new_frame_noise=new_frame_noise)
    dev = dit.device
    L = _lib.load()
    latents = encode_frames(vae, frames[:1].to(vae.device)).to(dev)
    n = latents.shape[1]
    if rng is not None:
        draw = rng.next_draw()
        ctx_noise = rng.normal(1, n - 1, latents.shape[2:], draw, 0, dev, noise_abs_max)
        new_frame_noise = rng.normal(1, 1, latents.shape[2:], draw, n - 1, dev, noise_abs_max)
    lvl = stabilization_level(ddim_noise_steps)
    ac = _alphas_cumprod(1e-6)
    ctx = latents[:, :-1].contiguous()
    x_ctx = torch.empty_like(ctx)
    alpha = ac[lvl - 1].reshape(1).repeat(n - 1).to(dev).contiguous()
    nz = ctx_noise.to(dev, torch.float32).contiguous()
    fsz = ctx[0, 0].numel()
    with torch.cuda.device(dev):
        _lib.check(L.gtav_add_noise(ctx.data_ptr(), nz.data_ptr(), alpha.data_ptr(), x_ctx.data_ptr(), n - 1, fsz, float(noise_abs_max),
                                    _lib.current_stream()))
    act = actions[:1].to(torch.float32) if actions is not None else None
    x = generate_latents(dit, x_ctx, n, ddim_noise_steps_inference, new_frame_noise, act, stabilization_level=lvl,
                         noise_abs_max=noise_abs_max, clamp_min=1e-6)
    x_old = torch.cat([x_ctx, new_frame_noise.to(dev, torch.float32)], dim=1).contiguous()      # the sequence before denoising
    with torch.cuda.device(dev):
        _lib.check(L.gtav_clamp_frames(x_old.data_ptr(), 1, n, n - 1, fsz, -float(noise_abs_max), float(noise_abs_max), _lib.current_stream()))
    return latents, x_old, x


# ------------------------------------------------------------------------------------------------------------------------
# Optimisation step.  Reference: train_dit.py:680 accelerator.backward, :232-260 AdamW + cosine schedule with
# warm-up and a floor, :965-970 clip_grad_norm_ / optimizer.step / scheduler.step / zero_grad; accelerate's DDP averages the
# gradients of the ranks.  Here: backward kernels into one contiguous gradient arena, ONE all-reduce over it (RCCL over xGMI:
# 2.4 GB of fp32 for DiT-S/2), clipping + AdamW fused on the GPU.
# ------------------------------------------------------------------------------------------------------------------------
def cosine_with_min_lr(step: int, base_lr: float, num_warmup_steps: int, num_training_steps: int, num_cycles: float = 0.25,
                       min_lr: float = 0.0) -> float:
    """transformers.get_cosine_with_min_lr_schedule_with_warmup as called at train_dit.py:253-260 (num_cycles=0.25): linear warm-up,
    then base_lr * (min_rate + (1 - min_rate) * 0.5 (1 + cos(2 pi cycles progress))), min_rate = min_lr / base_lr."""
    import math
    if step < num_warmup_steps:
        return base_lr * step / max(1, num_warmup_steps)
    progress = (step - num_warmup_steps) / max(1, num_training_steps - num_warmup_steps)
    factor = 0.5 * (1.0 + math.cos(math.pi * num_cycles * 2.0 * progress))
    rate = min_lr / base_lr
    return base_lr * max(0.0, factor * (1.0 - rate) + rate)


def all_reduce_gradients(dit, world_size: int):
    """Data-parallel gradient averaging (what DDP does under accelerate): ONE all-reduce (SUM) over the contiguous arena; the division by
    the world size is not a pass over the 2.4 GB arena but a factor of the optimizer's step coefficient (dit.grad_divisor ->
    gtav_dit_set_grad_divisor): arena / (loss scale x world) is the rank average."""
    if world_size > 1:
        import torch.distributed as dist
        dist.all_reduce(dit.grad_arena, op=dist.ReduceOp.SUM)
    dit.grad_divisor = float(max(1, world_size))


_BUCKET_PREFIXES = ("external_cond.", "t_embedder.", "x_embedder.")


def gradient_buckets(dit):
    """The all-reduce buckets of the overlapped backward, in the order their gradients become final: (phase after which the bucket is
    complete, arena offset, count).  One bucket per block (38 M floats = 151 MB for DiT-S/2: large enough for RCCL's ring over xGMI to run
    at link rate, small enough that 15 of the 16 hide behind the blocks still being differentiated), the final layer after phase 0, the
    embedders last.  The arena is laid out in lexicographic name order, so "blocks.<l>." is one contiguous slice.  Built and VALIDATED once per
    model (cached on it): the buckets must be disjoint and cover the arena — a model with parameters outside these prefixes fails here, before
    any collective is issued; prefixes the model does not have (external_cond_dim = 0) are skipped."""
    cached = getattr(dit, "_gradient_buckets", None)
    if cached is not None and cached[0] == dit.grad_arena.numel():
        return cached[1]
    L = dit.depth
    buckets = [(0,) + dit.param_range("final_layer.")]
    buckets += [(L - l,) + dit.param_range(f"blocks.{l}.") for l in reversed(range(L))]
    buckets += [(L + 1,) + dit.param_range(p) for p in _BUCKET_PREFIXES]
    buckets = [b for b in buckets if b[2] > 0]
    spans = sorted((off, off + cnt) for _, off, cnt in buckets)
    ok = spans and spans[0][0] == 0 and spans[-1][1] == dit.grad_arena.numel() and all(x[1] == y[0] for x, y in zip(spans, spans[1:]))
    if not ok:
        raise RuntimeError("gradient_buckets: the per-block / embedder slices do not tile the gradient arena (a parameter outside the known name "
                           f"prefixes?): spans {spans[:3]} ... {spans[-2:]}, arena {dit.grad_arena.numel()}")
    dit._gradient_buckets = (dit.grad_arena.numel(), buckets)
    return buckets


def backward_overlapped(dit, v_pred, v_target, world_size: int, comm_stream=None, all_reduce=None, bucket_timings=None):
    """backward_ in phases with the all-reduce (SUM) of each finished bucket enqueued on `comm_stream` while the compute stream differentiates
    the next block (what DDP's bucketed reducer does under accelerate).  `all_reduce(tensor)` defaults to
    torch.distributed.all_reduce (SUM) and may be gtav_amd.comm.Comm.all_reduce_.  The arena then holds the SUM over the ranks and
    dit.grad_divisor = world_size tells the optimizer (no pass over the arena).  `bucket_timings` (a list, measurement passes only) receives one
    (phase, bytes, start event, stop event) per bucket, recorded on the communication stream around its all-reduce."""
    if all_reduce is None:
        import torch.distributed as dist
        all_reduce = lambda t: dist.all_reduce(t, op=dist.ReduceOp.SUM)
    if comm_stream is None:
        comm_stream = getattr(dit, "_comm_stream", None)
        if comm_stream is None:
            comm_stream = dit._comm_stream = torch.cuda.Stream(device=dit.device)       # one per model, not one per step
    arena = dit.grad_arena
    buckets = gradient_buckets(dit)                                                     # validated: covers the arena
    L = dit.depth
    for phase in range(L + 2):
        dit.backward_phases_(v_pred, v_target, phase, phase + 1)
        ready = [b for b in buckets if b[0] == phase]
        if not ready or world_size == 1:
            continue
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dit.device))
        with torch.cuda.stream(comm_stream):
            comm_stream.wait_event(ev)
            for ph, off, cnt in ready:
                if bucket_timings is not None:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(comm_stream)
                all_reduce(arena[off: off + cnt])
                if bucket_timings is not None:
                    e1.record(comm_stream)
                    bucket_timings.append((ph, cnt * 4, e0, e1))
    if world_size > 1:
        torch.cuda.current_stream(dit.device).wait_stream(comm_stream)
    dit.grad_divisor = float(max(1, world_size))


@torch.inference_mode()
def training_step(dit, latents: torch.Tensor, actions: Optional[torch.Tensor], target_noise_idx=None, ctx_noise_idx=None, ctx_noise=None, noise=None,
                  lr: float = None, weight_decay: float = 0.0, max_grad_norm: float = 1.0, world_size: int = 1, noise_steps: int = 50,
                  n_prompt_frames: int = 4, noise_abs_max: float = 20.0, clamp_min: float = 1e-6, overlap_all_reduce: bool = True, comm_stream=None,
                  all_reduce=None, bucket_timings=None, rng=None, ctx_max_noise_idx: Optional[int] = None, action_keep=None):
    """One optimisation step on a batch of latent clips: for every target frame forward + loss and its backward (train_dit.py:590-680: each
    frame's loss is differentiated inside the frame loop, the gradients add up), gradient all-reduce (bucketed and overlapped with the LAST
    frame's backward pass when world_size > 1), clip, AdamW.  Returns the mean loss over the target frames, a (1,) tensor.
    rng / ctx_max_noise_idx: as forward_loss — the step draws its own noise indices and noise, the four draw arguments stay None.
    action_keep: as forward_loss — per-sample action dropout for classifier-free guidance (each rank draws its own samples' flags with draw_action_keep:
    nothing new is reduced across ranks)."""
    _rng.check_exclusive(rng, "training_step", target_noise_idx=target_noise_idx, ctx_noise_idx=ctx_noise_idx, ctx_noise=ctx_noise, noise=noise)
    if rng is not None and ctx_max_noise_idx is None:
        raise ValueError("training_step: rng= needs ctx_max_noise_idx (the upper end of the context noise index, config.ctx_max_noise_idx)")
    if lr is None:
        raise TypeError("training_step: lr is required")
    dit.zero_grad()
    n_iter = latents.shape[1] - n_prompt_frames
    overlap = world_size > 1 and overlap_all_reduce

    def on_frame(k, v_pred, v_target):
        if overlap and k == n_iter - 1:
            backward_overlapped(dit, v_pred, v_target, world_size, comm_stream, all_reduce, bucket_timings)
        else:
            dit.backward_(v_pred, v_target)

    loss, _, _ = forward_loss(dit, latents, actions, target_noise_idx, ctx_noise_idx, ctx_noise, noise, noise_steps, n_prompt_frames,
                              noise_abs_max, clamp_min, keep_activations=True, on_frame=on_frame, rng=rng, ctx_max_noise_idx=ctx_max_noise_idx,
                              action_keep=action_keep)
    if not overlap:
        all_reduce_gradients(dit, world_size)
    dit.adamw_step(lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    return loss


def draw_action_keep(B: int, p: float = 0.1, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The keep flags of per-sample action dropout (the reference's commented-out train_dit.py:704-705 drops the actions with probability 0.1): (B,) int32 on the
    host, 0 with probability p.  Drawn from `generator` (a CPU torch.Generator; None: the global one), so a seeded run repeats its mask."""
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"draw_action_keep: p={p} is not a probability")
    return (torch.rand(B, generator=generator) >= p).to(torch.int32)


ERR_F16_SAT = 2      # csrc/common.h: the saturation bit of a device error word


def merge_range_words(words, world_size: int = 1, all_reduce=None):
    """The data-parallel merge of the sticky saturation words (DiT.train_range_words(), one per layer group): the element-wise maximum over the ranks of whether
    the group saturated, so that every rank derives the SAME list of groups to switch — the union of the ranks' lists — as every rank takes the same overflow skip.
    Pure host code: `all_reduce(tensor)` reduces an int32 CPU tensor in place with MAX (default: torch.distributed.all_reduce(op=MAX), which gloo serves).
    Returns (merged words as a list of ints, the groups whose saturation bit is set)."""
    t = torch.tensor([1 if int(w) & ERR_F16_SAT else 0 for w in words], dtype=torch.int32)
    rest = torch.tensor([int(w) & ~ERR_F16_SAT for w in words], dtype=torch.int32)      # other bits stay this rank's: they are reported, not acted on
    if world_size > 1:
        if all_reduce is None:
            import torch.distributed as dist
            all_reduce = lambda x: dist.all_reduce(x, op=dist.ReduceOp.MAX)
        all_reduce(t)
    merged = [int(r) | (ERR_F16_SAT if int(v) else 0) for v, r in zip(t.tolist(), rest.tolist())]
    return merged, [g for g, v in enumerate(t.tolist()) if v]


def autorange_step(dit, world_size: int = 1, all_reduce=None):
    """Between two optimisation steps of a DiT(trainable=True, train_range_policy="auto"): reads this rank's sticky words, merges them over the ranks
    (merge_range_words) and switches the fp16 layer groups that saturated in a training forward on ANY rank to bf16 operands.  Returns the switched groups,
    the same list on every rank.  Raises what DiT.train_autorange raises (after the switch)."""
    merged, _ = merge_range_words(dit.train_range_words(), world_size, all_reduce)
    return dit.train_autorange(merged)


class LossScaler:
    """Dynamic loss scale for the fp16 backward pass (the reference trains under bf16 autocast and needs none).  The optimizer step skips
    itself on the device when a gradient overflowed (non-finite norm or a saturated fp16 store: gtav_dit_adamw_step); every `check_every`
    steps this reads the skip counter (one synchronisation) and halves the scale if steps were skipped since the last check, or doubles it
    after `growth_interval` clean steps — torch.cuda.amp.GradScaler's policy at a coarser cadence.
    On a train_range_policy="auto" model skipped steps are first put to autorange_step (world_size / all_reduce: its data-parallel arguments): when a layer
    group switched to bf16 the skips were a range problem of the forward, which no loss scale cures, and the scale is left alone for that interval."""

    def __init__(self, dit, check_every: int = 50, growth_interval: int = 2000, min_scale: float = 1.0, max_scale: float = 2.0 ** 24, world_size: int = 1,
                 all_reduce=None):
        self.dit, self.check_every, self.growth_interval = dit, int(check_every), int(growth_interval)
        self.world_size, self.all_reduce = int(world_size), all_reduce
        self.switched = []                   # the groups the last update() moved to bf16
        self.min_scale, self.max_scale = float(min_scale), float(max_scale)
        self._calls = 0
        self._clean = 0
        # the counter's value when this scaler starts watching (a resumed run restores it from the checkpoint); a handle that is not built yet
        # gives it on the first update instead
        try:
            self._skipped_seen = int(dit.train_stats()[1]) if getattr(dit, "_handle", None) else None
        except Exception:
            self._skipped_seen = None

    def update(self) -> float:
        """Call once per optimisation step (after adamw_step).  Returns the loss scale the NEXT step will use."""
        self._calls += 1
        if self._calls % self.check_every:
            return self.dit.loss_scale
        _, skipped, _ = self.dit.train_stats()
        if self._skipped_seen is None:
            # first look at the counter: a resumed run restores it from the checkpoint (set_opt_step) — steps skipped BEFORE this scaler existed
            # say nothing about the restored loss scale
            self._skipped_seen = skipped
            return self.dit.loss_scale
        self.switched = []
        if skipped > self._skipped_seen and getattr(self.dit, "train_range_policy", "report") == "auto":
            self.switched = autorange_step(self.dit, self.world_size, self.all_reduce)
        if self.switched:
            self._clean = 0
        elif skipped > self._skipped_seen:
            self.dit.loss_scale = max(self.min_scale, self.dit.loss_scale * 0.5)
            self._clean = 0
        else:
            self._clean += self.check_every
            if self._clean >= self.growth_interval:
                self.dit.loss_scale = min(self.max_scale, self.dit.loss_scale * 2.0)
                self._clean = 0
        self._skipped_seen = skipped
        return self.dit.loss_scale


# ------------------------------------------------------------------------------------------------------------------------
# Checkpoint / resume (reference train_dit.py:746-849): `save_model` = the weights alone as one .safetensors with the reference's key
# names (train_dit.py:758-762); `save_checkpoint` = accelerator.save_state (model + optimizer) + step.json {step, epoch}; `load_checkpoint`
# = load_state + step.json, then the caller skips `steps_in_epoch * gradient_accumulation_steps` batches (train_dit.py:841-843).
# ------------------------------------------------------------------------------------------------------------------------
def ema_decay_at(n: int, decay: float, warmup: bool = False) -> float:
    """The decay d_n the optimizer launch applies to the averaged weights at applied step n >= 1 (DiT(train_ema_decay=decay, train_ema_warmup=warmup)): `decay`
    rounded to float32, or with warm-up min(decay, (1 + n) / (10 + n)) — computed in float32 exactly as the device computes it (both sums are exact integers,
    the division is correctly rounded), returned as a Python float holding that float32 value."""
    import numpy as np
    if int(n) < 1 or int(n) >= 1 << 24:
        raise ValueError(f"ema_decay_at: applied step n={n} (the first applied step is 1; the device keeps the count as an exact fp32 integer, below 2^24)")
    d = np.float32(decay)
    if not 0.0 < float(d) < 1.0:
        raise ValueError(f"ema_decay_at: decay={decay} outside (0, 1)")
    if warmup:
        d = min(d, np.float32(1 + int(n)) / np.float32(10 + int(n)))
    return float(d)


def save_model(dit, path: str, ema: bool = False):
    """train_dit.py:746-763: weights only, safetensors, reference key names (incl. the de-duplicated rotary `freqs`).  ema=True: the averaged weights of a
    DiT(train_ema_decay=...) in the same layout — the file an inference model loads to sample from the average."""
    from . import weights as _w
    if ema:
        if getattr(dit, "lora_rank", None):
            raise _lib.GtavError("save_model(ema=True): this DiT averages its low-rank adapters, not the weights; save them with save_lora(dit, path, ema=True)")
        _w.save_state_dict_file(dit.ema_state_dict(), path)
        return
    if getattr(dit, "_trainable", False) and dit._handle:
        dit.pull_weights()
    _w.save_state_dict_file(dit.state_dict(), path)


def _lora_meta(dit):
    """{"rank", "alpha"} of a LoRA model (DiT(train_lora_rank=...)), None for any other."""
    rank = getattr(dit, "lora_rank", None)
    return {"rank": int(rank), "alpha": float(dit.lora_alpha)} if rank else None


def save_lora(dit, path: str, ema: bool = False):
    """The adapters of a LoRA model alone as one .safetensors (a few MB beside the caller's frozen checkpoint); metadata {"rank", "alpha"}, as strings.
    ema=True: the averaged adapters of a DiT(train_lora_rank=..., train_ema_decay=...) under the same keys."""
    from safetensors.torch import save_file
    meta = _lora_meta(dit)
    if meta is None:
        raise _lib.GtavError("save_lora: this DiT has no adapters (construct it with trainable=True, train_lora_rank=...)")
    sd = dit.ema_state_dict() if ema else dit.lora_state_dict()
    save_file({k: v.contiguous() for k, v in sd.items()}, path, metadata={k: repr(v) for k, v in meta.items()})


def _operand_dtype_name(dit) -> str:
    """step.json's "operand_dtype": the training step's operand type ("bf16" for DiT(train_dtype=torch.bfloat16), else "fp16")."""
    return "bf16" if getattr(dit, "train_dtype", torch.float16) == torch.bfloat16 else "fp16"


def _step_state(dit, global_step: int, epoch: int) -> dict:
    """step.json's own fields: "operand_dtype" is the type the training handle started on, "bf16_groups" the layer groups that run on bf16 operands now (all of
    them on a bf16 handle, none on an fp16 one, some after train_autorange / train_set_group_dtype on a train_range_policy="auto" model)."""
    bf16 = [g for g, d in enumerate(dit.operand_dtypes()) if d == torch.bfloat16] if hasattr(dit, "operand_dtypes") else []
    return {"step": int(global_step), "epoch": int(epoch), "loss_scale": float(dit.loss_scale), "operand_dtype": _operand_dtype_name(dit), "bf16_groups": bf16}


def _restore_groups(dit, state: dict):
    """load_state, before any weight reaches the handle: a checkpoint with SOME groups on bf16 needs a model that can hold them (DiT.restore_operand_groups
    raises by name on one that cannot); a train_range_policy="auto" model takes the checkpoint's groups whatever they are."""
    groups = state.get("bf16_groups")
    if groups is None:
        return
    n = getattr(dit, "n_operand_groups", len(groups))
    if 0 < len(groups) < n or getattr(dit, "train_range_policy", "report") == "auto":
        dit.restore_operand_groups(groups)


def save_state(dit, ckpt_dir: str, global_step: int, epoch: int, extra: Optional[dict] = None, rng=None):
    """A LoRA model (DiT(train_lora_rank=...)) writes <dir>/lora.safetensors (the adapters; no model.safetensors: the base is the caller's frozen checkpoint), the
    adapters' moments and step.json with "lora": {"rank", "alpha"}; load_state restores the three into a LoRA model of the same rank, onto whatever base it holds.
    A model with averaged weights (DiT(train_ema_decay=...)) also writes <dir>/ema.safetensors and step.json's "ema": {"decay", "warmup"}; load_state restores the
    average after the weights, leaves it equal to the loaded weights when the checkpoint has none, and ignores the file on a model without a shadow.
    train_dit.py:765-800 `save_checkpoint`: <dir>/model.safetensors (fp32 masters), <dir>/optimizer.safetensors (AdamW moments + step
    counters), <dir>/step.json {"step", "epoch", "loss_scale", "operand_dtype", "bf16_groups", ...}.  Rank 0 writes; the caller barriers around it like the reference.
    rng (a NoiseSource): its {"seed", "draw"} goes into step.json as "rng" — the whole noise stream of the resumed run."""
    import json
    import os
    from safetensors.torch import save_file
    os.makedirs(ckpt_dir, exist_ok=True)
    lora = _lora_meta(dit)
    # a LoRA model: lora.safetensors (the adapters) in place of model.safetensors — the base is the caller's frozen checkpoint —, the adapters' moments, and
    # step.json's "lora": {"rank", "alpha"}
    if lora is not None:
        save_lora(dit, os.path.join(ckpt_dir, "lora.safetensors"))
        extra = dict(extra or {}, lora=lora)
    else:
        save_model(dit, os.path.join(ckpt_dir, "model.safetensors"))
    save_file({k: v.contiguous() for k, v in dit.opt_state_dict().items()}, os.path.join(ckpt_dir, "optimizer.safetensors"))
    # a model with averaged weights: ema.safetensors (the trainable tensors' fp32 shadow) and step.json's "ema": {"decay", "warmup"}
    if getattr(dit, "ema_decay", None) is not None:
        shapes = dit._train_shapes()
        save_file({k: v.contiguous() for k, v in dit.ema_state_dict().items() if k in shapes}, os.path.join(ckpt_dir, "ema.safetensors"))
        extra = dict(extra or {}, ema={"decay": float(dit.ema_decay), "warmup": bool(dit.ema_warmup)})
    state = _step_state(dit, global_step, epoch)
    state.update(extra or {})
    if rng is not None:
        state["rng"] = rng.state_dict()
    with open(os.path.join(ckpt_dir, "step.json"), "w") as f:
        json.dump(state, f)


def load_state(dit, ckpt_dir: str, steps_per_epoch: Optional[int] = None, gradient_accumulation_steps: int = 1, rng=None) -> dict:
    """train_dit.py:802-849 `load_checkpoint`: restores weights, AdamW state and the loss scale into `dit` (trainable=True) and returns
    step.json's dict plus "skip_iter" = (step % steps_per_epoch) * gradient_accumulation_steps, the number of batches of the current
    epoch the resumed loop has to skip (train_dit.py:841-843), when steps_per_epoch is given.  rng (a NoiseSource) is set to the checkpoint's
    "rng" entry; a checkpoint without one leaves it untouched."""
    import json
    import os
    from safetensors.torch import load_file
    from . import weights as _w
    with open(os.path.join(ckpt_dir, "step.json")) as f:
        state = json.load(f)
    lora, ck = _lora_meta(dit), state.get("lora")
    if lora is not None and ck is None:
        raise _lib.GtavError(f"load_state: {ckpt_dir} is a full checkpoint (model.safetensors, every parameter's moments) and this DiT trains rank-{lora['rank']} "
                             "adapters on a frozen base: load its model.safetensors with load_state_dict and start the adapters afresh")
    if lora is None and ck is not None:
        raise _lib.GtavError(f"load_state: {ckpt_dir} is a LoRA checkpoint (rank {ck['rank']} adapters, no base weights) and this DiT trains every parameter: "
                             f"construct it with trainable=True, train_lora_rank={ck['rank']}")
    if lora is not None and int(ck["rank"]) != lora["rank"]:
        raise _lib.GtavError(f"load_state: the checkpoint's adapters have rank {ck['rank']}, this DiT's rank {lora['rank']}")
    _restore_groups(dit, state)              # (first: the masters below are converted into each group's type as they are sent)
    if lora is not None:
        dit.load_lora_state_dict(_w.load_state_dict_file(os.path.join(ckpt_dir, "lora.safetensors")))
    else:
        dit.load_state_dict(_w.load_state_dict_file(os.path.join(ckpt_dir, "model.safetensors")))
    dit.load_opt_state_dict(load_file(os.path.join(ckpt_dir, "optimizer.safetensors")))
    # the averaged weights, after the weights (whose upload set the average to them: what a checkpoint without ema.safetensors leaves); a model without a
    # shadow ignores the file
    if getattr(dit, "ema_decay", None) is not None and os.path.exists(os.path.join(ckpt_dir, "ema.safetensors")):
        dit.load_ema_state_dict(load_file(os.path.join(ckpt_dir, "ema.safetensors")))
    # the loss scale belongs to the operand type it was found for: a bf16 run's scale (1 by default) would let an fp16 backward underflow, so it is restored
    # only into a handle of the same type (a checkpoint without "operand_dtype" is fp16).  The masters and moments are fp32 and load either way.
    if "loss_scale" in state and state.get("operand_dtype", "fp16") == _operand_dtype_name(dit):
        dit.loss_scale = float(state["loss_scale"])
    if rng is not None and "rng" in state:
        rng.load_state_dict(state["rng"])
    if steps_per_epoch:
        state["skip_iter"] = (state["step"] % int(steps_per_epoch)) * int(gradient_accumulation_steps)
    return state
