"""Play sessions: one generated frame per call, for as long as the caller likes, in constant memory.

generate_latents needs the length of the clip and its whole action track before the first frame.  A PlaySession keeps the last max_frames frames and their
actions in two rings (absolute frame f lives in slot f % F, F = dit.max_frames) and runs every frame through generate.denoise_frame — the per-frame body of
generate_latents — on the ring form of the fused sampler step (include/gtav_amd.h: start > cur).  No frame is ever moved, and frame k of a session is bit for
bit the generated frame k of the clip generate_latents makes from the same prompt, actions and noise."""
from __future__ import annotations

from typing import Optional

import torch

from . import generate as _gen
from . import lib as _lib
from .rng import check_exclusive
from .utils import alphas_cumprod as _alphas_cumprod

DECODE_MODES = ("sync", None)


def ring_window(n_seen: int, F: int):
    """(start, cur, T) of the window that generates absolute frame `n_seen` (the clip holds frames 0 .. n_seen - 1) in a ring of F slots: the window
    generate_latents uses, [max(0, n_seen + 1 - F), n_seen], with both ends taken modulo F.  start > cur is the ring form of the sampler step."""
    if F < 1 or n_seen < 0:
        raise ValueError(f"ring_window: n_seen={n_seen}, F={F}")
    first = max(0, n_seen + 1 - F)
    return first % F, n_seen % F, n_seen - first + 1


def ring_slot(f: int, F: int) -> int:
    """The ring slot of absolute frame f.  Its noise is stream slot f itself (gtav_rng_normal's slot0): what generate_latents(rng=) draws for frame f."""
    return f % F


def check_session_args(*, n_latents, n_frames, has_vae, has_prompt_actions, guidance_scale, decode):
    """The argument rules of PlaySession(), before anything touches the device.  n_latents / n_frames: the frame count of prompt_latents / prompt_frames, None
    where not given."""
    if (n_latents is None) == (n_frames is None):
        raise ValueError("PlaySession: give exactly one of prompt_latents and prompt_frames")
    if (n_latents if n_frames is None else n_frames) < 1:
        raise ValueError("PlaySession: the prompt is empty (the first generated frame needs at least one context frame)")
    if n_frames is not None and not has_vae:
        raise ValueError("PlaySession: prompt_frames needs a vae to encode them")
    if decode not in DECODE_MODES:
        raise ValueError(f"PlaySession: decode={decode!r} (one of 'sync', None; a decode on a second stream was measured slower than 'sync' and is not "
                         "offered: profiles/play/frame_time.txt)")
    if decode is not None and not has_vae:
        raise ValueError(f"PlaySession: decode={decode!r} needs a vae (decode=None returns latents)")
    if guidance_scale is not None and not has_prompt_actions:
        raise ValueError("PlaySession: guidance_scale needs actions (guidance pushes the frame from the action-free prediction towards the conditioned one): "
                         "give prompt_actions")


def check_step_args(*, rng, has_actions, action, noise):
    """The argument rules of PlaySession.step(): the draw comes from exactly one of the session's rng and noise=; a session that was given prompt_actions
    takes an action with every step, one without takes none."""
    check_exclusive(rng, "PlaySession.step", noise=noise)
    if has_actions and action is None:
        raise ValueError("PlaySession.step: this session was given prompt_actions: every step needs an action (B, A)")
    if not has_actions and action is not None:
        raise ValueError("PlaySession.step: this session has no actions (prompt_actions=None): action must be None")


class PlaySession:
    """PlaySession(dit, vae=None, *, prompt_latents | prompt_frames, prompt_actions=None, noise_steps, rng=None, ...); use as a context manager or close() it.

    prompt_latents (B, n, C, h, w), or prompt_frames (B, n, 3, H, W) in [0, 1] encoded by `vae`; prompt_actions (B, n, A) or None.  Of a prompt longer than
    F - 1 frames only the last F - 1 enter the ring: the frames generate_latents' window would see.
    rng: a NoiseSource — the session takes ONE draw number here and fills frame f from stream slot f, clamp included, as generate_latents(rng=) does.  Without
    it every step(noise=) brings its own standard-normal draw (B, C, h, w).
    ctx_cache / hoist_cond / stabilization_level / noise_abs_max / clamp_min / guidance_scale: as in generate_latents (ctx_cache defaults to True here).  The
    model's own guidance setting comes back at close().
    decode: None — step returns the latent frame; "sync" — latents_to_tokens + vae.decode + frames_to_u8 of the finished frame on the current stream.
    (The same three calls on a second stream, beside the next frame's steps, made every frame slower, not faster: profiles/play/frame_time.txt)
    Under the model's range_policy="auto" a frame whose fp16 stores saturated is made again from its own initial noise on the switched operand types (one
    dit.check(), a device synchronisation, per frame); under "report" the session never synchronises for it and check() is the caller's."""

    def __init__(self, dit, vae=None, *, prompt_latents=None, prompt_frames=None, prompt_actions=None, noise_steps: int, rng=None,
                 stabilization_level: int = 15, noise_abs_max: float = 20.0, clamp_min: float = 1e-4, ctx_cache: bool = True, hoist_cond: bool = True,
                 guidance_scale: Optional[float] = None, decode: Optional[str] = "sync"):
        check_session_args(n_latents=None if prompt_latents is None else prompt_latents.shape[1],
                           n_frames=None if prompt_frames is None else prompt_frames.shape[1], has_vae=vae is not None,
                           has_prompt_actions=prompt_actions is not None, guidance_scale=guidance_scale, decode=decode)
        self.dit, self.vae, self.rng, self.decode = dit, vae, rng, decode
        self.noise_steps, self.stabilization_level, self.noise_abs_max = int(noise_steps), int(stabilization_level), float(noise_abs_max)
        self.ctx_cache, self.hoist_cond = bool(ctx_cache), bool(hoist_cond)
        if prompt_latents is None:
            prompt_latents = _gen.vae_encode(prompt_frames.to(vae.device), vae, prompt_frames.shape[1])
        dev = dit.device
        B, n_prompt = prompt_latents.shape[:2]
        if prompt_actions is not None and tuple(prompt_actions.shape[:2]) != (B, n_prompt):
            raise ValueError(f"PlaySession: prompt_actions {tuple(prompt_actions.shape)} for a prompt of {B} x {n_prompt} frames")
        self.F = F = int(dit.max_frames)
        # the two rings (ordinary tensors, not inference tensors: restore() and the caller's own code may write them outside inference mode)
        self._x = torch.zeros((B, F, *prompt_latents.shape[2:]), device=dev, dtype=torch.float32)
        self._act = None if prompt_actions is None else torch.zeros((B, F, prompt_actions.shape[2]), device=dev, dtype=torch.float32)
        self._first = n_prompt - min(n_prompt, F - 1)                          # oldest absolute frame the ring holds
        for f in range(self._first, n_prompt):                                 # copies only: torch is storage here
            self._x[:, ring_slot(f, F)] = prompt_latents[:, f].to(dev, torch.float32)
            if self._act is not None:
                self._act[:, ring_slot(f, F)] = prompt_actions[:, f].to(dev, torch.float32)
        self._frame = n_prompt - 1
        self._fsz = self._x[0, 0].numel()
        # staging: the frame's draw (explicit noise is clamped here; under range_policy "auto" it is what a redo starts from), the step's action, and the
        # finished frame on its way to the decoder
        self._noise0 = torch.empty((B, 1, *self._x.shape[2:]), device=dev, dtype=torch.float32)
        self._act_in = None if self._act is None else torch.empty((B, self._act.shape[2]), device=dev, dtype=torch.float32)
        self._stage = torch.empty_like(self._noise0) if decode is not None else None
        self._draw = rng.next_draw() if rng is not None else None
        self._t_of, self._order = _gen.noise_schedule(self.noise_steps)
        self._was_guidance = dit._guidance
        self._closed = False
        try:
            if guidance_scale is not None:
                dit.set_guidance(guidance_scale)
            dit.set_schedule(_alphas_cumprod(clamp_min))
            dit._internal_batch(B)                                             # (a guided session on a model that is too small is refused here, not grown)
            dit.reserve(B, F, self.noise_steps if self.hoist_cond else 0)      # one handle for the whole session: its captured steps stay
        except BaseException:
            self.close()                                                       # (the model's own guidance setting back)
            raise

    # ------------------------------------------------------------------------------------------
    @property
    def frame_index(self) -> int:
        """Absolute index of the last finished frame (the prompt's last frame before the first step)."""
        return self._frame

    def window(self) -> torch.Tensor:
        """(B, T, C, h, w): a copy of the frames the ring holds, oldest first."""
        first = max(self._first, self._frame - self.F + 1)
        idx = torch.tensor([ring_slot(f, self.F) for f in range(first, self._frame + 1)], device=self._x.device)
        return self._x.index_select(1, idx)

    def snapshot(self) -> dict:
        """The session's state: both rings, the frame index and the noise position."""
        return {"x": self._x.clone(), "act": None if self._act is None else self._act.clone(), "frame": self._frame, "first": self._first,
                "draw": self._draw}

    def restore(self, s: dict):
        """Back to a snapshot of THIS session, copied into the same buffers: the pointers, and with them the captured steps, stay."""
        self._x.copy_(s["x"])
        if self._act is not None:
            self._act.copy_(s["act"])
        self._frame, self._first, self._draw = s["frame"], s["first"], s["draw"]

    def check(self):
        """dit.check() (and vae.check() when the session decodes): raises if an fp16 activation saturated; synchronises."""
        self.dit.check()
        if self.decode is not None:
            self.vae.check()

    def close(self):
        if not self._closed:
            self._closed = True
            if self.dit._guidance != self._was_guidance:
                self.dit.set_guidance(self._was_guidance)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def step(self, action: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Generates the next frame: uint8 (B, H, W, 3), or the latents (B, C, h, w) when decode is None.  action (B, A) is appended to the action ring before
        the frame is made; noise (B, C, h, w) is the frame's standard-normal draw on a session without rng."""
        check_step_args(rng=self.rng, has_actions=self._act is not None, action=action, noise=noise)
        if self._closed:
            raise RuntimeError("PlaySession.step: the session is closed")
        L, dit, x, F = _lib.load(), self.dit, self._x, self.F
        B, i = x.shape[0], self._frame + 1
        start, cur, _ = ring_window(i, F)
        if action is not None:
            self._act_in.copy_(action.reshape(self._act_in.shape))
            self._act[:, cur].copy_(self._act_in)
        auto = getattr(dit, "range_policy", "report") == "auto"
        with torch.cuda.device(x.device):
            if self.rng is not None:                                           # generate.py:201-202 randn + clamp of frame i, in place in its slot
                _lib.check(L.gtav_rng_normal(x[:, cur].data_ptr(), F * self._fsz, B, self._fsz, self.rng.seed, self._draw, self.rng.sample0 & 0xFFFFFFFF,
                                             i & 0xFFFFFFFF, 1, self.noise_abs_max, _lib.current_stream()))
                if auto:
                    self._noise0[:, 0].copy_(x[:, cur])
            else:
                self._noise0.copy_(noise.reshape(self._noise0.shape))
                _lib.check(L.gtav_clamp_frames(self._noise0.data_ptr(), B, 1, 0, self._fsz, -self.noise_abs_max, self.noise_abs_max, _lib.current_stream()))
                x[:, cur].copy_(self._noise0[:, 0])
        for attempt in range(1 + (dit.n_operand_groups if auto else 0)):
            _gen.denoise_frame(dit, x, start, cur, self._t_of, self._order, self._act, self.stabilization_level, self.ctx_cache, self.hoist_cond)
            if not auto:
                break
            try:
                dit.check()
                break
            except _lib.GtavRangeSwitch:
                # the layers whose fp16 stores saturated run on bf16 operands from here on: this frame only is made again (each retry can only add layer
                # groups, so the loop ends); the frames before it stay as they were shown
                x[:, cur].copy_(self._noise0[:, 0])
        self._frame = i
        if self.decode is None:
            return x[:, cur].clone()
        return self._decode_frame(x[:, cur])

    def _decode_frame(self, lat: torch.Tensor) -> torch.Tensor:
        self._stage[:, 0].copy_(lat)
        return _gen.vae_decode_frames(self._stage, self.vae)[:, 0]
