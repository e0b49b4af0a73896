"""Drop-in mirror of the reference `model/dit.py` public surface (model/dit.py:228-392): `DiT`,
`DiT_S_2`, `DiT_models` — same constructor signature, `forward(x, t, external_cond)` call shape,
`max_frames` / `patch_size` attributes and state-dict names — with every FLOP executed by the HIP
kernels of libgtav_amd.so through the C-ABI (`gtav_dit_*`, include/gtav_amd.h).  torch is used for
storage (device tensors, the fp32 master copy of the weights) and host-side constant tables only.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from collections import OrderedDict
from typing import Dict, Iterator, Optional

import torch

from .. import lib as _lib
from .. import weights as _w


def _rope_tables_axial(freqs: torch.Tensor, gh: int, gw: int):
    """cos/sin tables (gh*gw, 64) of `RotaryEmbedding.get_axial_freqs(gh, gw)` for pixel freqs
    (model/rotary_embedding_torch.py:290-345), identity beyond the rotated dims."""
    def ang(n):
        a = torch.linspace(-1, 1, steps=n)[:, None] * freqs[None, :]
        return a.repeat_interleave(2, dim=-1)
    ah, aw = ang(gh), ang(gw)
    a = torch.cat([ah[:, None, :].expand(gh, gw, -1), aw[None, :, :].expand(gh, gw, -1)], dim=-1).reshape(gh * gw, -1)
    cos, sin = torch.ones(gh * gw, 64), torch.zeros(gh * gw, 64)
    cos[:, : a.shape[1]] = a.cos()
    sin[:, : a.shape[1]] = a.sin()
    return cos.contiguous(), sin.contiguous()


def _rope_tables_temporal(freqs: torch.Tensor, T: int):
    """`rotate_queries_or_keys` angles for positions 0..T-1 (rotary_embedding_torch.py:186-209)."""
    a = (torch.arange(T, dtype=torch.float32)[:, None] * freqs[None, :]).repeat_interleave(2, dim=-1)
    return a.cos().contiguous(), a.sin().contiguous()


def _timestep_table() -> torch.Tensor:
    """TimestepEmbedder.timestep_embedding for every t in [0, 999] (model/dit.py:96-118): (1000, 256)."""
    half = 128
    freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)
    args = torch.arange(1000, dtype=torch.float32)[:, None] * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1).contiguous()


def _checked_tensors(sd, shapes, who, *, strict=True, allow_unexpected=False, note=""):
    """The tensors of `sd` that the shape table names, as CPU fp32 contiguous copies in table order, each checked against its shape.  strict: a key the table
    has and `sd` lacks raises, and (unless allow_unexpected) so does one `sd` has and the table lacks; otherwise absent keys are left out."""
    if strict:
        dots = lambda keys: f"{keys[:5]}{'...' if len(keys) > 5 else ''}"
        missing = [k for k in shapes if k not in sd]
        unexpected = [] if allow_unexpected else [k for k in sd if k not in shapes]
        if missing or unexpected:
            raise RuntimeError(f"{who}: missing keys {dots(missing)}" + ("" if allow_unexpected else f", unexpected keys {dots(unexpected)}"))
    out = OrderedDict()
    for k, shp in shapes.items():
        if k in sd:
            v = sd[k].detach().to("cpu", torch.float32).contiguous()
            if tuple(v.shape) != tuple(shp):
                raise RuntimeError(f"{who}: {k} has shape {tuple(v.shape)}, expected {tuple(shp)}{note}")
            out[k] = v
    return out


_ALWAYS = object()     # a handle setting with this default is replayed onto every new handle


class _HipModule:
    """Shared plumbing of DiT / AutoencoderKL: fp32 master weights on the host, a C-ABI handle on the GPU."""

    _prefix = ""  # gtav_dit / gtav_vae
    # the settings that survive a re-created handle, in replay order: attribute -> (C setter, stage of handle creation that replays it, the default that
    # needs no call, value -> the setter's arguments).  A public setter is: validate, _set()
    _SETTINGS = {}

    def __init__(self):
        self._sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        self._handle = C.c_void_p(None)
        self._dirty = True
        self.training = False
        self.device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cuda")
        for attr, (_, _, default, _) in self._SETTINGS.items():
            setattr(self, attr, default)

    def _set(self, attr, value):
        """Records a handle setting and applies it to the handle if there is one."""
        setattr(self, attr, value)
        if self._handle:
            symbol, _, _, args = self._SETTINGS[attr]
            _lib.check(getattr(_lib.load(), symbol)(self._handle, *args(value)))

    def _replay(self, stage):
        """The recorded settings of one stage onto the handle, in table order."""
        for attr, (symbol, at, default, args) in self._SETTINGS.items():
            value = getattr(self, attr)
            if at == stage and value != default:
                _lib.check(getattr(_lib.load(), symbol)(self._handle, *args(value)))

    def _pull(self, symbol, shapes, ptrs=1, cpu=True):
        """name -> fp32 tensor (ptrs > 1: tuple of tensors) of the shapes in the table, each filled by `symbol(handle, name, ptr..., numel, stream)`."""
        fn, stream, out = getattr(_lib.load(), symbol), _lib.current_stream(), OrderedDict()
        with torch.cuda.device(self.device):
            for k, shp in shapes.items():
                d = [torch.empty(tuple(shp), device=self.device, dtype=torch.float32) for _ in range(ptrs)]
                _lib.check(fn(self._handle, k.encode(), *[t.data_ptr() for t in d], d[0].numel(), stream))
                if cpu:
                    d = [t.cpu() for t in d]
                out[k] = d[0] if ptrs == 1 else tuple(d)
        return out

    def _push(self, symbol, tensors, finalize=False, synchronize=True):
        """`symbol(handle, name, ptr..., numel, stream)` for every name -> tensor (or tuple of tensors) of the mapping, copied to the device as fp32; then
        the handle's finalize and a device synchronisation where asked."""
        L, stream = _lib.load(), _lib.current_stream()
        fn = getattr(L, symbol)
        with torch.cuda.device(self.device):
            for k, v in tensors.items():
                d = [t.to(self.device, torch.float32).contiguous() for t in (v if isinstance(v, tuple) else (v,))]
                _lib.check(fn(self._handle, k.encode(), *[t.data_ptr() for t in d], d[0].numel(), stream))
                del d
            if finalize:
                _lib.check(getattr(L, self._prefix + "_finalize")(self._handle, stream))
            if synchronize:
                torch.cuda.synchronize()

    # --- nn.Module-like surface the reference callers use (SURVEY.md §8(b) "Attributes read") ---
    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        self.training = mode
        return self

    def to(self, *args, **kwargs):
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, (str, torch.device)) and torch.device(a).type == "cuda":
                self.device = torch.device(a)
        return self

    def cuda(self, device=None):
        return self.to(torch.device("cuda", device if device is not None else torch.cuda.current_device()))

    def parameters(self) -> Iterator[torch.Tensor]:
        return iter(self._sd.values())

    def named_parameters(self):
        return iter(self._sd.items())

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        sd = OrderedDict(self._sd)
        sd.update(self._extra_state())
        return sd

    def _extra_state(self) -> Dict[str, torch.Tensor]:
        return {}

    def _shapes(self):
        raise NotImplementedError

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        params, sf, tf = _w.split_freq_keys(dict(sd))
        shapes = self._shapes()
        missing = [k for k in shapes if k not in params]
        unexpected = [k for k in params if k not in shapes]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing keys {missing[:5]}..., unexpected keys {unexpected[:5]}...")
        self._sd.update(_checked_tensors(params, shapes, "load_state_dict", strict=False))
        self._load_freqs(sf, tf)
        self._dirty = True
        return missing, unexpected

    def _load_freqs(self, sf, tf):
        pass

    def _free(self):
        if self._handle:
            getattr(_lib.load(), self._prefix + "_destroy")(self._handle)
            self._handle = C.c_void_p(None)

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass

    def _upload(self, extra: Dict[str, torch.Tensor]):
        self._push(self._prefix + "_set_weight", {**self._sd, **extra}, finalize=True)
        self._dirty = False


MAX_FRAMES = 32        # gtav_dit_create's range (include/gtav_amd.h gtav_dit_config.max_frames)
TRAIN_MAX_FRAMES = 8   # gtav_dit_train_enable's default; DiT(train_max_frames=n) raises it to n <= MAX_FRAMES (gtav_dit_train_allow_window)


def _train_options(trainable, max_frames, recompute, dtype, range_policy, lora_rank, lora_alpha, ema_decay, ema_warmup):
    """The seven train_* options of DiT(), checked and normalised: (train_max_frames or None, recompute, bf16 operands?, range policy, LoRA rank or None,
    LoRA alpha or None, EMA decay or None, EMA warm-up)."""
    # opt-in to training windows of up to train_max_frames frames (include/gtav_amd.h gtav_dit_train_allow_window); None: TRAIN_MAX_FRAMES.  The saved
    # activations are sized by max_batch x min(max_frames, train_max_frames): about 1.3 MB per token for DiT-S/2, 6 GB for one 32-frame sample
    if max_frames is not None:
        if not TRAIN_MAX_FRAMES <= int(max_frames) <= MAX_FRAMES:
            raise ValueError(f"train_max_frames={max_frames}: the training step serves windows of {TRAIN_MAX_FRAMES} to {MAX_FRAMES} frames")
        if not trainable:
            raise ValueError("train_max_frames needs trainable=True (an inference model serves windows of up to max_frames as it is)")
        max_frames = int(max_frames)
    # opt-in to activation recomputation (include/gtav_amd.h gtav_dit_train_set_recompute): the forward keeps the block inputs only and the backward re-runs
    # each block before differentiating it: the same bits as the default, 0.147 MB of saved activations per token instead of 1.31 for DiT-S/2, and a step
    # that takes 0.96 of a training forward longer (measured at batch 16 x 5 frames: 48.5 -> 62.7 ms)
    if recompute and not trainable:
        raise ValueError("train_recompute=True needs trainable=True (an inference model saves no activations)")
    # operand type of the training step (include/gtav_amd.h gtav_dit_train_enable_typed): torch.bfloat16 is the reference's `--mixed_precision bf16`
    # (fp32 range, no loss scaling needed), torch.float16 the default (loss-scaled)
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"train_dtype: {dtype} (torch.float16 or torch.bfloat16)")
    if dtype == torch.bfloat16 and not trainable:
        raise ValueError("train_dtype=torch.bfloat16 needs trainable=True (an inference model picks its operand type with set_operand_dtype)")
    # opt-in to operand groups of both types on the training handle (include/gtav_amd.h gtav_dit_train_allow_mixed): "auto" lets train_autorange() /
    # train_set_group_dtype() move single layer groups to bf16 while the run goes on; train_dtype is then the type every group starts on.  "report" (default):
    # one type for every group, a saturating forward skips every step (train_stats) and nothing switches
    if range_policy not in ("report", "auto"):
        raise ValueError("train_range_policy must be 'report' (one operand type for every layer group) or 'auto' (train_autorange() moves the layer groups "
                         "whose training forward saturated to bf16 operands)")
    if range_policy == "auto" and not trainable:
        raise ValueError("train_range_policy='auto' needs trainable=True (an inference model has range_policy)")
    # opt-in to low-rank adapter training on a frozen backbone (include/gtav_amd.h gtav_dit_train_set_lora): every half-block's to_qkv / to_out / fc1 / fc2 computes
    # with W0 + (alpha / rank) B A, the adapter pairs lora_A (rank, K) / lora_B (N, rank) are the only trainable parameters (grad, param_range, grad_arena and the
    # optimizer state see them alone); state_dict() / load_state_dict() mean the frozen base, lora_state_dict() / load_lora_state_dict() the adapters,
    # merged_state_dict() the reference-layout weights with the adapters folded in.  alpha defaults to the rank (scale 1)
    if lora_rank is None and lora_alpha is not None:
        raise ValueError("train_lora_alpha needs train_lora_rank")
    if lora_rank is not None:
        if not trainable:
            raise ValueError("train_lora_rank needs trainable=True (the adapters exist for the training step; run inference from merged_state_dict())")
        if int(lora_rank) != lora_rank or int(lora_rank) not in _w.LORA_RANKS:
            raise ValueError(f"train_lora_rank={lora_rank}: the adapters fill whole MFMA tiles, rank must be one of {_w.LORA_RANKS}")
        if range_policy == "auto":
            raise ValueError("train_lora_rank together with train_range_policy='auto' is not implemented (a type switch remakes the weight images from the "
                             "fp32 masters, without the adapters)")
        lora_alpha = float(lora_rank if lora_alpha is None else lora_alpha)
        if not (lora_alpha > 0.0 and math.isfinite(lora_alpha)):
            raise ValueError(f"train_lora_alpha={lora_alpha}: a positive number")
        lora_rank = int(lora_rank)
    # opt-in to averaged weights (include/gtav_amd.h gtav_dit_train_set_ema): the optimizer launch keeps ema <- d_n ema + (1 - d_n) w of every trainable parameter
    # in fp32 on the GPU, 4 bytes per trainable parameter more; d_n = train_ema_decay, or with train_ema_warmup min(decay, (1 + n) / (10 + n)) at applied step n
    # (gtav_amd.train.ema_decay_at).  ema_state_dict() / load_ema_state_dict() move the average, `with dit.ema_weights():` computes with it
    if ema_decay is None and ema_warmup:
        raise ValueError("train_ema_warmup needs train_ema_decay")
    if ema_decay is not None:
        if not trainable:
            raise ValueError("train_ema_decay needs trainable=True (the average is kept by the optimizer step; an inference model loads ema_state_dict())")
        ema_decay = float(ema_decay)
        if not 0.0 < ema_decay < 1.0:
            raise ValueError(f"train_ema_decay={ema_decay}: the decay of the averaged weights must lie in (0, 1)")
    return max_frames, bool(recompute), trainable and dtype == torch.bfloat16, range_policy, lora_rank, lora_alpha, ema_decay, bool(ema_warmup)


class DiT(_HipModule):
    """model/dit.py:228-376.  `max_batch` (keyword-only, not in the reference) pre-sizes the HBM workspace;
    it grows automatically when a larger batch arrives."""

    _prefix = "gtav_dit"
    # stages: "create" right after gtav_dit_create, "train" at the end of enabling training, "weights" after every weight upload
    _SETTINGS = {
        "_fused_temporal": ("gtav_dit_set_fused_temporal", "create", False, lambda v: (int(v),)),
        "_fused_spatial": ("gtav_dit_set_fused_spatial", "create", None, lambda v: (int(v),)),   # None: the library's default (on where the geometry allows)
        "_fold": ("gtav_dit_set_fold", "create", None, lambda v: v),                             # (experiments library only)
        "_weight_prefetch": ("gtav_dit_set_weight_prefetch", "create", None, lambda v: (v,)),
        "_weight_fill_policy": ("gtav_dit_set_weight_fill_policy", "create", None, lambda v: (v,)),
        # classifier-free guidance scale of the fused sampler step (set_guidance); None: off
        "_guidance": ("gtav_dit_set_guidance", "create", None, lambda v: (int(v is not None), 1.0 if v is None else v)),
        "_loss_scale": ("gtav_dit_set_loss_scale", "train", _ALWAYS, lambda v: (v,)),
        "_grad_divisor": ("gtav_dit_set_grad_divisor", "train", 1.0, lambda v: (v,)),
        "_schedule": ("gtav_dit_set_schedule", "weights", None, lambda v: (v, 1000)),            # (a C float[1000])
    }

    def __init__(self, input_h=18, input_w=32, patch_size=2, in_channels=16, hidden_size=1024, depth=12, num_heads=16,
                 mlp_ratio=4.0, external_cond_dim=25, max_frames=5, *, max_batch=1, init_weights=True, trainable=False, range_policy="report",
                 train_dtype=torch.float16, train_max_frames=None, train_recompute=False, train_range_policy="report", train_lora_rank=None,
                 train_lora_alpha=None, train_ema_decay=None, train_ema_warmup=False):
        super().__init__()
        self._trainable = bool(trainable)    # keyword-only, not in the reference: keeps fp32 masters, gradients and AdamW state on the GPU
        (self._train_max_frames, self._train_recompute, self._train_bf16, self.train_range_policy, self._lora_rank, self._lora_alpha, self._ema_decay,
         self._ema_warmup) = _train_options(self._trainable, train_max_frames, train_recompute, train_dtype, train_range_policy, train_lora_rank,
                                            train_lora_alpha, train_ema_decay, train_ema_warmup)
        # the longest window _ensure serves: a trainable handle's saved activations are sized for the training window
        self._window_limit = self._train_window if self._trainable else MAX_FRAMES
        self._ema_swapped = False
        self._lora_sd: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        self._lora_host_fresh = True         # the host copies of the adapters are the truth (until an optimizer step moves the handle's)
        self._grads = None
        self._loss_scale = 1.0 if self._train_bf16 else 65536.0
        self.in_channels = in_channels
        self.out_channels = in_channels
        self.patch_size = patch_size
        self.num_heads = num_heads
        if max_frames > MAX_FRAMES:
            raise ValueError(f"max_frames={max_frames}: the temporal attention serves windows of at most {MAX_FRAMES} frames")
        self._max_frames = max_frames
        self.input_h, self.input_w, self.hidden_size, self.depth = input_h, input_w, hidden_size, depth
        self.mlp_ratio, self.external_cond_dim = mlp_ratio, external_cond_dim
        self._cfg_kwargs = dict(input_h=input_h, input_w=input_w, patch_size=patch_size, in_channels=in_channels,
                                hidden_size=hidden_size, depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio,
                                external_cond_dim=external_cond_dim)
        # a trainable handle is never sized beyond the window the training step implements: _ensure refuses longer ones by name
        self._capacity_b, self._capacity_t = max_batch, min(max(max_frames, 1), self._window_limit)
        self._capacity_rows = 0
        hd = hidden_size // num_heads
        self._spatial_freqs = _w.rope_freqs_pixel(hd // 2, 256)   # model/dit.py:259-261
        self._temporal_freqs = _w.rope_freqs_lang(hd)             # model/dit.py:262
        # operand groups (include/gtav_amd.h "operand type"): 2 l / 2 l + 1 = spatial / temporal half of block l, 2 depth = patch embedding, 2 depth + 1 = final layer
        self.n_operand_groups = 2 * depth + 2
        self._bf16_groups = set(range(self.n_operand_groups)) if self._train_bf16 else set()
        self.range_policy = range_policy
        if range_policy not in ("report", "auto"):
            raise ValueError("range_policy must be 'report' (check() raises when an fp16 activation saturated) or 'auto' (check() moves the saturated "
                             "layers to bf16 operands and raises GtavRangeSwitch: recompute)")
        if init_weights:
            self.initialize_weights()
        if self._lora_rank:
            self.init_lora()

    @property
    def _train_window(self):
        """Longest window the training step of this model serves: TRAIN_MAX_FRAMES unless train_max_frames opted in to more."""
        return TRAIN_MAX_FRAMES if self._train_max_frames is None else self._train_max_frames

    # `max_frames` is read AND assigned by callers (generate.py:139,204)
    @property
    def max_frames(self):
        return self._max_frames

    @max_frames.setter
    def max_frames(self, v):
        if int(v) > MAX_FRAMES:   # before the handle is touched: the model stays as it was
            raise ValueError(f"max_frames={int(v)}: the temporal attention serves windows of at most {MAX_FRAMES} frames")
        self._max_frames = int(v)
        cap = min(int(v), self._train_window) if self._trainable else int(v)
        if cap > self._capacity_t:
            if self._handle and self._trainable and self._grads is not None:
                raise RuntimeError("a trainable DiT cannot grow its window after training was enabled: construct it with the largest max_frames")
            self._capacity_t = cap
            self._free()

    def _shapes(self):
        return _w.dit_param_shapes(**self._cfg_kwargs)

    def _lora_shapes(self):
        return _w.lora_param_shapes(self._lora_rank, **self._cfg_kwargs)

    def _train_shapes(self):
        """The trainable parameters: every parameter, or on a LoRA model the adapters alone."""
        return self._lora_shapes() if self._lora_rank else self._shapes()

    def _extra_state(self):
        # same de-duplicated aliases the reference's own writer keeps (train_dit.py:758-762)
        return {"spatial_rotary_emb.freqs": self._spatial_freqs, "temporal_rotary_emb.freqs": self._temporal_freqs}

    def _load_freqs(self, sf, tf):
        if sf is not None:
            self._spatial_freqs = sf.detach().float().cpu()
        if tf is not None:
            self._temporal_freqs = tf.detach().float().cpu()

    def initialize_weights(self):
        """Distribution-identical restatement of model/dit.py:295-326 (N(0,.02) linears, zero biases,
        t-MLP std .01, adaLN zeroed, final adaLN std .01, final linear std .001)."""
        for k, shp in self._shapes().items():
            if k.endswith(".bias"):
                v = torch.zeros(shp)
            elif "adaLN_modulation" in k and k.startswith("blocks."):
                v = torch.zeros(shp)
            elif k.startswith("t_embedder.mlp") or k.startswith("final_layer.adaLN_modulation"):
                v = torch.randn(shp) * 0.01
            elif k == "final_layer.linear.weight":
                v = torch.randn(shp) * 0.001
            else:
                v = torch.randn(shp) * 0.02
            self._sd[k] = v
        self._dirty = True

    # ------------------------------------------------------------------------------------------
    def _ensure(self, B: int, T: int, cond_rows: int = 0):
        """A handle with room for B x T frames (and cond_rows conditioning rows) that holds the current weights.  The usual call (handle there, nothing
        dirty, no growth) is the four tests below and nothing else."""
        if T > self._window_limit:           # window limits first, before a handle is rebuilt or destroyed
            self._refuse_window(T)
        if (cond_rows > max(self._capacity_rows, self._capacity_b * self._capacity_t)) or T > self._capacity_t or B > self._capacity_b:
            self._grow(B, T, cond_rows)
        if not self._handle:
            self._create_handle()
        if self._dirty:
            self._sync_weights()

    def _refuse_window(self, T):
        if T > MAX_FRAMES:
            raise ValueError(f"a window of {T} frames: the temporal attention serves at most {MAX_FRAMES} (max_frames <= {MAX_FRAMES})")
        if self._train_max_frames is not None:
            raise ValueError(f"a window of {T} frames on a trainable DiT constructed with train_max_frames={self._train_max_frames}: the handle's saved "
                             f"activations are sized for at most {self._train_max_frames} frames (train_max_frames <= {MAX_FRAMES})")
        raise ValueError(f"a window of {T} frames on a trainable DiT: the training step (backward temporal attention, adaLN-gradient reduction) is "
                         f"implemented for at most {TRAIN_MAX_FRAMES} frames; windows up to {MAX_FRAMES} need trainable=False")

    def _grow(self, B, T, cond_rows):
        """Raises the capacities to what the call needs and drops the handle, or refuses."""
        if self._handle and self._trainable and self._grads is not None:
            # the fp32 masters and the AdamW state live only in the handle: refuse BEFORE anything is destroyed (the handle stays usable)
            raise RuntimeError(f"a trainable DiT cannot grow its workspace after training was enabled (batch {B} > {self._capacity_b}, window {T} > "
                               f"{self._capacity_t} or {cond_rows} conditioning rows > {max(self._capacity_rows, self._capacity_b * self._capacity_t)}): "
                               "size it with max_batch / max_frames / reserve() before the first step")
        self._capacity_rows = max(self._capacity_rows, cond_rows)
        self._capacity_t = max(self._capacity_t, T)
        self._capacity_b = max(self._capacity_b, B)
        self._free()

    def _create_handle(self):
        L = _lib.load()
        cfg = _lib.DitConfig(max_frames=self._capacity_t, max_batch=self._capacity_b,
                             max_cond_rows=max(self._capacity_b * self._capacity_t, self._capacity_rows), **self._cfg_kwargs)
        with torch.cuda.device(self.device):
            _lib.check(L.gtav_dit_create(C.byref(cfg), C.byref(self._handle)))
            self._replay("create")
            if not self._train_mixed:
                for g in sorted(self._bf16_groups):                      # a re-created handle keeps the operand types chosen before
                    _lib.check(L.gtav_dit_set_operand_dtype(self._handle, g, 1))
            if self._trainable:
                self._enable_training(L)
        self._dirty = True
        self._lora_host_fresh = True         # (a new handle holds no adapters yet: the host copies are all there is)
        self._ema_swapped = False

    def _enable_training(self, L):
        """Training on a new handle; the order matters."""
        if self._lora_rank:                                              # (first: the adapters are then what train_param_count counts)
            _lib.check(L.gtav_dit_train_set_lora(self._handle, self._lora_rank, self._lora_alpha))
        if self._ema_decay is not None:
            _lib.check(L.gtav_dit_train_set_ema(self._handle, self._ema_decay, int(self._ema_warmup)))
        n = C.c_int64(0)
        _lib.check(L.gtav_dit_train_param_count(self._handle, C.byref(n)))
        # one contiguous fp32 gradient arena owned by torch: a single all-reduce covers the whole model (train.py)
        self._grads = torch.zeros(n.value, device=self.device, dtype=torch.float32)
        if self._train_max_frames is not None:
            _lib.check(L.gtav_dit_train_allow_window(self._handle, self._train_max_frames))
        if self._train_recompute:
            _lib.check(L.gtav_dit_train_set_recompute(self._handle, 1))
        if self._train_mixed:
            _lib.check(L.gtav_dit_train_allow_mixed(self._handle, 1))
        if self._train_bf16:
            _lib.check(L.gtav_dit_train_enable_typed(self._handle, self._grads.data_ptr(), n.value, 1))
        else:
            _lib.check(L.gtav_dit_train_enable(self._handle, self._grads.data_ptr(), n.value))
        if self._train_mixed:                                            # a re-created handle keeps the per-group types (no weight is set yet: nothing to convert)
            start = set(range(self.n_operand_groups)) if self._train_bf16 else set()
            for g in sorted(self._bf16_groups ^ start):
                _lib.check(L.gtav_dit_train_set_group_dtype(self._handle, g, 1 if g in self._bf16_groups else 0, _lib.current_stream()))
        self._replay("train")

    def _sync_weights(self):
        if self._ema_swapped:
            raise _lib.GtavError("new weights while the averaged weights are swapped in (ema_weights()): leave the context first")
        keep_ema = None
        if self._lora_rank and not self._lora_host_fresh:                # the re-upload below sends the adapters too: the trained ones, not the stale host copies
            # (and a weight upload sets the average to the weight: the trained adapters' average is put back behind it)
            keep_ema = self._pull_ema() if self._ema_decay is not None else None
            self._pull_lora()
        gh, gw = self.input_h // self.patch_size, self.input_w // self.patch_size
        sc, ss = _rope_tables_axial(self._spatial_freqs, gh, gw)
        tc, ts = _rope_tables_temporal(self._temporal_freqs, self._capacity_t)
        extra = {"tables.timestep_sincos": _timestep_table(), "tables.rope_spatial_cos": sc, "tables.rope_spatial_sin": ss,
                 "tables.rope_temporal_cos": tc, "tables.rope_temporal_sin": ts}
        extra.update(self._lora_sd)
        self._upload(extra)
        self._lora_host_fresh = True
        if keep_ema is not None:
            self._push_ema(keep_ema)
        self._replay("weights")

    def reserve(self, max_batch: int, max_frames: Optional[int] = None, noise_steps: int = 0):
        """Sizes the handle's HBM workspace once for the largest batch / window / per-frame conditioning table a run will use
        (noise_steps + 1 row sets per generated frame), so that no later call has to rebuild the handle (which re-uploads the
        weights and drops the captured hipGraphs).  While guidance is on (set_guidance) `max_batch` counts user samples: the handle is sized for the
        2 x max_batch internal samples and the doubled conditioning table of a guided step."""
        T = max_frames or self._capacity_t
        max_batch *= 2 if self._guidance is not None else 1
        self._ensure(max_batch, T, cond_rows=max_batch * (T - 1 + noise_steps + 1) if noise_steps else 0)

    def forward(self, x: torch.Tensor, t: torch.Tensor, external_cond: Optional[torch.Tensor] = None) -> torch.Tensor:
        """model/dit.py:343-376.  x (B,T,C,H,W), t (B,T) integer timesteps, external_cond (B,T,25) or None."""
        B, T, Cc, H, W = x.shape
        assert H == self.input_h and W == self.input_w, (
            f"Input image size ({H}*{W}) doesn't match model ({self.input_h}*{self.input_w}).")  # model/dit.py:67-69
        self._ensure(B, T)
        dev = self.device
        xd = x.to(dev, torch.float32).contiguous()
        td = t.to(dev, torch.int64).contiguous()
        ad = external_cond.to(dev, torch.float32).contiguous() if torch.is_tensor(external_cond) else None
        out = torch.empty_like(xd)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gtav_dit_forward(self._handle, xd.data_ptr(), td.data_ptr(), _lib.ptr(ad), out.data_ptr(),
                                                    B, T, _lib.current_stream()))
        return out

    __call__ = forward

    # ------------------------------------------------------------------------------------------
    # training step (reference: train_dit.py:649-650, :680, :232-238, :965-970)
    # ------------------------------------------------------------------------------------------
    def forward_train(self, x: torch.Tensor, t: torch.Tensor, external_cond: Optional[torch.Tensor] = None, action_keep=None) -> torch.Tensor:
        """DiT.forward keeping the activations `backward_` needs (same result as forward).  action_keep (B,) of 0 / 1 (None: everyone keeps): per-sample
        action dropout — a sample with 0 is conditioned as external_cond=None in all its frames, and backward_ honours the mask (gtav_dit_train_forward_keep)."""
        assert self._trainable, "construct the model with trainable=True"
        B, T, Cc, H, W = x.shape
        assert H == self.input_h and W == self.input_w
        self._ensure(B, T)
        dev = self.device
        xd = x.to(dev, torch.float32).contiguous()
        td = t.to(dev, torch.int64).contiguous()
        ad = external_cond.to(dev, torch.float32).contiguous() if torch.is_tensor(external_cond) else None
        out = torch.empty_like(xd)
        if action_keep is not None:
            if ad is None:
                raise ValueError("forward_train: action_keep without external_cond (there is nothing to drop)")
            kd = torch.as_tensor(action_keep).reshape(-1).ne(0).to(dev, torch.int32).contiguous()
            if kd.numel() != B:
                raise ValueError(f"forward_train: action_keep has {kd.numel()} flags for a batch of {B}")
            with torch.cuda.device(dev):
                _lib.check(_lib.load().gtav_dit_train_forward_keep(self._handle, xd.data_ptr(), td.data_ptr(), ad.data_ptr(), kd.data_ptr(), out.data_ptr(), B, T,
                                                                   _lib.current_stream()))
            return out
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gtav_dit_train_forward(self._handle, xd.data_ptr(), td.data_ptr(), _lib.ptr(ad), out.data_ptr(), B, T,
                                                          _lib.current_stream()))
        return out

    def backward_(self, v_pred: torch.Tensor, v_target: torch.Tensor):
        """Adds d mean((v_pred[:, -1] - v_target)^2) / d theta (times the loss scale) to the gradient arena (`accelerator.backward`)."""
        vt = v_target.to(self.device, torch.float32).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gtav_dit_train_backward(self._handle, v_pred.data_ptr(), vt.data_ptr(), _lib.current_stream()))

    def backward_phases_(self, v_pred: torch.Tensor, v_target: torch.Tensor, phase_begin: int, phase_end: int):
        """Phases [phase_begin, phase_end) of backward_: 0 = loss + final layer, p in 1..depth = block depth - p, depth + 1 = embedders."""
        vt = v_target.to(self.device, torch.float32).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gtav_dit_train_backward_phases(self._handle, v_pred.data_ptr(), vt.data_ptr(), phase_begin, phase_end,
                                                                 _lib.current_stream()))

    def param_range(self, prefix: str):
        """(offset, count) of the gradient-arena slice of the parameters whose names start with `prefix` (lexicographic layout)."""
        off, cnt = C.c_int64(0), C.c_int64(0)
        _lib.check(_lib.load().gtav_dit_train_param_range(self._handle, prefix.encode(), C.byref(off), C.byref(cnt)))
        return off.value, cnt.value

    def zero_grad(self):
        if not self._handle:
            self._ensure(self._capacity_b, self._capacity_t)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gtav_dit_zero_grad(self._handle, _lib.current_stream()))

    @property
    def grad_arena(self) -> torch.Tensor:
        """All gradients (loss-scaled), contiguous, parameters in lexicographic name order: what a data-parallel run all-reduces."""
        return self._grads

    @property
    def loss_scale(self) -> float:
        return self._loss_scale

    @property
    def train_dtype(self):
        """Operand type of the training step: torch.bfloat16 (train_dtype=torch.bfloat16) or torch.float16."""
        return torch.bfloat16 if self._train_bf16 else torch.float16

    @property
    def _train_mixed(self) -> bool:
        return self._trainable and self.train_range_policy == "auto"

    def _read_group_dtypes(self):
        """_bf16_groups from the handle (gtav_dit_get_operand_dtype): the handle is the truth after a call that may have switched groups and failed."""
        L, d, new = _lib.load(), C.c_int32(0), set()
        for g in range(self.n_operand_groups):
            _lib.check(L.gtav_dit_get_operand_dtype(self._handle, g, C.byref(d)))
            if d.value == 1:
                new.add(g)
        switched = sorted(new ^ self._bf16_groups)
        self._bf16_groups = new
        return switched

    def _mixed_handle(self, who):
        assert self._trainable, "construct the model with trainable=True"
        if not self._train_mixed:
            raise _lib.GtavError(f"{who}: this trainable DiT has one operand type for every layer group; construct it with train_range_policy='auto'")
        if not self._handle:
            self._ensure(self._capacity_b, self._capacity_t)

    def train_set_group_dtype(self, dtype, groups=None):
        """torch.float16 / torch.bfloat16 for the layer groups `groups` (None = all) of a train_range_policy="auto" model, in place (gtav_dit_train_set_group_dtype):
        the groups' kernels and the 2-byte images of their GEMM weights change type, the fp32 masters and the AdamW state on the GPU stay as they are."""
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"train_set_group_dtype: {dtype} (torch.float16 or torch.bfloat16)")
        self._mixed_handle("train_set_group_dtype")
        gs = range(self.n_operand_groups) if groups is None else [int(g) for g in groups]
        L = _lib.load()
        try:
            with torch.cuda.device(self.device):
                for g in gs:
                    _lib.check(L.gtav_dit_train_set_group_dtype(self._handle, g, 1 if dtype == torch.bfloat16 else 0, _lib.current_stream()))
        finally:
            self._read_group_dtypes()

    def train_range_words(self):
        """The sticky per-group saturation words of the training forwards since the last read (gtav_dit_train_range_words; synchronises, clears them): a list
        of n_operand_groups ints, what gtav_amd.train.autorange_step merges over the ranks."""
        self._mixed_handle("train_range_words")
        buf = (C.c_int32 * self.n_operand_groups)()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gtav_dit_train_range_words(self._handle, buf, _lib.current_stream()))
        return list(buf)

    def train_autorange(self, merged_words=None):
        """Between two optimisation steps: moves the fp16 layer groups whose training forward saturated since the last call to bf16 operands
        (gtav_dit_train_autorange; synchronises) and returns their numbers.  merged_words: the words to act on in place of the handle's own (the data-parallel
        merge of train_range_words()).  Anything else in the error words raises as check() raises it — after the switch, and operand_dtypes() is right either way."""
        self._mixed_handle("train_autorange")
        n = C.c_int32(0)
        words = None if merged_words is None else (C.c_int32 * self.n_operand_groups)(*[int(w) for w in merged_words])
        try:
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().gtav_dit_train_autorange(self._handle, words, C.byref(n), _lib.current_stream()))
        finally:
            switched = self._read_group_dtypes()
        assert len(switched) == n.value, (switched, n.value)
        return switched

    def restore_operand_groups(self, bf16_groups):
        """The bf16 layer groups of a checkpoint (step.json "bf16_groups", gtav_amd.train.load_state) onto this model, before its weights are sent: needs
        train_range_policy="auto" unless they are the groups the model has anyway."""
        new = {int(g) for g in bf16_groups}
        if any(g < 0 or g >= self.n_operand_groups for g in new):
            raise ValueError(f"restore_operand_groups: groups {sorted(new)} outside [0, {self.n_operand_groups})")
        if new == self._bf16_groups:
            return
        if not self._train_mixed:
            raise _lib.GtavError(f"restore_operand_groups: the checkpoint trains the layer groups {sorted(new)} on bf16 operands and the others on fp16; this model "
                                 "has one operand type for every layer group (construct it with trainable=True, train_range_policy='auto')")
        if self._handle:
            self.train_set_group_dtype(torch.bfloat16, sorted(new - self._bf16_groups))
            self.train_set_group_dtype(torch.float16, sorted(self._bf16_groups - new))
        else:
            self._bf16_groups = new                # (_ensure applies them to the handle it builds)

    @property
    def train_recompute(self) -> bool:
        """True when the training step recomputes each block's activations in the backward pass (train_recompute=True); fixed at construction."""
        return self._train_recompute

    def train_saved_bytes(self) -> int:
        """Bytes of the saved-activation buffers of the training handle (gtav_dit_train_saved_bytes), sized by max_batch x the training window; builds the
        handle if it does not exist yet."""
        assert self._trainable, "construct the model with trainable=True"
        if not self._handle:
            self._ensure(self._capacity_b, self._capacity_t)
        n = C.c_int64(0)
        _lib.check(_lib.load().gtav_dit_train_saved_bytes(self._handle, C.byref(n)))
        return n.value

    @loss_scale.setter
    def loss_scale(self, v: float):
        self._set("_loss_scale", float(v))

    def grad(self, name: str) -> torch.Tensor:
        """Unscaled gradient of one trainable parameter in its state-dict shape (a LoRA model: of an adapter; the base is frozen and refused by name)."""
        shapes = self._train_shapes()
        if name not in shapes:
            raise _lib.GtavError(f"grad: '{name}' is not a trainable parameter" + (" (a LoRA model trains its lora_A / lora_B adapters only)" if self._lora_rank else ""))
        out = self._pull("gtav_dit_get_grad", {name: shapes[name]}, cpu=False)[name]     # (stays on the device)
        return out / (self._loss_scale * self._grad_divisor)

    def residual_after(self, k: int, B: int, T: int) -> torch.Tensor:
        """Residual stream of the last forward_train after k branch additions (4 per block; k = 4 (i + 1) is the output of block i),
        as (B, T, h, w, D) like the reference's block outputs."""
        gh, gw = self.input_h // self.patch_size, self.input_w // self.patch_size
        out = torch.empty(B * T * gh * gw, self.hidden_size, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gtav_dit_train_get_residual(self._handle, k, out.data_ptr(), out.numel(), _lib.current_stream()))
        return out.reshape(B, T, gh, gw, self.hidden_size)

    def adamw_step(self, lr: float, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-7, max_grad_norm: float = 0.0):
        """clip_grad_norm_ + AdamW.step on the GPU masters (train_dit.py:232-238, 965-968); refreshes the fp16 GEMM operands."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gtav_dit_adamw_step(self._handle, float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                                       float(max_grad_norm), _lib.current_stream()))
        self._lora_host_fresh = False

    def train_stats(self):
        """(step applied?, skipped steps so far, unscaled global gradient norm of the last step); synchronises."""
        buf = (C.c_float * 4)()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gtav_dit_train_stats(self._handle, buf, _lib.current_stream()))
        return buf[1] != 0.0, int(buf[2]), float(buf[3])

    def opt_state_dict(self) -> Dict[str, torch.Tensor]:
        """AdamW state of every trainable parameter as CPU tensors: "m.<name>" / "v.<name>" (first / second moments, state-dict shapes)
        plus "step" = [applied steps, skipped steps] — what accelerator.save_state keeps for the optimizer (train_dit.py:765-800)."""
        assert self._trainable and self._handle, "no optimizer state: construct with trainable=True and run a step (or reserve()) first"
        out = {}
        for k, (m, v) in self._pull("gtav_dit_get_opt_state", self._train_shapes(), ptrs=2).items():
            out["m." + k], out["v." + k] = m, v
        a, sk = C.c_int64(0), C.c_int64(0)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gtav_dit_get_opt_step(self._handle, C.byref(a), C.byref(sk), _lib.current_stream()))
        out["step"] = torch.tensor([a.value, sk.value], dtype=torch.int64)
        return out

    def load_opt_state_dict(self, state: Dict[str, torch.Tensor]):
        """Inverse of opt_state_dict (the weights themselves: load_state_dict).  The handle is built first if it does not exist yet."""
        assert self._trainable, "construct the model with trainable=True"
        self._ensure(self._capacity_b, self._capacity_t)
        shapes = self._train_shapes()
        m, v = (_checked_tensors({k: state[p + k] for k in shapes}, shapes, "load_opt_state_dict") for p in ("m.", "v."))
        self._push("gtav_dit_set_opt_state", {k: (m[k], v[k]) for k in shapes}, synchronize=False)
        st = state["step"]
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gtav_dit_set_opt_step(self._handle, int(st[0]), int(st[1]), _lib.current_stream()))
            torch.cuda.synchronize()

    @property
    def grad_divisor(self) -> float:
        return self._grad_divisor

    @grad_divisor.setter
    def grad_divisor(self, v: float):
        """The gradient arena holds the SUM over this many ranks (all-reduce SUM): the optimizer step divides, the arena is not rescaled."""
        self._set("_grad_divisor", float(v))

    def pull_weights(self):
        """Copies the trained fp32 masters from the GPU back into the host state dict (checkpoints, state_dict())."""
        if self._ema_swapped:
            raise _lib.GtavError("pull_weights: the averaged weights are swapped in (ema_weights()); the trained ones are read outside the context (the average: ema_state_dict())")
        self._sd.update(self._pull("gtav_dit_get_weight", self._shapes()))

    # ------------------------------------------------------------------------------------------
    # averaged weights (train_ema_decay=...; include/gtav_amd.h gtav_dit_train_set_ema)
    # ------------------------------------------------------------------------------------------
    @property
    def ema_decay(self):
        """Decay of the averaged weights, None on a model without them; fixed at construction."""
        return self._ema_decay

    @property
    def ema_warmup(self) -> bool:
        return self._ema_warmup

    def _need_ema(self, who):
        if self._ema_decay is None:
            raise _lib.GtavError(f"{who}: this DiT keeps no averaged weights (construct it with trainable=True, train_ema_decay=...)")

    def _pull_ema(self):
        return self._pull("gtav_dit_get_ema", self._train_shapes())

    def _push_ema(self, sd):
        self._push("gtav_dit_set_ema", sd)

    def ema_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """The averaged weights as CPU tensors in the reference's key layout: every trainable tensor from the GPU's fp32 shadow, the constants (rotary
        frequencies) from state_dict().  A LoRA model returns the averaged ADAPTERS under the adapter keys — loaded into a LoRA model over the same base
        (load_lora_state_dict) they give the model `with ema_weights():` computes with; note that merging averaged adapters is not the average of the merged
        weights (B A is bilinear)."""
        self._need_ema("ema_state_dict")
        self._ensure(self._capacity_b, self._capacity_t)
        ema = self._pull_ema()
        if self._lora_rank:
            return ema
        sd = self.state_dict()
        sd.update(ema)
        return sd

    def load_ema_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Inverse of ema_state_dict: every trainable tensor's average in its shape (other keys, the rotary frequencies among them, are ignored).  The weights
        themselves: load_state_dict, which also sets the average to the weights it loads — so call this after it."""
        self._need_ema("load_ema_state_dict")
        new = _checked_tensors(sd, self._train_shapes(), "load_ema_state_dict", allow_unexpected=True)
        self._ensure(self._capacity_b, self._capacity_t)
        self._push_ema(new)

    @contextlib.contextmanager
    def ema_weights(self):
        """`with dit.ema_weights():` the model computes with the averaged weights — forward / __call__, the sampler step, gtav_amd.train.predict, state via
        gtav_dit_get_weight — and with the trained ones again afterwards, bit for bit (gtav_dit_train_swap_ema: masters and shadow change places on the GPU, the
        2-byte weight images are remade; nothing is copied to the host).  Inside, forward_train / backward_ / adamw_step and weight uploads raise GtavError;
        nesting raises."""
        self._need_ema("ema_weights")
        if self._ema_swapped:
            raise _lib.GtavError("ema_weights: the averaged weights are swapped in already (the context does not nest)")
        self._ensure(self._capacity_b, self._capacity_t)
        L = _lib.load()
        with torch.cuda.device(self.device):
            _lib.check(L.gtav_dit_train_swap_ema(self._handle, _lib.current_stream()))
        self._ema_swapped = True
        try:
            yield self
        finally:
            with torch.cuda.device(self.device):
                _lib.check(L.gtav_dit_train_swap_ema(self._handle, _lib.current_stream()))
            self._ema_swapped = False

    # ------------------------------------------------------------------------------------------
    # low-rank adapters (train_lora_rank=...; include/gtav_amd.h gtav_dit_train_set_lora)
    # ------------------------------------------------------------------------------------------
    @property
    def lora_rank(self):
        """Rank of the adapters, None on a model without them."""
        return self._lora_rank

    @property
    def lora_alpha(self):
        return self._lora_alpha

    def _need_lora(self, who):
        if not self._lora_rank:
            raise _lib.GtavError(f"{who}: this DiT has no adapters (construct it with trainable=True, train_lora_rank=16 / 32 / 64)")

    def init_lora(self, seed: int = 0):
        """The default adapters: lora_A ~ U(-1 / sqrt(K), 1 / sqrt(K)) from a CPU generator seeded with `seed` (drawn in name order), lora_B = 0, so that the
        model starts as its base."""
        self._need_lora("init_lora")
        g = torch.Generator(device="cpu").manual_seed(int(seed))
        sd = OrderedDict()
        for k, shp in self._lora_shapes().items():
            if k.endswith(".lora_A.weight"):
                bound = 1.0 / math.sqrt(shp[1])
                sd[k] = (torch.rand(shp, generator=g, dtype=torch.float32) * 2.0 - 1.0) * bound
            else:
                sd[k] = torch.zeros(shp, dtype=torch.float32)
        self._set_lora(sd)

    def _set_lora(self, sd):
        """New host copies of the adapters; a handle whose other weights are in place takes them at once (the library re-merges the images)."""
        self._lora_sd = OrderedDict((k, sd[k]) for k in self._lora_shapes())
        self._lora_host_fresh = True
        if self._handle and not self._dirty:
            self._push("gtav_dit_set_weight", self._lora_sd, finalize=True)

    def _pull_lora(self):
        if self._ema_swapped:
            raise _lib.GtavError("the averaged adapters are swapped in (ema_weights()); the trained ones are read outside the context (the average: ema_state_dict())")
        self._lora_sd.update(self._pull("gtav_dit_get_weight", self._lora_shapes()))
        self._lora_host_fresh = True

    def lora_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """The adapters as CPU tensors (the trained ones, copied back from the GPU when an optimizer step moved them)."""
        self._need_lora("lora_state_dict")
        if self._handle and not self._lora_host_fresh:
            self._pull_lora()
        return OrderedDict(self._lora_sd)

    def load_lora_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Inverse of lora_state_dict: every adapter, nothing else, in its shape."""
        self._need_lora("load_lora_state_dict")
        self._set_lora(_checked_tensors(sd, self._lora_shapes(), "load_lora_state_dict", note=f" (rank {self._lora_rank})"))

    def merged_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """The reference's key layout with the adapters folded in: every adapted weight is the fp32 W0 + (alpha / rank) B A that the GPU casts into its
        weight images (gtav_dit_lora_get_merged), everything else the frozen base.  Loaded into any DiT it computes what this model computes."""
        self._need_lora("merged_state_dict")
        self._ensure(self._capacity_b, self._capacity_t)
        sd, shapes = self.state_dict(), self._shapes()
        adapted = [k[: -len(".lora_A.weight")] + ".weight" for k in self._lora_shapes() if k.endswith(".lora_A.weight")]
        sd.update(self._pull("gtav_dit_lora_get_merged", OrderedDict((name, shapes[name]) for name in adapted)))
        return sd

    # ------------------------------------------------------------------------------------------
    # fused sampler entry (train_dit.denoise_step + generate.py:220), used by gtav_amd.generate
    # ------------------------------------------------------------------------------------------
    def set_schedule(self, alphas_cumprod: torch.Tensor):
        ac = alphas_cumprod.detach().reshape(-1).float().cpu().contiguous()
        assert ac.numel() == 1000
        self._set("_schedule", (C.c_float * 1000).from_buffer_copy(ac.numpy().tobytes()))

    def set_guidance(self, scale: Optional[float]):
        """Classifier-free guidance on the actions for the fused sampler step (gtav_dit_set_guidance): with a scale s, prepare_frame_ / denoise_step_ run the
        conditional and the external_cond=None branch as one forward over 2 B internal samples and update frame `cur` from v_c + (s - 1)(v_c - v_u)
        (s = 1: v_c itself, s = 0: v_u).  None switches it off (the default: today's step bit for bit).  The model needs max_batch >= 2 B.  Changing the
        scale between steps costs nothing (one captured step serves every scale); switching on / off drops the prepared table and the context cache."""
        if scale is not None:
            scale = float(scale)
            if not math.isfinite(scale):
                raise ValueError(f"set_guidance: scale {scale} is not finite")
            if not self.external_cond_dim or self.external_cond_dim <= 0:
                raise ValueError("set_guidance: this model has no external_cond (external_cond_dim=0): there are no actions to guide towards")
        self._set("_guidance", scale)

    def _internal_batch(self, B: int) -> int:
        """Samples a sampler step of batch B runs inside the handle: 2 B while guidance is on.  A guided step never grows the handle by itself."""
        if self._guidance is None:
            return B
        if 2 * B > self._capacity_b:
            raise ValueError(f"a guided sampler step of batch {B} runs 2 B = {2 * B} internal samples: this model was built with max_batch={self._capacity_b}; "
                             f"construct it with max_batch={2 * B} (or call reserve({B}) while guidance is on)")
        return 2 * B

    def prepare_frame_(self, B: int, F: int, start: int, cur: int, t_ctx: int, t_steps, actions: Optional[torch.Tensor] = None):
        """Builds the conditioning (adaLN) table for every noise step of one generated frame (gtav_dit_prepare_frame);
        step k of that frame then passes cond_step=k to denoise_step_.  start > cur is the ring window start .. F-1, 0 .. cur (include/gtav_amd.h)."""
        n = len(t_steps)
        Bi = self._internal_batch(B)
        T = cur - start + 1 + (F if cur < start else 0)
        self._ensure(Bi, T, cond_rows=Bi * (T - 1 + n))
        arr = (C.c_int32 * n)(*[int(v) for v in t_steps])
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gtav_dit_prepare_frame(self._handle, B, F, start, cur, int(t_ctx), arr, n, _lib.ptr(actions),
                                                          _lib.current_stream()))

    def denoise_step_(self, x: torch.Tensor, start: int, cur: int, t_ctx: int, t_cur: int, t_next: int, is_final: bool,
                      actions: Optional[torch.Tensor] = None, cached: bool = False, v_out: Optional[torch.Tensor] = None,
                      cond_step: int = -1):
        """In-place fused step on latents x (B, F, C, H, W) fp32 contiguous on the model's device.  start > cur is the ring window start .. F-1, 0 .. cur
        (include/gtav_amd.h)."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        B, F = x.shape[:2]
        if cond_step < 0:
            self._ensure(self._internal_batch(B), cur - start + 1 + (F if cur < start else 0))
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gtav_dit_denoise_step(
                self._handle, x.data_ptr(), B, F, start, cur, int(t_ctx), int(t_cur), int(t_next), int(bool(is_final)),
                _lib.ptr(actions), 1 if cached else 0, int(cond_step), _lib.ptr(v_out), _lib.current_stream()))

    PROFILE_CLASSES = ("ln_modulate", "gemm_qkv", "attn_spatial", "attn_temporal", "gemm_out", "gemm_fc1", "gemm_fc2", "other",
                       "empty_event_pair")
    assert len(PROFILE_CLASSES) == _lib.CONSTANTS["GTAV_PROFILE_CLASSES"]

    def profile(self, enable: bool):
        """In-situ per-kernel-class HIP-event timing (measurement passes only; see include/gtav_amd.h).  Not one of the recorded settings: a handle that is
        re-created (growth) comes back with it off."""
        _lib.check(_lib.load().gtav_dit_profile(self._handle, int(bool(enable))))

    def profile_read(self):
        ms = (C.c_double * _lib.CONSTANTS["GTAV_PROFILE_CLASSES"])()
        n = (C.c_int64 * _lib.CONSTANTS["GTAV_PROFILE_CLASSES"])()
        _lib.check(_lib.load().gtav_dit_profile_read(self._handle, ms, n))
        return {k: (ms[i], n[i]) for i, k in enumerate(self.PROFILE_CLASSES)}

    def set_graph(self, enable: bool):
        """hipGraph replay of the fused sampler step on/off (on by default).  Not one of the recorded settings: a handle that is re-created (growth)
        comes back with the default."""
        _lib.check(_lib.load().gtav_dit_set_graph(self._handle, int(bool(enable))))

    def set_fused_temporal(self, enable: bool):
        """Temporal QKV projection + temporal attention as one kernel on batch-1 full-window steps (off by default; bit-identical to the two-kernel path;
        1-2 % slower per eager forward, 1-1.6 % faster per replayed captured step: generate.tune_weight_prefetch times both and keeps the faster)."""
        self._set("_fused_temporal", bool(enable))

    def set_fused_spatial(self, enable: bool):
        """Spatial QKV projection + spatial attention as one kernel on steps of 5 or more frames of 144 tokens (gtav_dit_set_fused_spatial; ON by default where
        the geometry allows; bit-identical to the two-kernel path; generate.tune_weight_prefetch times both on the shape it tunes and keeps the faster)."""
        self._set("_fused_spatial", bool(enable))

    def fused_launches(self, B: int, T: int, t0: int = 0) -> int:
        """Bit 0: a step of B x T frames runs the fused spatial to_qkv + attention launch on this handle as it is now; bit 1: the fused temporal one
        (gtav_dit_fused_launches).  The profiler books those launches under attn_spatial / attn_temporal."""
        self._ensure(B, T)
        return int(_lib.load().gtav_dit_fused_launches(self._handle, int(B), int(T), int(t0)))

    def set_weight_prefetch(self, mode):
        """L2 prefetch of the next GEMM's weight at small token counts (gtav_dit_set_weight_prefetch; on by default, bit-identical results under every
        mode): False / 0 off, True / 1 every weight, or a per-class word from gtav_amd.generate.prefetch_mode."""
        mode = int(mode)
        if mode not in (0, 1) and (mode >> 16) != 1:
            raise ValueError(f"set_weight_prefetch: mode {mode:#x} is neither 0, 1 nor a per-class word (gtav_amd.generate.prefetch_mode)")
        self._set("_weight_prefetch", mode)

    def set_weight_fill_policy(self, mode: int):
        """Cache policy of the small-M GEMMs' weight fills per class (gtav_dit_set_weight_fill_policy; all default when never called; bit-identical results under
        every word): a per-class word from gtav_amd.generate.fill_policy_mode, nibble 0 = default policy, 1 = non-temporal."""
        mode = int(mode)
        if mode & ~0x1111:
            raise ValueError(f"set_weight_fill_policy: mode {mode:#x} is not a per-class word of nibbles 0 / 1 (gtav_amd.generate.fill_policy_mode)")
        self._set("_weight_fill_policy", mode)

    def set_fold(self, mode: int, min_tokens_a: int = -1, min_tokens_b: int = -1):
        """EXPERIMENTS BUILD ONLY (gtav_amd.lib.load_experiments(), tools/fold_bench.py): the LayerNorm fold of round 3 (gtav_dit_set_fold, csrc/experiments.h) —
        0 = separate LayerNorm launches everywhere, 1 = folded into the GEMM epilogues from min_tokens_* tokens on, 2 = every seam at every size.
        Correct, and measured slower than the LayerNorm launches at every size: the product library does not carry it."""
        if not getattr(_lib.load(), "_gtav_experiments", False):
            raise _lib.GtavError("set_fold: the LayerNorm fold exists only in the experiments build (gtav_amd.lib.load_experiments())")
        self._set("_fold", (int(mode), int(min_tokens_a), int(min_tokens_b)))

    # ------------------------------------------------------------------------------------------
    # operand type / range safety (include/gtav_amd.h "operand type"; reference: bf16 autocast, generate.py:125-127, train_dit.py:190-198)
    # ------------------------------------------------------------------------------------------
    def set_operand_dtype(self, dtype, groups=None):
        """torch.float16 (default: 6-9e-4 relative L2 per forward against the fp32 reference, range +-65504) or torch.bfloat16 (the reference's own autocast type:
        fp32 range, ~8e-3) for the 2-byte GEMM / attention operands of `groups` (None = every layer group; group numbering: n_operand_groups).  The weights of
        the changed groups are converted again from the fp32 host copies at the next call.  A trainable model keeps the type of its train_dtype: bf16 is
        a no-op on a bf16-trainable model and fp16 raises there; an fp16-trainable model refuses bf16."""
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"set_operand_dtype: {dtype} (torch.float16 or torch.bfloat16)")
        if self._train_bf16 and dtype == torch.float16:
            raise _lib.GtavError("set_operand_dtype: a bf16-trainable DiT (train_dtype=torch.bfloat16) keeps bf16 operands in every layer group")
        if self._trainable and not self._train_bf16 and dtype == torch.bfloat16:
            raise _lib.GtavError("set_operand_dtype: a trainable DiT keeps fp16 operands (its backward pass and loss scaling are fp16)")
        gs = set(range(self.n_operand_groups)) if groups is None else {int(g) for g in groups}
        if any(g < 0 or g >= self.n_operand_groups for g in gs):
            raise ValueError(f"set_operand_dtype: groups {sorted(gs)} outside [0, {self.n_operand_groups})")
        new = (self._bf16_groups | gs) if dtype == torch.bfloat16 else (self._bf16_groups - gs)
        if new == self._bf16_groups:
            return
        if self._train_mixed:
            raise _lib.GtavError("set_operand_dtype: a trainable DiT changes the type of a layer group with train_set_group_dtype (train_range_policy='auto')")
        if self._handle:
            L = _lib.load()
            for g in sorted(new ^ self._bf16_groups):
                _lib.check(L.gtav_dit_set_operand_dtype(self._handle, g, 1 if g in new else 0))
            self._dirty = True               # the changed groups' weight images are stale: the next call re-sends the weights and finalizes
        self._bf16_groups = new

    def operand_dtypes(self):
        """torch dtype of every operand group, in group order (a train_range_policy="auto" model: as train_autorange / train_set_group_dtype left them)."""
        return [torch.bfloat16 if g in self._bf16_groups else torch.float16 for g in range(self.n_operand_groups)]

    def check(self):
        """Raises if a timestep was out of range, an input held NaN / inf, or an fp16 activation saturated since the last call (synchronises).
        range_policy "auto": a saturation moves exactly the layer groups that saturated to bf16 operands (gtav_dit_autorange) and raises GtavRangeSwitch —
        what was computed since the last check is clipped and must be recomputed; the recomputation runs the switched layers in bf16."""
        if not self._handle:
            return
        L = _lib.load()
        with torch.cuda.device(self.device):
            if self.range_policy != "auto" or self._trainable:
                _lib.check(L.gtav_dit_check(self._handle, _lib.current_stream()))
                return
            n = C.c_int32(0)
            try:
                _lib.check(L.gtav_dit_autorange(self._handle, C.byref(n), _lib.current_stream()))
            finally:                         # (the groups switch before another error of the same check is reported: the handle is the truth either way)
                switched = self._read_group_dtypes()
                if switched:
                    self._dirty = True
            if n.value:
                raise _lib.GtavRangeSwitch(f"DiT: an activation exceeded the fp16 range (|x| > 65504) in operand group(s) {switched}; those layers now run "
                                           "on bf16 operands (the reference's own autocast type): results since the last check are clipped — recompute them", switched)


def DiT_S_2(**kwargs):
    """model/dit.py:379-389."""
    return DiT(input_h=18, input_w=32, patch_size=2, hidden_size=1024, depth=16, num_heads=16, max_frames=5, **kwargs)


DiT_models = {"DiT-S/2": DiT_S_2}
