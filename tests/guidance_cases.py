"""Cases, inputs and the CPU oracle of the classifier-free-guidance tests (tests/test_host_guidance.py, tests/test_gpu_guidance.py): one place, computed once.

The oracle is composed from oracle/ref_cpu.py: two `O.dit_forward` calls (with the actions, and with external_cond=None) combined as
v_g = v_c + (s - 1)(v_c - v_u), handed to `O.denoise_step` / `O.generate_latents` as their dit_fn.

The bound of a guided prediction.  The fused step is within TOL_SMALL of the oracle on v_c and on v_u separately (the unguided bound of the toy model).  v_g is
the combination s v_c + (1 - s) v_u, so its absolute error is at most TOL_SMALL (|s| |v_c| + |s - 1| |v_u|), and relative to |v_g| that is TOL_SMALL times
    amp(s) = (|s| |v_c| + |s - 1| |v_u|) / |v_g(s)|
with every norm taken from the ORACLE's values on frame `cur` (never from the code under test).  amp(0) = amp(1) = 1."""
import functools

import torch

from oracle import ref_cpu as O
import gtav_amd.weights as W

SMALL_DIT = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)
TOL_SMALL = 2e-3       # tests/test_gpu_models.py: toy widths, one forward
TOL_ROLLOUT = 1.5e-3   # tests/test_gpu_models.py: tens of chained forwards
SEED = 4               # the checkpoint of tests/test_gpu_models.py::test_denoise_step_mirror_and_fused_and_cached
B, FRAMES, START = 2, 6, 1            # a 5-frame window [1, 5]
NOISE_STEPS, NOISE_IDX = 10, (10, 4, 0)
SCALES = (0.0, 1.0, 3.0)
T_CTX = 15


def state_dict(seed=SEED):
    return W.synth_state_dict(W.dit_param_shapes(**SMALL_DIT), seed=seed)


def config():
    return O.DiTConfig(**SMALL_DIT)


def inputs():
    """Latents (B, 6, 16, 8, 16) and actions ("W" held) of the single-step tests: the inputs of the unguided step test."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, FRAMES, 16, 8, 16, generator=g)
    a = torch.zeros(B, FRAMES, 25)
    a[:, :, 3] = 1
    return x, a


def noise_range():
    return torch.linspace(0, 999, NOISE_STEPS + 1)


def timesteps(noise_idx):
    nr = noise_range()
    return int(nr[noise_idx]), int(nr[max(0, noise_idx - 1)])


def combine(v_c, v_u, s):
    """v_c + (s - 1)(v_c - v_u) on torch fp32 CPU tensors: difference, product, sum, each rounded once."""
    d = v_c - v_u
    m = (torch.tensor(s, dtype=torch.float32) - 1.0) * d
    return v_c + m


def amp(v_c, v_u, s):
    v_g = combine(v_c, v_u, s)
    return ((abs(s) * v_c.double().norm() + abs(s - 1.0) * v_u.double().norm()) / v_g.double().norm()).item()


def guided_fn(sd, cfg, s, amps=None):
    """dit_fn of the oracle's sampler: the guided prediction from two oracle forwards.  `amps` (a list) collects amp(s) on the last frame of every call."""
    def fn(xx, tt, aa):
        v_c = O.dit_forward(sd, cfg, xx, tt, aa)
        v_u = O.dit_forward(sd, cfg, xx, tt, None)
        if amps is not None:
            amps.append(amp(v_c[:, -1], v_u[:, -1], s))
        return combine(v_c, v_u, s)
    return fn


@functools.lru_cache(maxsize=None)
def oracle_branches(noise_idx):
    """(v_c, v_u) of the oracle on frame `cur` (B, C, H, W each) for the window step at this noise index."""
    sd, cfg = state_dict(), config()
    x, a = inputs()
    t_cur, _ = timesteps(noise_idx)
    t = torch.full((B, FRAMES - START), T_CTX, dtype=torch.long)
    t[:, -1] = t_cur
    with torch.no_grad():
        v_c = O.dit_forward(sd, cfg, x[:, START:], t, a[:, START:])
        v_u = O.dit_forward(sd, cfg, x[:, START:], t, None)
    return v_c[:, -1].contiguous(), v_u[:, -1].contiguous()


@functools.lru_cache(maxsize=None)
def oracle_step(noise_idx, s):
    """(x_pred of frame cur, v_g of frame cur) of O.denoise_step under the guided dit_fn."""
    from gtav_amd.utils import alphas_cumprod
    sd, cfg = state_dict(), config()
    x, a = inputs()
    with torch.no_grad():
        xr, vr = O.denoise_step(guided_fn(sd, cfg, s), x, a, noise_idx, T_CTX, noise_range(), alphas_cumprod(1e-4)[:, None, None, None], start_frame=START)
    return xr[:, -1].contiguous(), vr[:, -1].contiguous()
