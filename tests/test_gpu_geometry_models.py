"""Forward, sampler step, rollout and VAE at patch geometries and latent widths other than (patch 2, 16 channels): nothing in the suite had run them.
The six DiT geometries of tests/test_gpu_geometry_train.py (F = in_channels * patch_size^2 from 16 to 256 features per patch, 32 tokens per frame), the
VAE at latent_dim 4, 8 and 32, and one VAE + DiT pair on 4-channel latents end to end.

Bounds are those of tests/test_gpu_models.py for the same comparisons: TOL_SMALL 2e-3 per forward at toy widths, TOL_ROLLOUT 1.5e-3 for chained forwards;
bf16 operands 1.5e-2 (tests/test_gpu_range.py TOL_BF16).  Captured and replayed sampler steps and the context-cached step reproduce the eager window step
bit for bit.  The posterior sample: 2^-17 std + 2^-22 |result| per element (tests/test_gpu_rng.py).  `pytest -s` prints every margin
(profiles/geometry/margins.txt)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import dev  # noqa: E402
from helpers import rel_l2_logged  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402
import gtav_amd.weights as W  # noqa: E402
from gtav_amd import rng as R  # noqa: E402
from gtav_amd.model.dit import DiT  # noqa: E402
from gtav_amd.model.vae import AutoencoderKL  # noqa: E402

TOL_SMALL = 2e-3       # tests/test_gpu_models.py
TOL_ROLLOUT = 1.5e-3   # tests/test_gpu_models.py
TOL_BF16 = 1.5e-2      # tests/test_gpu_range.py
NORMAL_BOUND = 2.0 ** -17   # tests/test_gpu_rng.py BOUND

SMALL = dict(hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)
GEO = {
    "p2c4": dict(input_h=8, input_w=16, patch_size=2, in_channels=4),
    "p2c8": dict(input_h=8, input_w=16, patch_size=2, in_channels=8),
    "p1c16": dict(input_h=4, input_w=8, patch_size=1, in_channels=16),
    "p4c4": dict(input_h=16, input_w=32, patch_size=4, in_channels=4),
    "p2c32": dict(input_h=8, input_w=16, patch_size=2, in_channels=32),
    "p4c16": dict(input_h=16, input_w=32, patch_size=4, in_channels=16),
}
GEOS = sorted(GEO)
SMALL_VAE = dict(input_height=64, input_width=96, patch_size=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=256, dec_depth=2, dec_heads=4)   # tests/test_gpu_models.py, less latent_dim


rel_l2 = functools.partial(rel_l2_logged, tag="geometry")       # rel_l2(a, b, what): (-s shows the measured margins)


def _mk_dit(geo, seed, max_batch=2, **extra):
    kw = dict(SMALL, **GEO[geo])
    sd = W.synth_state_dict(W.dit_param_shapes(**kw), seed=seed)
    m = DiT(**kw, max_batch=max_batch, init_weights=False, **extra)
    m.load_state_dict(sd)
    return m, sd, O.DiTConfig(**kw)


def _one_hot(B, T, g):
    a = torch.zeros(B, T, 25)
    a[torch.arange(B)[:, None], torch.arange(T)[None], torch.randint(0, 25, (B, T), generator=g)] = 1
    return a


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", GEOS)
def test_forward_matches_the_oracle(geo):
    """fp16 and bf16 operands, with and without actions, against one oracle forward each."""
    m, sd, cfg = _mk_dit(geo, seed=3)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, cfg.in_channels, cfg.input_h, cfg.input_w, generator=g)
    t = torch.randint(0, 1000, (2, 3), generator=g)
    for a in (_one_hot(2, 3, g), None):
        with torch.no_grad():
            ref = O.dit_forward(sd, cfg, x, t, a)
        m.set_operand_dtype(torch.float16)
        out = m(x, t, a)
        assert out.shape == ref.shape and out.dtype == torch.float32
        assert rel_l2(out, ref, f"fp16 actions={a is not None}") < TOL_SMALL
        m.check()
        m.set_operand_dtype(torch.bfloat16)
        assert rel_l2(m(x, t, a), ref, f"bf16 actions={a is not None}") < TOL_BF16
        m.check()


@pytest.mark.parametrize("geo", ["p4c4", "p2c8"])
def test_forward_and_denoise_step_match_reference_fixture_g14(geo):
    """Against the reference's own module directly (tests/golden/g14_geometry.safetensors): v_pred, and the last frame of denoise_step at noise index 50 of 50."""
    from safetensors.torch import load_file
    from gtav_amd.sampler import denoise_step
    from gtav_amd.utils import alphas_cumprod
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_geometry.safetensors")
    g = {k[len(geo) + 1:]: v for k, v in load_file(path).items() if k.startswith(geo + ".")}
    m, sd, cfg = _mk_dit(geo, seed=3)
    assert rel_l2(m(g["x"], g["t"], g["actions"]), g["v_pred"], "v_pred") < TOL_SMALL
    xp, _ = denoise_step(m, g["x"], g["actions"], 50, 15, torch.linspace(0, 999, 51), alphas_cumprod(1e-4)[:, None, None, None], start_frame=0)
    assert rel_l2(xp[:, -1:], g["x_pred_last_50"], "x_pred_last_50") < TOL_SMALL
    m.check()


# ---- 2. one sampler step ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", GEOS)
def test_sampler_step_eager_captured_replayed_and_cached(geo):
    from gtav_amd.utils import alphas_cumprod
    m, sd, cfg = _mk_dit(geo, seed=4)
    g = torch.Generator().manual_seed(2)
    B, n, start = 2, 5, 1
    x = torch.randn(B, n, cfg.in_channels, cfg.input_h, cfg.input_w, generator=g)
    a = _one_hot(B, n, g)
    ac = alphas_cumprod(1e-4)
    nr = torch.linspace(0, 999, 11)
    noise_idx = 4
    dit_fn = lambda xx, tt, aa: O.dit_forward(sd, cfg, xx, tt, aa)
    with torch.no_grad():
        xr, _ = O.denoise_step(dit_fn, x, a, noise_idx, 15, nr, ac[:, None, None, None], start_frame=start)
    m.set_schedule(ac)
    t_cur, t_next = int(nr[noise_idx]), int(nr[noise_idx - 1])
    xd, ad = x.to(dev()).contiguous(), a.to(dev())
    steps = []
    for k in range(3):                                        # eager, captured, replayed
        xd[:, -1] = x[:, -1].to(dev())
        m.denoise_step_(xd, start, n - 1, 15, t_cur, t_next, False, ad)
        steps.append(xd[:, -1].clone())
    assert rel_l2(steps[0], xr[:, -1], "window step") < TOL_SMALL
    assert torch.equal(steps[0], steps[1]) and torch.equal(steps[1], steps[2])
    assert torch.equal(xd[:, :-1].cpu(), x[:, :-1])
    xd[:, -1] = x[:, -1].to(dev())
    m.denoise_step_(xd, start, n - 1, 15, t_cur, t_next, False, ad, cached=True)
    assert torch.equal(xd[:, -1], steps[0])                   # the context-cached step on the K/V caches the window step left
    m.check()


# ---- 3. a 9-forward rollout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", GEOS)
def test_rollout_matches_the_oracle_with_explicit_noise_and_with_rng(geo):
    """One prompt frame -> 4 frames, 2 noise steps (3 forwards per frame, windows of 2, 3 and 4 frames); rng=: the same rollout on the draws of a NoiseSource,
    the oracle fed the materialised normals of the documented slots (frame f of sample b = slot f of sample sample0 + b)."""
    from gtav_amd.generate import generate_latents
    m, sd, cfg = _mk_dit(geo, seed=6)
    shape = (cfg.in_channels, cfg.input_h, cfg.input_w)
    g = torch.Generator().manual_seed(9)
    B, total, steps = 2, 4, 2
    x0 = torch.randn(B, 1, *shape, generator=g) * 0.5
    noise = torch.randn(B, total - 1, *shape, generator=g)
    a = _one_hot(B, total, g)
    dit_fn = lambda xx, tt, aa: O.dit_forward(sd, cfg, xx, tt, aa)
    with torch.no_grad():
        ref = O.generate_latents(dit_fn, x0, total, steps, noise, a, max_frames=5)
    out = generate_latents(m, x0, total, steps, noise, a)
    out_c = generate_latents(m, x0, total, steps, noise, a, ctx_cache=True)
    assert rel_l2(out, ref, "window") < TOL_ROLLOUT and rel_l2(out_c, ref, "cached") < TOL_ROLLOUT
    src = R.NoiseSource(0x1357, sample0=3)
    mat = src.clone()
    noise_r = mat.normal(B, total - 1, shape, mat.next_draw(), 1, dev()).cpu()
    with torch.no_grad():
        ref_r = O.generate_latents(dit_fn, x0, total, steps, noise_r, a, max_frames=5)
    assert rel_l2(generate_latents(m, x0, total, steps, actions=a, rng=src), ref_r, "rng") < TOL_ROLLOUT
    assert src.draw == mat.draw
    m.check()


# ---- 4. the VAE at other latent widths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("latent_dim", [4, 8, 32])
def test_vae_encode_decode_and_posterior_sample(latent_dim):
    kw = dict(SMALL_VAE, latent_dim=latent_dim)
    sd = W.synth_state_dict(W.vae_param_shapes(**kw), seed=5)
    v = AutoencoderKL(**kw, init_weights=False)
    v.load_state_dict(sd)
    cfg = O.VAEConfig(**kw)
    g = torch.Generator().manual_seed(1)
    img = torch.rand(3, 3, 64, 96, generator=g) * 2 - 1
    with torch.no_grad():
        mom = O.vae_encode_moments(sd, cfg, img)
    post = v.encode(img)
    assert post.mean.shape == (3, cfg.seq_len, latent_dim)
    assert rel_l2(post.mean, mom[..., :latent_dim], "mean") < TOL_SMALL
    assert rel_l2(post.logvar, mom[..., latent_dim:].clamp(-30, 20), "logvar") < TOL_SMALL
    z = torch.randn(3, cfg.seq_len, latent_dim, generator=g)
    with torch.no_grad():
        ref = O.vae_decode(sd, cfg, z)
    assert rel_l2(v.decode(z), ref, "decode") < TOL_SMALL
    # sample(rng=) on this posterior against the host restatement of the stream: frame r = sample sample0 + r, slot 0
    seed = 0x0123456789ABCDEF
    src = R.NoiseSource(seed, sample0=5)
    zs = post.sample(rng=src)
    assert src.draw == 1 and zs.shape == post.mean.shape
    normal = R.host_normal(3, cfg.seq_len * latent_dim, seed, 0, 5, 0, 1).reshape(3, cfg.seq_len, latent_dim)
    std = np.exp(0.5 * post.logvar.cpu().numpy().astype(np.float64))
    want = post.mean.cpu().numpy().astype(np.float64) + std * normal
    err = np.abs(zs.cpu().numpy().astype(np.float64) - want)
    bound = NORMAL_BOUND * std + 2.0 ** -22 * np.abs(want)
    print(f"[geometry posterior latent_dim={latent_dim}] max error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    v.check()


# ---- 5. a VAE and a DiT on 4-channel latents, end to end ------------------------------------------------------------------------------------------
def test_vae_and_dit_on_4_channel_latents_end_to_end():
    """AutoencoderKL(latent_dim=4, patch 8, 64 x 96 frames) feeds DiT(in_channels=4, patch 2, 8 x 12 latents: 24 tokens per frame, F = 16).  generate_clip and
    training_step on frames against the same composition of oracle calls.  Bounds, from the per-stage bounds above: the rollout starts from encoded latents
    that are within TOL_SMALL, and the prompt frame enters every window as context, so the final latents are held to TOL_SMALL + TOL_ROLLOUT; the decoder
    adds its own TOL_SMALL to the float frames.  The training loss |v - v_target|^2 / n moves by at most 2 |dv| / |v - v_target| relative; dv is one
    forward's TOL_SMALL on top of the encoder's, and |v - v_target| >= |v| to within the two being uncorrelated: 4 x TOL_SMALL."""
    from gtav_amd.generate import generate_clip
    from gtav_amd.train import encode_frames, training_step
    vkw = dict(SMALL_VAE, latent_dim=4)
    dkw = dict(SMALL, input_h=8, input_w=12, patch_size=2, in_channels=4)
    vsd = W.synth_state_dict(W.vae_param_shapes(**vkw), seed=5)
    dsd = W.synth_state_dict(W.dit_param_shapes(**dkw), seed=6)
    vae = AutoencoderKL(**vkw, init_weights=False)
    vae.load_state_dict(vsd)
    vcfg, dcfg = O.VAEConfig(**vkw), O.DiTConfig(**dkw)
    dit_fn = lambda xx, tt, aa: O.dit_forward(dsd, dcfg, xx, tt, aa)
    g = torch.Generator().manual_seed(21)
    B, total, steps = 2, 3, 2
    frames = torch.rand(B, 1, 3, 64, 96, generator=g)
    noise = torch.randn(B, total - 1, 4, 8, 12, generator=g)
    a = _one_hot(B, total, g)
    dit = DiT(**dkw, max_batch=B, init_weights=False)
    dit.load_state_dict(dsd)
    lat, out = generate_clip(dit, vae, frames, noise, total, steps, actions=a, to_uint8=False, gather=False)
    with torch.no_grad():
        x0 = O.vae_encode_frames(vsd, vcfg, frames)
        lat_ref = O.generate_latents(dit_fn, x0, total, steps, noise, a, max_frames=5)
        z = lat_ref.permute(0, 1, 3, 4, 2).reshape(B * total, 8 * 12, 4)
        img_ref = ((O.vae_decode(vsd, vcfg, z / 0.07843137255) + 1) / 2).reshape(B, total, 3, 64, 96)
    assert lat.shape == (B, total, 4, 8, 12)
    assert rel_l2(lat[:, :1], x0, "encoded prompt") < TOL_SMALL
    assert rel_l2(lat, lat_ref, "clip latents") < TOL_SMALL + TOL_ROLLOUT
    assert rel_l2(out, img_ref, "clip frames") < 2 * TOL_SMALL + TOL_ROLLOUT
    dit.check()
    # training_step on frames: encode, then one optimisation step on a trainable model of the same weights
    clip = torch.rand(B, 3, 3, 64, 96, generator=g)
    tgt, ctx = torch.tensor([30, 10]), torch.tensor([5, 20])
    cn = torch.randn(B, 2, 4, 8, 12, generator=g)
    nz = torch.randn(B, 1, 4, 8, 12, generator=g)
    mt = DiT(**dkw, max_batch=B, max_frames=3, init_weights=False, trainable=True)
    mt.load_state_dict(dsd)
    lat_t = encode_frames(vae, clip)
    loss = training_step(mt, lat_t, a, tgt, ctx, cn, nz, lr=3e-4, weight_decay=0.01, max_grad_norm=1.0, n_prompt_frames=2)
    with torch.no_grad():
        lat_o = O.vae_encode_frames(vsd, vcfg, clip)
        loss_o = O.train_forward_loss(dit_fn, lat_o, a, tgt, ctx, cn, nz, n_prompt_frames=2)[0]
    assert rel_l2(lat_t, lat_o, "encoded clip") < TOL_SMALL
    e = abs(float(loss) - float(loss_o)) / float(loss_o)
    print(f"[geometry end-to-end] training loss {float(loss):.6f} oracle {float(loss_o):.6f} rel {e:.3e}")
    assert e < 4 * TOL_SMALL
    applied, skipped, _ = mt.train_stats()
    assert applied and skipped == 0
    mt.check()
    vae.check()
