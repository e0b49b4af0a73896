"""The noise kernels against the stream contract (DESIGN.md "Noise streams", restated on the host by gtav_amd.rng) and the rng= paths of the training step,
the checkpoint and the sampler against the paths with explicit draws.

Bounds.  Raw words, geometry independence, the fused window launch against the composition of the existing kernels, rng= against materialised draws: equality
bit for bit (deterministic integer arithmetic, and fp32 expressions that are one text in every kernel).  Normals against the fp64 host restatement: 2^-17
absolute per element — 1-ulp logf and sqrtf on r <= 5.77, 2-ulp sincos, together <= 3.6e-6, and a factor 2 on top.  Posterior sample: 2^-17 exp(0.5 logvar)
+ 2^-22 |result| (the normal's bound scaled by the standard deviation, plus 1-ulp expf and the rounding of the sum).

Shapes: n = 2048 (the toy latent frame 16 x 8 x 16: two full blocks of 256 threads x 4 elements), 148 (the grid's tail: 37 of 256 threads), 9216 (the
shipped latent frame 16 x 18 x 32: nine blocks); up to 4 x 5 rows."""
import math

import numpy as np
import pytest
import torch

import train_cases as TC
from gtav_amd import lib as L
from gtav_amd import rng as R
from gtav_amd.model.dit import DiT
from helpers import dev, stream
from test_host_rng import N as N_MOMENTS
from test_host_rng import SEED, moment_checks

pytestmark = pytest.mark.gpu

SIZES = [2048, 148, 9216]
INF = float("inf")
BOUND = 2.0 ** -17


def _bits(rows, n, seed, draw, sample0=0, slot0=0, sps=1):
    out = torch.zeros((rows, n), dtype=torch.int32, device=dev())
    L.check(L.load().gtav_op_rng_bits(out.data_ptr(), rows, n, seed, draw, sample0, slot0, sps, stream()))
    return out.cpu().numpy().view(np.uint32)


def _normal_into(ptr, sample_stride, rows, n, seed, draw, sample0, slot0, sps, clamp=INF):
    L.check(L.load().gtav_rng_normal(ptr, sample_stride, rows, n, seed, draw, sample0, slot0, sps, clamp, stream()))


def _normal(B, slots, n, seed, draw, sample0=0, slot0=0, clamp=INF):
    out = torch.full((B, slots, n), float("nan"), device=dev())
    _normal_into(out.data_ptr(), slots * n, B * slots, n, seed, draw, sample0, slot0, slots, clamp)
    return out


# ---- 1: raw words ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sample0,slot0,sps", [(0, 0, 5), (0xFFFFFFF0, 30, 5), (3, 0xFFFFFFFE, 3)], ids=["origin", "high-sample", "wrapping-slot"])
def test_bits_equal_the_host_stream(n, sample0, slot0, sps):
    """(0xFFFFFFF0, 30): sample ids up to 0xFFFFFFF3 and slots 30 .. 34 — no counter field runs into another; the third case wraps the slot field itself."""
    seed, draw = 0x9E3779B97F4A7C15, 0xC0FFEE
    got = _bits(20, n, seed, draw, sample0, slot0, sps)
    assert np.array_equal(got, R.host_bits(20, n, seed, draw, sample0, slot0, sps))


# ---- 2: normals -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_normal_against_the_fp64_restatement_and_the_clamp(n):
    seed, draw, sample0, slot0 = SEED, 5, 7, 1
    z = _normal(4, 5, n, seed, draw, sample0, slot0)
    want = R.host_normal(20, n, seed, draw, sample0, slot0, 5).reshape(4, 5, n)
    err = np.abs(z.cpu().numpy().astype(np.float64) - want).max()
    print(f"[normal vs fp64] n={n}: max |error| {err:.3e} (bound {BOUND:.3e}), max |z| {float(z.abs().max()):.4f}")
    assert err <= BOUND
    assert float(z.abs().max()) <= 5.7682
    clamped = _normal(4, 5, n, seed, draw, sample0, slot0, clamp=0.5)
    assert torch.equal(clamped.cpu(), z.cpu().clamp(-0.5, 0.5))
    assert float(clamped.abs().max()) == 0.5


def test_device_moments():
    """2^20 normals of one row (1 024 blocks) inside the five-sigma bounds of tests/test_host_rng.py."""
    z = _normal(1, 1, N_MOMENTS, SEED, 0)[0, 0].cpu().numpy()
    for name, got, bound in moment_checks(z):
        print(f"[device normal] {name}: {got:.3e} (bound {bound:.3e})")
        assert abs(got) < bound, name
    assert np.abs(z).max() <= 5.7682


# ---- 3: geometry ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_a_draw_does_not_depend_on_the_call_geometry(n):
    seed, draw, sample0, slot0 = 0xABCDEF0123456789, 11, 40, 2
    whole = _normal(4, 5, n, seed, draw, sample0, slot0)
    per_sample = torch.cat([_normal(1, 5, n, seed, draw, sample0 + b, slot0) for b in range(4)])
    assert torch.equal(per_sample, whole)
    per_row = torch.stack([torch.cat([_normal(1, 1, n, seed, draw, sample0 + b, slot0 + w) for w in range(5)], dim=1)[0] for b in range(4)])
    assert torch.equal(per_row, whole)
    # frames 2 .. 6 of a (4, 7, n) buffer, the way the sampler fills x[:, n_prompt:]: the other frames stay as they were
    buf = torch.full((4, 7, n), -7.0, device=dev())
    _normal_into(buf[:, 2:].data_ptr(), 7 * n, 20, n, seed, draw, sample0, slot0, 5)
    assert torch.equal(buf[:, 2:], whole)
    assert bool((buf[:, :2] == -7.0).all())
    # and other draw numbers / seeds are other noise
    assert not torch.equal(_normal(4, 5, n, seed, draw + 1, sample0, slot0), whole)
    assert not torch.equal(_normal(4, 5, n, seed ^ (1 << 40), draw, sample0, slot0), whole)


# ---- 4: the fused window launch -------------------------------------------------------------------------------------------------------------
def _window_inputs(B, Wn, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, Wn, n, generator=g) * 0.7).to(dev())
    alpha = torch.rand(B, Wn, generator=g)
    alpha.reshape(-1)[0] = 1.0
    alpha.reshape(-1)[-1] = 1e-6
    return x, alpha.to(dev()).contiguous()


def _window_fused(x, alpha, seed, draw, sample0, clamp):
    B, Wn, n = x.shape
    x_noisy, vt = torch.full_like(x, float("nan")), torch.full((B, n), float("nan"), device=x.device)
    L.check(L.load().gtav_noise_window_rng(x.data_ptr(), alpha.data_ptr(), x_noisy.data_ptr(), vt.data_ptr(), B, Wn, n, seed, draw, sample0, clamp, stream()))
    return x_noisy, vt


def _window_composed(x, alpha, seed, draw, sample0, clamp):
    """gtav_rng_normal, then gtav_add_noise and gtav_vtarget exactly as train._frame_step calls them."""
    B, Wn, n = x.shape
    lib = L.load()
    all_noise = _normal(B, Wn, n, seed, draw, sample0)
    x_noisy = torch.empty_like(x)
    L.check(lib.gtav_add_noise(x.data_ptr(), all_noise.data_ptr(), alpha.data_ptr(), x_noisy.data_ptr(), B * Wn, n, clamp, stream()))
    x_last, nz_last, a_last = x[:, -1].contiguous(), all_noise[:, -1].contiguous(), alpha[:, -1].contiguous()
    vt = torch.empty_like(x_last)
    L.check(lib.gtav_vtarget(x_last.data_ptr(), nz_last.data_ptr(), a_last.data_ptr(), vt.data_ptr(), B, n, clamp, stream()))
    return x_noisy, vt


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("Wn", [5, 1])
@pytest.mark.parametrize("clamp", [20.0, 1.5], ids=["clamp20", "clamp1.5"])
def test_noise_window_equals_the_composition_of_the_existing_kernels(n, Wn, clamp):
    """clamp 20 is the trainer's (never reached: |z| <= 5.77); 1.5 makes the clamp act on one element in seven."""
    seed, draw, sample0 = 0x5DEECE66D, 4, 9
    x, alpha = _window_inputs(3, Wn, n)
    got, want = _window_fused(x, alpha, seed, draw, sample0, clamp), _window_composed(x, alpha, seed, draw, sample0, clamp)
    for name, g, w in zip(("x_noisy", "v_target"), got, want):
        assert torch.isfinite(w).all()
        assert torch.equal(g, w), f"{name}: {int((g != w).sum())} of {g.numel()} elements differ, max |diff| {float((g - w).abs().max()):.3e}"


@pytest.mark.parametrize("n", SIZES)
def test_noise_window_does_not_depend_on_the_batch_split(n):
    seed, draw = 0x5DEECE66D, 6
    x, alpha = _window_inputs(4, 5, n)
    xn, vt = _window_fused(x, alpha, seed, draw, 0, 20.0)
    for lo in (0, 2):
        xn_h, vt_h = _window_fused(x[lo:lo + 2].contiguous(), alpha[lo:lo + 2].contiguous(), seed, draw, lo, 20.0)
        assert torch.equal(xn_h, xn[lo:lo + 2]) and torch.equal(vt_h, vt[lo:lo + 2])
    assert not torch.equal(xn[:2], xn[2:])


# ---- 5: the VAE posterior -------------------------------------------------------------------------------------------------------------------
def test_vae_posterior_sample():
    from gtav_amd.model.vae import DiagonalGaussianDistribution
    frames, tokens, Ld = 2, 8, 16
    g = torch.Generator().manual_seed(2)
    mean = torch.randn(frames, tokens, Ld, generator=g)
    logvar = torch.tensor([-40.0, 0.0, 25.0])[torch.randint(0, 3, (frames, tokens, Ld), generator=g)]       # both clamps and the middle
    post = DiagonalGaussianDistribution(torch.cat([mean, logvar], dim=2).to(dev()))
    src = R.NoiseSource(SEED, sample0=5)
    src.next_draw()
    z = post.sample(rng=src)
    assert src.draw == 2 and z.shape == (frames, tokens, Ld)
    normal = R.host_normal(frames, tokens * Ld, SEED, 1, 5, 0, 1).reshape(frames, tokens, Ld)
    std = np.exp(0.5 * np.clip(logvar.numpy().astype(np.float64), -30, 20))
    want = mean.numpy().astype(np.float64) + std * normal
    err = np.abs(z.cpu().numpy().astype(np.float64) - want)
    bound = BOUND * std + 2.0 ** -22 * np.abs(want)
    print(f"[posterior vs fp64] max error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    # frames as slots of one sample: the same call through the other mapping
    z2 = post.sample(rng=src, slot0=3, slots_per_sample=2)
    normal2 = R.host_normal(frames, tokens * Ld, SEED, 2, 5, 3, 2).reshape(frames, tokens, Ld)
    want2 = mean.numpy().astype(np.float64) + std * normal2
    assert (np.abs(z2.cpu().numpy().astype(np.float64) - want2) <= BOUND * std + 2.0 ** -22 * np.abs(want2)).all()
    # the default is still the CPU draw of torch's generator
    torch.manual_seed(4)
    a = post.sample()
    torch.manual_seed(4)
    assert torch.equal(a, post.mean + post.std * torch.randn(post.mean.shape).to(dev()))


# ---- 6: the training step -------------------------------------------------------------------------------------------------------------------
KW = dict(TC.TOY_KW, depth=3)             # tests/test_gpu_train_recompute.py
STEP_KW = dict(lr=3e-4, weight_decay=0.01, max_grad_norm=1.0)
NOISE_STEPS, CTX_MAX = 50, 40


def _sd():
    return TC.state_dict(KW)


def _model(dtype=TC.F16):
    return TC.model(KW, 2, 5, dtype)


def _clip(F):
    """Latents and actions of TC.clip: the noise and the indices come from the stream under test."""
    return TC.clip(KW, F=F)[:2]


def _masters(m):
    m.pull_weights()
    return {k: v.clone() for k, v in m._sd.items()}


def _materialise(src, B, F, n_prompt, max_frames=5):
    """The four draws of one step from `src` in the documented order: per target frame one draw number, the two index draws, the context noise from slots
    0 .. W - 2 and the target noise from slot W - 1 of the frame's window."""
    tgt, ctx, cn, nz = [], [], [], []
    for i in range(n_prompt, F):
        Wn = min(i + 1, max_frames)
        d = src.next_draw()
        tgt.append(src.randint(1, NOISE_STEPS + 1, B, R.SLOT_TARGET_IDX, d))
        ctx.append(src.randint(1, CTX_MAX + 1, B, R.SLOT_CTX_IDX, d))
        cn.append(src.normal(B, Wn - 1, (16, 8, 16), d, 0, dev()))
        nz.append(src.normal(B, 1, (16, 8, 16), d, Wn - 1, dev()))
    return tgt, ctx, cn, nz


@TC.DTYPES
@pytest.mark.parametrize("F,n_prompt", [(5, 4), (6, 3)], ids=["one-target", "three-targets"])
def test_training_step_with_rng_equals_materialised_draws(F, n_prompt, dtype):
    from gtav_amd.train import training_step
    lat, a = _clip(F)
    src = R.NoiseSource(0x0123456789ABCDEF, sample0=6)
    ref = src.clone()
    ma, mb = _model(dtype), _model(dtype)
    for step in range(2):
        la = training_step(ma, lat, a, rng=src, ctx_max_noise_idx=CTX_MAX, noise_steps=NOISE_STEPS, n_prompt_frames=n_prompt, **STEP_KW)
        lb = training_step(mb, lat, a, *_materialise(ref, 2, F, n_prompt), noise_steps=NOISE_STEPS, n_prompt_frames=n_prompt, **STEP_KW)
        assert torch.equal(la, lb) and math.isfinite(float(la)), step
        assert ma.train_stats() == mb.train_stats() and ma.train_stats()[0], step
    assert src.draw == ref.draw == 2 * (F - n_prompt)
    wa, wb = _masters(ma), _masters(mb)
    for k in wb:
        assert torch.equal(wa[k], wb[k]), k
    assert not torch.equal(wa["blocks.1.s_mlp.fc1.weight"], _sd()["blocks.1.s_mlp.fc1.weight"])


def test_forward_loss_with_rng_equals_materialised_draws():
    from gtav_amd.train import forward_loss
    lat, a = _clip(5)
    src = R.NoiseSource(77)
    m = _model()
    got = forward_loss(m, lat, a, rng=src, ctx_max_noise_idx=CTX_MAX)
    want = forward_loss(m, lat, a, *_materialise(R.NoiseSource(77), 2, 5, 4))
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_resume_restores_the_noise_stream(tmp_path):
    """Two steps, save_state(rng=), a fresh model and a fresh NoiseSource, load_state(rng=), one step == three straight steps, bit for bit; without restoring
    the source the third step draws other noise and the weights differ; a checkpoint without the entry leaves the source untouched."""
    import json
    from gtav_amd.train import load_state, save_state, training_step
    lat, a = _clip(5)
    kw = dict(ctx_max_noise_idx=CTX_MAX, **STEP_KW)
    m1, s1 = _model(), R.NoiseSource(0xFEEDFACECAFEBEEF)
    for _ in range(3):
        training_step(m1, lat, a, rng=s1, **kw)
    straight = _masters(m1)
    m2, s2 = _model(), R.NoiseSource(0xFEEDFACECAFEBEEF)
    for _ in range(2):
        training_step(m2, lat, a, rng=s2, **kw)
    ck = str(tmp_path / "ck")
    save_state(m2, ck, global_step=2, epoch=0, rng=s2)
    assert json.load(open(tmp_path / "ck" / "step.json"))["rng"] == {"seed": 0xFEEDFACECAFEBEEF, "draw": 2}
    m3, s3 = DiT(**KW, max_batch=2, max_frames=5, init_weights=True, trainable=True), R.NoiseSource(1)
    assert load_state(m3, ck, rng=s3)["step"] == 2 and s3.state_dict() == s2.state_dict()
    training_step(m3, lat, a, rng=s3, **kw)
    resumed = _masters(m3)
    for k in straight:
        assert torch.equal(resumed[k], straight[k]), k
    m4, s4 = DiT(**KW, max_batch=2, max_frames=5, init_weights=True, trainable=True), R.NoiseSource(0xFEEDFACECAFEBEEF)
    load_state(m4, ck)                                   # the source is not restored: draw 0 again
    training_step(m4, lat, a, rng=s4, **kw)
    assert not torch.equal(_masters(m4)["blocks.1.s_mlp.fc1.weight"], straight["blocks.1.s_mlp.fc1.weight"])
    save_state(m2, str(tmp_path / "plain"), global_step=2, epoch=0)
    load_state(m4, str(tmp_path / "plain"), rng=s4)
    assert s4.draw == 1


# ---- 7: the sampler -------------------------------------------------------------------------------------------------------------------------
def test_sampler_with_rng_equals_materialised_noise_and_any_batch_split():
    from gtav_amd.generate import generate_latents
    B, n_prompt, total, steps = 2, 1, 4, 3
    x0 = torch.randn(B, n_prompt, 16, 8, 16, generator=torch.Generator().manual_seed(8)) * 0.5
    a = torch.zeros(B, total, 25)
    a[:, :, 3] = 1
    m = DiT(**KW, max_batch=B, init_weights=False)
    m.load_state_dict(_sd())
    src = R.NoiseSource(0x1357, sample0=0)
    src.next_draw()
    ref = src.clone()
    got = generate_latents(m, x0, total, steps, actions=a, rng=src).clone()
    assert src.draw == 2
    chunks = ref.normal(B, total - n_prompt, (16, 8, 16), ref.next_draw(), n_prompt, dev())
    want = generate_latents(m, x0, total, steps, chunks, a).clone()
    m.check()
    assert torch.isfinite(got).all() and torch.equal(got, want)
    for b in range(B):
        one = R.NoiseSource(0x1357, sample0=b)
        one.next_draw()
        assert torch.equal(generate_latents(m, x0[b:b + 1], total, steps, actions=a[b:b + 1], rng=one), got[b:b + 1]), b
