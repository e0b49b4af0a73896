"""Range safety: the bf16-operand mode and the automatic fp16 -> bf16 switch (include/gtav_amd.h "operand type").

The reference runs this path under bf16 autocast by default (generate.py:125-127, train_dit.py:190-198, denoise_step's dtype=torch.bfloat16); the product's
default is fp16 operands (1e-3 parity with the fp32 reference).  A checkpoint with activations beyond +-65504 is clamped and flagged in fp16; with
range_policy="auto" the layer groups that saturated move to bf16 operands — the same kernels compiled for v_mfma_f32_16x16x32_bf16 — and the recomputed
result matches the fp32 oracle to the bf16 bound.  Tolerances: bf16 operands (8 mantissa bits) give 6-9e-3 relative L2 per full-size forward
(measured in round 1); the bound asserted here is 1.5e-2 for an all-bf16 model and 1e-2 when only the saturated group is bf16."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import dev  # noqa: E402
from helpers import rel_l2_logged as rel_l2  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402
import gtav_amd.weights as W  # noqa: E402
from gtav_amd.lib import GtavError, GtavRangeSwitch  # noqa: E402
from gtav_amd.model.dit import DiT, DiT_models  # noqa: E402
from gtav_amd.model.vae import AutoencoderKL  # noqa: E402

TOL_BF16 = 1.5e-2      # every operand group bf16
TOL_BF16_ONE_GROUP = 1e-2   # VERDICT r5 item 5's bound: only the saturated layers are bf16
TOL_SMALL = 2e-3       # the fp16 bound of the toy widths (tests/test_gpu_models.py)

SMALL_DIT = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)
SMALL_VAE = dict(latent_dim=16, input_height=64, input_width=96, patch_size=8, enc_dim=128, enc_depth=2, enc_heads=2, dec_dim=256, dec_depth=2, dec_heads=4)


def _inputs(cfg, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, cfg.in_channels, cfg.input_h, cfg.input_w, generator=g)
    t = torch.randint(0, 1000, (B, T), generator=g)
    a = torch.zeros(B, T, 25)
    a[torch.arange(B)[:, None], torch.arange(T)[None], torch.randint(0, 25, (B, T), generator=g)] = 1
    return x, t, a


def test_bf16_operands_small_dit_every_token_count_class():
    """Every layer group on bf16 operands, toy width: the skinny / loader-wave / 128 x 128 tiles, the split-K slab path and both attention kernels, at
    144-token (cached-step-like T = 1), window (T = 5) and a few-thousand-token batches; then back to fp16: bit-identical to the first fp16 result."""
    sd = W.synth_state_dict(W.dit_param_shapes(**SMALL_DIT), seed=3)
    m = DiT(**SMALL_DIT, init_weights=False, max_batch=16)
    m.load_state_dict(sd)
    cfg = O.DiTConfig(**SMALL_DIT)
    cases = [(1, 1, 5), (1, 5, 6), (3, 4, 7), (16, 5, 8)]
    fp16_out = {}
    for B, T, seed in cases:
        x, t, a = _inputs(cfg, B, T, seed)
        fp16_out[(B, T)] = m(x, t, a).clone()
    m.check()
    m.set_operand_dtype(torch.bfloat16)
    assert all(d == torch.bfloat16 for d in m.operand_dtypes())
    for B, T, seed in cases:
        x, t, a = _inputs(cfg, B, T, seed)
        with torch.no_grad():
            ref = O.dit_forward(sd, cfg, x, t, a)
        out = m(x, t, a)
        e = rel_l2(out, ref)
        assert 5e-4 < e < TOL_BF16, (B, T, e)           # bf16 precision: not better than fp16's either — the mode really ran
        assert torch.equal(out, m(x, t, a))
    m.check()
    m.set_operand_dtype(torch.float16)
    for B, T, seed in cases:
        x, t, a = _inputs(cfg, B, T, seed)
        assert torch.equal(m(x, t, a), fp16_out[(B, T)])
    m.check()


def test_bf16_operands_full_size_dit_batch8_and_cached_step():
    """DiT-S/2 at B = 8, T = 5 (M = 5 760: the large-M kernels — 128 x 192 tiles, the persistent kernel's in-place residual epilogue, the wave-per-row
    LayerNorm, 640-item attention grids) with every group on bf16 operands against the fp32 oracle; the context-cached sampler step (M = 1 152: 128 x 144 frame
    tiles, slabs) reproduces the window step in bf16 as it does in fp16."""
    from gtav_amd.utils import alphas_cumprod
    m = DiT_models["DiT-S/2"](init_weights=False, max_batch=8)
    sd = W.synth_state_dict(W.dit_param_shapes(depth=16), seed=0)
    m.load_state_dict(sd)
    m.set_operand_dtype(torch.bfloat16)
    cfg = O.dit_s_2()
    x, t, a = _inputs(cfg, 8, 5, seed=41)
    t[:, :4] = 15
    with torch.no_grad():
        ref = O.dit_forward(sd, cfg, x, t, a)
    e = rel_l2(m(x, t, a), ref)
    print("full DiT B=8 T=5 bf16 operands rel-L2", e)
    assert e < TOL_BF16
    m.check()
    m.set_schedule(alphas_cumprod(1e-4))
    ad = a.to(dev())
    xd = x.to(dev()).contiguous()
    m.denoise_step_(xd, 0, 4, 15, 500, 490, False, ad)
    xc = x.to(dev()).contiguous()
    m.denoise_step_(xc, 0, 4, 15, 500, 490, False, ad)
    xc[:, -1] = x[:, -1].to(dev())
    m.denoise_step_(xc, 0, 4, 15, 500, 490, False, ad, cached=True)
    assert rel_l2(xc[:, -1], xd[:, -1]) < 1e-3          # same kernels on other K slices: fp32 summation order -> a few bf16 roundings flip (fp16: 1.4e-5, bf16: 1.1e-4)
    m.check()
    # batch 1 (M = 720: the headline's tiles, next-weight prefetch, split-K slabs) and its captured graph
    x1, t1, a1 = x[:1], t[:1], a[:1]
    with torch.no_grad():
        ref1 = O.dit_forward(sd, cfg, x1, t1, a1)
    assert rel_l2(m(x1, t1, a1), ref1) < TOL_BF16
    xs = x1.to(dev()).contiguous()
    a1d = a1.to(dev())
    outs = []
    for _ in range(3):                                  # eager, capture, replay
        xx = xs.clone()
        xs2 = xs                                        # (the graph is keyed by the buffer: step the same one, restore it in between)
        m.denoise_step_(xs2, 0, 4, 15, 500, 490, False, a1d)
        outs.append(xs2.clone())
        xs.copy_(xx)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    m.check()


@functools.lru_cache(maxsize=None)
def _outlier_case():
    """(clean weights, outlier weights, config, x, t, a, the fp32 oracle's output for the outlier weights) at B = 1, T = 2; read-only."""
    sd = W.synth_state_dict(W.dit_param_shapes(**SMALL_DIT), seed=3)
    big = dict(sd)
    big["blocks.0.s_mlp.fc1.weight"] = sd["blocks.0.s_mlp.fc1.weight"] * 3e5
    cfg = O.DiTConfig(**SMALL_DIT)
    x, t, a = _inputs(cfg, 1, 2, seed=11)
    with torch.no_grad():
        ref = O.dit_forward(big, cfg, x, t, a)
    return sd, big, cfg, x, t, a, ref


def test_autorange_moves_exactly_the_saturated_layers_to_bf16():
    """the x3e5 outlier checkpoint of test_fp16_saturation_is_clamped_and_reported (fc1 of block 0's spatial MLP scaled so that the GELU
    output exceeds 65504).  range_policy="report": clamped + reported, as before.  range_policy="auto": check() switches operand group 0 — that half-block
    only — to bf16 and raises GtavRangeSwitch; the recomputed forward is clean and matches the fp32 oracle to the bf16 bound instead of returning clamped values."""
    sd, big, cfg, x, t, a, ref = _outlier_case()
    m = DiT(**SMALL_DIT, init_weights=False, max_batch=1, range_policy="auto")
    m.load_state_dict(big)
    clipped = m(x, t, a).clone()
    with pytest.raises(GtavRangeSwitch) as ei:
        m.check()
    assert ei.value.groups == [0]
    assert [d == torch.bfloat16 for d in m.operand_dtypes()] == [True] + [False] * (m.n_operand_groups - 1)
    out = m(x, t, a)
    m.check()                                            # clean: nothing saturates any more
    e_clip, e = rel_l2(clipped, ref), rel_l2(out, ref)
    print(f"outlier checkpoint: clamped fp16 result {e_clip:.3e} from the oracle, after the switch {e:.3e}")
    assert e < TOL_BF16_ONE_GROUP and e_clip > 10 * e
    # a clean checkpoint on the same model object: the group stays bf16 until told otherwise; back to fp16 restores the fp16 margin
    m.load_state_dict(sd)
    with torch.no_grad():
        ref0 = O.dit_forward(sd, cfg, x, t, a)
    assert rel_l2(m(x, t, a), ref0) < TOL_BF16_ONE_GROUP
    m.set_operand_dtype(torch.float16)
    assert rel_l2(m(x, t, a), ref0) < TOL_SMALL
    m.check()


def test_autorange_that_also_reports_another_error_leaves_the_model_usable():
    """A check() that finds a saturation AND another error: gtav_dit_autorange moves the saturated group to bf16 on the handle (which un-finalizes it) and then
    fails with the other error, here a timestep of 1000 (clamped to 999 and flagged by the conditioning kernel; nothing is read out of range).  check() raises that
    error, and the model has followed the handle all the same: operand_dtypes() is what gtav_dit_get_operand_dtype reports group by group, and the next forward
    re-sends the weights, runs, and matches the fp32 oracle to the bf16 bound."""
    from gtav_amd import lib as L
    sd, big, cfg, x, t, a, ref = _outlier_case()
    m = DiT(**SMALL_DIT, init_weights=False, max_batch=1, range_policy="auto")
    m.load_state_dict(big)
    bad = t.clone()
    bad[0, 0] = 1000
    m(x, bad, a)
    with pytest.raises(GtavError, match=r"timestep outside \[0, 999\]") as ei:
        m.check()
    assert not isinstance(ei.value, GtavRangeSwitch)
    d, on_handle = ctypes.c_int32(0), []
    for g in range(m.n_operand_groups):
        L.check(L.load().gtav_dit_get_operand_dtype(m._handle, g, ctypes.byref(d)))
        on_handle.append(torch.bfloat16 if d.value == 1 else torch.float16)
    assert m.operand_dtypes() == on_handle and on_handle.count(torch.bfloat16) >= 1
    out = m(x, t, a)
    m.check()
    e = rel_l2(out, ref)
    print(f"after a check() that switched and failed: {e:.3e} from the oracle, bf16 groups {[g for g, v in enumerate(on_handle) if v == torch.bfloat16]}")
    assert e < TOL_BF16


def test_autorange_in_the_generation_loop():
    """generate_latents with range_policy="auto": the clip generated with the outlier checkpoint is regenerated from the same inputs after the switch and
    agrees with the oracle's rollout; with "report" the same call raises."""
    from gtav_amd.generate import generate_latents
    sd = W.synth_state_dict(W.dit_param_shapes(**SMALL_DIT), seed=3)
    big = dict(sd)
    big["blocks.1.t_mlp.fc1.weight"] = sd["blocks.1.t_mlp.fc1.weight"] * 3e5
    cfg = O.DiTConfig(**SMALL_DIT)
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(1, 2, 16, 8, 16, generator=g) * 0.5
    nz = torch.randn(1, 1, 16, 8, 16, generator=g)
    dit_fn = lambda xx, tt, aa: O.dit_forward(big, cfg, xx, tt, aa)
    with torch.no_grad():
        ref = O.generate_latents(dit_fn, x0, 3, 4, nz, None)
    m = DiT(**SMALL_DIT, init_weights=False, max_batch=1, range_policy="auto")
    m.load_state_dict(big)
    out = generate_latents(m, x0, 3, 4, nz, None).cpu()
    assert m.operand_dtypes()[3] == torch.bfloat16 and sum(d == torch.bfloat16 for d in m.operand_dtypes()) == 1     # group 2 * 1 + 1: block 1, temporal half
    assert rel_l2(out, ref) < 2e-2
    m2 = DiT(**SMALL_DIT, init_weights=False, max_batch=1)
    m2.load_state_dict(big)
    with pytest.raises(GtavError, match="fp16 range"):
        generate_latents(m2, x0, 3, 4, nz, None)


def test_denoise_step_honours_dtype():
    """train_dit.denoise_step's `dtype` argument (train_dit.py:30-41, 105-107: the autocast type): torch.bfloat16 -> bf16 operands, torch.float16 -> fp16
    operands, None (this mirror's default) leaves the model as it is."""
    from gtav_amd.sampler import denoise_step
    from gtav_amd.utils import alphas_cumprod
    sd = W.synth_state_dict(W.dit_param_shapes(**SMALL_DIT), seed=5)
    m = DiT(**SMALL_DIT, init_weights=False, max_batch=2)
    m.load_state_dict(sd)
    cfg = O.DiTConfig(**SMALL_DIT)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 4, 16, 8, 16, generator=g) * 0.7
    a = torch.zeros(2, 4, 25)
    a[:, :, 3] = 1
    nr = torch.linspace(0, 999, 11)
    ac = alphas_cumprod(1e-4)[:, None, None, None]
    dit_fn = lambda xx, tt, aa: O.dit_forward(sd, cfg, xx, tt, aa)
    with torch.no_grad():
        xr, vr = O.denoise_step(dit_fn, x, a, 6, 15, nr, ac, start_frame=1)
    xp, vp = denoise_step(m, x, a, 6, 15, nr, ac, start_frame=1)                       # default: fp16 operands
    assert rel_l2(vp, vr) < TOL_SMALL and all(d == torch.float16 for d in m.operand_dtypes())
    xb, vb = denoise_step(m, x, a, 6, 15, nr, ac, start_frame=1, dtype=torch.bfloat16)
    eb = rel_l2(vb, vr)
    assert 5e-4 < eb < TOL_BF16 and all(d == torch.bfloat16 for d in m.operand_dtypes())
    assert rel_l2(xb, xr) < TOL_BF16
    xh, vh = denoise_step(m, x, a, 6, 15, nr, ac, start_frame=1, dtype=torch.float16)
    assert torch.equal(vh, vp) and all(d == torch.float16 for d in m.operand_dtypes())
    with pytest.raises(ValueError):
        denoise_step(m, x, a, 6, 15, nr, ac, start_frame=1, dtype=torch.float32)


def test_bf16_operands_vae():
    """The VAE handle on bf16 operands (affine LayerNorm, biased QKV + partial RoPE, both attention kernels' S = 96 form, erf-GELU, predictor) against the
    oracle, and back to fp16 bit for bit."""
    vsd = W.synth_state_dict(W.vae_param_shapes(**SMALL_VAE), seed=5)
    v = AutoencoderKL(**SMALL_VAE, init_weights=False, max_frames_per_call=24)
    v.load_state_dict(vsd)
    vcfg = O.VAEConfig(**SMALL_VAE)
    g = torch.Generator().manual_seed(2)
    img = torch.rand(24, 3, 64, 96, generator=g) * 2 - 1
    z = torch.randn(24, vcfg.seq_len, 16, generator=g)
    with torch.no_grad():
        mom = O.vae_encode_moments(vsd, vcfg, img)
        dec = O.vae_decode(vsd, vcfg, z)
    e16, d16 = v.encode(img).mean.clone(), v.decode(z).clone()
    assert rel_l2(e16, mom[..., :16]) < TOL_SMALL and rel_l2(d16, dec) < TOL_SMALL
    v.set_operand_dtype(torch.bfloat16)
    eb, db = rel_l2(v.encode(img).mean, mom[..., :16]), rel_l2(v.decode(z), dec)
    assert 5e-4 < eb < TOL_BF16 and 5e-4 < db < TOL_BF16
    v.check()
    v.set_operand_dtype(torch.float16)
    assert torch.equal(v.encode(img).mean, e16) and torch.equal(v.decode(z), d16)
    v.check()


def test_bf16_operands_full_size_vae_flash_attention():
    """ViT-L/20 on 360 x 640 frames with bf16 operands: the S = 576 flash attention kernel (K / Vt streamed through the LDS ring, probabilities as bf16 MFMA
    operands, q pre-scaled in the to_qkv epilogue) and the large-M GEMM tiles, encode of 8 frames and decode of 2 against the oracle."""
    from gtav_amd.model.vae import VAE_models
    v = VAE_models["vit-l-20-shallow-encoder"](init_weights=False, max_frames_per_call=8)
    sd = W.synth_state_dict(W.vae_param_shapes(), seed=1)
    v.load_state_dict(sd)
    v.set_operand_dtype(torch.bfloat16)
    cfg = O.vit_l_20_shallow_encoder()
    g = torch.Generator().manual_seed(6)
    img = torch.rand(8, 3, 360, 640, generator=g) * 2 - 1
    with torch.no_grad():
        mom = O.vae_encode_moments(sd, cfg, img[:2])
    assert rel_l2(v.encode(img).mean[:2], mom[..., :16]) < TOL_BF16
    z = torch.randn(2, 576, 16, generator=g)
    with torch.no_grad():
        dec = O.vae_decode(sd, cfg, z)
    assert rel_l2(v.decode(z), dec) < TOL_BF16
    v.check()


def test_weight_beyond_fp16_range_is_reported_and_recovered():
    """A GEMM weight beyond +-65504 is clamped by the fp16 conversion: it must not be clamped in silence.  The conversion raises the saturation bit of the weight's
    operand group; range_policy="auto" moves that group to bf16 (whose weight image holds the value) and the recomputed forward matches the oracle."""
    sd = W.synth_state_dict(W.dit_param_shapes(**SMALL_DIT), seed=3)
    big = dict(sd)
    w = sd["blocks.1.s_attn.to_out.weight"].clone()
    w[5, 7] = 3.0e5                                           # one outlier weight (fp16 would hold 65504)
    big["blocks.1.s_attn.to_out.weight"] = w
    cfg = O.DiTConfig(**SMALL_DIT)
    x, t, a = _inputs(cfg, 1, 3, seed=12)
    with torch.no_grad():
        ref = O.dit_forward(big, cfg, x, t, a)
    m = DiT(**SMALL_DIT, init_weights=False, max_batch=1)
    m.load_state_dict(big)
    m(x, t, a)
    with pytest.raises(GtavError, match="fp16 range"):
        m.check()
    m2 = DiT(**SMALL_DIT, init_weights=False, max_batch=1, range_policy="auto")
    m2.load_state_dict(big)
    m2(x, t, a)
    with pytest.raises(GtavRangeSwitch) as ei:
        m2.check()
    assert ei.value.groups == [2]                            # block 1, spatial half
    out = m2(x, t, a)
    m2.check()
    assert rel_l2(out, ref) < TOL_BF16_ONE_GROUP


def test_training_handle_refuses_bf16_operands():
    m = DiT(**SMALL_DIT, init_weights=False, max_batch=1, trainable=True)
    with pytest.raises(GtavError, match="fp16 operands"):
        m.set_operand_dtype(torch.bfloat16)
