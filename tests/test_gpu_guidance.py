"""Classifier-free guidance in the fused sampler step (gtav_dit_set_guidance) on the GPU: against the CPU oracle, bit for bit against two unguided steps,
context-cached, hoisted conditioning, captured-graph replay under a changing scale, toggling, refusals, and a sliding-window rollout.
Cases, inputs, the oracle and the derivation of the bound TOL_SMALL amp(s): tests/guidance_cases.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guidance_cases as G  # noqa: E402
from helpers import dev  # noqa: E402
from helpers import rel_l2_logged as rel_l2  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402
import gtav_amd.weights as W  # noqa: E402
from gtav_amd import lib as L  # noqa: E402
from gtav_amd.model.dit import DiT  # noqa: E402
from gtav_amd.sampler import ddim_update, guided_combine  # noqa: E402
from gtav_amd.utils import alphas_cumprod  # noqa: E402

CUR = G.FRAMES - 1
MAX_BATCH = 4


def _mk(max_batch=MAX_BATCH, kw=G.SMALL_DIT, sd=None):
    m = DiT(**kw, max_batch=max_batch, init_weights=False)
    m.load_state_dict(sd or G.state_dict())
    m.set_schedule(alphas_cumprod(1e-4))
    return m


@functools.lru_cache(maxsize=None)
def _model():
    """The handle most tests share (max_batch 4: a guided step of batch 2).  Every test leaves it unguided."""
    return _mk()


def _step(m, x_cpu, a_dev, noise_idx, cached=False, cond_step=-1, xd=None, actions=True):
    """One fused step on a fresh device copy of x (or on `xd`): returns (xd, v_out)."""
    t_cur, t_next = G.timesteps(noise_idx)
    xd = x_cpu.to(dev()).contiguous() if xd is None else xd
    v = torch.full((xd.shape[0], *xd.shape[2:]), float("nan"), device=dev())
    m.denoise_step_(xd, G.START, CUR, G.T_CTX, t_cur, t_next, noise_idx <= 0, a_dev if actions else None, cached=cached, v_out=v, cond_step=cond_step)
    return xd, v


def _ddim_cpu(xc, v, noise_idx):
    """train_dit.py:110-125 on frame `cur` in float64 on the CPU."""
    ac = alphas_cumprod(1e-4).double()
    t_cur, t_next = G.timesteps(noise_idx)
    at, an = ac[t_cur], ac[t_next]
    xc, v = xc.double().cpu(), v.double().cpu()
    x0 = at.sqrt() * xc - (1 - at).sqrt() * v
    if noise_idx <= 0:
        return x0
    eps = ((1 / at).sqrt() * xc - x0) / (1 / at - 1).sqrt()
    return an.sqrt() * x0 + (1 - an).sqrt() * eps


@pytest.mark.parametrize("s", G.SCALES)
@pytest.mark.parametrize("noise_idx", G.NOISE_IDX)
def test_guided_fused_step_against_the_oracle(noise_idx, s):
    m = _model()
    x, a = G.inputs()
    xr, vr = G.oracle_step(noise_idx, s)
    bound = G.TOL_SMALL * G.amp(*G.oracle_branches(noise_idx), s)
    try:
        m.set_guidance(s)
        xd, v = _step(m, x, a.to(dev()), noise_idx)
    finally:
        m.set_guidance(None)
    e = rel_l2(v, vr, f"v_out s={s} (bound {bound:.2e})")
    assert e < bound
    assert rel_l2(xd[:, CUR], _ddim_cpu(x[:, CUR], v, noise_idx), "x[:, cur] vs the DDIM update of v_out") < 1e-5
    rel_l2(xd[:, CUR], xr, "x[:, cur] vs the oracle")          # (printed only: the bound is derived for v)
    assert torch.equal(xd[:, :CUR].cpu(), x[:, :CUR])          # context frames are untouched
    m.check()


@pytest.mark.parametrize("noise_idx", G.NOISE_IDX)
def test_guided_step_is_the_exact_composition_of_two_unguided_steps(noise_idx):
    """The guided step over 2 B internal samples runs the kernels of an unguided step at batch 2 B: same token count, same launch plans, same per-row arithmetic.
    So v_c / v_u are the bits of two unguided steps on [x; x] — with [a; a] and with no actions — and the guided v_out is their three-operation numpy combine."""
    m = _model()
    x, a = G.inputs()
    x2, a2 = torch.cat([x, x]), torch.cat([a, a]).to(dev())
    _, v_c2 = _step(m, x2, a2, noise_idx)
    _, v_u2 = _step(m, x2, a2, noise_idx, actions=False)
    v_c2, v_u2 = v_c2.cpu(), v_u2.cpu()
    assert torch.equal(v_c2[:G.B], v_c2[G.B:]) and torch.equal(v_u2[:G.B], v_u2[G.B:])     # a sample's bits do not depend on its batch position
    t_cur, t_next = G.timesteps(noise_idx)
    ac = alphas_cumprod(1e-4)
    for s in G.SCALES:
        try:
            m.set_guidance(s)
            xd, v = _step(m, x, a2[:G.B].contiguous(), noise_idx)
        finally:
            m.set_guidance(None)
        want = guided_combine(v_c2[:G.B].numpy(), v_u2[:G.B].numpy(), s)
        assert np.array_equal(v.cpu().numpy(), want), s
        if s == 1.0:
            assert torch.equal(v.cpu(), v_c2[:G.B])
        at = torch.full((G.B,), float(ac[t_cur]), device=dev())
        an = torch.full((G.B,), float(ac[t_next]), device=dev())
        xw = ddim_update(x[:, CUR].to(dev()).contiguous(), torch.from_numpy(want).to(dev()), at, an, noise_idx <= 0)
        assert torch.equal(xd[:, CUR], xw), s


@pytest.mark.parametrize("noise_idx", G.NOISE_IDX)
def test_guided_context_cached_step_reproduces_the_window_step(noise_idx):
    m = _model()
    x, a = G.inputs()
    ad = a.to(dev())
    try:
        m.set_guidance(3.0)
        xd, v = _step(m, x, ad, noise_idx)
        xc, _ = _step(m, x, ad, noise_idx)
        xc[:, CUR] = x[:, CUR].to(dev())                         # the K/V caches of 2 B samples are in place: restore the frame, then the cached step
        xc, vc = _step(m, x, ad, noise_idx, cached=True, xd=xc)
    finally:
        m.set_guidance(None)
    assert rel_l2(xc[:, CUR], xd[:, CUR], "cached vs window x") < 1e-5 and rel_l2(vc, v, "cached vs window v_out") < 1e-5
    assert torch.equal(xc[:, :CUR].cpu(), x[:, :CUR])


@pytest.mark.parametrize("cached", (False, True))
def test_guided_hoisted_conditioning_matches_the_inline_step(cached):
    """gtav_dit_prepare_frame builds the doubled table (conditional rows, then unconditional rows) once; a frame's steps then match the steps that compute their
    conditioning inline — the comparison of the unguided pair (tests/test_gpu_models.py: hoisting is the same arithmetic, rel-L2 < 1e-6)."""
    m = _model()
    x, a = G.inputs()
    ad = a.to(dev())
    order = G.NOISE_IDX
    outs = {}
    try:
        m.set_guidance(3.0)
        for hoist in (False, True):
            xd = x.to(dev()).contiguous()
            if hoist:
                m.prepare_frame_(G.B, G.FRAMES, G.START, CUR, G.T_CTX, [G.timesteps(k)[0] for k in order], ad)
            vs = []
            for step, noise_idx in enumerate(order):
                xd, v = _step(m, x, ad, noise_idx, cached=cached and step > 0, cond_step=step if hoist else -1, xd=xd)
                vs.append(v)
            outs[hoist] = (xd, vs)
    finally:
        m.set_guidance(None)
    assert rel_l2(outs[True][0], outs[False][0], "hoisted vs inline x") < 1e-6
    for k in range(len(order)):
        assert rel_l2(outs[True][1][k], outs[False][1][k], f"hoisted vs inline v_out step {k}") < 1e-6
    m.check()


def test_guidance_scale_is_not_baked_into_the_captured_graph():
    """One graph key, four scales: the first step of the key runs eagerly, the second is captured, the third and fourth replay the capture.  Each must be the
    bits of the same step without graphs: the scale is read from device memory."""
    m = _mk()                                                    # a fresh handle: this key has never been seen
    x, a = G.inputs()
    ad = a.to(dev())
    scales = (3.0, 0.0, 1.5, 3.0)
    xd = x.to(dev()).contiguous()
    v = torch.empty((G.B, *x.shape[2:]), device=dev())
    t_cur, t_next = G.timesteps(4)

    def run(s):
        xd.copy_(x)
        m.set_guidance(s)
        m.denoise_step_(xd, G.START, CUR, G.T_CTX, t_cur, t_next, False, ad, v_out=v)
        return xd.clone(), v.clone()

    m.set_guidance(3.0)
    m.reserve(G.B)                   # (builds the handle: set_graph needs one)
    m.set_graph(False)
    ref = [run(s) for s in scales]
    m.set_graph(True)
    got = [run(s) for s in scales]
    for k, s in enumerate(scales):
        assert torch.equal(got[k][0], ref[k][0]) and torch.equal(got[k][1], ref[k][1]), (k, s)
    assert torch.equal(ref[0][1], ref[3][1]) and not torch.equal(ref[0][1], ref[1][1]) and not torch.equal(ref[2][1], ref[1][1])
    m.check()


def test_guidance_off_again_is_a_handle_that_was_never_guided():
    x, a = G.inputs()
    ad = a.to(dev())
    m, fresh = _model(), _mk()
    m.set_guidance(3.0)
    _step(m, x, ad, 4)
    m.set_guidance(None)
    outs = []
    for mm in (m, fresh):
        inline = _step(mm, x, ad, 4)                                                    # conditioning inside the step
        mm.prepare_frame_(G.B, G.FRAMES, G.START, CUR, G.T_CTX, [G.timesteps(k)[0] for k in (4, 0)], ad)
        xd, v0 = _step(mm, x, ad, 4, cond_step=0)                                       # hoisted, full window
        xd = xd.clone()
        x1, v1 = _step(mm, x, ad, 0, cached=True, cond_step=1, xd=xd.clone())           # hoisted, context-cached
        outs.append((*inline, xd, v0, x1, v1))
    for k, (got, want) in enumerate(zip(*outs)):
        assert torch.equal(got, want), k


def test_guidance_refusals_by_name():
    m = _model()
    x, a = G.inputs()
    ad = a.to(dev())
    lib = L.load()
    try:
        m.set_guidance(3.0)
        with pytest.raises(L.GtavError, match="guidance is on and actions == NULL"):
            _step(m, x, ad, 4, actions=False)
        with pytest.raises(L.GtavError, match="guidance is on and actions == NULL"):
            m.prepare_frame_(G.B, G.FRAMES, G.START, CUR, G.T_CTX, [399, 0], None)
        # 2 B > max_batch: the Python layer names the max_batch the model needs, the C entry points refuse on their own
        x4 = torch.cat([x, x]).to(dev()).contiguous()
        a4 = torch.cat([ad, ad]).contiguous()
        with pytest.raises(ValueError, match="max_batch=8"):
            m.denoise_step_(x4, G.START, CUR, G.T_CTX, 399, 299, False, a4)
        assert lib.gtav_dit_denoise_step(m._handle, x4.data_ptr(), 4, G.FRAMES, G.START, CUR, G.T_CTX, 399, 299, 0, a4.data_ptr(), 0, -1, None, L.current_stream()) != 0
        assert b"2 B = 8 internal samples, max_batch is 4" in lib.gtav_last_error()
        arr = (ctypes.c_int32 * 2)(399, 0)
        assert lib.gtav_dit_prepare_frame(m._handle, 4, G.FRAMES, G.START, CUR, G.T_CTX, arr, 2, a4.data_ptr(), L.current_stream()) != 0
        assert b"2 B = 8 internal samples, max_batch is 4" in lib.gtav_last_error()
        assert lib.gtav_dit_set_guidance(m._handle, 1, float("nan")) != 0 and b"not finite" in lib.gtav_last_error()
        # the doubled conditioning table beyond max_cond_rows (a fresh handle: 4 x 5 = 20 rows): 2 B (T - 1 + n) = 4 (4 + 2) = 24
        m1 = _mk()
        m1.set_guidance(3.0)
        m1.reserve(G.B)
        assert lib.gtav_dit_prepare_frame(m1._handle, G.B, G.FRAMES, G.START, CUR, G.T_CTX, arr, 2, ad.data_ptr(), L.current_stream()) != 0
        assert b"exceed max_cond_rows" in lib.gtav_last_error() and b"guidance doubles the table" in lib.gtav_last_error()
        m.set_guidance(None)
        # switching guidance on or off invalidates the context cache and the prepared table
        for first, then in ((None, 3.0), (3.0, None)):
            m.set_guidance(first)
            xd, _ = _step(m, x, ad, 4)
            m.set_guidance(then)
            with pytest.raises(L.GtavError, match="without a preceding full-window step"):
                _step(m, x, ad, 4, cached=True, xd=xd)
            m.set_guidance(first)
            m.prepare_frame_(G.B, G.FRAMES, G.START, CUR, G.T_CTX, [399, 0], ad)
            m.set_guidance(then)
            with pytest.raises(L.GtavError, match="gtav_dit_prepare_frame was not called"):
                _step(m, x, ad, 4, cond_step=0)
            # changing only the scale invalidates neither
            m.set_guidance(first)
            m.prepare_frame_(G.B, G.FRAMES, G.START, CUR, G.T_CTX, [399, 0], ad)
            xd, _ = _step(m, x, ad, 4, cond_step=0)
            if first is not None:
                m.set_guidance(1.5)
            _step(m, x, ad, 0, cached=True, cond_step=1, xd=xd)
    finally:
        m.set_guidance(None)
    # a model without external_cond
    kw = dict(G.SMALL_DIT, external_cond_dim=0)
    m0 = _mk(2, kw, W.synth_state_dict(W.dit_param_shapes(**kw), seed=G.SEED))
    with pytest.raises(ValueError, match="no external_cond"):
        m0.set_guidance(3.0)
    m0._ensure(2, 5)
    assert lib.gtav_dit_set_guidance(m0._handle, 1, 3.0) != 0 and b"model has no external_cond" in lib.gtav_last_error()


def test_guided_rollout_with_a_sliding_window():
    """generate_latents(guidance_scale=3): 7 frames from 1 prompt frame, windows 2 .. 5 then sliding, 4 noise steps (30 guided steps), window-recompute and
    context-cached, against the oracle loop under the guided dit_fn.  The bound is TOL_ROLLOUT times the largest amp(3) the oracle met on a denoised frame."""
    from gtav_amd.generate import generate_latents
    m = _model()
    sd, cfg = G.state_dict(), G.config()
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(G.B, 1, 16, 8, 16, generator=g) * 0.5
    noise = torch.randn(G.B, 6, 16, 8, 16, generator=g)
    a = torch.zeros(G.B, 7, 25)
    a[:, :, 3] = 1
    amps = []
    with torch.no_grad():
        ref = O.generate_latents(G.guided_fn(sd, cfg, 3.0, amps), x0, 7, 4, noise, a, max_frames=5)
    bound = G.TOL_ROLLOUT * max(amps)
    assert m.max_frames == 5
    out = generate_latents(m, x0, 7, 4, noise, a, guidance_scale=3.0)
    out_c = generate_latents(m, x0, 7, 4, noise, a, ctx_cache=True, guidance_scale=3.0)
    assert m._guidance is None                                  # the model's own setting is back
    e, ec = rel_l2(out, ref, "window"), rel_l2(out_c, ref, "cached")
    print(f"[guidance rollout] largest amp(3) {max(amps):.3f} -> bound {bound:.3e}; window {e:.3e} ({e / bound:.2f} of it), cached {ec:.3e} ({ec / bound:.2f} of it), "
          f"cached vs window {rel_l2(out_c, out, 'cached vs window'):.3e}")
    assert e < bound and ec < bound
    unguided = generate_latents(m, x0, 7, 4, noise, a)
    assert rel_l2(unguided, ref, "unguided vs guided oracle") > 10 * bound      # and the bound tells a guided rollout from an unguided one
    m.check()
