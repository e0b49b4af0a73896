"""Temporal windows of 9 .. 32 frames (GPU): the streaming temporal attention kernel (csrc/attention.hip attn_temporal_stream_kernel) at the op level,
and DiT(max_frames <= 32) through forward, sampler step (window and context-cached; eager, captured, replayed), generate_latents and bf16 operands,
against the CPU oracle and against fixtures recorded from the reference with max_frames up to 32 (tests/golden/g12_long_window.safetensors,
g13_long_window_steps.safetensors; tools/make_golden.py g12_long_window).

Every bound is one the project already uses for the same kind of comparison on five-frame windows (tests/test_gpu_ops.py, test_gpu_models.py,
test_gpu_range.py); `pytest -s` prints every measured margin."""
import os

import pytest
import torch
from safetensors.torch import load_file

pytestmark = pytest.mark.gpu

from helpers import dev, stream, untile  # noqa: E402
from helpers import rel_l2_logged as rel_l2  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402
import gtav_amd.weights as W  # noqa: E402
from gtav_amd import lib as L  # noqa: E402
from gtav_amd.model.dit import DiT, DiT_models  # noqa: E402

TOL_FULL = 1e-3        # tests/test_gpu_models.py
TOL_SMALL = 2e-3       # tests/test_gpu_models.py
TOL_ROLLOUT = 1.5e-3   # tests/test_gpu_models.py
TOL_BF16 = 1.5e-2      # tests/test_gpu_range.py
TOL_ATTN_OP = 6e-4     # tests/test_gpu_ops.py test_attention_temporal

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL_DIT = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)
SEED = 21              # tools/make_golden.py g12_long_window


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _mk_dit(seed=SEED, **kw):
    sd = W.synth_state_dict(W.dit_param_shapes(**SMALL_DIT), seed=seed)
    m = DiT(**SMALL_DIT, init_weights=False, **kw)
    m.load_state_dict(sd)
    return m, sd, O.DiTConfig(**SMALL_DIT)


def _inputs(cfg, B, T, seed, actions=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, cfg.in_channels, cfg.input_h, cfg.input_w, generator=g)
    t = torch.randint(0, 1000, (B, T), generator=g)
    a = None
    if actions:
        a = torch.zeros(B, T, 25)
        a[torch.arange(B)[:, None], torch.arange(T)[None], torch.randint(0, 25, (B, T), generator=g)] = 1
    return x, t, a


# ------------------------------------------------------------------------------------------------------------------------
# 1, 2: the kernel through the C-ABI
# ------------------------------------------------------------------------------------------------------------------------
def _attn_temporal_op(q, kv, Tq, t0, Tmax):
    """q (B, Tq, P, D) fp16, kv (B, Tmax, P, 2, D) fp16 (CPU) -> the launch's tile-major output buffer (device) and its row-major (B Tq P, D) view (CPU)."""
    B, _, P, D = q.shape
    rows = B * Tq * P
    o = torch.zeros((rows + 127) // 128 * 128, D, device=dev(), dtype=torch.float16)
    qd, kvd = q.contiguous().to(dev()), kv.contiguous().to(dev())
    L.check(L.load().gtav_op_attn_temporal(qd.data_ptr(), kvd.data_ptr(), o.data_ptr(), B, P, D, Tq, t0, Tmax, stream()))
    torch.cuda.synchronize()
    return o, untile(o, rows, D)


def _attn_temporal_ref(q, kv, Tq, t0):
    B, _, P, D = q.shape
    Tk, h = t0 + Tq, D // 64
    qf = q.float().reshape(B, Tq, P, h, 64).permute(0, 2, 3, 1, 4)             # B P h Tq d
    kf = kv[:, :Tk, :, 0].float().reshape(B, Tk, P, h, 64).permute(0, 2, 3, 1, 4)
    vf = kv[:, :Tk, :, 1].float().reshape(B, Tk, P, h, 64).permute(0, 2, 3, 1, 4)
    s = qf @ kf.transpose(-1, -2) / 8.0
    mask = torch.arange(Tk)[None, :] > (t0 + torch.arange(Tq))[:, None]
    s = s.masked_fill(mask, float("-inf"))
    return (s.softmax(-1) @ vf).permute(0, 3, 1, 2, 4).reshape(B * Tq * P, D)


def _poison_hidden_frames(kv, Tk):
    """Cache frames no query of the launch may see hold NaN bit patterns (an uninitialised or stale cache): they must never be read."""
    kv = kv.clone()
    kv[:, Tk:] = float("nan")
    return kv


ATTN_CASES = [(32, 0, 32), (1, 31, 32), (12, 0, 12), (9, 0, 9), (3, 13, 16), (1, 8, 32)]


@pytest.mark.parametrize("Tq,t0,Tmax", ATTN_CASES)
def test_attention_temporal_long_window_op(Tq, t0, Tmax):
    B, P, D = 2, 24, 256
    q = _rand(B, Tq, P, D, seed=1).half()
    kv = _poison_hidden_frames(_rand(B, Tmax, P, 2, D, seed=2).half(), t0 + Tq)
    _, got = _attn_temporal_op(q, kv, Tq, t0, Tmax)
    assert torch.isfinite(got.float()).all()
    assert rel_l2(got.float(), _attn_temporal_ref(q, kv, Tq, t0)) < TOL_ATTN_OP


@pytest.mark.parametrize("Tq,t0,Tmax", [(32, 0, 32), (1, 31, 32), (3, 13, 16)])
def test_attention_temporal_long_window_op_production_width(Tq, t0, Tmax):
    B, P, D = 3, 144, 1024
    q = _rand(B, Tq, P, D, seed=3).half()
    kv = _poison_hidden_frames(_rand(B, Tmax, P, 2, D, seed=4).half(), t0 + Tq)
    _, got = _attn_temporal_op(q, kv, Tq, t0, Tmax)
    assert torch.isfinite(got.float()).all()
    assert rel_l2(got.float(), _attn_temporal_ref(q, kv, Tq, t0)) < TOL_ATTN_OP


def test_attention_temporal_long_window_is_repeatable_and_launch_independent():
    """The same launch twice gives the same bits; frame t of the window launch (Tq = 32, t0 = 0) and the context-cached launch (Tq = 1, t0 = t) fed that
    frame's queries give the same bits — the cached sampler step rests on it."""
    for (B, P, D) in ((2, 24, 256), (1, 144, 1024)):
        q = _rand(B, 32, P, D, seed=5).half()
        kv = _rand(B, 32, P, 2, D, seed=6).half()
        o1, w1 = _attn_temporal_op(q, kv, 32, 0, 32)
        o2, w2 = _attn_temporal_op(q, kv, 32, 0, 32)
        assert torch.equal(o1, o2)
        w = w1.reshape(B, 32, P, D)
        for t in (8, 15, 31):
            c1, one = _attn_temporal_op(q[:, t:t + 1], _poison_hidden_frames(kv, t + 1), 1, t, 32)
            c2, _ = _attn_temporal_op(q[:, t:t + 1], _poison_hidden_frames(kv, t + 1), 1, t, 32)
            assert torch.equal(c1, c2)
            assert torch.equal(one.reshape(B, 1, P, D)[:, 0], w[:, t]), (B, P, D, t)


def test_attention_temporal_window_above_32_is_refused():
    q = _rand(1, 1, 8, 256, seed=1).half().to(dev())
    kv = _rand(1, 33, 8, 2, 256, seed=2).half().to(dev())
    o = torch.zeros(128, 256, device=dev(), dtype=torch.float16)
    rc = L.load().gtav_op_attn_temporal(q.data_ptr(), kv.data_ptr(), o.data_ptr(), 1, 8, 256, 1, 32, 33, stream())
    assert rc != 0 and b"max 32" in L.load().gtav_last_error()


# ------------------------------------------------------------------------------------------------------------------------
# 3: the dispatch rule — windows of <= 8 frames do not see the handle's capacity
# ------------------------------------------------------------------------------------------------------------------------
def test_short_windows_are_bit_identical_on_a_32_frame_handle():
    from gtav_amd.utils import alphas_cumprod
    m32, _, cfg = _mk_dit(max_frames=32, max_batch=2)
    m5, _, _ = _mk_dit(max_frames=5, max_batch=2)
    x, t, a = _inputs(cfg, 2, 5, seed=12)
    m32.reserve(2, 32)
    assert torch.equal(m32(x, t, a), m5(x, t, a))
    ac = alphas_cumprod(1e-4)
    ad = a.to(dev())
    outs = []
    for m in (m32, m5):
        m.set_schedule(ac)
        xd = x.to(dev()).contiguous()
        got = []
        for k in range(3):                                        # eager, captured, replayed
            xd[:, -1] = x[:, -1].to(dev())
            m.denoise_step_(xd, 0, 4, 15, 500, 400, False, ad)
            got.append(xd[:, -1].clone())
        xd[:, -1] = x[:, -1].to(dev())
        m.denoise_step_(xd, 0, 4, 15, 500, 400, False, ad, cached=True)
        got.append(xd[:, -1].clone())
        m.check()
        outs.append(got)
    for g32, g5 in zip(*outs):
        assert torch.equal(g32, g5)
    assert torch.equal(outs[0][0], outs[0][1]) and torch.equal(outs[0][1], outs[0][2])


# ------------------------------------------------------------------------------------------------------------------------
# 4: the small model against the oracle and the reference's fixture
# ------------------------------------------------------------------------------------------------------------------------
def test_small_dit_long_window_forwards():
    g = load_file(os.path.join(GOLD, "g12_long_window.safetensors"))
    m, sd, cfg = _mk_dit(max_frames=32, max_batch=2)
    for tag, a in (("b1t32", g["a_b1t32"]), ("b2t12", None)):
        x, t = g["x_" + tag], g["t_" + tag]
        with torch.no_grad():
            ref = O.dit_forward(sd, cfg, x, t, a)
        out = m(x, t, a)
        assert rel_l2(out, ref) < TOL_SMALL and rel_l2(out, g["out_" + tag]) < TOL_SMALL
    x, t, a = _inputs(cfg, 2, 9, seed=13)
    with torch.no_grad():
        ref = O.dit_forward(sd, cfg, x, t, a)
    assert rel_l2(m(x, t, a), ref) < TOL_SMALL
    m.check()
    # the largest conditioning batch a 32-frame handle meets at batch 8: 256 rows of (timestep, action) through the fp32 conditioning GEMMs
    x, t, a = _inputs(cfg, 8, 32, seed=20)
    with torch.no_grad():
        ref = O.dit_forward(sd, cfg, x, t, a)
    assert rel_l2(m(x, t, a), ref) < TOL_SMALL
    m.check()


def test_small_dit_long_window_denoise_step_mirror_fused_and_cached():
    from gtav_amd.sampler import denoise_step
    from gtav_amd.utils import alphas_cumprod
    g = load_file(os.path.join(GOLD, "g13_long_window_steps.safetensors"))
    m, sd, cfg = _mk_dit(max_frames=16, max_batch=1)
    x, a = g["x"], g["actions"]
    n, start = x.shape[1], 4
    ac = alphas_cumprod(1e-4)
    nr = torch.linspace(0, 999, 11)
    dit_fn = lambda xx, tt, aa: O.dit_forward(sd, cfg, xx, tt, aa)
    ad = a.to(dev())
    for noise_idx in (4, 0):
        with torch.no_grad():
            xr, vr = O.denoise_step(dit_fn, x, a, noise_idx, 15, nr, ac[:, None, None, None], start_frame=start)
        xp, vp = denoise_step(m, x, a, noise_idx, 15, nr, ac[:, None, None, None], start_frame=start)
        assert rel_l2(vp, vr) < TOL_SMALL and rel_l2(xp, xr) < TOL_SMALL
        assert rel_l2(vp, g[f"v_pred_{noise_idx}"]) < TOL_SMALL and rel_l2(xp[:, -1:], g[f"x_pred_last_{noise_idx}"]) < TOL_SMALL
        m.set_schedule(ac)
        t_cur, t_next = int(nr[noise_idx]), int(nr[max(0, noise_idx - 1)])
        xd = x.to(dev()).contiguous()
        steps = []
        for k in range(3):                                        # eager, captured, replayed
            xd[:, -1] = x[:, -1].to(dev())
            m.denoise_step_(xd, start, n - 1, 15, t_cur, t_next, noise_idx <= 0, ad)
            steps.append(xd[:, -1].clone())
            assert rel_l2(xd[:, -1], xr[:, -1]) < TOL_SMALL
            assert rel_l2(xd[:, -1:], g[f"x_pred_last_{noise_idx}"]) < TOL_SMALL
        assert torch.equal(steps[0], steps[1]) and torch.equal(steps[1], steps[2])
        assert torch.equal(xd[:, :-1].cpu(), x[:, :-1])
        # the context-cached step on the K/V caches that window step left (t0 = 15: the streaming kernel's one-query form)
        xd[:, -1] = x[:, -1].to(dev())
        m.denoise_step_(xd, start, n - 1, 15, t_cur, t_next, noise_idx <= 0, ad, cached=True)
        assert rel_l2(xd[:, -1], steps[0]) < 1e-5                 # tests/test_gpu_models.py test_denoise_step_mirror_and_fused_and_cached
    m.check()


# ------------------------------------------------------------------------------------------------------------------------
# 5: rollout with a nine-frame window
# ------------------------------------------------------------------------------------------------------------------------
def test_small_rollout_with_a_9_frame_window():
    """The fixture's rollout: 1 prompt frame -> 11 frames, 3 noise steps, max_frames = 9 (40 chained forwards; windows of 2 .. 8 frames run the
    register-resident kernels, the 9-frame windows and the two slides the streaming kernel)."""
    from gtav_amd.generate import generate_latents
    g = load_file(os.path.join(GOLD, "g13_long_window_steps.safetensors"))
    m, sd, cfg = _mk_dit(max_frames=9, max_batch=2)
    x0, noise, a, ref = g["roll_x_prompt"], g["roll_noise"], g["roll_actions"], g["roll_latents"]
    out = generate_latents(m, x0, 11, 3, noise, a)
    out_c = generate_latents(m, x0, 11, 3, noise, a, ctx_cache=True)
    out_i = generate_latents(m, x0, 11, 3, noise, a, hoist_cond=False)
    out_ci = generate_latents(m, x0, 11, 3, noise, a, ctx_cache=True, hoist_cond=False)
    e, ec, eci = rel_l2(out, ref), rel_l2(out_c, ref), rel_l2(out_ci, ref)
    assert e < TOL_ROLLOUT and ec < TOL_ROLLOUT and eci < TOL_ROLLOUT
    assert rel_l2(out_c, out) < 1e-4          # tests/test_gpu_models.py test_small_rollout_config1_shape
    assert rel_l2(out_i, out) < 1e-6
    assert rel_l2(out_ci, out_c) < 1e-6
    m.check()


# ------------------------------------------------------------------------------------------------------------------------
# 6: full size
# ------------------------------------------------------------------------------------------------------------------------
def test_full_dit_long_window_forward_and_steps():
    """DiT-S/2 with a 32-frame handle: the forward at B = 1, T = 32 (M = 4 608 tokens) against the oracle; a window step and a context-cached step of a
    16-frame window at B = 2 (M = 4 608 / 288); the forward at B = 8, T = 32 (M = 36 864)."""
    from gtav_amd.utils import alphas_cumprod
    m = DiT_models["DiT-S/2"](init_weights=False, max_batch=2)
    m.max_frames = 32
    sd = W.synth_state_dict(W.dit_param_shapes(depth=16), seed=0)
    m.load_state_dict(sd)
    cfg = O.dit_s_2()
    x32, t32, a32 = _inputs(cfg, 1, 32, seed=51)
    t32[:, :31] = 15
    with torch.no_grad():
        ref32 = O.dit_forward(sd, cfg, x32, t32, a32)
    assert rel_l2(m(x32, t32, a32), ref32) < TOL_FULL
    m.check()
    # The step is the one tests/test_gpu_models.py test_full_dit_batch8_production_shapes takes (unit-variance latents, one step of generate.py's default 100:
    # t 499 -> 489), because its cached-vs-window bound is reused below: the compared quantity is the updated frame, in which the difference of the two
    # v predictions enters with a weight that grows with the step length (measured with a 100-timestep step on half-variance latents: 2.0-2.3e-4 at every
    # window length from 5 to 32 frames, five-frame windows on an 8-frame handle included — a property of the comparison, not of the window length).
    x, _, a = _inputs(cfg, 2, 16, seed=52)
    ac = alphas_cumprod(1e-4)
    nr = torch.linspace(0, 999, 101)
    dit_fn = lambda xx, tt, aa: O.dit_forward(sd, cfg, xx, tt, aa)
    with torch.no_grad():
        xr, _ = O.denoise_step(dit_fn, x, a, 50, 15, nr, ac[:, None, None, None], start_frame=0)
    m.set_schedule(ac)
    ad = a.to(dev())
    xd = x.to(dev()).contiguous()
    t_cur, t_next = int(nr[50]), int(nr[49])
    m.denoise_step_(xd, 0, 15, 15, t_cur, t_next, False, ad)
    win = xd[:, -1].clone()
    assert rel_l2(win, xr[:, -1]) < TOL_FULL
    xd[:, -1] = x[:, -1].to(dev())
    m.denoise_step_(xd, 0, 15, 15, t_cur, t_next, False, ad, cached=True)
    assert rel_l2(xd[:, -1], win) < 1e-4      # tests/test_gpu_models.py test_full_dit_batch8_production_shapes
    m.check()
    # the largest shape of a 32-frame handle at batch 8: M = 36 864 tokens, 256 conditioning rows, 2.4 GB of K/V caches.  Samples never interact, so sample 0
    # of the batch, given the inputs of the B = 1 forward above, is held to that forward's oracle (the whole batch through the CPU oracle would take minutes).
    m.reserve(8, 32)
    x8, t8, a8 = _inputs(cfg, 8, 32, seed=53)
    x8[0], t8[0], a8[0] = x32[0], t32[0], a32[0]
    out8 = m(x8, t8, a8)
    assert torch.isfinite(out8).all()
    assert rel_l2(out8[:1], ref32) < TOL_FULL
    m.check()


# ------------------------------------------------------------------------------------------------------------------------
# 7: bf16 operands
# ------------------------------------------------------------------------------------------------------------------------
def test_bf16_operands_small_dit_32_frames():
    g = load_file(os.path.join(GOLD, "g12_long_window.safetensors"))
    m, sd, cfg = _mk_dit(max_frames=32, max_batch=1)
    x, t, a = g["x_b1t32"], g["t_b1t32"], g["a_b1t32"]
    fp16 = m(x, t, a).clone()
    m.set_operand_dtype(torch.bfloat16)
    out = m(x, t, a)
    e = rel_l2(out, g["out_b1t32"])
    assert 5e-4 < e < TOL_BF16                 # tests/test_gpu_range.py: bf16 precision, and not better than fp16's — the mode really ran
    assert torch.equal(out, m(x, t, a))
    m.set_operand_dtype(torch.float16)
    assert torch.equal(m(x, t, a), fp16)
    m.check()


# ------------------------------------------------------------------------------------------------------------------------
# 8: limits
# ------------------------------------------------------------------------------------------------------------------------
def test_window_limits_leave_the_model_usable():
    m, sd, cfg = _mk_dit(max_frames=5, max_batch=1)
    x, t, a = _inputs(cfg, 1, 5, seed=14)
    first = m(x, t, a).clone()
    with pytest.raises((ValueError, L.GtavError), match="32"):
        DiT(**SMALL_DIT, init_weights=False, max_frames=33)
    with pytest.raises((ValueError, L.GtavError), match="32"):
        m.max_frames = 33
        xx, tt, aa = _inputs(cfg, 1, 33, seed=15)
        m(xx, tt, aa)
    with pytest.raises((ValueError, L.GtavError), match="32"):
        xx, tt, aa = _inputs(cfg, 1, 33, seed=15)
        m(xx, tt, aa)
    assert torch.equal(m(x, t, a), first)
    m.max_frames = 32
    x32, t32, a32 = _inputs(cfg, 1, 32, seed=16)
    with torch.no_grad():
        ref = O.dit_forward(sd, cfg, x32, t32, a32)
    assert rel_l2(m(x32, t32, a32), ref) < TOL_SMALL
    assert torch.equal(m(x, t, a), first)


def test_trainable_model_refuses_windows_above_8_and_still_trains():
    sd = W.synth_state_dict(W.dit_param_shapes(**SMALL_DIT), seed=1)
    m = DiT(**SMALL_DIT, init_weights=False, max_batch=2, max_frames=12, trainable=True)
    m.load_state_dict(sd)
    cfg = O.DiTConfig(**SMALL_DIT)
    x12, t12, a12 = _inputs(cfg, 2, 12, seed=17)
    with pytest.raises((ValueError, L.GtavError), match="8 frames"):
        m.forward_train(x12, t12, a12)
    x, t, a = _inputs(cfg, 2, 5, seed=18)
    vt = _rand(2, 1, 16, 8, 16, seed=19)
    with torch.no_grad():
        ref = O.dit_forward(sd, cfg, x, t, a)
    v = m.forward_train(x, t, a)
    assert rel_l2(v, ref) < TOL_SMALL
    m.zero_grad()
    m.backward_(v, vt)
    m.adamw_step(1e-3, weight_decay=0.01, max_grad_norm=1.0)
    m.check()
    assert m.train_stats()[0]                                   # the step was applied
    with pytest.raises((ValueError, L.GtavError), match="8 frames"):   # still refused after training was enabled, and still usable after the refusal
        m.forward_train(x12, t12, a12)
    assert torch.isfinite(m.forward_train(x, t, a)).all()
    # the library itself refuses to enable training on a handle sized for more than 8 frames, before it allocates anything
    import ctypes as C
    lib = L.load()
    h = C.c_void_p()
    c = L.DitConfig(max_frames=12, max_batch=1, max_cond_rows=12, mlp_ratio=4.0, **SMALL_DIT)
    L.check(lib.gtav_dit_create(C.byref(c), C.byref(h)))
    try:
        assert lib.gtav_dit_train_enable(h, None, 0) != 0
        assert b"at most 8 frames" in lib.gtav_last_error()
    finally:
        lib.gtav_dit_destroy(h)
