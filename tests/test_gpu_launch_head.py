"""The launch head of the batch-1 step (docs/LABNOTES.md 13.2): the cache policy of the loader-wave kernels' weight fills (GemmParams::wfill,
gtav_dit_set_weight_fill_policy) moves the same bytes in the same order, so every result is EQUAL BIT FOR BIT under every setting — at the kernel level (every
loader-wave block shape, every epilogue of the step, both operand types, the two fused to_qkv + attention launches), at the model level (forward, captured
sampler steps, a context-cached step, with the next-weight prefetch on and off) and through the tuner, which may keep non-temporal fills for a class.

Sizes of the kernel-level cases: M = 160 tokens (one full and one ragged row tile of every shape: 96-, 48- and 144-row tiles), N = 192 features (two 96-column
tiles; one full 128-row weight tile and half of a second), K = 192 (three K-steps: the four-stage ring takes them all in its prologue) and K = 512 in two K
slices for the split-K slabs (four K-steps per slice: the ring wraps once).  The QKV epilogues need N = 3 D with D a multiple of 128: D = 128, N = 384 is the
smallest the launcher takes."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import dev, stream, tiled_index, to_tiled, to_tiled_f16  # noqa: E402
from gtav_amd import lib as L  # noqa: E402
import gtav_amd.weights as W  # noqa: E402
from gtav_amd.model.dit import DiT, DiT_models  # noqa: E402

NT = 0x100                        # include/gtav_amd_testing.h GTAV_GEMM_WM_NT_WEIGHT_FILLS
SHAPES = (20, 24, 26, 29)         # the loader-wave block shapes (csrc/gemm.hip launch_epi)
M, N = 160, 192


def _rand(*shape, scale=1.0, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.fixture(scope="module")
def operands():
    """Tile-major operands, built once: K = 192 and K = 512, fp16 and bf16; the QKV operands (D = 128); RoPE tables."""
    lib = L.load()
    o = {}
    for K in (192, 512):
        x, w = _rand(M, K, seed=K).half(), _rand(N, K, scale=1 / math.sqrt(K), seed=K + 1)
        o[K] = (to_tiled_f16(x), to_tiled_f16(w))
        o[K, "bf16"] = (to_tiled(x, torch.bfloat16), to_tiled(w, torch.bfloat16))
    o["bias"] = _rand(N, seed=5).to(dev())
    D = 128
    o["qkv"] = (to_tiled_f16(_rand(M, D, seed=7).half()), to_tiled_f16(_rand(3 * D, D, scale=1 / math.sqrt(D), seed=8)), _rand(3 * D, seed=9).to(dev()))
    ang = (_rand(32, 32, seed=3) * 3).repeat_interleave(2, dim=-1)
    cd, sd = ang.cos().to(dev()).contiguous(), ang.sin().to(dev()).contiguous()
    cs = torch.empty_like(cd)
    L.check(lib.gtav_op_rope_interleave(cd.data_ptr(), sd.data_ptr(), cs.data_ptr(), 32, stream()))
    o["cs"] = cs
    torch.cuda.synchronize()
    return o


def _both_policies(run, wm):
    """run() -> tensors; once with the default fills and once with non-temporal weight fills under block shape `wm`: equal bits."""
    lib = L.load()
    outs = []
    try:
        for fill in (0, NT):
            lib.gtav_op_gemm_set_wm(wm | fill)
            outs.append([t.clone() for t in run()])
            torch.cuda.synchronize()
    finally:
        lib.gtav_op_gemm_set_wm(0)
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b)), f"shape {wm}: non-temporal weight fills changed the result"
    return outs[0]


def _gemm(xd, wd, bias, out, ldo, K, epi, gate_stride=0):
    L.check(L.load().gtav_op_gemm_f16(xd.data_ptr(), K, wd.data_ptr(), L.ptr(bias), out.data_ptr(), ldo, M, N, K, epi, 0, gate_stride, 1, stream()))


@pytest.mark.parametrize("wm", SHAPES)
def test_gemm_epilogues_are_bit_equal_under_nt_weight_fills(operands, wm):
    """fp32, GELU-tanh (f16 tile-major) and the split-K slabs (two K slices of K = 512) on every loader-wave shape."""
    xd, wd = operands[192]
    xd5, wd5 = operands[512]
    bias = operands["bias"]

    def run():
        f32 = torch.full((M, N), 7.0, device=dev())
        gelu = torch.full((256, N), 7.0, device=dev(), dtype=torch.float16)
        slabs = torch.full((2, M, N), 7.0, device=dev())
        _gemm(xd, wd, bias, f32, N, 192, 0)
        _gemm(xd, wd, bias, gelu, N, 192, 2)
        _gemm(xd5, wd5, None, slabs, N, 512, 6, gate_stride=2)
        return f32, gelu, slabs

    f32, gelu, slabs = _both_policies(run, wm)
    assert torch.isfinite(f32).all() and torch.isfinite(slabs).all() and not (f32 == 7.0).all()


@pytest.mark.parametrize("wm", SHAPES)
def test_qkv_epilogues_are_bit_equal_under_nt_weight_fills(operands, wm):
    """The spatial (S = 32) and the temporal (P = 32, 5 frames) QKV epilogue, D = 128."""
    xd, wd, bias = operands["qkv"]
    cs = operands["cs"]
    D, S, Tq = 128, 32, 5
    lib = L.load()

    def run():
        q, k, vt = (torch.full((M // S, D // 64, S, 64), 7.0, device=dev(), dtype=torch.float16) for _ in range(3))
        L.check(lib.gtav_op_gemm_qkv(xd.data_ptr(), D, wd.data_ptr(), bias.data_ptr(), M, D, 0, q.data_ptr(), k.data_ptr(), vt.data_ptr(), S, 0, 0, 0,
                                     cs.data_ptr(), stream()))
        qt = torch.full((M, D), 7.0, device=dev(), dtype=torch.float16)
        kv = torch.full((1, Tq, S, 2, D), 7.0, device=dev(), dtype=torch.float16)
        L.check(lib.gtav_op_gemm_qkv(xd.data_ptr(), D, wd.data_ptr(), 0, M, D, 1, qt.data_ptr(), kv.data_ptr(), kv.data_ptr(), S, Tq, 0, Tq, cs.data_ptr(),
                                     stream()))
        return q, k, vt, qt, kv

    outs = _both_policies(run, wm)
    assert all(torch.isfinite(t.float()).all() for t in outs)


def test_bf16_twin_is_bit_equal_under_nt_weight_fills(operands):
    """The bf16 twins carry the same loader: GELU-tanh on shape 20 with bf16 operands."""
    lib = L.load()
    xd, wd = operands[192, "bf16"]
    lib.gtav_op_set_operand_dtype(1)
    try:
        def run():
            out = torch.full((256, N), 7.0, device=dev(), dtype=torch.bfloat16)
            _gemm(xd, wd, operands["bias"], out, N, 192, 2)
            return (out,)
        _both_policies(run, 20)
    finally:
        lib.gtav_op_set_operand_dtype(0)


@pytest.mark.parametrize("wm", (20, 29))
def test_nt_weight_fills_read_the_rows_the_default_fills_read(operands, wm):
    """NaN bit patterns in the weight rows beyond N (rows 192 .. 255 of the second 128-row tile): the loaders of both policies fetch whole tiles, the epilogue
    drops the columns past N — equal bits and no NaN in any of the N columns."""
    xd, wd = operands[192]
    flat = wd.clone().reshape(-1)
    flat[tiled_index(256, 192)[N:].reshape(-1).to(dev())] = float("nan")     # rows N .. 255 of the tile-major image, every K tile
    wn = flat.reshape(wd.shape)

    def run():
        out = torch.full((M, N), 7.0, device=dev())
        _gemm(xd, wn, operands["bias"], out, N, 192, 0)
        return (out,)

    (out,) = _both_policies(run, wm)
    ref = torch.full((M, N), 7.0, device=dev())
    try:
        L.load().gtav_op_gemm_set_wm(wm)
        _gemm(xd, wd, operands["bias"], ref, N, 192, 0)       # the same shape on the clean weight
    finally:
        L.load().gtav_op_gemm_set_wm(0)
    assert torch.isfinite(out).all() and torch.equal(out, ref)


def test_fused_qkv_attention_launches_are_bit_equal_under_nt_weight_fills():
    """The two fused to_qkv + attention launches share the loader: one frame of 144 tokens (spatial) and 2 x 5 frames of 32 positions (temporal), D = 256."""
    lib = L.load()
    D = 256
    w16 = to_tiled_f16(_rand(3 * D, D, scale=1 / math.sqrt(D), seed=2))
    ang = (_rand(144, 32, seed=3) * 3).repeat_interleave(2, dim=-1)
    cd, sd = ang.cos().to(dev()).contiguous(), ang.sin().to(dev()).contiguous()
    cs = torch.empty_like(cd)
    L.check(lib.gtav_op_rope_interleave(cd.data_ptr(), sd.data_ptr(), cs.data_ptr(), 144, stream()))
    w_s, w_t = torch.empty_like(w16), torch.empty_like(w16)
    L.check(lib.gtav_op_qkv_head_major_spatial(w16.data_ptr(), w_s.data_ptr(), D, stream()))
    L.check(lib.gtav_op_qkv_head_major(w16.data_ptr(), w_t.data_ptr(), D, stream()))
    xs = to_tiled_f16(_rand(144, D, seed=1).half())
    B, P, Tq = 2, 32, 5
    xt = to_tiled_f16(_rand(B * Tq * P, D, seed=4).half())

    def run():
        o_s = torch.full((256, D), 7.0, device=dev(), dtype=torch.float16)
        L.check(lib.gtav_op_gemm_qkvs_attn(xs.data_ptr(), w_s.data_ptr(), 144, D, 144, cs.data_ptr(), o_s.data_ptr(), stream()))
        kv = torch.zeros(B, Tq, P, 2, D, device=dev(), dtype=torch.float16)
        o_t = torch.zeros(384, D, device=dev(), dtype=torch.float16)
        L.check(lib.gtav_op_gemm_qkvt_attn(xt.data_ptr(), w_t.data_ptr(), B * Tq * P, D, P, Tq, 0, Tq, cs.data_ptr(), kv.data_ptr(), o_t.data_ptr(), stream()))
        return o_s, kv, o_t

    outs = _both_policies(run, 0)
    assert all(torch.isfinite(t.float()).all() for t in outs)


# ------------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_dit():
    m = DiT_models["DiT-S/2"](init_weights=False, max_batch=1)
    m.load_state_dict(W.synth_state_dict(W.dit_param_shapes(depth=16), seed=0))
    return m


def _steps(m, x0):
    """three sampler steps (eager warm-up, capture, replay) and a context-cached step on the K/V caches they wrote"""
    x = x0.clone()
    for k in range(3):
        m.denoise_step_(x, 0, 4, 15, 900 - 10 * k, 890 - 10 * k, False, None)
    m.denoise_step_(x, 0, 4, 15, 870, 860, False, None, cached=True)
    return x


def test_model_is_bit_equal_under_every_fill_policy(full_dit):
    from gtav_amd.generate import fill_policy_mode
    from gtav_amd.utils import alphas_cumprod
    m = full_dit
    g = torch.Generator().manual_seed(17)
    xf = torch.randn(1, 5, 16, 18, 32, generator=g) * 0.5
    x0 = xf.to(dev()).contiguous()
    t = torch.tensor([[15, 15, 15, 15, 700]])
    m.set_schedule(alphas_cumprod(1e-4))
    fwd, lat = [], []
    try:
        for prefetch in (True, False):
            m.set_weight_prefetch(prefetch)
            for word in (0, 0x1111, fill_policy_mode((0, 1, 0, 1))):
                m.set_weight_fill_policy(word)
                fwd.append(m(xf, t).clone())
                lat.append(_steps(m, x0))
                m.check()
    finally:
        m.set_weight_prefetch(True)
        m.set_weight_fill_policy(0)
    assert all(torch.equal(fwd[0], o) for o in fwd[1:]), "forward differs under a weight fill policy"
    assert all(torch.equal(lat[0], o) for o in lat[1:]), "sampler steps differ under a weight fill policy"
    assert torch.isfinite(lat[0]).all() and not torch.equal(lat[0], x0)


def test_setter_refuses_malformed_words_and_drops_the_graphs(full_dit):
    """A malformed word is refused by name on both sides of the binding.  A captured step bakes the kernel parameters in, so a changed word has to drop the
    handle's graphs: the steps after the change run eager warm-up, capture and replay again, and give the bits of the steps before it."""
    from gtav_amd.utils import alphas_cumprod
    m = full_dit
    lib = L.load()
    for bad in (2, 0x10000, 0x1112, -1):
        with pytest.raises(ValueError, match="set_weight_fill_policy"):
            m.set_weight_fill_policy(bad)
        with pytest.raises(L.GtavError, match="dit_set_weight_fill_policy"):
            L.check(lib.gtav_dit_set_weight_fill_policy(m._handle, bad))
    m.set_schedule(alphas_cumprod(1e-4))
    x0 = (torch.randn(1, 5, 16, 18, 32, generator=torch.Generator().manual_seed(5)) * 0.5).to(dev()).contiguous()
    try:
        m.set_weight_fill_policy(0)
        a = _steps(m, x0)                      # captures the step
        m.set_weight_fill_policy(0x0101)       # a change: the captured graphs carry the old kernel parameters and are dropped
        b = _steps(m, x0)                      # eager, capture, replay again — under the new word
        m.set_weight_fill_policy(0x0101)       # no change: nothing to drop
        c = _steps(m, x0)
        assert torch.equal(a, b) and torch.equal(a, c)
        m.check()
    finally:
        m.set_weight_fill_policy(0)


def test_tuner_reports_the_fill_policy_and_keeps_the_bits():
    """generate.tune_weight_prefetch on a toy model (5 frames of 64 tokens: 320 tokens, inside the loader-wave range): the new key, a valid word left on the
    model, equal latents before and after, and a JSON-serialisable report (bench.py prints it)."""
    import json
    from gtav_amd.generate import PREFETCH_CLASSES, fill_policy_mode, tune_weight_prefetch
    from gtav_amd.utils import alphas_cumprod
    kw = dict(input_h=16, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)
    m = DiT(**kw, max_batch=1, init_weights=False)
    m.load_state_dict(W.synth_state_dict(W.dit_param_shapes(**kw), seed=3))
    m.set_schedule(alphas_cumprod(1e-4))
    x0 = (torch.randn(1, 5, 16, 16, 16, generator=torch.Generator().manual_seed(1)) * 0.5).to(dev()).contiguous()
    before = _steps(m, x0)
    r = tune_weight_prefetch(m, 1, steps=4, rounds=1)
    f = r["weight_fill_policy"]
    assert f is not None and set(f["classes"]) == set(PREFETCH_CLASSES) and all(v in (0, 1) for v in f["classes"].values())
    assert f["mode"] == fill_policy_mode(tuple(f["classes"][c] for c in PREFETCH_CLASSES)) and m._weight_fill_policy == f["mode"]
    assert set(f["ms"]) == set(PREFETCH_CLASSES) and all(a > 0 and b > 0 for a, b in f["ms"].values())
    for c in PREFETCH_CLASSES:                  # the 0.3 % rule: non-temporal only where it was decisively faster than what was kept
        if f["classes"][c]:
            assert f["ms"][c][1] < f["ms"][c][0]
    json.dumps(r)
    m.set_schedule(alphas_cumprod(1e-4))        # (the tuner sets its own, equal, schedule)
    assert torch.equal(_steps(m, x0), before)
    m.check()
