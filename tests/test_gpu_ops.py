"""Kernel-level parity (GPU): every HIP kernel against fp32 torch math on the SAME fp16-rounded operands,
through the C-ABI (gtav_op_*).  Tolerances: fp32-accumulated GEMMs on identical inputs 2e-5 rel-L2; paths that
round an intermediate to fp16 (GELU out, attention P) 1.5e-3."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import parity_bounds as PB  # noqa: E402
from helpers import assert_declared_plan, dev, gemm, pad_weight_f16, rel_l2, stream, tiled_index, to_tiled_f16, untile  # noqa: E402
from gtav_amd import lib as L  # noqa: E402


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.mark.parametrize("M,N,K", [(720, 1024, 1024), (100, 256, 64), (144, 1200, 1024), (257, 64, 4096), (5760, 4096, 1024)])
def test_gemm_f32_epilogue(M, N, K):
    x = _rand(M, K, seed=1).half()
    w = _rand(N, K, scale=1 / math.sqrt(K), seed=2)
    b = _rand(N, seed=3)
    w16 = pad_weight_f16(w)
    xd, bd = to_tiled_f16(x), b.to(dev())
    out = torch.full((M, N), float("nan"), device=dev())
    gemm(xd, w16, bd, M, N, K, 0, out, N)
    ref = x.float() @ w.half().float().t() + b
    assert rel_l2(out, ref) < 2e-5
    assert torch.isfinite(out).all()


def test_gemm_f16_and_gelu_epilogues():
    M, N, K = 300, 512, 256
    x = _rand(M, K, seed=1).half()
    w = _rand(N, K, scale=1 / math.sqrt(K), seed=2)
    b = _rand(N, seed=3)
    w16 = pad_weight_f16(w)
    xd, bd = to_tiled_f16(x), b.to(dev())
    pre = x.float() @ w.half().float().t() + b
    for epi, fn in ((1, lambda z: z), (2, lambda z: torch.nn.functional.gelu(z, approximate="tanh")),
                    (3, lambda z: torch.nn.functional.gelu(z))):
        out = torch.zeros(((M + 127) // 128 * 128, N), device=dev(), dtype=torch.float16)
        gemm(xd, w16, bd, M, N, K, epi, out, N)
        got = out[:M].float().cpu() if epi == 1 else untile(out, M, N).float()   # GELU outputs are tile-major (next GEMM's A)
        assert rel_l2(got, fn(pre)) < 6e-4, epi


def test_gelu_erf_epilogue_absolute_error():
    """EPI_GELU_ERF (VAE Mlp, model/vae.py:128: torch.nn.GELU()) is a degree-9 polynomial on a clamped range (csrc/common.h gelu_erf_f4), not libm's erf:
    its contract is an ABSOLUTE error of 3.0e-5 on the fp32 value before the fp16 store (tools/gelu_poly_fit.py).  Sweep the pre-activation over [-9, 9]
    (one non-zero operand per row: pre[m][n] = v_m + bias_n exactly) and compare with torch's exact GELU: |error| <= 3.2e-5 + the fp16 rounding of the stored
    value.  In the negative tail (x < -4, |GELU| < 1e-4) that bound is all that holds: the RELATIVE error there may exceed 100 % and the sign may flip."""
    M, N, K = 1152, 128, 64
    v = torch.linspace(-9.0, 9.0, M).half().float()
    x = torch.zeros(M, K)
    x[:, 0] = v
    w = torch.zeros(N, K)
    w[:, 0] = 1.0
    b = (torch.arange(N, dtype=torch.float32) - N / 2) * (1.0 / 1024)       # offsets of +-1/16 in steps of 2^-10: fills the gaps of the fp16 sweep
    xd, w16, bd = to_tiled_f16(x), pad_weight_f16(w), b.to(dev())
    out = torch.zeros(((M + 127) // 128 * 128, N), device=dev(), dtype=torch.float16)
    gemm(xd, w16, bd, M, N, K, 3, out, N)
    got = untile(out, M, N).double()
    pre = (v[:, None] + b[None, :]).double()
    ref = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
    err = (got - ref).abs()
    tol = 3.2e-5 + ref.abs() * 2.0 ** -11 + 6e-8          # polynomial bound + half an ulp of the fp16 store (+ half a subnormal step)
    worst = (err - tol).max().item()
    print("GELU-erf epilogue: max |error| %.3e (at pre = %.4f), max over the negative tail x < -4: %.3e" %
          (err.max().item(), pre.flatten()[err.argmax()].item(), err[pre < -4].max().item()))
    assert worst <= 0, worst
    # the tanh form (DiT) through the same harness: exp2 + rcp, 1 ulp each -> relative accuracy everywhere, tails exact
    out2 = torch.zeros_like(out)
    gemm(xd, w16, bd, M, N, K, 2, out2, N)
    ref2 = torch.nn.functional.gelu(pre.float(), approximate="tanh").double()
    err2 = (untile(out2, M, N).double() - ref2).abs()
    assert (err2 <= 2e-6 + ref2.abs() * 2.0 ** -10.5 + 6e-8).all(), err2.max().item()


def test_gemm_residual_gate_epilogue():
    M, N, K, P = 288, 256, 512, 48   # 6 frames of 48 tokens
    x = _rand(M, K, seed=1).half()
    w = _rand(N, K, scale=1 / math.sqrt(K), seed=2)
    b = _rand(N, seed=3)
    resid = _rand(M, N, seed=4)
    modw = 3 * N
    mod = _rand(M // P, modw, seed=5)
    w16 = pad_weight_f16(w)
    r = resid.clone().to(dev())
    md, xd, bd = mod.to(dev()), to_tiled_f16(x), b.to(dev())
    gate_view = md[:, N:]   # gate vector lives at column offset N of each mod row
    L.check(L.load().gtav_op_gemm_f16(xd.data_ptr(), K, w16.data_ptr(), bd.data_ptr(), r.data_ptr(), N, M, N, K, 4,
                                      gate_view.data_ptr(), modw, P, stream()))
    y = x.float() @ w.half().float().t() + b
    ref = resid + mod[:, N:2 * N].repeat_interleave(P, dim=0) * y
    assert rel_l2(r, ref) < 2e-5
    # plain residual (gate == NULL), VAE style
    r2 = resid.clone().to(dev())
    L.check(L.load().gtav_op_gemm_f16(xd.data_ptr(), K, w16.data_ptr(), bd.data_ptr(), r2.data_ptr(), N, M, N, K, 4,
                                      0, 0, 1, stream()))
    assert rel_l2(r2, resid + y) < 2e-5


def _rope_ref(x, cos, sin):
    """x (..., 64) with per-row cos/sin (..., 64): interleaved-pair rotation."""
    x2 = x.reshape(*x.shape[:-1], 32, 2)
    rot = torch.stack((-x2[..., 1], x2[..., 0]), dim=-1).reshape(x.shape)
    return x * cos + rot * sin


def test_gemm_qkv_spatial_layout_and_rope():
    NB, S, D, heads = 3, 48, 256, 4
    M = NB * S
    x = _rand(M, D, seed=1).half()
    w = _rand(3 * D, D, scale=1 / math.sqrt(D), seed=2)
    bias = _rand(3 * D, seed=7)
    ang = (_rand(S, 32, seed=3) * 3).repeat_interleave(2, dim=-1)   # each frequency repeated twice (rotary_embedding_torch.py:337)
    cos, sin = ang.cos(), ang.sin()
    w16 = pad_weight_f16(w)
    q = torch.zeros(NB, heads, S, 64, device=dev(), dtype=torch.float16)
    k = torch.zeros_like(q)
    vt = torch.zeros(NB, heads, 64, S, device=dev(), dtype=torch.float16)
    xd, bd, cd, sd_ = to_tiled_f16(x), bias.to(dev()), cos.to(dev()).contiguous(), sin.to(dev()).contiguous()
    cs = torch.empty_like(cd)
    L.check(L.load().gtav_op_rope_interleave(cd.data_ptr(), sd_.data_ptr(), cs.data_ptr(), S, stream()))
    L.check(L.load().gtav_op_gemm_qkv(xd.data_ptr(), D, w16.data_ptr(), bd.data_ptr(), M, D, 0, q.data_ptr(),
                                      k.data_ptr(), vt.data_ptr(), S, 0, 0, 0, cs.data_ptr(), stream()))
    y = (x.float() @ w.half().float().t() + bias).reshape(NB, S, 3, heads, 64)
    qr = _rope_ref(y[:, :, 0].permute(0, 2, 1, 3), cos[None, None], sin[None, None])
    kr = _rope_ref(y[:, :, 1].permute(0, 2, 1, 3), cos[None, None], sin[None, None])
    vr = y[:, :, 2].permute(0, 2, 3, 1)  # (NB, heads, 64, S)
    assert rel_l2(q.float(), qr) < 6e-4
    assert rel_l2(k.float(), kr) < 6e-4
    assert rel_l2(vt.float(), vr) < 6e-4


def test_gemm_qkv_temporal_layout():
    B, Tq, t0, Tmax, P, D = 2, 2, 1, 4, 16, 256
    M = B * Tq * P
    x = _rand(M, D, seed=1).half()
    w = _rand(3 * D, D, scale=1 / math.sqrt(D), seed=2)
    ang = (_rand(Tmax, 32, seed=3) * 3).repeat_interleave(2, dim=-1)
    cos, sin = ang.cos(), ang.sin()
    w16 = pad_weight_f16(w)
    q = torch.zeros(M, D, device=dev(), dtype=torch.float16)
    kv = torch.zeros(B, Tmax, P, 2, D, device=dev(), dtype=torch.float16)
    xd, cd, sd_ = to_tiled_f16(x), cos.to(dev()).contiguous(), sin.to(dev()).contiguous()
    cs = torch.empty_like(cd)
    L.check(L.load().gtav_op_rope_interleave(cd.data_ptr(), sd_.data_ptr(), cs.data_ptr(), Tmax, stream()))
    L.check(L.load().gtav_op_gemm_qkv(xd.data_ptr(), D, w16.data_ptr(), 0, M, D, 1, q.data_ptr(), kv.data_ptr(),
                                      kv.data_ptr(), P, Tq, t0, Tmax, cs.data_ptr(), stream()))
    y = (x.float() @ w.half().float().t()).reshape(B, Tq, P, 3, D // 64, 64)
    pos = torch.arange(t0, t0 + Tq)
    c, s = cos[pos][None, :, None, None, :], sin[pos][None, :, None, None, :]
    qr = _rope_ref(y[:, :, :, 0], c, s).reshape(M, D)
    kr = _rope_ref(y[:, :, :, 1], c, s).reshape(B, Tq, P, D)
    vr = y[:, :, :, 2].reshape(B, Tq, P, D)
    assert rel_l2(q.float(), qr) < 6e-4
    assert rel_l2(kv[:, t0:t0 + Tq, :, 0].float(), kr) < 6e-4
    assert rel_l2(kv[:, t0:t0 + Tq, :, 1].float(), vr) < 6e-4
    assert kv[:, :t0].abs().max().item() == 0  # untouched cache slots


def _skinny(lib, xd, ldx, wd, bd, M, N, K, act, ldy):
    y = torch.full((M, ldy), float("nan"), device=dev())
    L.check(lib.gtav_op_skinny_f32(xd.data_ptr(), ldx, wd.data_ptr(), L.ptr(bd), y.data_ptr(), ldy, M, N, K, act, stream()))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("M,N,K,act,call", PB.SKINNY_CASES, ids=[f"{m}-{n}-{k}-{a}" for m, n, k, a, _ in PB.SKINNY_CASES])
def test_skinny_f32(M, N, K, act, call):
    """Every instantiation of skinny_f32_kernel (tests/parity_bounds.py SKINNY_CASES says which case selects which, and why it has its shape), with and without
    a bias, on contiguous rows and with ldx > K, ldy > N between NaN guard columns.  Two assertions (derived in parity_bounds.py, controlled on the CPU in
    tests/test_host_parity_bounds.py): every element inside its fp64 bound; and three 64-column windows of the output — the first block, a block boundary, the
    ragged tail — equal BIT FOR BIT to the 64-feature launch on the same rows of W, which runs the (act, 1, 1, 0) kernel: the same fp32 fma chain in the same
    order for every (FT, RT, KC), as csrc/skinny.hip promises.  profiles/op_parity_instantiations/margins.txt holds the measured margins."""
    lib = L.load()
    inst, _ = assert_declared_plan("skinny", M, N, K, act)
    c = PB.skinny_case(M, N, K, act, bias=call != "nobias")
    pad = 0 if call == "" else 4
    ldx, ldy = K + pad, N + pad
    x = torch.full((M, ldx), float("nan"))
    x[:, :K] = c.x
    xd, wd, bd = x.to(dev()), c.w.to(dev()), (c.b.to(dev()) if c.b is not None else None)
    y = _skinny(lib, xd, ldx, wd, bd, M, N, K, act, ldy)
    assert torch.isnan(y[:, N:]).all(), "the guard columns behind a row of Y were written"
    got = y[:, :N].cpu()
    assert torch.isfinite(got).all()
    frac, worst = PB.outside((got.double() - c.ref).abs(), c.tol)
    name = f"skinny {M}x{N}x{K} act={act}{' ' + call if call else ''} <{inst[1]},{inst[2]},{inst[3]},{inst[4]}>"
    print(f"[margin {name}] per element: worst error / bound {worst:.3f}")
    assert worst <= 1.0, (name, worst, frac)
    windows = c.windows(inst[2])
    for n_a in windows:
        assert PB.query_plan(lib, "skinny", (M, 64, K, act)) == ((inst[0], act, 1, 1, 0), None)
        ys = _skinny(lib, xd, ldx, wd[n_a:n_a + 64], bd[n_a:n_a + 64] if bd is not None else None, M, 64, K, act, 64)
        same = torch.equal(ys.view(torch.int32), y[:, n_a:n_a + 64].contiguous().view(torch.int32))
        assert same, f"{name}: columns {n_a} .. {n_a + 63} differ in their bits from the <{act},1,1,0> launch on the same rows of W"
    print(f"[margin {name}] bit-equal to the <{act},1,1,0> launch in the 64-column windows at {windows}")


@pytest.mark.parametrize("D,M", PB.LN_OPS_SHAPES)
def test_layernorm_kernels(D, M):
    """No pending update: D = 128 runs the one-block-per-row kernel, the others the one-wave-per-row kernel (NV = D / 256 float4 per lane; round 5) — 1027 rows
    leave a ragged last block, 46 080 are the batched VAE's rows (80 frames)."""
    P = 32 if M % 32 == 0 else 1
    x = _rand(M, D, seed=1) * 3 + 0.5
    mod = _rand(M // P, 2 * D, seed=2)
    out = torch.zeros((M + 127) // 128 * 128, D, device=dev(), dtype=torch.float16)
    md, xd = mod.to(dev()), x.to(dev())
    assert_declared_plan("layernorm", 0, M, D, 0, 0, 0, 0)
    L.check(L.load().gtav_op_ln_modulate(xd.data_ptr(), out.data_ptr(), M, D, md.data_ptr(), md[:, D:].data_ptr(), 2 * D, P,
                                         stream()))
    xh = torch.nn.functional.layer_norm(x, (D,), eps=1e-6)
    shift, scale = mod[:, :D].repeat_interleave(P, 0), mod[:, D:].repeat_interleave(P, 0)
    ref = xh * (1 + (scale + 1e-6)) + shift
    assert rel_l2(untile(out, M, D).float(), ref) < 5e-4
    g, b = _rand(D, seed=3) * 0.1 + 1, _rand(D, seed=4) * 0.1
    gd, bd = g.to(dev()), b.to(dev())
    assert_declared_plan("layernorm", 1, M, D, 0, 0, 0, 0)
    L.check(L.load().gtav_op_ln_affine(xd.data_ptr(), out.data_ptr(), M, D, gd.data_ptr(), bd.data_ptr(), stream()))
    assert rel_l2(untile(out, M, D).float(), torch.nn.functional.layer_norm(x, (D,), g, b, eps=1e-6)) < 5e-4


@pytest.mark.parametrize("D", PB.LN_LARGE_MEAN_D)
def test_layernorm_statistics_with_a_large_mean(D):
    """The one-pass statistics subtract the row's first element before squaring (both LayerNorm kernels): a row of 300 +- 0.02 must not lose its variance
    to cancellation (E[x^2] - E[x]^2 in fp32 would: 9e4 against 4e-4)."""
    M = PB.LN_LARGE_MEAN_M
    x = 300.0 + 0.02 * _rand(M, D, seed=5)
    g, b = _rand(D, seed=3) * 0.1 + 1, _rand(D, seed=4) * 0.1
    out = torch.zeros(128, D, device=dev(), dtype=torch.float16)
    xd, gd, bd = x.to(dev()), g.to(dev()), b.to(dev())
    assert_declared_plan("layernorm", 1, M, D, 0, 0, 0, 0)
    L.check(L.load().gtav_op_ln_affine(xd.data_ptr(), out.data_ptr(), M, D, gd.data_ptr(), bd.data_ptr(), stream()))
    ref = torch.nn.functional.layer_norm(x.double(), (D,), g.double(), b.double(), eps=1e-6)
    assert rel_l2(untile(out, M, D).float(), ref) < 1e-3


@pytest.mark.parametrize("NB,heads,S", PB.ATTN_OPS_SHAPES)
def test_attention_spatial(NB, heads, S):
    assert_declared_plan("attn_spatial", NB, heads, S, 0)
    q, k, v = (_rand(NB, heads, S, 64, seed=i).half() for i in (1, 2, 3))
    q = q * 1.5
    vt = v.transpose(-1, -2).contiguous()
    o = torch.zeros((NB * S + 127) // 128 * 128, heads * 64, device=dev(), dtype=torch.float16)
    qd, kd, vd = q.to(dev()), k.to(dev()), vt.to(dev())
    L.check(L.load().gtav_op_attn_spatial(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), NB, heads, S, stream()))
    ref = torch.nn.functional.scaled_dot_product_attention(q.float(), k.float(), v.float())
    ref = ref.permute(0, 2, 1, 3).reshape(NB * S, heads * 64)
    assert rel_l2(untile(o, NB * S, heads * 64).float(), ref) < 1.5e-3


def test_attention_spatial_online_softmax_spike():
    """Forces the running max to jump in a LATER key block (the rescale branch of the online softmax)."""
    NB, heads, S = PB.ATTN_OPS_SPIKE
    assert_declared_plan("attn_spatial", NB, heads, S, 0)
    q, k, v = (_rand(NB, heads, S, 64, seed=i).half() for i in (1, 2, 3))
    k[0, 0, 130] = q[0, 0, 7] * 4  # key 130 (third block) dominates query 7
    vt = v.transpose(-1, -2).contiguous()
    o = torch.zeros(256, 64, device=dev(), dtype=torch.float16)   # tile-major output, rows padded to 128
    qd, kd, vd = q.to(dev()), k.to(dev()), vt.to(dev())
    L.check(L.load().gtav_op_attn_spatial(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), NB, heads, S, stream()))
    ref = torch.nn.functional.scaled_dot_product_attention(q.float(), k.float(), v.float())[0, 0]
    got = untile(o, S, 64).float()
    assert rel_l2(got, ref) < 1.5e-3
    assert rel_l2(got[7], ref[7]) < 2e-3


@pytest.mark.parametrize("S,jump", PB.ATTN_OPS_JUMP)
def test_attention_flash_running_max_jump(S, jump):
    """Long sequences run the flash kernel (csrc/attention.hip attn_flash_kernel), whose reference maximum moves only when a key block's maximum
    exceeds it by more than 8 in the exponent: a key in a LATE block that dominates one query by far more than that (jump = 4: the rescale
    branch), and one that stays under the threshold (jump = 0.45: probabilities up to 2^8 against the stale maximum), against fp32 math on
    every row; 50 repetitions must agree bit for bit (the ring is refilled by LDS-DMA while it is read)."""
    NB, heads = PB.ATTN_NB, PB.ATTN_HEADS
    assert_declared_plan("attn_spatial", NB, heads, S, 0)
    q, k, v = (_rand(NB, heads, S, 64, seed=i).half() for i in (1, 2, 3))
    late = S - 9
    k[1, 2, late] = q[1, 2, 7] * jump           # key `late` (last key block) against query 7
    k[0, 1, 70] = q[0, 1, 150] * jump           # a jump in the second key block too
    vt = v.transpose(-1, -2).contiguous()
    rows = (NB * S + 127) // 128 * 128
    qd, kd, vd = q.to(dev()), k.to(dev()), vt.to(dev())
    outs = []
    for _ in range(50):
        o = torch.zeros(rows, heads * 64, device=dev(), dtype=torch.float16)
        L.check(L.load().gtav_op_attn_spatial(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), NB, heads, S, stream()))
        outs.append(o)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    ref = torch.nn.functional.scaled_dot_product_attention(q.float(), k.float(), v.float())
    ref = ref.permute(0, 2, 1, 3).reshape(NB * S, heads * 64)
    got = untile(outs[0], NB * S, heads * 64).float()
    assert rel_l2(got, ref) < 1.5e-3
    for (b, h, row) in ((1, 2, 7), (0, 1, 150)):
        assert rel_l2(got[b * S + row, h * 64:(h + 1) * 64], ref[b * S + row, h * 64:(h + 1) * 64]) < 2e-3


@pytest.mark.parametrize("Tq,t0", PB.TEMPORAL_OPS_WINDOWS)
def test_attention_temporal(Tq, t0):
    B, P, D, Tmax = PB.TEMPORAL_OPS_GEOMETRY
    assert_declared_plan("attn_temporal", B, P, D, Tq, t0, Tmax)
    Tk = t0 + Tq
    q = _rand(B, Tq, P, D, seed=1).half()
    kv = _rand(B, Tmax, P, 2, D, seed=2).half()
    o = torch.zeros((B * Tq * P + 127) // 128 * 128, D, device=dev(), dtype=torch.float16)
    qd, kvd = q.to(dev()), kv.to(dev())
    L.check(L.load().gtav_op_attn_temporal(qd.data_ptr(), kvd.data_ptr(), o.data_ptr(), B, P, D, Tq, t0, Tmax, stream()))
    h = D // 64
    qf = q.float().reshape(B, Tq, P, h, 64).permute(0, 2, 3, 1, 4)             # B P h Tq d
    kf = kv[:, :Tk, :, 0].float().reshape(B, Tk, P, h, 64).permute(0, 2, 3, 1, 4)
    vf = kv[:, :Tk, :, 1].float().reshape(B, Tk, P, h, 64).permute(0, 2, 3, 1, 4)
    s = qf @ kf.transpose(-1, -2) / 8.0
    mask = torch.arange(Tk)[None, :] > (t0 + torch.arange(Tq))[:, None]
    s = s.masked_fill(mask, float("-inf"))
    ref = (s.softmax(-1) @ vf).permute(0, 3, 1, 2, 4).reshape(B * Tq * P, D)
    assert rel_l2(untile(o, B * Tq * P, D).float(), ref) < 6e-4


@pytest.mark.parametrize("NB,D", [(5, 1024), (1, 256), (7, 512), (16, 1024), (5, 1792), (5, 2048)])
def test_fused_spatial_qkv_attention_equals_the_two_kernel_path(NB, D):
    """gemm_qkvs_attn_kernel (to_qkv projection + RoPE + spatial attention of 144-token frames in one launch; the q / k / v^T images stay in LDS) against
    gtav_op_gemm_qkv (spatial mode) + gtav_op_attn_spatial on the same operands: a BIT-EQUAL attention output (same fp16 q / k / v, the same tile body —
    csrc/attn_tile.h), both within fp16 rounding of fp32 math (model/attention.py:16-38).  Repeated launches must agree (race screen: the LDS image reuses the
    ring), and the rows behind the last frame must stay untouched."""
    S, heads = 144, D // 64
    M = NB * S
    lib = L.load()
    x = _rand(M, D, seed=1).half()
    w = _rand(3 * D, D, scale=1 / math.sqrt(D), seed=2)
    ang = (_rand(S, 32, seed=3) * 3).repeat_interleave(2, dim=-1)
    cd, sd_ = ang.cos().to(dev()).contiguous(), ang.sin().to(dev()).contiguous()
    cs = torch.empty_like(cd)
    L.check(lib.gtav_op_rope_interleave(cd.data_ptr(), sd_.data_ptr(), cs.data_ptr(), S, stream()))
    w16 = pad_weight_f16(w)
    xd = to_tiled_f16(x)
    Mp = (M + 127) // 128 * 128
    q = torch.zeros(NB, heads, S, 64, device=dev(), dtype=torch.float16)
    k = torch.zeros_like(q)
    vt = torch.zeros(NB, heads, 64, S, device=dev(), dtype=torch.float16)
    o = torch.full((Mp, D), 7.0, device=dev(), dtype=torch.float16)
    L.check(lib.gtav_op_gemm_qkv(xd.data_ptr(), D, w16.data_ptr(), 0, M, D, 0, q.data_ptr(), k.data_ptr(), vt.data_ptr(), S, 0, 0, 0, cs.data_ptr(), stream()))
    L.check(lib.gtav_op_attn_spatial(q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), NB, heads, S, stream()))
    w_hm = torch.empty_like(w16)
    L.check(lib.gtav_op_qkv_head_major_spatial(w16.data_ptr(), w_hm.data_ptr(), D, stream()))
    first = None
    for rep in range(20):
        o2 = torch.full_like(o, 7.0)
        L.check(lib.gtav_op_gemm_qkvs_attn(xd.data_ptr(), w_hm.data_ptr(), M, D, S, cs.data_ptr(), o2.data_ptr(), stream()))
        torch.cuda.synchronize()
        if first is None:
            first = o2.clone()
            assert torch.equal(untile(o2, M, D), untile(o, M, D)), "attention output differs from the two-kernel path"
            assert torch.equal(o2, o), "rows / padding outside the frames differ from the two-kernel path"
        else:
            assert torch.equal(o2, first), f"launch {rep} differs from launch 0"
    y = (x.float() @ w.half().float().t()).reshape(NB, S, 3, heads, 64)
    c, s_ = ang.cos()[None, None], ang.sin()[None, None]
    qf = _rope_ref(y[:, :, 0].permute(0, 2, 1, 3), c, s_).half().float()
    kf = _rope_ref(y[:, :, 1].permute(0, 2, 1, 3), c, s_).half().float()
    vf = y[:, :, 2].permute(0, 2, 1, 3).half().float()
    ref = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf).permute(0, 2, 1, 3).reshape(M, D)
    assert rel_l2(untile(first, M, D).float(), ref) < 1.5e-3


@pytest.mark.parametrize("D", list(range(128, 2048 + 1, 128)))
def test_qkv_head_major_every_hidden_size(D):
    """launch_qkv_head_major at every hidden size a handle accepts, both row orders, bit for bit against the row permutation the kernel documents:
    mode 0 (fused temporal launch) row hd 192 + which 64 + d, mode 1 (fused spatial launch) row hd 192 + w 48 + which 16 + e with d = 16 w + e, both <- source row
    which D + hd 64 + d; chunks keep their place inside the tile-major row.  The destination starts as a sentinel no source element holds, so a row the launch
    never wrote shows.  (It found the launch capped at 4096 blocks of 256 chunks with no grid-stride loop in the kernel: at D = 1792 the rows from 4681 on,
    at D = 2048 those from 4096 on — heads 21 .. 31 — kept the sentinel.)"""
    lib = L.load()
    R = 3 * D
    src = torch.randint(0, 30000, (R, D), generator=torch.Generator().manual_seed(D), dtype=torch.int16)
    idx = tiled_index(R, D).reshape(-1)                      # R % 128 == 0 and D % 64 == 0: the image has exactly R D elements
    image = torch.empty(R * D, dtype=torch.int16)
    image[idx] = src.reshape(-1)
    sd = image.to(dev())
    nd = torch.arange(R)
    hd, rem = nd // 192, nd % 192
    rows = {0: (rem // 64) * D + hd * 64 + rem % 64,
            1: ((rem % 48) // 16) * D + hd * 64 + 16 * (rem // 48) + rem % 16}
    for mode, fn in ((0, lib.gtav_op_qkv_head_major), (1, lib.gtav_op_qkv_head_major_spatial)):
        assert sorted(rows[mode].tolist()) == list(range(R))
        dst = torch.full((R * D,), 0x7B7B, dtype=torch.int16, device=dev())
        L.check(fn(sd.data_ptr(), dst.data_ptr(), D, stream()))
        torch.cuda.synchronize()
        got = dst.cpu()
        want = torch.empty(R * D, dtype=torch.int16)
        want[idx] = src[rows[mode]].reshape(-1)
        unwritten = (got == 0x7B7B).sum().item()
        assert unwritten == 0, f"D={D} mode {mode}: {unwritten} of {R * D} elements never written (first logical row {(got[idx].reshape(R, D) == 0x7B7B).any(1).nonzero()[0].item()})"
        assert torch.equal(got, want), f"D={D} mode {mode}"
    assert torch.equal(sd.cpu(), image)


def test_fused_spatial_qkv_attention_refuses_other_geometries():
    lib = L.load()
    z = torch.zeros(1 << 16, device=dev(), dtype=torch.float16)
    cs = torch.zeros(144 * 64, device=dev())
    for M, D, P in ((128, 256, 128), (100, 256, 144), (144, 96, 144), (0, 256, 144)):   # frames of 128 tokens, a ragged frame, hidden % 64, nothing — all refused before any launch
        with pytest.raises(L.GtavError, match="qkvs_attn"):
            L.check(lib.gtav_op_gemm_qkvs_attn(z.data_ptr(), z.data_ptr(), M, D, P, cs.data_ptr(), z.data_ptr(), stream()))


@pytest.mark.parametrize("B,P,D", [(1, 144, 1024), (2, 32, 256), (3, 16, 256), (1, 16, 2048)])
def test_fused_temporal_qkv_attention_equals_the_two_kernel_path(B, P, D):
    """gemm_qkvt_attn_kernel (to_qkv projection + RoPE + causal temporal attention + K/V cache rows in one launch) against
    gtav_op_gemm_qkv + gtav_op_attn_temporal on the same operands: BIT-EQUAL cache rows and attention output (same fp16 q / k / v,
    same arithmetic order), and both within fp16 rounding of fp32 math (model/attention.py:41-71).  Repeated launches must agree too
    (race screen: the fused kernel's LDS image reuses the ring)."""
    Tq, t0, Tmax = 5, 0, 5
    M = B * Tq * P
    lib = L.load()
    x = _rand(M, D, seed=1).half()
    w = _rand(3 * D, D, scale=1 / math.sqrt(D), seed=2)
    ang = (_rand(Tmax, 32, seed=3) * 3).repeat_interleave(2, dim=-1)
    cd, sd_ = ang.cos().to(dev()).contiguous(), ang.sin().to(dev()).contiguous()
    cs = torch.empty_like(cd)
    L.check(lib.gtav_op_rope_interleave(cd.data_ptr(), sd_.data_ptr(), cs.data_ptr(), Tmax, stream()))
    w16 = pad_weight_f16(w)
    Mp = (M + 127) // 128 * 128
    # two-kernel path
    q = torch.zeros(M, D, device=dev(), dtype=torch.float16)
    kv = torch.zeros(B, Tmax, P, 2, D, device=dev(), dtype=torch.float16)
    o = torch.zeros(Mp, D, device=dev(), dtype=torch.float16)
    L.check(lib.gtav_op_gemm_qkv(to_tiled_f16(x).data_ptr(), D, w16.data_ptr(), 0, M, D, 1, q.data_ptr(), kv.data_ptr(), kv.data_ptr(), P, Tq,
                                 t0, Tmax, cs.data_ptr(), stream()))
    L.check(lib.gtav_op_attn_temporal(q.data_ptr(), kv.data_ptr(), o.data_ptr(), B, P, D, Tq, t0, Tmax, stream()))
    # fused: rows (b, t, p) -> (b, p // 16, t, p % 16), head-major weight rows
    xp = x.reshape(B, Tq, P // 16, 16, D).permute(0, 2, 1, 3, 4).reshape(M, D)
    w_hm = torch.empty_like(w16)
    L.check(lib.gtav_op_qkv_head_major(w16.data_ptr(), w_hm.data_ptr(), D, stream()))
    xpd = to_tiled_f16(xp)
    first = None
    for rep in range(20):
        kv2 = torch.zeros_like(kv)
        o2 = torch.zeros_like(o)
        L.check(lib.gtav_op_gemm_qkvt_attn(xpd.data_ptr(), w_hm.data_ptr(), M, D, P, Tq, t0, Tmax, cs.data_ptr(), kv2.data_ptr(), o2.data_ptr(),
                                           stream()))
        torch.cuda.synchronize()
        if first is None:
            first = (kv2.clone(), o2.clone())
            assert torch.equal(kv2, kv), "K / V cache rows differ from the two-kernel path"
            assert torch.equal(untile(o2, M, D), untile(o, M, D)), "attention output differs from the two-kernel path"
        else:
            assert torch.equal(kv2, first[0]) and torch.equal(o2, first[1]), f"launch {rep} differs from launch 0"
    # and against fp32 math
    h = D // 64
    y = (x.float() @ w.half().float().t()).reshape(B, Tq, P, 3, h, 64)
    pos = torch.arange(Tq)
    c, s = ang.cos()[pos][None, :, None, None, :], ang.sin()[pos][None, :, None, None, :]
    qf = _rope_ref(y[:, :, :, 0], c, s).half().float().permute(0, 2, 3, 1, 4)     # B P h T d
    kf = _rope_ref(y[:, :, :, 1], c, s).half().float().permute(0, 2, 3, 1, 4)
    vf = y[:, :, :, 2].half().float().permute(0, 2, 3, 1, 4)
    sc = qf @ kf.transpose(-1, -2) / 8.0
    sc = sc.masked_fill(torch.arange(Tq)[None, :] > torch.arange(Tq)[:, None], float("-inf"))
    ref = (sc.softmax(-1) @ vf).permute(0, 3, 1, 2, 4).reshape(M, D)
    assert rel_l2(untile(first[1], M, D).float(), ref) < 6e-4


@pytest.mark.parametrize("NB,heads,S", PB.ATTN_BWD_OPS_SHAPES)
def test_attention_spatial_backward_mfma(NB, heads, S):
    """attn_spatial_bwd_mfma_kernel (train.hip) against torch.autograd of softmax(q k^T / 8) v on the same fp16 q / k / v / dO
    (model/attention.py:99-136): dv, and dq / dk rotated back through the RoPE the forward applied (cos / sin per (position, pair)).
    The kernel rounds P and dS to fp16 for its MFMA operands: 2e-3."""
    lib = L.load()
    assert_declared_plan("attn_spatial_bwd", NB, heads, S)
    D = heads * 64
    q = _rand(NB, heads, S, 64, seed=1).half()
    k = _rand(NB, heads, S, 64, seed=2).half()
    v = _rand(NB, heads, S, 64, seed=3).half()
    do = _rand(NB * S, D, seed=4).half()
    ang = (_rand(S, 32, seed=5) * 3)
    cs = torch.stack([ang.cos(), ang.sin()], dim=-1).reshape(S, 64).contiguous()          # [pos][pair][cos, sin]
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    o = torch.softmax(qf @ kf.transpose(-1, -2) / 8.0, dim=-1) @ vf                            # NB h S 64
    o.backward(do.float().reshape(NB, S, heads, 64).permute(0, 2, 1, 3))
    co, si = ang.cos()[None, None], ang.sin()[None, None]                                      # RoPE^T: rotation by the negative angle

    def unrope(gr):
        a, b = gr[..., 0::2], gr[..., 1::2]
        return torch.stack([a * co + b * si, b * co - a * si], dim=-1).reshape(gr.shape)

    ref = torch.cat([unrope(qf.grad), unrope(kf.grad), vf.grad], dim=1)                        # NB (3 h) S 64
    ref = ref.reshape(NB, 3, heads, S, 64).permute(0, 3, 1, 2, 4).reshape(NB * S, 3 * D)
    Mp = (NB * S + 127) // 128 * 128
    out = torch.zeros(Mp, 3 * D, device=dev(), dtype=torch.float16)
    qd, kd, vtd, dod, csd = (t.to(dev()).contiguous() for t in (q, k, v.transpose(-1, -2), do, cs))   # keep the device copies alive over the call
    L.check(lib.gtav_op_attn_spatial_bwd(qd.data_ptr(), kd.data_ptr(), vtd.data_ptr(), dod.data_ptr(), NB, heads, S, csd.data_ptr(), out.data_ptr(), stream()))
    torch.cuda.synchronize()
    out2 = torch.zeros_like(out)
    L.check(lib.gtav_op_attn_spatial_bwd(qd.data_ptr(), kd.data_ptr(), vtd.data_ptr(), dod.data_ptr(), NB, heads, S, csd.data_ptr(), out2.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert torch.equal(out, out2)          # no atomics: launches are bitwise reproducible
    got = untile(out, NB * S, 3 * D).float()
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        e = rel_l2(got[:, sl], ref[:, sl])
        assert e < 2e-3, (name, e)


@pytest.mark.parametrize("T,M,N", [(320, 1024, 2048), (64, 128, 128), (1152, 384, 256)])
def test_gemm_tn_weight_gradient(T, M, N):
    """gemm_tn_kernel: out[m][n] += sum_t x[t][m] w[t][n] on the tile-major [tokens][features] operands (transposing LDS reads; the dW of every
    Linear in the training step) against fp32 math on the same fp16 values, accumulating into a non-zero output, twice (bitwise equal)."""
    lib = L.load()
    x = _rand(T, M, seed=1).half()
    w = _rand(T, N, seed=2).half()
    base = _rand(M, N, seed=3)
    xd, wd = to_tiled_f16(x), to_tiled_f16(w)
    outs = []
    for _ in range(2):
        out = base.to(dev()).clone()
        L.check(lib.gtav_op_gemm_tn(xd.data_ptr(), wd.data_ptr(), M, N, T, out.data_ptr(), N, stream()))
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    ref = base + x.float().t() @ w.float()
    assert rel_l2(outs[0], ref) < 2e-5


@pytest.mark.parametrize("groups,K", [([(1024, 256), (256, 1024), (768, 256), (256, 256)], 320), ([(512, 512)], 64), ([(256, 768), (1280, 256)], 1152),
                                      ([(1024, 1024), (256, 256), (256, 512)], 128)])
def test_gemm_dw_grouped_weight_gradients(groups, K):
    """gemm256_dw_grouped_kernel: one to four weight-gradient GEMMs out_g[m][n] += sum_k X_g[m][k] W_g[n][k] (X_g / W_g = transposed activations,
    K = tokens) as ONE grid of 256 x 256 tiles: every group's tiles land in its own output (12, 4, 8 and 19 tiles: grids that are and are not
    multiples of the 8 XCDs), 1 to 18 K-steps, accumulating into non-zero outputs, twice (bitwise equal)."""
    import ctypes as C
    lib = L.load()
    n = len(groups)
    xs = [_rand(M, K, seed=10 + i).half() for i, (M, N) in enumerate(groups)]
    ws = [_rand(N, K, scale=1 / math.sqrt(K), seed=20 + i).half() for i, (M, N) in enumerate(groups)]
    base = [_rand(M, N, seed=30 + i) for i, (M, N) in enumerate(groups)]
    xd, wd = [to_tiled_f16(x) for x in xs], [to_tiled_f16(w) for w in ws]
    runs = []
    for _ in range(2):
        outs = [b.to(dev()).clone() for b in base]
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        ints = lambda v: (C.c_int32 * n)(*v)
        L.check(lib.gtav_op_gemm_dw_grouped(n, arr(xd), arr(wd), arr(outs), ints([g[0] for g in groups]), ints([g[1] for g in groups]), ints([g[1] for g in groups]),
                                            K, stream()))
        torch.cuda.synchronize()
        runs.append(outs)
    for i in range(n):
        assert torch.equal(runs[0][i], runs[1][i])
        ref = base[i] + xs[i].float() @ ws[i].float().t()
        assert rel_l2(runs[0][i], ref) < 2e-5, (i, groups[i])


def test_ddim_update_matches_reference_formula():
    rows, n = 6, 1000
    x, v = _rand(rows, n, seed=1), _rand(rows, n, seed=2)
    at = torch.rand(rows, generator=torch.Generator().manual_seed(3)) * 0.98 + 0.01
    an = torch.rand(rows, generator=torch.Generator().manual_seed(4)) * 0.98 + 0.01
    an[:3] = 1.0
    from gtav_amd.sampler import ddim_update
    for final in (False, True):
        out = ddim_update(x.to(dev()), v.to(dev()), at.to(dev()), an.to(dev()), final)
        a_t, a_n = at[:, None], an[:, None]
        x0 = a_t.sqrt() * x - (1 - a_t).sqrt() * v
        eps = ((1 / a_t).sqrt() * x - x0) / (1 / a_t - 1).sqrt()
        ref = x0 if final else a_n.sqrt() * x0 + (1 - a_n).sqrt() * eps
        assert rel_l2(out, ref) < 1e-6


@pytest.mark.parametrize("M,N,K,splitk", [(720, 1024, 4096, 0), (720, 1024, 1024, 4), (144, 1024, 4096, 8), (300, 256, 512, 1), (5760, 1024, 1024, 0)])
def test_gemm_splitk_partials_reduced_by_layernorm(M, N, K, splitk):
    """The residual path as the model runs it: EPI_PARTIAL slabs + the LN kernel's deferred
    `resid += gate * (sum parts + bias)` (model/dit.py:207-223) followed by LN + modulate."""
    P = 36 if M % 36 == 0 else M
    x = _rand(M, K, seed=1).half()
    w = _rand(N, K, scale=1 / math.sqrt(K), seed=2)
    b = _rand(N, seed=3)
    resid = _rand(M, N, seed=4)
    mod = _rand(M // P, 3 * N, seed=5)      # [gate | shift | scale]
    w16 = pad_weight_f16(w)
    sk = splitk or L.load().gtav_op_gemm_choose_splitk(M, N, K)
    assert 1 <= sk <= 8
    xd, bd, rd, md = to_tiled_f16(x), b.to(dev()), resid.clone().to(dev()), mod.to(dev())
    parts = torch.full((sk, M, N), float("nan"), device=dev())
    out = torch.zeros((M + 127) // 128 * 128, N, device=dev(), dtype=torch.float16)
    L.check(L.load().gtav_op_gemm_splitk_ln(xd.data_ptr(), K, w16.data_ptr(), bd.data_ptr(), M, N, K, splitk, parts.data_ptr(),
                                            rd.data_ptr(), md.data_ptr(), 3 * N, P, out.data_ptr(), md[:, N:].data_ptr(),
                                            md[:, 2 * N:].data_ptr(), 3 * N, stream()))
    y = x.float() @ w.half().float().t() + b
    gate, shift, scale = (mod[:, i * N:(i + 1) * N].repeat_interleave(P, 0) for i in range(3))
    new_resid = resid + gate * y
    assert rel_l2(rd, new_resid) < 2e-5
    ref = torch.nn.functional.layer_norm(new_resid, (N,), eps=1e-6) * (1 + (scale + 1e-6)) + shift
    assert rel_l2(untile(out, M, N).float(), ref) < 5e-4


@pytest.mark.parametrize("M,K,splitk", [(720, 4096, 4), (1152, 4096, 4), (720, 1024, 2)])
def test_inplace_pending_layernorm_is_bit_reproducible(M, K, splitk):
    """VERDICT r3 #6 / ADVICE r3: the LayerNorm that applies a pending split-K update IN PLACE — `resid += gate (sum of slabs + bias)` written back to the
    row it then normalises (ln_row_block_kernel<*, true>: every thread stores its chunk of the row behind the statistics' barrier) — 50 runs from the same
    inputs must agree bit for bit in both outputs (the updated residual and the fp16 operand); a store that overtakes another thread's read of the row, or a
    slab read before its GEMM's store, shows up as run-to-run differences.  Shapes: fc2 / out-proj of the batch-1 window step and of the batch-8 cached step."""
    N, P = 1024, 144
    x = _rand(M, K, seed=1).half()
    w = _rand(N, K, scale=1 / math.sqrt(K), seed=2)
    b = _rand(N, seed=3)
    resid = _rand(M, N, seed=4)
    mod = _rand(M // P, 3 * N, seed=5)
    w16, xd, bd, md = pad_weight_f16(w), to_tiled_f16(x), b.to(dev()), mod.to(dev())
    first = None
    for r in range(50):
        rd = resid.clone().to(dev())
        parts = torch.full((splitk, M, N), float("nan"), device=dev())
        out = torch.zeros((M + 127) // 128 * 128, N, device=dev(), dtype=torch.float16)
        L.check(L.load().gtav_op_gemm_splitk_ln(xd.data_ptr(), K, w16.data_ptr(), bd.data_ptr(), M, N, K, splitk, parts.data_ptr(),
                                                rd.data_ptr(), md.data_ptr(), 3 * N, P, out.data_ptr(), md[:, N:].data_ptr(),
                                                md[:, 2 * N:].data_ptr(), 3 * N, stream()))
        if first is None:
            first = (rd.clone(), out.clone())
            y = x.float() @ w.half().float().t() + b
            assert rel_l2(rd, resid + mod[:, :N].repeat_interleave(P, 0) * y) < 2e-5
        else:
            assert torch.equal(rd, first[0]) and torch.equal(out, first[1]), r


@pytest.mark.parametrize("M,K", [(5760, 1024), (5760, 4096)])
def test_inplace_residual_persistent_epilogue_is_bit_reproducible(M, K):
    """the in-place gated residual epilogue of the persistent loader-wave kernel (shape 31, EPI_RESID: the residual tile is requested at the head of
    the tile's K loop, bias / gate rows staged in LDS by tile parity) as the batch-8 forward runs it (out-proj K = 1024, fc2 K = 4096, 144-token frames): 50 runs
    from the same residual must agree bit for bit."""
    lib = L.load()
    N, P = 1024, 144
    x = _rand(M, K, seed=1).half()
    w = _rand(N, K, scale=1 / math.sqrt(K), seed=2)
    b = _rand(N, seed=3)
    resid, gate = _rand(M, N, seed=4), _rand(M // P, N, seed=5)
    w16, xd, bd, gd = pad_weight_f16(w), to_tiled_f16(x), b.to(dev()), gate.to(dev())
    assert lib.gtav_op_gemm_resid_inplace(M, N, K) == 1          # the heuristic's own choice at this size
    first = None
    for r in range(50):
        rd = resid.clone().to(dev())
        L.check(lib.gtav_op_gemm_f16(xd.data_ptr(), K, w16.data_ptr(), bd.data_ptr(), rd.data_ptr(), N, M, N, K, 4, gd.data_ptr(), N, P, stream()))
        if first is None:
            first = rd.clone()
            assert rel_l2(rd, resid + gate.repeat_interleave(P, dim=0) * (x.float() @ w.half().float().t() + b)) < 2e-5
        else:
            assert torch.equal(rd, first), r


@pytest.mark.parametrize("ns", [2, 4])
def test_gemm_pipeline_depths_agree(ns):
    """Both LDS ring depths (2 and 4 stages) of the GEMM give the same result, incl. K as short as one tile."""
    lib = L.load()
    try:
        lib.gtav_op_gemm_set_stages(ns)
        for (M, N, K) in ((720, 1024, 1024), (130, 128, 64), (257, 384, 192)):
            x = _rand(M, K, seed=1).half()
            w = _rand(N, K, scale=1 / math.sqrt(K), seed=2)
            w16 = pad_weight_f16(w)
            xd = to_tiled_f16(x)
            out = torch.full((M, N), float("nan"), device=dev())
            gemm(xd, w16, None, M, N, K, 0, out, N)
            assert rel_l2(out, x.float() @ w.half().float().t()) < 2e-5, (ns, M, N, K)
    finally:
        lib.gtav_op_gemm_set_stages(0)


@pytest.mark.parametrize("M,N,K", [(5760, 1024, 1024), (700, 384, 192), (256, 128, 64), (1300, 256, 4096)])
def test_gemm_8wave_tile_matches(M, N, K):
    """The 128 x 128 block shapes (2: 4 waves, 3: 8 waves with staggered fills) at both ring depths against fp32 math, incl. ragged
    last tiles.  (Round 1's shapes 4 / 5 / 6 / 10 — 128 x 256 and loader-wave variants — measured slower and were removed.)"""
    lib = L.load()
    try:
      for shape in (2, 3):
        lib.gtav_op_gemm_set_wm(shape)
        for ns in (2, 4):
            lib.gtav_op_gemm_set_stages(ns)
            x = _rand(M, K, seed=1).half()
            w = _rand(N, K, scale=1 / math.sqrt(K), seed=2)
            b = _rand(N, seed=3)
            w16, xd, bd = pad_weight_f16(w), to_tiled_f16(x), b.to(dev())
            out = torch.full((M, N), float("nan"), device=dev())
            gemm(xd, w16, bd, M, N, K, 0, out, N)
            assert rel_l2(out, x.float() @ w.half().float().t() + b) < 2e-5, (shape, ns, M, N, K)
    finally:
        lib.gtav_op_gemm_set_wm(0)
        lib.gtav_op_gemm_set_stages(0)


@pytest.mark.parametrize("shape", [7, 11, 12, 13, 14, 20, 24, 26, 29])
def test_gemm_other_tiles_all_epilogues(shape):
    """Block shapes 7 (256 x 256, phased K-tile, mainloop256), 11 / 14 (64 x 48, 64 x 96), 12 (128 x 192; piece-granular mainloop_g) and
    20 (128 x 96 loader-wave kernel) through every epilogue they support, incl. ragged token and feature edges, K of one and two tiles
    (prologue / tail paths of the pipelines) and split-K slabs.  (Shapes 8, 9, 16, 21, 23, 25 measured slower than these and exist only
    in the experiments build, csrc/build.sh exp.)"""
    lib = L.load()
    try:
        lib.gtav_op_gemm_set_wm(shape)
        for (M, N, K) in ((5760, 1024, 1024), (700, 384, 192), (256, 128, 64), (1300, 256, 4096), (513, 512, 128), (100, 768, 320),
                          (720, 3072, 1024), (96, 96, 64), (97, 100, 128), (1152, 4096, 1024), (1000, 384, 256)):
            x = _rand(M, K, seed=1).half()
            w = _rand(N, K, scale=1 / math.sqrt(K), seed=2)
            b = _rand(N, seed=3)
            w16, xd, bd = pad_weight_f16(w), to_tiled_f16(x), b.to(dev())
            out = torch.full((M, N), float("nan"), device=dev())
            gemm(xd, w16, bd, M, N, K, 0, out, N)
            assert rel_l2(out, x.float() @ w.half().float().t() + b) < 2e-5, (M, N, K)
        test_gemm_f16_and_gelu_epilogues()
        test_gemm_residual_gate_epilogue()
        if shape not in (7, 17):     # the 256 x 256 tile has no QKV epilogue in the product build (never selected for it)
            test_gemm_qkv_spatial_layout_and_rope()
            test_gemm_qkv_temporal_layout()
        for args in ((720, 1024, 4096, 2), (720, 1024, 1024, 4), (300, 256, 512, 1), (5760, 1024, 1024, 2)):
            test_gemm_splitk_partials_reduced_by_layernorm(*args)
    finally:
        lib.gtav_op_gemm_set_wm(0)


EXPERIMENT_SHAPES = (8, 9, 16, 17, 18, 21, 22, 23, 25, 27, 28, 30, 32, 33, 40, 41, 42)


def test_product_refuses_the_experiment_block_shapes():
    """Every block shape of csrc/gemm_experiments.inc is refused by the product library by name, before anything is launched (the output
    stays as it was), and the refusal leaves nothing behind: the next unforced GEMM on the same buffers is right."""
    lib = L.load()
    M, N, K = 96, 96, 64
    x = _rand(M, K, seed=1).half()
    w = _rand(N, K, scale=1 / math.sqrt(K), seed=2)
    b = _rand(N, seed=3)
    w16, xd, bd = pad_weight_f16(w), to_tiled_f16(x), b.to(dev())
    out = torch.full((M, N), float("nan"), device=dev())
    try:
        for shape in EXPERIMENT_SHAPES:
            lib.gtav_op_gemm_set_wm(shape)
            with pytest.raises(L.GtavError) as e:
                gemm(xd, w16, bd, M, N, K, 0, out, N)
            assert f"block shape {shape}" in str(e.value) and "exists only in the experiments build" in str(e.value), (shape, str(e.value))
            assert torch.isnan(out).all(), shape
    finally:
        lib.gtav_op_gemm_set_wm(0)
    gemm(xd, w16, bd, M, N, K, 0, out, N)
    assert rel_l2(out, x.float() @ w.half().float().t() + b) < 2e-5


@pytest.mark.parametrize("shape", [31])
@pytest.mark.parametrize("M,N,K", [(5760, 4096, 1024), (5760, 1024, 4096), (2312, 384, 896), (192, 128, 64), (11520, 1024, 1024), (100, 256, 128)])
def test_persistent_loader_wave_kernel(shape, M, N, K):
    """Block shape 31 (round 3; 30 / 32 / 33, its 4-stage and 256 x 128 / 128 x 256 forms, live in the experiments build and passed this test there): the persistent loader-wave kernel — one block per CU walking several 128 x 192 tiles with the LDS ring
    running on across tile boundaries, epilogue straight from the accumulators — on the GELU (fp16 tile-major) and full-K slab (fp32) epilogues:
    one tile per block, several tiles per block (960 tiles on 256 CUs), ragged token / feature edges, K of 1, 2, 14, 16 and 64 K-steps; two runs
    must agree bit for bit (a fill that lands after its first read, or a ring slot refilled too early, shows up as run-to-run differences)."""
    lib = L.load()
    x = _rand(M, K, seed=1).half()
    w = _rand(N, K, scale=1 / math.sqrt(K), seed=2)
    b = _rand(N, seed=3)
    w16, xd, bd = pad_weight_f16(w), to_tiled_f16(x), b.to(dev())
    pre = x.float() @ w.half().float().t()
    try:
        lib.gtav_op_gemm_set_wm(shape)
        outs = []
        for _ in range(2):
            out = torch.zeros(((M + 127) // 128 * 128, N), device=dev(), dtype=torch.float16)
            gemm(xd, w16, bd, M, N, K, 2, out, N)
            outs.append(out.clone())
        assert torch.equal(outs[0], outs[1])
        assert rel_l2(untile(outs[0], M, N).float(), torch.nn.functional.gelu(pre + b, approximate="tanh")) < 6e-4
        parts = torch.full((M, N), float("nan"), device=dev())
        L.check(lib.gtav_op_gemm_f16(xd.data_ptr(), K, w16.data_ptr(), 0, parts.data_ptr(), N, M, N, K, 6, 0, 1, 1, stream()))
        assert rel_l2(parts, pre) < 2e-5
        # in-place gated residual epilogue (the residual tile is requested at the head of the tile's K loop): frames of 36 tokens where M allows, else one frame
        P = 36 if M % 36 == 0 else M
        resid, gate = _rand(M, N, seed=4), _rand(M // P, N, seed=5)
        rs = []
        for _ in range(2):
            r = resid.clone().to(dev())
            gd = gate.to(dev())
            L.check(lib.gtav_op_gemm_f16(xd.data_ptr(), K, w16.data_ptr(), bd.data_ptr(), r.data_ptr(), N, M, N, K, 4, gd.data_ptr(), N, P, stream()))
            rs.append(r.cpu())
        assert torch.equal(rs[0], rs[1])
        assert rel_l2(rs[0], resid + gate.repeat_interleave(P, dim=0) * (pre + b)) < 2e-5
    finally:
        lib.gtav_op_gemm_set_wm(0)
