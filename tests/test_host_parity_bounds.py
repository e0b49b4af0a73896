"""The bounds of tests/test_gpu_ops_typed.py, checked on the CPU (no library, no GPU): a bound is only worth asserting if a correct kernel stays inside it and a
subtly wrong one does not.  For every per-element bound, an emulation in fp32 arithmetic with a round-to-nearest-even 2-byte store must leave NO element
outside, and the same emulation with a TRUNCATING store (a dropped guard bit, a wrong pack instruction) must put at least 1 % of the elements outside.  For
every per-row bound, the fp64 reference rounded to the operand type — the best any kernel can return — must stay below 0.6 of the bound in its worst row.
`pytest -s` prints every figure."""
import pytest
import torch

import parity_bounds as PB

DTYPES = pytest.mark.parametrize("dtype", PB.DTYPES, ids=[PB.NAME[d] for d in PB.DTYPES])


def _control(name, dtype, value32, ref, tol):
    """value32: the emulated fp32 value in front of the store"""
    f_rne, w_rne = PB.outside((PB.store_rne(value32, dtype).double() - ref).abs(), tol)
    f_tr, w_tr = PB.outside((PB.store_trunc(value32, dtype).double() - ref).abs(), tol)
    print(f"[bound control {name} {PB.NAME[dtype]}] round to nearest: {100 * f_rne:.2f} % outside, worst ratio {w_rne:.3f}; truncating: {100 * f_tr:.2f} % outside, "
          f"worst ratio {w_tr:.3f}")
    assert f_rne == 0.0, (name, f_rne, w_rne)
    assert f_tr >= 0.01, (name, f_tr)


def test_truncating_store_is_a_truncation():
    x = torch.tensor([1.0 + 2.0 ** -9, -1.0 - 2.0 ** -9, 1.0 + 3 * 2.0 ** -11, 70000.0, -70000.0, 2.0 ** -25, 0.0, 1.5])
    for dtype in PB.DTYPES:
        t = PB.store_trunc(x, dtype).double()
        assert (t.abs() <= x.double().abs()).all() and torch.isfinite(t).all()
        assert (torch.sign(t) * torch.sign(x.double()) >= 0).all()
        inr = x.abs() < 65000.0                                                       # (70000 is beyond fp16: it stops at the largest finite value)
        assert ((x.double() - t).abs() <= 2 * PB.U[dtype] * x.double().abs() + PB.SUBNORMAL[dtype])[inr].all()
        assert t[7] == 1.5
    assert PB.store_trunc(x, PB.F16)[2].item() == 1.0 + 2.0 ** -10 and PB.store_rne(x, PB.F16)[2].item() == 1.0 + 2 * 2.0 ** -10
    assert PB.store_trunc(x, PB.BF16)[0].item() == 1.0 and PB.store_trunc(x, PB.F16)[3].item() == 65504.0


@DTYPES
@pytest.mark.parametrize("M,N,K", sorted(set(PB.GEMM_STORE_SHAPES + PB.GEMM_SHAPE_SIZES + [PB.GEMM_PERSISTENT_SIZE])))
def test_gemm_store_bound(M, N, K, dtype):
    """EPI_F16 / EPI_F16_TILED (the store bound), EPI_F32 (the accumulation term alone) and EPI_GELU_TANH behind a GEMM"""
    c = PB.gemm_case(M, N, K, dtype)
    pre = c.emulate()
    acc = PB.acc_term(K, c.absdot)
    _control(f"gemm store {M}x{N}x{K}", dtype, pre, c.ref, PB.store_bound(c.ref, acc, dtype))
    f, w = PB.outside((pre.double() - c.ref).abs(), acc)
    print(f"[bound control gemm f32 {M}x{N}x{K} {PB.NAME[dtype]}] fp32 arithmetic: worst ratio {w:.3f}")
    assert f == 0.0
    ref, tol = PB.gelu_tanh_gemm_bound(c)
    _control(f"gemm gelu-tanh {M}x{N}x{K}", dtype, PB.gelu_tanh_emulate(pre), ref, tol)


def test_per_element_bounds_lose_their_edge_at_large_k():
    """Why no per-element test uses K > 256: the accumulation term swallows the difference between the two stores."""
    c = PB.GemmCase(64, 128, 4096, PB.BF16)
    tol = PB.store_bound(c.ref, PB.acc_term(4096, c.absdot), PB.BF16)
    f_tr, _ = PB.outside((PB.store_trunc(c.emulate(), PB.BF16).double() - c.ref).abs(), tol)
    print(f"[bound control gemm store K=4096 bf16] truncating: {100 * f_tr:.2f} % outside")
    assert f_tr < 0.01


@DTYPES
def test_gelu_sweep_bounds(dtype):
    M, N, K, x, w, b, pre = PB.gelu_sweep(dtype)
    assert torch.equal((x.float() @ w.float().t() + b).double(), pre)            # pre = v + bias exactly, in fp32 already
    ref = PB.gelu_tanh64(pre)
    _control("gelu-tanh sweep", dtype, PB.gelu_tanh_emulate(pre), ref, PB.gelu_tanh_bound(ref, dtype))
    ref = PB.gelu_erf64(pre)                                                      # the polynomial's own error is the kernel's: here the exact function in fp32
    _control("gelu-erf sweep", dtype, ref.float(), ref, PB.gelu_erf_bound(ref, dtype))


@DTYPES
@pytest.mark.parametrize("layout", ["spatial", "temporal"])
def test_qkv_rope_bound(layout, dtype):
    c = PB.qkv_spatial_case(dtype) if layout == "spatial" else PB.qkv_temporal_case(dtype)
    _control(f"qkv {layout}", dtype, c.emulate(), c.ref, c.tol)


@DTYPES
@pytest.mark.parametrize("B,P,D,Tq,t0,Tmax", PB.TEMPORAL_CASES)
def test_temporal_attention_bound(B, P, D, Tq, t0, Tmax, dtype):
    c = PB.temporal_case(B, P, D, Tq, t0, Tmax, dtype)
    _control(f"attn_temporal Tq={Tq} t0={t0} Tmax={Tmax} P={P}", dtype, c.emulate(), c.ref, c.tol)
    best = PB.row_rel_l2(c.ref.to(dtype).reshape(-1, 64), c.ref.reshape(-1, 64)) / (PB.TEMPORAL_TOL * PB.FACTOR[dtype])
    print(f"[bound control attn_temporal rows {PB.NAME[dtype]}] rounded fp64 reference: {best:.3f} of the per-row bound")
    assert best < 0.6


@DTYPES
@pytest.mark.parametrize("D,M", PB.LN_SHAPES)
def test_layernorm_row_bound(D, M, dtype):
    c = PB.ln_case(D, M)
    for name, ref in (("modulate", c.ref_modulate), ("affine", c.ref_affine)):
        best = PB.row_rel_l2(ref.to(dtype), ref) / (PB.LN_TOL * PB.FACTOR[dtype])
        print(f"[bound control ln_{name} D={D} M={M} {PB.NAME[dtype]}] rounded fp64 reference: {best:.3f} of the per-row bound")
        assert best < 0.6
    if D in (128, 1024):
        ref = PB.ln_large_mean_case(D)[3]
        best = PB.row_rel_l2(ref.to(dtype), ref) / (PB.LN_TOL * PB.FACTOR[dtype])
        print(f"[bound control ln_affine large mean D={D} {PB.NAME[dtype]}] rounded fp64 reference: {best:.3f} of the per-row bound")
        assert best < 0.6


@DTYPES
def test_layernorm_large_mean_needs_the_centred_difference(dtype):
    """A row of 300 +- 0.02 in fp32 arithmetic: centred as (x - K) - mean(x - K) (K = the row's first element, what both kernels do) it stays far inside the
    per-row bound; centred as x - fl(K + mean(x - K)) the mean is rounded to an ulp of 300 first, 7.6e-4 of the standard deviation at worst, and rows of the
    fp16 output leave the bound — the form the kernels had until this test's GPU twin found it."""
    x, g, b, ref = PB.ln_large_mean_case(1024)
    a = x - x[:, :1]
    m1 = a.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((a * a).mean(-1, keepdim=True) - m1 * m1).clamp_min(0) + 1e-6)
    tol = PB.LN_TOL * PB.FACTOR[dtype]
    good = PB.row_rel_l2(((a - m1) * rstd * g + b).to(dtype), ref) / tol
    bad = PB.row_rel_l2(((x - (x[:, :1] + m1)) * rstd * g + b).to(dtype), ref) / tol
    print(f"[bound control ln_affine large mean {PB.NAME[dtype]}] (x - K) - mean: {good:.3f} of the per-row bound; x - fl(K + mean): {bad:.3f}")
    assert good < 0.6
    if dtype is PB.F16:
        assert bad > 1.0


@DTYPES
@pytest.mark.parametrize("M,N,K", [(300, 256, 512), (720, 1024, 1024)])
def test_splitk_layernorm_operand_row_bound(M, N, K, dtype):
    """the operand rows of test_splitk_partials_reduced_by_layernorm: LN + modulate of the updated residual, rounded"""
    ref = PB.splitk_ln_case(M, N, K, dtype)[-1]
    best = PB.row_rel_l2(ref.to(dtype), ref) / (PB.LN_TOL * PB.FACTOR[dtype])
    print(f"[bound control splitk_ln {M}x{N}x{K} operand {PB.NAME[dtype]}] rounded fp64 reference: {best:.3f} of the per-row bound")
    assert best < 0.6


@DTYPES
@pytest.mark.parametrize("S", PB.ATTN_S)
def test_spatial_attention_row_bound(S, dtype):
    """P rounded to 2 bytes, as the one-pass and the flash kernel hold it, and the output rounded: per (item, head, query) row"""
    c = PB.attn_case(S, dtype)
    best = PB.row_rel_l2(PB.attn_rows(c.control()), PB.attn_rows(c.ref4)) / (PB.ATTN_TOL * PB.FACTOR[dtype])
    print(f"[bound control attn_spatial S={S} {PB.NAME[dtype]}] P and output rounded: {best:.3f} of the per-row bound")
    assert best < 0.6


@DTYPES
@pytest.mark.parametrize("S", [200, 576])
def test_spatial_attention_prescaled_row_bound(S, dtype):
    c = PB.attn_case(S, dtype, None, True)
    best = PB.row_rel_l2(PB.attn_rows(c.control()), PB.attn_rows(c.ref4)) / (PB.ATTN_TOL * PB.FACTOR[dtype])
    print(f"[bound control attn_spatial prescaled S={S} {PB.NAME[dtype]}] P and output rounded: {best:.3f} of the per-row bound")
    assert best < 0.6


@pytest.mark.parametrize("jump", [4.0, 0.45])
def test_spatial_attention_jump_row_bound(jump):
    """The two running-max-jump cases on bf16 operands.  A kernel that rounds P and the output stays at 0.27 of the per-row bound; one that ALSO rounds
    q * (log2 e / 8) to bf16 again (the plain-q form of the flash kernel as it was) leaves it at jump 4.0 in a row that sees the planted key of norm 32 at a
    moderate score — the figure the MI355X returned for that row was 1.005.  The dominated rows themselves stay far inside their 2e-3 x 8."""
    c = PB.attn_case(576, PB.BF16, jump)
    tol = PB.ATTN_TOL * PB.FACTOR[PB.BF16]
    best = PB.row_rel_l2(PB.attn_rows(c.control()), PB.attn_rows(c.ref4)) / tol
    again = PB.row_rel_l2(PB.attn_rows(c.control(requantized_q=True)), PB.attn_rows(c.ref4)) / tol
    print(f"[bound control attn_spatial jump {jump} bf16] P and output rounded: {best:.3f} of the per-row bound; q rounded a second time as well: {again:.3f}")
    assert best < 0.6
    if jump == 4.0:
        assert again > 1.0
    ctl = c.control()
    for (b, h, row) in c.dominated:
        assert PB.rel_l2(ctl[b, h, row], c.ref4[b, h, row]) < 0.6 * PB.ATTN_DOMINATED_TOL * PB.FACTOR[PB.BF16]
