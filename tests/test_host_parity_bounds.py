"""The bounds of tests/test_gpu_ops_typed.py, (second half) of tests/test_gpu_ops_train.py and tests/test_gpu_ops_ln_pending.py, of
tests/test_gpu_ops_attn_bwd_bounds.py and (last section) of tests/test_gpu_ops_optimizer.py, checked on the CPU (no library, no GPU): a bound is only worth asserting if a correct kernel stays inside it and a
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


# ======================================================================================================================================================
# The bounds of tests/test_gpu_ops_train.py (the backward-only training kernels).  For every bound: the fp32 emulation leaves NO element outside, and each
# wrong variant puts at least 1 % of the elements it affects outside (a per-row bound: it is exceeded in the worst affected row).
# ======================================================================================================================================================
def _inside(name, got, ref, tol):
    f, w = PB.outside((got.double() - ref).abs(), tol)
    print(f"[bound control {name}] fp32 emulation: {100 * f:.2f} % outside, worst ratio {w:.3f}")
    assert f == 0.0, (name, f, w)


def _caught(name, what, got, ref, tol, affected=None):
    err, tol = (got.double() - ref).abs(), tol.expand_as(ref) if tol.dim() else tol
    if affected is not None:
        err, tol = err[affected], tol[affected]
    f, w = PB.outside(err, tol)
    print(f"[bound control {name}] WRONG ({what}): {100 * f:.2f} % of the affected elements outside, worst ratio {w:.3g}")
    assert f >= 0.01, (name, what, f)


def _store_control(name, dtype, c_emulate, ref, tol):
    """c_emulate(store) -> the 2-byte output under the given store"""
    _inside(f"{name} {PB.NAME[dtype]}", c_emulate(PB.store_rne), ref, tol)
    _caught(f"{name} {PB.NAME[dtype]}", "truncating store", c_emulate(PB.store_trunc), ref, tol)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("D,frames,P", PB.LN_BWD_SHAPES)
def test_ln_mod_bwd_bounds(D, frames, P, accumulate):
    c = PB.ln_bwd_case(D, frames, P)
    name = f"ln_mod_bwd D={D} frames={frames} P={P} accumulate={accumulate}"
    ref, tol = c.ref_dres(accumulate), c.tol_dres(accumulate)
    dres, dshift, dscale = c.emulate(accumulate)
    _inside(name + " dres", dres, ref, tol)
    _inside(name + " dshift", dshift, c.ref_dshift, c.tol_dshift)
    _inside(name + " dscale", dscale, c.ref_dscale, c.tol_dscale)
    if frames > 1:
        later = torch.arange(c.M) >= P                                           # the rows of every frame but the first
        _caught(name + " dres", "scale row of frame 0 for every frame", c.emulate(accumulate, "scale0")[0], ref, tol, later)
    if accumulate:
        _caught(name + " dres", "accumulate ignored", c.emulate(accumulate, "noacc")[0], ref, tol)
    if D <= 1024:
        _caught(name + " dres", "variance over D - 1", c.emulate(accumulate, "var")[0], ref, tol)
    _, dshift, dscale = c.emulate(accumulate, "drop")
    _caught(name + " dshift", "last token left out", dshift, c.ref_dshift, c.tol_dshift)
    _caught(name + " dscale", "last token left out", dscale, c.ref_dscale, c.tol_dscale)


@pytest.mark.parametrize("D", [256, 1024])
def test_ln_mod_bwd_large_mean_needs_the_centred_difference(D):
    """rows of 300 +- 0.02.  Centred on the row's first element, as the kernels do it, the fp32 emulation stays inside the per-element bounds and far inside the
    per-row LN_TOL of dres and dscale.  With x - fl(mean x) the mean is off by an ulp of 300, 7.6e-4 of the standard deviation: dscale leaves both its bounds —
    the form the kernels had until the GPU twin of this test found it (dres barely moves: a constant shift of xhat meets the small means of g there)."""
    c = PB.ln_bwd_case(D, 2, 24, True)
    name = f"ln_mod_bwd large mean D={D}"
    ref = c.ref_dres(0)
    dres, dshift, dscale = c.emulate(0)
    _inside(name + " dres", dres, ref, c.tol_dres(0))
    _inside(name + " dshift", dshift, c.ref_dshift, c.tol_dshift)
    _inside(name + " dscale", dscale, c.ref_dscale, c.tol_dscale)
    good = (PB.row_rel_l2(dres, ref) / PB.LN_TOL, PB.row_rel_l2(dscale, c.ref_dscale) / PB.LN_TOL)
    pres, _, pscale = c.emulate(0, "plain")
    bad = (PB.row_rel_l2(pres, ref) / PB.LN_TOL, PB.row_rel_l2(pscale, c.ref_dscale) / PB.LN_TOL)
    print(f"[bound control {name}] of the per-row bound (dres, dscale): centred {good[0]:.2e}, {good[1]:.2e}; x - fl(mean x): {bad[0]:.3f}, {bad[1]:.3f}")
    assert max(good) < 0.6
    assert bad[1] > 1.0
    _caught(name + " dscale", "x - fl(mean x)", pscale, c.ref_dscale, c.tol_dscale)
    var = PB.row_rel_l2(c.emulate(0, "var")[0], ref) / PB.LN_TOL
    sc0 = PB.row_rel_l2(c.emulate(0, "scale0")[0][c.P:], ref[c.P:]) / PB.LN_TOL
    print(f"[bound control {name}] dres rows: variance over D - 1: {var:.3f} of the per-row bound; scale row of frame 0: {sc0:.3g}")
    assert sc0 > 1.0
    if D == 256:
        assert var > 1.0        # (D = 1024: the relative change of rstd is 1 / 2046 = 4.9e-4, inside LN_TOL — the per-element bound catches it, below)
    _caught(name + " dres", "variance over D - 1", c.emulate(0, "var")[0], ref, c.tol_dres(0))


@DTYPES
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("D,frames,P", PB.GATE_BWD_SHAPES)
def test_gate_bwd_bounds(D, frames, P, gated, dtype):
    c = PB.gate_bwd_case(D, frames, P, dtype, gated)
    name = f"gate_bwd D={D} frames={frames} P={P} gate={'yes' if gated else 'null'}"
    if gated:           # (without a gate dy is the rounded dres itself: both stores of an fp32 value are checked by the gated form)
        _store_control(name + " dy", dtype, lambda st: c.emulate(True, st)[0], c.ref_dy, c.tol_dy)
    for fused in (True, False):
        tag = f"{name} {'fused' if fused else 'unfused'} {PB.NAME[dtype]}"
        dy, dgate, db = c.emulate(fused)
        _inside(tag + " dy", dy, c.ref_dy, c.tol_dy)
        _inside(tag + " dgate", dgate, c.ref_dgate, c.tol_dgate)
        _inside(tag + " db", db, c.ref_db, c.tol_db(fused))
        _caught(tag + " db", "= in place of +=", c.emulate(fused, assign=True)[2], c.ref_db, c.tol_db(fused))
    _, dgate, db = c.emulate(True, drop=True)
    _caught(name + " dgate", "last token left out", dgate, c.ref_dgate, c.tol_dgate)
    _caught(name + " fused bias parts", "last token left out", db, c.ref_db, c.tol_db(True))


@DTYPES
@pytest.mark.parametrize("sweep", [True, False], ids=["sweep", "random"])
@pytest.mark.parametrize("M,N", PB.GELU_BWD_SHAPES)
def test_gelu_bwd_bounds(M, N, sweep, dtype):
    c = PB.gelu_bwd_case(M, N, dtype, sweep)
    name = f"gelu_bwd {M}x{N} {'sweep' if sweep else 'random'}"
    _store_control(name + " du", dtype, lambda st: c.emulate(True, st)[0], c.ref_du, c.tol_du)
    pad = PB.rand(N, seed=9)                                                     # a pad row of ordinary magnitude
    for fused in (True, False):
        tag = f"{name} {'fused' if fused else 'unfused'} {PB.NAME[dtype]}"
        _inside(tag + " db", c.emulate(fused)[1], c.ref_db, c.tol_db(fused))
        _caught(tag + " db", "one pad row included", c.emulate(fused, pad_row=pad)[1], c.ref_db, c.tol_db(fused))
        _caught(tag + " db", "= in place of +=", c.emulate(fused, assign=True)[1], c.ref_db, c.tol_db(fused))


def test_gelu_grad_reference_and_evaluation_error():
    """gelu_grad64 against torch's autograd of GELU(tanh) in fp64, and the fp32 evaluation inside gelu_grad_eval_error over the whole sweep, fp32 grid included"""
    u = torch.linspace(-9.0, 9.0, 200001, dtype=torch.float64).requires_grad_(True)
    torch.nn.functional.gelu(u, approximate="tanh").sum().backward()
    g = PB.gelu_grad64(u.detach())[0]
    assert (g - u.grad).abs().max().item() < 1e-14
    u32 = u.detach().float()
    f, w = PB.outside((PB.gelu_grad_emulate(u32).double() - PB.gelu_grad64(u32)[0]).abs(), PB.gelu_grad_eval_error(u32))
    print(f"[bound control gelu' evaluation] fp32 emulation: {100 * f:.2f} % outside, worst ratio {w:.3f}")
    assert f == 0.0


@pytest.mark.parametrize("N", PB.COLSUM_TILED_N)
@pytest.mark.parametrize("M", PB.COLSUM_TILED_M)
@DTYPES
def test_colsum_tiled_bound(M, N, dtype):
    c = PB.colsum_case(M, N, dtype, 2)
    _inside(f"colsum_tiled {M}x{N} {PB.NAME[dtype]}", c.emulate(), c.ref, c.tol)
    _caught(f"colsum_tiled {M}x{N} {PB.NAME[dtype]}", "= in place of +=", c.emulate(assign=True), c.ref, c.tol)


@pytest.mark.parametrize("N", PB.COLSUM_F32_N)
@pytest.mark.parametrize("M", PB.COLSUM_F32_M + PB.COLSUM_MULTI_SPLITS)
def test_colsum_f32_bound(M, N):
    """launch_colsum_f32 and (M = the number of splits) a job of launch_colsum_reduce_multi"""
    c = PB.colsum_case(M, N)
    _inside(f"colsum_f32 {M}x{N}", c.emulate(), c.ref, c.tol)
    _caught(f"colsum_f32 {M}x{N}", "= in place of +=", c.emulate(assign=True), c.ref, c.tol)


@DTYPES
def test_mse_bwd_patch_bound(dtype):
    for shape in PB.MSE_BWD_SHAPES:
        c = PB.mse_bwd_case(*shape, dtype)
        name = f"mse_bwd_patch {shape}"
        last = c.ref[:, -1]
        _store_control(name, dtype, lambda st: c.emulate(st)[:, -1], last, c.tol[:, -1])
        _inside(name + " all frames", c.emulate(), c.ref, c.tol)
        if shape[1] > 1:
            _caught(name, "gradient also written for the frame in front of the last", c.emulate(every_frame=True)[:, -2], c.ref[:, -2], c.tol[:, -2])


def test_silu_bounds():
    c = PB.silu_case()
    y, dx = c.emulate()
    _inside("silu", y, c.ref_y, c.tol_y)
    _inside("silu_bwd", dx, c.ref_dx, c.tol_dx)
    # the derivative without its second term, x (1 - s): what a kernel that returned dy s would give
    _caught("silu_bwd", "dy sigmoid(x) alone", c.dy * torch.sigmoid(c.x), c.ref_dx, c.tol_dx)
    assert c.emulate()[0][0, 4].item() == 0.0 and abs(c.ref_y[0, 4].item()) > 2.0 ** -126      # x = -90: the flushed value SILU_ABS exists for


@pytest.mark.parametrize("n,I,J,accumulate,mfma", [(R, N, K, True, True) for (R, N, K) in PB.GEMM_TN_F32_MFMA] + [(R, N, K, True, False) for (R, N, K, _) in PB.GEMM_TN_F32_VALU] +
                         [(N, R, K, False, False) for (R, N, K) in PB.GEMM_NN_F32] + [(MODW, R, D, False, True) for (MODW, D, R) in PB.ADA_BWD_MFMA] +
                         [(MODW, R, D, False, False) for (MODW, D, R) in PB.ADA_BWD_VALU])
def test_gemm_f32_bounds(n, I, J, accumulate, mfma):
    """gemm_tn_f32 (accumulating), gemm_nn_f32 and ada_bwd_dx at the shapes of the GPU tests"""
    c = PB.gemm_f32_case(n, I, J, accumulate, mfma)
    name = f"gemm f32 {n} terms {I}x{J}{' mfma' if mfma else ''}"
    _inside(name, c.emulate(), c.ref, c.tol)
    if accumulate:
        _caught(name, "= in place of +=", c.emulate(assign=True), c.ref, c.tol)
    # the last term of every sum left out.  The bound grows with n^2 (n + 2 roundings of a sum of n magnitudes) and one term with n: from about 8192 terms on
    # a single one disappears in it (0.21 of the bound at the 28672 of a hidden-2048 ada_bwd_dx), so there the wrong sum leaves out the last 1024 terms — one
    # split of ada_bwd_dx's workspace, the part a wrong split count loses
    k = 1 if n < 8192 else 1024
    drop = (c.a[:-k].t() @ c.b[:-k]) + (c.old if accumulate else 0.0)
    _caught(name, f"last {k} term(s) left out", drop, c.ref, c.tol)


@pytest.mark.parametrize("M,N,K,act,bias", PB.SKINNY_HOST_CASES)
def test_skinny_bounds(M, N, K, act, bias):
    """tests/test_gpu_ops.py test_skinny_f32: the kernel's chain in fp32 arithmetic (skinny_emulate) sits inside the per-element bound, with and without SiLU and
    a bias; a dropped last K chunk of 128 columns and a bias added twice leave it"""
    c = PB.skinny_case(M, N, K, act, bias)
    name = f"skinny {M}x{N}x{K} act={act}{'' if bias else ' no bias'}"
    _inside(name, PB.skinny_emulate(c.x, c.w, c.b, act), c.ref, c.tol)
    if K > 128:
        _caught(name, "the last K chunk of 128 columns left out", PB.skinny_emulate(c.x, c.w, c.b, act, "chunk"), c.ref, c.tol)
    if bias:
        _caught(name, "the bias added twice", PB.skinny_emulate(c.x, c.w, c.b, act, "bias2"), c.ref, c.tol)
    # the windows of the bit-equality check lie inside N, on multiples of 4, and hold a block boundary and the last column
    for ft in (1, 4, 8):
        w = c.windows(ft)
        assert w[0] == 0 and w[-1] == N - 64 and all(n % 4 == 0 and 0 <= n <= N - 64 for n in w)
        assert N < 64 * ft + 32 or any(n < 64 * ft < n + 64 for n in w)


@DTYPES
@pytest.mark.parametrize("S,prescaled", sorted({(s, p) for nb, h, s, p in PB.ATTN_EXTRA}))
def test_spatial_attention_extra_row_bound(S, prescaled, dtype):
    """the sequence lengths of PB.ATTN_EXTRA (the instantiations the 2 x 3 cases of ATTN_S do not select), at 2 x 3 items: P and the output rounded"""
    c = PB.attn_case(S, dtype, None, bool(prescaled))
    best = PB.row_rel_l2(PB.attn_rows(c.control()), PB.attn_rows(c.ref4)) / (PB.ATTN_TOL * PB.FACTOR[dtype])
    print(f"[bound control attn_spatial{' prescaled' if prescaled else ''} S={S} {PB.NAME[dtype]}] P and output rounded: {best:.3f} of the per-row bound")
    assert best < 0.6


# ---- the deferred-residual LayerNorm (tests/test_gpu_ops_ln_pending.py) ------------------------------------------------------------------------------------
def _ln_pend_margins(c, dtype, wrong=None):
    """(worst ratio of bound 1, worst row / global relative L2 as a fraction of bound 3) of the fp32 emulation; the operand is read back through the DOCUMENTED
    output row order, as the GPU test reads the kernel's"""
    v, out = c.emulate(dtype, wrong)
    w1 = PB.outside((v.double() - c.ref_new).abs(), c.tol_new)[1] if c.nsplit else 0.0
    nat, tol = out[c.out_rows()], PB.LN_TOL * PB.FACTOR[dtype]
    return w1, max(PB.row_rel_l2(nat, c.ref_operand), PB.rel_l2(nat, c.ref_operand)) / tol


@DTYPES
@pytest.mark.parametrize("name", list(PB.LN_PEND_CASES))
def test_ln_pending_emulation_is_inside(name, dtype):
    c = PB.ln_pend_case(name)
    w1, w3 = _ln_pend_margins(c, dtype)
    print(f"[bound control ln_pending {name} {PB.NAME[dtype]}] fp32 emulation: residual {w1:.3f} of bound 1, operand {w3:.3f} of bound 3")
    assert w1 <= 1.0 and w3 < 1.0
    # the branch image is a clamped round to nearest of a sum the bound of assertion 1 also covers (without gate and residual)
    if c.nsplit:
        y64 = c.slabs[:, :, :c.D].double().sum(0) + (c.bias.double() if c.bias is not None else 0.0)
        assert (c.y_save(dtype).double() - y64).abs().max() <= 2 * PB.U[dtype] * y64.abs().max()


@DTYPES
@pytest.mark.parametrize("wrong", PB.LN_PEND_WRONG)
def test_ln_pending_wrong_variants_are_outside(wrong, dtype):
    """every wrong variant leaves bound 1 or bound 3 on at least one case; `caught` names them"""
    caught = []
    for name in PB.LN_PEND_CASES:
        w1, w3 = _ln_pend_margins(PB.ln_pend_case(name), dtype, wrong)
        if w1 > 1.0 or w3 >= 1.0:
            caught.append(f"{name} ({w1:.3g} / {w3:.3g})")
    print(f"[bound control ln_pending {PB.NAME[dtype]}] WRONG ({wrong}) outside on: {', '.join(caught) or 'nothing'}")
    assert caught, wrong
    # and each where it should be: a slab added again only where the load chunk has an unused slot, the exchanged permutation only where P > 16
    expect = {"again": {"d256_rows", "d1280", "d1280_tperm"}, "tperm": {"d256_tperm", "d1280_tperm"}}.get(wrong)
    if expect:
        assert {s.split()[0] for s in caught} == expect, caught


def test_ln_pending_saturating_branch_image():
    c = PB.ln_pend_sat_case()
    y16, ybf = c.y_save(PB.F16), c.y_save(PB.BF16)
    assert y16[3, 5].item() == PB.F16_MAX and y16[6, 60].item() == -PB.F16_MAX and torch.isfinite(y16.float()).all()
    assert ybf[3, 5].item() == 79872.0 and ybf[6, 60].item() == -70144.0                   # bf16's grid around 80000 / 70000.5 has steps of 512
    assert (c.branch32().abs() > PB.F16_MAX).sum().item() == 2


# ======================================================================================================================================================
# The bounds of tests/test_gpu_ops_attn_bwd_bounds.py (the four attention backward kernels).  For every case of the GPU file: "what a perfect kernel of the
# design returns" (fp64 math with exactly the design's 2-byte roundings: P, dS and the outputs for the spatial pair, the outputs only for the temporal pair) has
# NO element outside the bound, and every wrong kernel of tests/parity_bounds.py's list puts at least one element of dq / dk / dv outside.  A truncating output
# store and a truncated dS are PRINTED for the spatial pair and not required caught (P and dS are rounded to 2 bytes by design, so the bound carries u-sized
# terms of its own: the limit stated in the head comment there); the temporal bound has no such term and must catch the truncating store.
# ======================================================================================================================================================
ATTN_BWD_CASES = [(s, k, 0) for s in PB.ATTN_BWD_SHAPES for k in PB.ATTN_BWD_KINDS] + \
                 [(s, k, e) for s in PB.ATTN_BWD_SCALED_SHAPES for k in PB.ATTN_BWD_KINDS for e in PB.ATTN_BWD_SCALES]
ATTN_BWD_IDS = [f"{s[0]}x{s[1]}x{s[2]}-{k}-2^{e}" for s, k, e in ATTN_BWD_CASES]
TEMPORAL_BWD_CASES = [(s, k) for s in PB.TEMPORAL_BWD_SHAPES for k in PB.TEMPORAL_BWD_KINDS]
TEMPORAL_BWD_IDS = ["x".join(map(str, s)) + "-" + k for s, k in TEMPORAL_BWD_CASES]
THIRDS = ("dq", "dk", "dv")


def _thirds(c, got):
    """worst ratio error / bound of dq, dk, dv"""
    r = (got.double() - c.ref).abs() / c.tol
    D = r.shape[1] // 3
    return [r[:, i * D:(i + 1) * D].max().item() for i in range(3)]


def _fmt(w):
    return " ".join(f"{n} {x:.3g}" for n, x in zip(THIRDS, w))


@DTYPES
@pytest.mark.parametrize("shape,kind,e", ATTN_BWD_CASES, ids=ATTN_BWD_IDS)
def test_attn_spatial_bwd_control_is_inside(shape, kind, e, dtype):
    c = PB.attn_bwd_case(*shape, kind, e, dtype)
    name = f"attn_spatial_bwd {shape} {kind} dO x 2^{e} {PB.NAME[dtype]}"
    w = _thirds(c, c.control())
    print(f"[bound control {name}] perfect kernel of the design: worst ratio {_fmt(w)}")
    assert max(w) <= 1.0, (name, w)
    assert c.peak < 0.25 * (PB.F16_MAX if dtype is PB.F16 else 3.3895313892515355e38), (name, c.peak)      # the GPU test expects a clear error word here
    print(f"[bound control {name}] not required caught: truncating store {_fmt(_thirds(c, c.control(store=PB.store_trunc)))}; "
          f"truncated dS {_fmt(_thirds(c, c.control(trunc_ds=True)))}")
    if kind == "sharp" and e == 0 and shape[2] >= 32:
        assert 0.4 < c.pmax_median < 0.9, c.pmax_median                # peaked rows: the largest probability of a row has a median of about 0.65
    if kind == "flat" and shape[2] == 144:
        assert c.pmax_median < 0.1


@DTYPES
@pytest.mark.parametrize("shape,kind", [(s, k) for s in PB.ATTN_BWD_SHAPES if s[2] <= PB.ATTN_BWD_MUTANT_MAX_S for k in PB.ATTN_BWD_KINDS],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_attn_spatial_bwd_wrong_kernels_are_outside(shape, kind, dtype):
    c = PB.attn_bwd_case(*shape, kind, 0, dtype)
    wrongs = ["drop_last", "rope_sign"] + (["stale_max", "dq_chunk"] if shape[2] > 64 else [])
    for wrong in wrongs:
        w = _thirds(c, c.control(wrong))
        print(f"[bound control attn_spatial_bwd {shape} {kind} {PB.NAME[dtype]}] WRONG ({wrong}): worst ratio {_fmt(w)}")
        assert max(w) > 1.0, (wrong, w)
        if wrong == "rope_sign":
            assert min(w[:2]) > 1.0 and w[2] <= 1.0, w            # dq AND dk, and only they


@DTYPES
@pytest.mark.parametrize("shape,kind", TEMPORAL_BWD_CASES, ids=TEMPORAL_BWD_IDS)
def test_attn_temporal_bwd_control_and_wrong_kernels(shape, kind, dtype):
    """T = 1 has P = 1, dS = 0 and dq = dk = 0 identically: no statistic, mask or rotation can be wrong there, so the wrong kernels start at T = 5."""
    c = PB.temporal_bwd_case(*shape, kind, dtype)
    T = shape[3]
    name = f"attn_temporal_bwd {shape} {kind} {PB.NAME[dtype]}"
    w = _thirds(c, c.control())
    print(f"[bound control {name}] perfect kernel of the design: worst ratio {_fmt(w)}")
    assert max(w) <= 1.0, (name, w)
    assert c.peak < 0.25 * PB.F16_MAX
    if T == 1:                                                      # (dv = dO there, a 2-byte value already: no store can round it wrongly either)
        assert max(w) == 0.0
        return
    w = _thirds(c, c.control(store=PB.store_trunc))
    print(f"[bound control {name}] WRONG (truncating store): worst ratio {_fmt(w)}")
    # P and dS stay fp32, the store's u |ref| is the bound's only 2-byte term: dv leaves it in every case.  (dq / dk of a peaked row are sums of dS ~ 0 that cancel:
    # there the fp32 terms of the bound outweigh u |ref|, and the truncation stays inside — 0.65 on `sharp` fp16 dq.)
    # (One case of 2304 elements holds no dv element that shows it: `sharp` at T = 3 in fp16, 0.975 of the bound as printed; its bf16 twin and the four other kinds at
    # T = 3 do.)
    if not (T == 3 and kind == "sharp" and dtype is PB.F16):
        assert w[2] > 1.0, w
    for wrong in ["drop_last", "rope_sign", "mask_plus", "mask_minus"] + (["stale_max"] if kind == "ladder" else []):
        w = _thirds(c, c.control(wrong))
        print(f"[bound control {name}] WRONG ({wrong}): worst ratio {_fmt(w)}")
        if kind == "diagonal" and T <= 8 and wrong in ("rope_sign", "mask_plus"):
            # k_t = 3 q_t puts the own frame 24 above every other score (sd 3): with so few keys every other probability is e^-15 at most, dS, dq and dk are
            # next to zero in fp64 already, and neither a rotation of them nor one more key of that weight moves anything by as much as the bound (printed
            # above: 0.03 .. 0.15 of it).  Both are caught on `diagonal` from T = 9 on, where some off-diagonal score comes close enough.
            continue
        if kind == "first" and T == 2 and wrong == "drop_last":
            # two frames, key 0 far above key 1: the only last key that can be dropped is key 1 of query 1, whose probability is next to zero in fp64 already
            # (0.50 .. 0.91 of the bound, printed above).  `first` shows a dropped last key from T = 3 on, the four other kinds at T = 2 as well.
            continue
        assert max(w) > 1.0, (wrong, w)


@pytest.mark.parametrize("shape", PB.ATTN_BWD_SAT, ids=lambda s: "x".join(map(str, s)))
def test_attn_spatial_bwd_saturation_preconditions(shape):
    """fp16, sharp, dO x 2^13: some output leaves fp16 while dS stays far inside — what the GPU test's ERR_F16_SAT case needs of its inputs.  The perfect kernel
    (clamped stores) stays inside the bound of the clamped reference: clamping cannot increase an error."""
    c = PB.attn_bwd_case(*shape, "sharp", PB.ATTN_BWD_SAT_SCALE, PB.F16)
    D = c.ref.shape[1] // 3
    peaks = [c.ref[:, i * D:(i + 1) * D].abs().max().item() for i in range(3)]
    print(f"[bound control attn_spatial_bwd saturation {shape}] fp64 max |dS| {c.max_ds:.4g}, max |dq| |dk| |dv| {_fmt(peaks)}")
    assert max(peaks) > PB.F16_MAX and c.max_ds < 0.25 * PB.F16_MAX
    got = c.control()
    assert torch.isfinite(got.float()).all()
    f, w = PB.outside((got.double() - c.ref.clamp(-PB.F16_MAX, PB.F16_MAX)).abs(), c.tol)
    print(f"[bound control attn_spatial_bwd saturation {shape}] perfect kernel against the clamped reference: worst ratio {w:.3f}")
    assert f == 0.0


# ======================================================================================================================================================
# The bounds of tests/test_gpu_ops_optimizer.py (sumsq_kernel, clip_coef_kernel, adamw_multi_kernel).  "The kernel as designed" is a float32 emulation of the
# source's arithmetic (tests/parity_bounds.py adam_emulate, SumsqCase.emulate, ClipCase.emulate), run with every product the source leaves to the compiler
# rounded on its own AND fused into the following sum, and with a powf that is exact, 2 ulp low and 2 ulp high: all of them inside every bound at every case
# the GPU file runs.  Every wrong kernel of the issue's list is outside on at least one element of at least one case; the cases that cannot show one are named.
# ======================================================================================================================================================
ADAM_CASES = [(s, c, st) for s in PB.ADAM_SETTINGS for c in PB.ADAM_COEFS for st in PB.ADAM_STARTS]
ADAM_IDS = [f"{s}-{c}-{st}" for s, c, st in ADAM_CASES]


def _ratio(got, ref, tol):
    """worst |got - ref| / tol; a non-finite result is outside whatever the bound"""
    r = (got.double() - ref).abs() / tol
    return torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf"))).max().item()


def _adam_coef(c):
    """ctl[1] as clip_coef_kernel forms it in fp32 from a correctly rounded norm"""
    import numpy as np
    inv, norm = np.float32(PB.ADAM_INV_SCALE), np.float32(c.norm64)
    return float(inv) if c.max_norm == 0.0 else float(inv * min(np.float32(1.0), np.float32(c.max_norm) / (norm + np.float32(1e-6))))


def _adam_step(c, state, coef, t, **kw):
    """one emulated launch from `state` (w, m, v per parameter) -> (new state, worst ratio per output against the reference of the same inputs)"""
    out, worst = [], {"w": 0.0, "m": 0.0, "v": 0.0}
    for p, g, (w0, m0, v0) in zip(c.params, c.g, state):
        r = PB.adam_reference(w0, g, m0, v0, coef, t, c.lr, c.wd)
        got = PB.adam_emulate(w0, g, m0, v0, coef, t, c.lr, c.wd, is_f32=not p.gemm, **kw)
        for k, x in zip("wmv", got):
            worst[k] = max(worst[k], _ratio(x, r[k], r["tol_" + k]))
        out.append(got)
    return out, worst


@pytest.mark.parametrize("setting,coef_kind,start", ADAM_CASES, ids=ADAM_IDS)
def test_adam_emulation_is_inside_the_bound(setting, coef_kind, start):
    c = PB.adam_case(setting, coef_kind, start)
    coef = _adam_coef(c)
    assert (coef == PB.ADAM_INV_SCALE) == (coef_kind == "unclipped") and 0.85 * PB.ADAM_INV_SCALE < coef
    gc = torch.cat([g.reshape(-1) for g in c.g]).double().abs() * coef
    assert gc[gc > 0].min() < 1e-12 and gc.max() > 1e2 and (gc == 0).any() and ((gc > PB.ADAM_EPS / 10 ** 0.5) & (gc < PB.ADAM_EPS * 10 ** 0.5)).sum() > 0.1 * gc.numel()
    for contract in (False, True):
        for ulps in (-PB.POWF_ULPS, 0, PB.POWF_ULPS):
            state = list(zip(c.w0, c.m0, c.v0))
            for t in c.steps:
                e0 = [PB.ema_emulate(e, s[0], 0.999) for e, s in zip(c.e0, state)]                 # (mode 1's shadow: any e0, the master of the step before)
                state, worst = _adam_step(c, state, coef, t, contract=contract, pow_ulps=ulps)
                we = max(_ratio(PB.ema_emulate(e, s[0], 0.999), 0.999 * e.double() + (1.0 - PB.f32(0.999)) * s[0].double() + (PB.f32(0.999) - 0.999) * e.double(),
                                PB.ema_step_bound(e, s[0])) for e, s in zip(e0, state))
                print(f"[bound control adamw {setting} {coef_kind} t={t} contraction {'on' if contract else 'off'} powf {ulps:+d} ulp] kernel as designed: worst ratio "
                      f"w {worst['w']:.3f} m {worst['m']:.3f} v {worst['v']:.3f} e {we:.3f}")
                assert max(worst.values()) <= 1.0 and we <= 1.0, (t, contract, ulps, worst, we)


def _adam_cannot_show(wrong, setting, coef_kind, start):
    """The cases in which a wrong kernel computes what the design computes, or differs by less than the design's own fp32 rounding allows:
      m_unclipped   without clipping the coefficient IS inv_scale
      no_decay_f32, decay_after   wd = 0: there is no decay to misplace
      decay_after   a fresh start: the misplaced decay moves the update by lr wd = 1e-5 of itself, and at t = 1 the fp32 bias correction 1 - powf(0.999, 1) alone
                    is allowed 2 ulp of 0.999 in 0.001, which is 6e-5 of the update
      bc_t_minus_1, no_sqrt_bc2   t = 100000: 0.999^t is below 1e-43, both corrections are 1 for either t, and so is the square root"""
    return (wrong == "m_unclipped" and coef_kind == "unclipped") or (wrong in ("no_decay_f32", "decay_after") and setting == "nowd") or \
           (wrong == "decay_after" and start == "fresh") or (wrong in ("bc_t_minus_1", "no_sqrt_bc2") and start == 100000)


@pytest.mark.parametrize("setting,coef_kind,start", ADAM_CASES, ids=ADAM_IDS)
def test_adam_wrong_kernels_are_outside(setting, coef_kind, start):
    c = PB.adam_case(setting, coef_kind, start)
    coef = _adam_coef(c)
    state = list(zip(c.w0, c.m0, c.v0))
    for wrong in PB.ADAM_WRONG:
        _, worst = _adam_step(c, state, coef, c.steps[0], contract=False, wrong=wrong)
        print(f"[bound control adamw {setting} {coef_kind} {start}] WRONG ({wrong}): worst ratio w {worst['w']:.3g} m {worst['m']:.3g} v {worst['v']:.3g}")
        assert (max(worst.values()) > 1.0) != _adam_cannot_show(wrong, setting, coef_kind, start), (wrong, worst)


def test_adam_every_wrong_kernel_is_shown_somewhere():
    for wrong in PB.ADAM_WRONG:
        assert any(not _adam_cannot_show(wrong, *case) for case in ADAM_CASES), wrong


def test_adam_probe_is_one_set_of_values():
    """what "one arithmetic" of the GPU file relies on: the interior tile, the element-wise tile and the fp32 run hold the same inputs"""
    c = PB.adam_case("base", "clipped", 1000)
    for lst in (c.w0, c.g, c.m0, c.v0, c.e0):
        a = c.probe(lst, "interior")
        assert a.numel() == 1024 and torch.equal(a, c.probe(lst, "edge")) and torch.equal(a, c.probe(lst, "run")) and a.abs().max() > 0
    assert [p.kind for p in c.params].count("f32_strided") == 1 and sum(not p.has_wT and p.gemm for p in c.params) == 1


@pytest.mark.parametrize("n", PB.SUMSQ_N)
def test_sumsq_emulation_and_dropped_tail(n):
    """n % 4 == 0 has no tail to drop or repeat; elsewhere a tail term shows when it is more than sumsq_depth(n) 2^-24 of the sum — always at n < 4 (the sum IS the
    tail), by the draw of the values at the larger n (printed)."""
    c = PB.sumsq_case(n)
    for contract in (False, True):
        w = abs(c.emulate(contract) - c.ref) / c.tol
        print(f"[bound control sumsq n={n} contraction {'on' if contract else 'off'}] kernel as designed: worst ratio {w:.3f} (chain of {PB.sumsq_depth(n)})")
        assert w <= 1.0
    for wrong in ("tail_dropped", "tail_twice"):
        w = abs(c.emulate(wrong=wrong) - c.ref) / c.tol
        print(f"[bound control sumsq n={n}] WRONG ({wrong}): ratio {w:.3g}")
        if n < 4:
            assert w > 1.0, (wrong, w)
        if n % 4 == 0:
            assert c.emulate(wrong=wrong) == c.emulate()


@pytest.mark.parametrize("name", list(PB.CLIP_CASES))
def test_clip_coefficient_bound(name):
    """norm + 1e-6 replaced by norm: within the fp32 range it shows where the norm is small — `small norm` (1e-3, a part in a thousand).  At the training-sized norms
    of the other clipped cases 1e-6 is a part in a million of the norm, about twice their bound: printed, not required."""
    c = PB.CLIP_CASES[name]
    if c.skip:
        assert c.err_in is None or c.err_in & PB.ClipCase.OTHER_BIT
        return
    got = c.emulate()
    if not c.clipped:
        assert got == c.coef == c.inv_scale
        return
    w, ww = abs(got - c.coef) / c.coef_tol, abs(c.emulate("no_1e-6") - c.coef) / c.coef_tol
    print(f"[bound control clip_coef {name}] kernel as designed: ratio {w:.3f}; WRONG (norm + 1e-6 -> norm): ratio {ww:.3g}")
    assert w <= 1.0
    if name == "small norm":
        assert ww > 100.0
