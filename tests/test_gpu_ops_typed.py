"""Kernel-level parity of the operand-typed kernels in BOTH operand types (GPU): the fp16 objects and their bf16 twins (gemm / attention / elementwise / train
compiled with f16 = __bf16), through the C-ABI (gtav_op_*) with the test hook gtav_op_set_operand_dtype (include/gtav_amd_testing.h).

References are fp64 math on the SAME 2-byte-rounded operands.  Operands are laid out on the host (helpers.to_tiled: torch's rounding + tiled_index), so no test
of a twin passes its inputs through the convert_pad twin.  The bounds — per element wherever the kernel rounds once, per row and global elsewhere — are derived
in tests/parity_bounds.py and checked against fp32 emulations with a correct and with a truncating store in tests/test_host_parity_bounds.py; none is taken
from what the kernels return.  `pytest -s` prints, per case, the worst ratio error / bound (profiles/op_parity_typed/margins.txt is such a printout)."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import parity_bounds as PB  # noqa: E402
from helpers import assert_declared_plan, dev, stream, tiled_index, to_tiled, untile_typed  # noqa: E402
from gtav_amd import lib as L  # noqa: E402

F16, BF16 = PB.F16, PB.BF16
DTYPES = pytest.mark.parametrize("dtype", PB.DTYPES, ids=[PB.NAME[d] for d in PB.DTYPES])
EPI_F32, EPI_F16, EPI_GELU_TANH, EPI_GELU_ERF, EPI_RESID, EPI_PARTIAL, EPI_F16_TILED = 0, 1, 2, 3, 4, 6, 7


@pytest.fixture(autouse=True)
def _restore_hooks():
    yield
    lib = L.load()
    lib.gtav_op_set_operand_dtype(0)
    lib.gtav_op_gemm_set_wm(0)
    lib.gtav_op_gemm_set_stages(0)


def _use(dtype):
    L.load().gtav_op_set_operand_dtype(1 if dtype is BF16 else 0)
    return L.load()


def _up(n, m):
    return (n + m - 1) // m * m


def _within(name, dtype, got, ref, tol):
    """per-element bound: prints and asserts the worst ratio |got - ref| / tol"""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), name
    frac, worst = PB.outside((got - ref).abs(), tol)
    print(f"[margin {name} {PB.NAME[dtype]}] per element: worst error / bound {worst:.3f}")
    assert worst <= 1.0, (name, PB.NAME[dtype], worst, frac)
    return worst


def _rel(name, dtype, got, ref, tol, rows=None):
    """global (and, with rows = the row length, per-row) relative L2"""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), name
    e = PB.rel_l2(got, ref)
    msg = f"[margin {name} {PB.NAME[dtype]}] rel-L2 {e:.3e} = {e / tol:.3f} of the bound"
    er = None
    if rows:
        er = PB.row_rel_l2(got.reshape(-1, rows), ref.reshape(-1, rows))
        msg += f"; worst row {er:.3e} = {er / tol:.3f}"
    print(msg)
    assert e < tol, (name, PB.NAME[dtype], e, tol)
    if rows:
        assert er < tol, (name, PB.NAME[dtype], "row", er, tol)


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), device=dev(), dtype=dtype)


def _gemm(lib, xd, wd, bias, out, ldo, M, N, K, epi, gate=None, gate_stride=0, rows_per_gate=1):
    L.check(lib.gtav_op_gemm_f16(xd.data_ptr(), K, wd.data_ptr(), L.ptr(bias), out.data_ptr(), ldo, M, N, K, epi, L.ptr(gate), gate_stride, rows_per_gate, stream()))


class _Operands:
    """device images of a PB.GemmCase, built on the host"""

    def __init__(self, c):
        self.xd, self.wd, self.bd = to_tiled(c.x, c.dtype), to_tiled(c.w, c.dtype), c.b.to(dev())


def _tiled_out(lib, c, ops, epi, bias=True):
    """a tile-major 2-byte epilogue (GELU / EPI_F16_TILED) into a NaN-filled image with one spare row tile -> (the M x N values, the whole buffer)"""
    M, N, K = c.M, c.N, c.K
    ldo = _up(N, 64)
    buf = _nan((_up(M, 128) + 128, ldo), c.dtype)
    _gemm(lib, ops.xd, ops.wd, ops.bd if bias else None, buf, ldo, M, N, K, epi)
    torch.cuda.synchronize()
    assert torch.isnan(buf[_up(M, 128):]).all(), "the row tile behind the last one was written"
    return untile_typed(buf, M, ldo)[:, :N], buf


# ---- a. GEMM stores, per element, on the heuristic's own shape -------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("M,N,K", PB.GEMM_STORE_SHAPES)
def test_gemm_epilogues_per_element(M, N, K, dtype):
    """EPI_F32 / EPI_RESID (gated and plain) / EPI_PARTIAL (1 and, where K allows, 4 slices): the accumulation term.  EPI_F16 / EPI_F16_TILED: the store bound.
    Outputs are NaN-filled with a leading dimension wider than N and spare rows: nothing at or beyond row M or column N of a row-major output may be written."""
    lib = _use(dtype)
    c = PB.gemm_case(M, N, K, dtype)
    ops = _Operands(c)
    acc = PB.acc_term(K, c.absdot)
    ldo, pad = N + 8, 8
    tag = f"gemm {M}x{N}x{K}"
    out = _nan((M + pad, ldo), torch.float32)
    _gemm(lib, ops.xd, ops.wd, ops.bd, out, ldo, M, N, K, EPI_F32)
    assert torch.isnan(out[M:]).all() and torch.isnan(out[:, N:]).all()
    _within(tag + " EPI_F32", dtype, out[:M, :N], c.ref, acc)
    out = _nan((M + pad, ldo), dtype)
    _gemm(lib, ops.xd, ops.wd, ops.bd, out, ldo, M, N, K, EPI_F16)
    assert torch.isnan(out[M:]).all() and torch.isnan(out[:, N:]).all()
    _within(tag + " EPI_F16", dtype, out[:M, :N], c.ref, PB.store_bound(c.ref, acc, dtype))
    got, _ = _tiled_out(lib, c, ops, EPI_F16_TILED)
    _within(tag + " EPI_F16_TILED", dtype, got, c.ref, PB.store_bound(c.ref, acc, dtype))
    # EPI_RESID: resid += gate[row / P] * (acc + bias); fl(r + fl(g fl(y))) adds two roundings, 2^-24 (2 |g| absdot + |r|) at most, to |g| times the dot
    # product's error — inside 2 (K + 2) 2^-24 (|g| absdot + |r|), whose doubling alone leaves (K + 2) of them spare
    P = max(d for d in range(1, 51) if M % d == 0)
    resid, gate = PB.rand(M, N, seed=4), PB.rand(M // P, N, seed=5)
    for name, g in (("gated", gate), ("plain", None)):
        r = _nan((M + pad, ldo), torch.float32)
        r[:M, :N] = resid.to(dev())
        gd = g.to(dev()) if g is not None else None
        _gemm(lib, ops.xd, ops.wd, ops.bd, r, ldo, M, N, K, EPI_RESID, gd, N if g is not None else 0, P if g is not None else 1)
        assert torch.isnan(r[M:]).all() and torch.isnan(r[:, N:]).all()
        g64 = g.double().repeat_interleave(P, 0) if g is not None else torch.ones(M, N, dtype=torch.float64)
        _within(f"{tag} EPI_RESID {name}", dtype, r[:M, :N], resid.double() + g64 * c.ref, PB.acc_term(K, g64.abs() * c.absdot + resid.double().abs()))
    for sk in (1, 4):
        if (K // 64) % sk:
            continue                                            # the slices are whole K tiles: 4 of them need K = 256
        parts = _nan((sk * M * N + 8 * N,), torch.float32)
        _gemm(lib, ops.xd, ops.wd, None, parts, N, M, N, K, EPI_PARTIAL, None, sk, 1)    # the split-K factor travels in gate_stride
        assert torch.isnan(parts[sk * M * N:]).all()
        slabs = parts[:sk * M * N].reshape(sk, M, N).double().cpu()
        Kc = K // sk
        for s in range(sk):
            xs, ws = c.x[:, s * Kc:(s + 1) * Kc].double(), c.w[:, s * Kc:(s + 1) * Kc].double()
            _within(f"{tag} EPI_PARTIAL slice {s} of {sk}", dtype, slabs[s], xs @ ws.t(), PB.acc_term(Kc, xs.abs() @ ws.abs().t()))


@DTYPES
def test_gelu_epilogues_sweep(dtype):
    """The sweep of test_gelu_erf_epilogue_absolute_error (one non-zero operand per row, pre = v + bias exactly) through both GELU epilogues."""
    lib = _use(dtype)
    M, N, K, x, w, b, pre = PB.gelu_sweep(dtype)
    xd, wd, bd = to_tiled(x, dtype), to_tiled(w, dtype), b.to(dev())
    for epi, name, ref in ((EPI_GELU_TANH, "EPI_GELU_TANH", PB.gelu_tanh64(pre)), (EPI_GELU_ERF, "EPI_GELU_ERF", PB.gelu_erf64(pre))):
        tol = PB.gelu_tanh_bound(ref, dtype) if epi == EPI_GELU_TANH else PB.gelu_erf_bound(ref, dtype)
        buf = _nan((_up(M, 128) + 128, N), dtype)
        _gemm(lib, xd, wd, bd, buf, N, M, N, K, epi)
        assert torch.isnan(buf[_up(M, 128):]).all()
        _within(f"sweep {name}", dtype, untile_typed(buf, M, N), ref, tol)


# ---- c. QKV + RoPE scatter -----------------------------------------------------------------------------------------------------------------------------------
def _rope_table(lib, c):
    cd = c.cos.repeat_interleave(2, dim=-1).contiguous().to(dev())      # each frequency twice (rotary_embedding_torch.py:337), as the product passes them
    sd = c.sin.repeat_interleave(2, dim=-1).contiguous().to(dev())
    cs = torch.empty_like(cd)
    L.check(lib.gtav_op_rope_interleave(cd.data_ptr(), sd.data_ptr(), cs.data_ptr(), c.cos.shape[0], stream()))
    return cs


def _qkv_spatial(dtype, tag=""):
    lib = _use(dtype)
    g, c = PB.QKV_SPATIAL, PB.qkv_spatial_case(dtype)
    NB, S, D = g["NB"], g["S"], g["D"]
    heads, M = D // 64, NB * S
    q = torch.zeros(NB, heads, S, 64, device=dev(), dtype=dtype)
    k = torch.zeros_like(q)
    vt = torch.zeros(NB, heads, 64, S, device=dev(), dtype=dtype)
    xd, wd, bd, cs = to_tiled(c.x, dtype), to_tiled(c.w, dtype), c.b.to(dev()), _rope_table(lib, c)
    L.check(lib.gtav_op_gemm_qkv(xd.data_ptr(), D, wd.data_ptr(), bd.data_ptr(), M, D, 0, q.data_ptr(), k.data_ptr(), vt.data_ptr(), S, 0, 0, 0, cs.data_ptr(), stream()))
    for name, part, got in (("q", 0, q), ("k", 1, k), ("v^T", 2, vt)):
        lay = lambda t: t[:, part * D:(part + 1) * D].reshape(NB, S, heads, 64).permute(0, 2, 1, 3) if part < 2 else \
            t[:, part * D:(part + 1) * D].reshape(NB, S, heads, 64).permute(0, 2, 3, 1)
        _within(f"qkv spatial {name}{tag}", dtype, got, lay(c.ref), lay(c.tol))


def _qkv_temporal(dtype, tag=""):
    lib = _use(dtype)
    g, c = PB.QKV_TEMPORAL, PB.qkv_temporal_case(dtype)
    B, Tq, t0, Tmax, P, D = (g[n] for n in ("B", "Tq", "t0", "Tmax", "P", "D"))
    M = B * Tq * P
    q = torch.zeros(M, D, device=dev(), dtype=dtype)
    kv = torch.zeros(B, Tmax, P, 2, D, device=dev(), dtype=dtype)
    xd, wd, cs = to_tiled(c.x, dtype), to_tiled(c.w, dtype), _rope_table(lib, c)
    L.check(lib.gtav_op_gemm_qkv(xd.data_ptr(), D, wd.data_ptr(), 0, M, D, 1, q.data_ptr(), kv.data_ptr(), kv.data_ptr(), P, Tq, t0, Tmax, cs.data_ptr(), stream()))
    _within(f"qkv temporal q{tag}", dtype, q, c.ref[:, :D], c.tol[:, :D])
    for name, part in (("k", 1), ("v", 2)):
        lay = lambda t: t[:, part * D:(part + 1) * D].reshape(B, Tq, P, D)
        _within(f"qkv temporal {name}{tag}", dtype, kv[:, t0:t0 + Tq, :, part - 1], lay(c.ref), lay(c.tol))
    kvc = kv.cpu().view(torch.int16)
    assert (kvc[:, :t0] == 0).all() and (kvc[:, t0 + Tq:] == 0).all(), "cache slots outside the launch's frames were written"


@DTYPES
def test_qkv_spatial_layout_and_rope(dtype):
    _qkv_spatial(dtype)


@DTYPES
def test_qkv_temporal_layout(dtype):
    _qkv_temporal(dtype)


# ---- b. every product block shape ---------------------------------------------------------------------------------------------------------------------------
BLOCK_SHAPES = [(2, 2), (2, 4), (3, 2), (3, 4)] + [(s, 0) for s in (7, 11, 12, 13, 14, 20, 24, 26, 29, 31)]     # (shape, forced ring depth)


def _shape_case(lib, c, shape, tag):
    """EPI_F32 (shape 31: its fp32 output, the full-K slab of EPI_PARTIAL) and EPI_GELU_TANH of one case under the forced shape -> the GELU buffer"""
    M, N, K, dtype = c.M, c.N, c.K, c.dtype
    ops = _Operands(c)
    out = _nan((M + 8, N), torch.float32)
    if shape == 31:       # the persistent loader-wave kernel has the GELU, slab, residual and tile-major epilogues only
        _gemm(lib, ops.xd, ops.wd, None, out, N, M, N, K, EPI_PARTIAL, None, 1, 1)
        ref, acc = c.ref_nb, PB.acc_term(K, c.absdot_nb)
    else:
        _gemm(lib, ops.xd, ops.wd, ops.bd, out, N, M, N, K, EPI_F32)
        ref, acc = c.ref, PB.acc_term(K, c.absdot)
    assert torch.isnan(out[M:]).all()
    _rel(f"{tag} {M}x{N}x{K} f32", dtype, out[:M], ref, 2e-5)
    _within(f"{tag} {M}x{N}x{K} f32", dtype, out[:M], ref, acc)
    got, buf = _tiled_out(lib, c, ops, EPI_GELU_TANH)
    gref, gtol = PB.gelu_tanh_gemm_bound(c)
    _within(f"{tag} {M}x{N}x{K} EPI_GELU_TANH", dtype, got, gref, gtol)
    return ops, buf


@DTYPES
@pytest.mark.parametrize("shape,ns", BLOCK_SHAPES, ids=[f"shape{s}" + (f"-ring{n}" if n else "") for s, n in BLOCK_SHAPES])
def test_every_block_shape(shape, ns, dtype):
    """gtav_op_gemm_set_wm / _set_stages reach the twin: every block shape of the product, forced, on ragged token and feature edges, one to four K steps, one
    and several row tiles — all at K <= 256, where the per-element bounds still tell a truncating store from a rounding one.
    What this test does NOT prove by its numbers is that the forced shape reached the twin: shapes 2 .. 29 return the same bits, so a launch that fell back to
    the heuristic's shape would pass every bound here.  That the twin's own forced shape is set is shown by the refusals: shape 31 at N % 8 != 0 below, and
    test_experiment_block_shape_is_refused (shape 8 under bf16) — both come from the twin's launch_epi reading the twin's thread_local."""
    lib = _use(dtype)
    lib.gtav_op_gemm_set_wm(shape)
    lib.gtav_op_gemm_set_stages(ns)
    tag = f"shape {shape}" + (f" ring {ns}" if ns else "")
    for (M, N, K) in PB.GEMM_SHAPE_SIZES:
        c = PB.gemm_case(M, N, K, dtype)
        if shape == 31 and N % 8:
            ops = _Operands(c)
            out = _nan((M, N), torch.float32)
            with pytest.raises(L.GtavError, match="persistent loader-wave"):       # refused by name, nothing launched
                _gemm(lib, ops.xd, ops.wd, None, out, N, M, N, K, EPI_PARTIAL, None, 1, 1)
            assert torch.isnan(out).all()
            continue
        _shape_case(lib, c, shape, tag)
    if shape == 31:       # several tiles per block: 540 tiles of 128 x 192 on 256 CUs, twice, bit-equal
        c = PB.GemmCase(*PB.GEMM_PERSISTENT_SIZE, dtype)
        _, a = _shape_case(lib, c, shape, tag)
        ops = _Operands(c)
        b = _nan(tuple(a.shape), dtype)
        _gemm(lib, ops.xd, ops.wd, ops.bd, b, c.N, c.M, c.N, c.K, EPI_GELU_TANH)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "two launches of the persistent kernel differ"
    elif shape != 7:      # the 256 x 256 tile and the persistent kernel have no QKV epilogue
        _qkv_spatial(dtype, f" ({tag})")
        _qkv_temporal(dtype, f" ({tag})")


@DTYPES
def test_experiment_block_shape_is_refused(dtype):
    """Block shape 8 lives in the experiments build: both operand types refuse it by name before anything is launched, and the next unforced launch is right."""
    lib = _use(dtype)
    c = PB.gemm_case(96, 96, 64, dtype)
    ops = _Operands(c)
    out = _nan((96, 96), torch.float32)
    lib.gtav_op_gemm_set_wm(8)
    with pytest.raises(L.GtavError) as e:
        _gemm(lib, ops.xd, ops.wd, ops.bd, out, 96, 96, 96, 64, EPI_F32)
    assert "block shape 8" in str(e.value) and "exists only in the experiments build" in str(e.value), str(e.value)
    assert torch.isnan(out).all()
    lib.gtav_op_gemm_set_wm(0)
    _gemm(lib, ops.xd, ops.wd, ops.bd, out, 96, 96, 96, 64, EPI_F32)
    _within("unforced launch behind a refusal", dtype, out, c.ref, PB.acc_term(64, c.absdot))


def test_fp16_only_launches_refuse_bf16_operands():
    """The fused QKV + attention launches and their weight reorder have no twin: under the bf16 hook they refuse by name, and work again once it is reset."""
    lib = _use(BF16)
    z = torch.zeros(1 << 16, device=dev(), dtype=torch.float16)
    cs = torch.zeros(144 * 64, device=dev())
    calls = {"op_qkv_head_major": lambda: lib.gtav_op_qkv_head_major(z.data_ptr(), z.data_ptr(), 256, stream()),
             "op_qkv_head_major_spatial": lambda: lib.gtav_op_qkv_head_major_spatial(z.data_ptr(), z.data_ptr(), 256, stream()),
             "op_gemm_qkvt_attn": lambda: lib.gtav_op_gemm_qkvt_attn(z.data_ptr(), z.data_ptr(), 80, 256, 16, 5, 0, 5, cs.data_ptr(), z.data_ptr(), z.data_ptr(), stream()),
             "op_gemm_qkvs_attn": lambda: lib.gtav_op_gemm_qkvs_attn(z.data_ptr(), z.data_ptr(), 144, 256, 144, cs.data_ptr(), z.data_ptr(), stream())}
    for name, call in calls.items():
        assert call() != 0
        msg = lib.gtav_last_error().decode()
        assert msg.startswith(name + ":") and "fp16 operands only" in msg, msg
    torch.cuda.synchronize()
    assert (z == 0).all()
    lib.gtav_op_set_operand_dtype(0)
    w, w_hm = torch.zeros(3 * 256, 256, device=dev(), dtype=torch.float16), torch.zeros(3 * 256, 256, device=dev(), dtype=torch.float16)
    L.check(lib.gtav_op_qkv_head_major(w.data_ptr(), w_hm.data_ptr(), 256, stream()))
    torch.cuda.synchronize()


# ---- d. LayerNorm --------------------------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("D,M", PB.LN_SHAPES)
def test_layernorm_kernels(D, M, dtype):
    """D = 128: one block per row; the others one wave per row (1027 rows leave a ragged last block); globally and in every row"""
    lib = _use(dtype)
    c = PB.ln_case(D, M)
    tol = PB.LN_TOL * PB.FACTOR[dtype]
    xd, md, gd, bd = c.x.to(dev()), c.mod.to(dev()), c.g.to(dev()), c.beta.to(dev())
    for mode in (0, 1):
        assert_declared_plan("layernorm", mode, M, D, 0, 0, 0, 0)
    out = _nan((_up(M, 128) + 128, D), dtype)
    L.check(lib.gtav_op_ln_modulate(xd.data_ptr(), out.data_ptr(), M, D, md.data_ptr(), md[:, D:].data_ptr(), 2 * D, c.P, stream()))
    assert torch.isnan(out[_up(M, 128):]).all()
    _rel(f"ln_modulate D={D} M={M}", dtype, untile_typed(out, M, D), c.ref_modulate, tol, rows=D)
    out = _nan((_up(M, 128) + 128, D), dtype)
    L.check(lib.gtav_op_ln_affine(xd.data_ptr(), out.data_ptr(), M, D, gd.data_ptr(), bd.data_ptr(), stream()))
    assert torch.isnan(out[_up(M, 128):]).all()
    _rel(f"ln_affine D={D} M={M}", dtype, untile_typed(out, M, D), c.ref_affine, tol, rows=D)


@DTYPES
@pytest.mark.parametrize("D", PB.LN_LARGE_MEAN_D)
def test_layernorm_statistics_with_a_large_mean(D, dtype):
    """A row of 300 +- 0.02 at the bound of every other LayerNorm case, globally and per row.  (This assertion found the kernels' x - fl(K + mean(x - K)): the
    mean rounded to an ulp of 300 put fp16 rows at 8.4e-4 / 8.1e-4 (D = 128 / 1024) and the D = 1024 total at 5.04e-4 against 5e-4; both kernels now centre
    the row as (x - K) - mean(x - K).)"""
    lib = _use(dtype)
    x, g, b, ref = PB.ln_large_mean_case(D)
    out = torch.zeros(128, D, device=dev(), dtype=dtype)
    xd, gd, bd = x.to(dev()), g.to(dev()), b.to(dev())
    assert_declared_plan("layernorm", 1, x.shape[0], D, 0, 0, 0, 0)
    L.check(lib.gtav_op_ln_affine(xd.data_ptr(), out.data_ptr(), x.shape[0], D, gd.data_ptr(), bd.data_ptr(), stream()))
    _rel(f"ln_affine large mean D={D}", dtype, untile_typed(out, x.shape[0], D), ref, PB.LN_TOL * PB.FACTOR[dtype], rows=D)


@DTYPES
@pytest.mark.parametrize("M,N,K,splitk", [(300, 256, 512, 1), (720, 1024, 1024, 4)])
def test_splitk_partials_reduced_by_layernorm(M, N, K, splitk, dtype):
    """EPI_PARTIAL slabs + the LayerNorm's pending update resid += gate (sum of slabs + bias), then LN + modulate: the fp32 residual and the 2-byte operand"""
    lib = _use(dtype)
    c = PB.gemm_case(M, N, K, dtype)
    ops = _Operands(c)
    P, resid, mod, new, operand = PB.splitk_ln_case(M, N, K, dtype)            # mod = [gate | shift | scale]
    rd, md = resid.clone().to(dev()), mod.to(dev())
    parts = _nan((splitk, M, N), torch.float32)
    out = _nan((_up(M, 128) + 128, N), dtype)
    L.check(lib.gtav_op_gemm_splitk_ln(ops.xd.data_ptr(), K, ops.wd.data_ptr(), ops.bd.data_ptr(), M, N, K, splitk, parts.data_ptr(), rd.data_ptr(), md.data_ptr(),
                                       3 * N, P, out.data_ptr(), md[:, N:].data_ptr(), md[:, 2 * N:].data_ptr(), 3 * N, stream()))
    _rel(f"splitk_ln {M}x{N}x{K}/{splitk} residual", dtype, rd, new, 2e-5)
    assert torch.isnan(out[_up(M, 128):]).all()
    _rel(f"splitk_ln {M}x{N}x{K}/{splitk} operand", dtype, untile_typed(out, M, N), operand, PB.LN_TOL * PB.FACTOR[dtype], rows=N)


# ---- e. spatial attention -----------------------------------------------------------------------------------------------------------------------------------
def _attn_spatial(lib, c, prescaled=False, reps=1):
    NB, heads, S = c.NB, c.heads, c.S
    assert_declared_plan("attn_spatial", NB, heads, S, 1 if prescaled else 0)
    qd, kd, vd = c.q.to(dev()), c.k.to(dev()), c.v.transpose(-1, -2).contiguous().to(dev())
    fn = lib.gtav_op_attn_spatial_prescaled if prescaled else lib.gtav_op_attn_spatial
    outs = []
    for _ in range(reps):
        o = _nan((_up(NB * S, 128) + 128, heads * 64), c.dtype)
        L.check(fn(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), NB, heads, S, stream()))
        outs.append(o)
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0].view(torch.int16), o.view(torch.int16)) for o in outs[1:]), "repeated launches differ"
    assert torch.isnan(outs[0][_up(NB * S, 128):]).all()
    return untile_typed(outs[0], NB * S, heads * 64)


@DTYPES
@pytest.mark.parametrize("S", PB.ATTN_S)
def test_attention_spatial(S, dtype):
    """S = 32 / 72 / 144: the one-pass kernel at 2, 6 and 10 key blocks (72: a padded tail); 200 / 256 / 576: the flash kernel, ragged, S % 64 == 0 and the VAE's
    length.  Globally and per (query, head) row of 64 features."""
    c = PB.attn_case(S, dtype)
    got = _attn_spatial(_use(dtype), c)
    _rel(f"attn_spatial S={S}", dtype, got, c.ref, PB.ATTN_TOL * PB.FACTOR[dtype], rows=64)


@DTYPES
@pytest.mark.parametrize("S", PB.ATTN_PRESCALED_S)
def test_attention_spatial_prescaled_q(S, dtype):
    """attn_flash_kernel<..., PS_ = true>, the instantiation the VAE runs: q carries log2 e / 8 (rounded on the host), the reference is the base-2 softmax of it"""
    c = PB.attn_case(S, dtype, None, True)
    got = _attn_spatial(_use(dtype), c, prescaled=True)
    _rel(f"attn_spatial prescaled S={S}", dtype, got, c.ref, PB.ATTN_TOL * PB.FACTOR[dtype], rows=64)


@DTYPES
@pytest.mark.parametrize("NB,heads,S,prescaled", PB.ATTN_EXTRA, ids=[f"{nb}x{h}x{s}{'-prescaled' if p else ''}" for nb, h, s, p in PB.ATTN_EXTRA])
def test_attention_spatial_every_instantiation(NB, heads, S, prescaled, dtype):
    """The instantiations and launch forms the 2 x 3 cases above do not select (tests/parity_bounds.py ATTN_EXTRA; DECLARED_PLANS says what each runs): the
    one-pass kernel at 4 and 8 key blocks; the flash kernel at three query tiles per wave on a ragged S, at two on S % 64 == 0 with a prescaled q, and at four
    (a padding tie once the grid fills the chip: 256 (frame, head) pairs); and the one-pass kernel without a query split (512 pairs: the batch-8 launch) at 6, 8
    and 10 key blocks.  Globally and per (query, head) row, at the bound of the cases above."""
    c = PB.attn_case(S, dtype, None, bool(prescaled), NB, heads)
    got = _attn_spatial(_use(dtype), c, prescaled=bool(prescaled))
    _rel(f"attn_spatial {NB}x{heads} S={S}{' prescaled' if prescaled else ''}", dtype, got, c.ref, PB.ATTN_TOL * PB.FACTOR[dtype], rows=64)


@DTYPES
def test_attention_spatial_prescaled_refuses_the_plain_q_kernels(dtype):
    lib = _use(dtype)
    z = torch.zeros(1 << 16, device=dev(), dtype=dtype)
    for S in (144, 100):
        assert lib.gtav_op_attn_spatial_prescaled(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 1, S, stream()) != 0
        msg = lib.gtav_last_error().decode()
        assert "attn_spatial_prescaled" in msg and f"S={S}" in msg and "plain q" in msg, msg


@pytest.mark.parametrize("jump", [4.0, 0.45])
def test_attention_flash_running_max_jump_bf16(jump):
    """test_attention_flash_running_max_jump on bf16 operands: a late key far above the running maximum (the rescale branch) and one under the threshold; 10 launches
    bit-equal; the dominated rows at the project's 2e-3 (x 8).
    (This is the assertion that found the twin's plain-q rounding: with q * (1/8 log2 e) rounded to bf16 again, row (0, 1, 382) — a query that sees the planted
    key of norm 32 at a moderate score — came out at 1.005 of the per-row bound at jump 4.0, the figure an emulation of that one rounding reproduces (1.011);
    csrc/attention.hip kPlainQNaturalUnit removed the rounding.)"""
    S, dtype = 576, BF16
    c = PB.attn_case(S, dtype, jump)
    got = _attn_spatial(_use(dtype), c, reps=10)
    _rel(f"attn_spatial jump {jump} S={S}", dtype, got, c.ref, PB.ATTN_TOL * PB.FACTOR[dtype], rows=64)
    for (b, h, row) in c.dominated:
        sl = (b * S + row, slice(h * 64, (h + 1) * 64))
        _rel(f"attn_spatial jump {jump} dominated row ({b}, {h}, {row})", dtype, got[sl], c.ref[sl], PB.ATTN_DOMINATED_TOL * PB.FACTOR[dtype])


# ---- f. temporal attention ----------------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("B,P,D,Tq,t0,Tmax", PB.TEMPORAL_CASES)
def test_attention_temporal(B, P, D, Tq, t0, Tmax, dtype):
    """gtav_op_attn_temporal[_bf16]: the register-resident kernel (t0 + Tq <= 8) and the streaming one (9 .. 32 visible frames; Tq = 1: the cached step, Tq > 8: two
    query groups).  Cache frames no query may see hold NaN; two launches are bit-equal; P stays fp32, so every element has its own bound."""
    lib = L.load()
    fn = lib.gtav_op_attn_temporal if dtype is F16 else lib.gtav_op_attn_temporal_bf16
    assert_declared_plan("attn_temporal", B, P, D, Tq, t0, Tmax)
    c = PB.temporal_case(B, P, D, Tq, t0, Tmax, dtype)
    kv = c.kv.clone()
    kv[:, t0 + Tq:] = float("nan")
    qd, kvd = c.q.to(dev()), kv.to(dev())
    M = B * Tq * P
    outs = []
    for _ in range(2):
        o = _nan((_up(M, 128) + 128, D), dtype)
        L.check(fn(qd.data_ptr(), kvd.data_ptr(), o.data_ptr(), B, P, D, Tq, t0, Tmax, stream()))
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    assert torch.isnan(outs[0][_up(M, 128):]).all()
    got = untile_typed(outs[0], M, D)
    tag = f"attn_temporal Tq={Tq} t0={t0} Tmax={Tmax} P={P}"
    _within(tag, dtype, got, c.ref, c.tol)
    _rel(tag, dtype, got, c.ref, PB.TEMPORAL_TOL * PB.FACTOR[dtype], rows=64)


# ---- g. weight-gradient GEMMs -------------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("T,M,N", [(64, 128, 128), (320, 256, 256)])
def test_gemm_tn_weight_gradient(T, M, N, dtype):
    """out[m][n] += sum_t x[t][m] w[t][n] on tile-major [tokens][features] operands, into a non-zero output"""
    lib = _use(dtype)
    x, w, base = PB.rand(T, M, seed=1).to(dtype), PB.rand(T, N, seed=2).to(dtype), PB.rand(M, N, seed=3)
    xd, wd = to_tiled(x, dtype), to_tiled(w, dtype)
    out = base.to(dev()).clone()
    L.check(lib.gtav_op_gemm_tn(xd.data_ptr(), wd.data_ptr(), M, N, T, out.data_ptr(), N, stream()))
    ref = base.double() + x.double().t() @ w.double()
    _rel(f"gemm_tn T={T} {M}x{N}", dtype, out, ref, 2e-5)
    _within(f"gemm_tn T={T} {M}x{N}", dtype, out, ref, PB.acc_term(T, base.double().abs() + x.double().abs().t() @ w.double().abs()))


@DTYPES
def test_gemm_dw_grouped_weight_gradients(dtype):
    """two weight gradients as ONE grid of 256 x 256 tiles (1 + 2 tiles), K = 64 tokens, into non-zero outputs"""
    lib = _use(dtype)
    groups, K = [(256, 256), (512, 256)], 64
    n = len(groups)
    xs = [PB.rand(M, K, seed=10 + i).to(dtype) for i, (M, N) in enumerate(groups)]
    ws = [PB.rand(N, K, seed=20 + i, scale=1 / math.sqrt(K)).to(dtype) for i, (M, N) in enumerate(groups)]
    base = [PB.rand(M, N, seed=30 + i) for i, (M, N) in enumerate(groups)]
    xd, wd = [to_tiled(x, dtype) for x in xs], [to_tiled(w, dtype) for w in ws]
    outs = [b.to(dev()).clone() for b in base]
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    ints = lambda v: (C.c_int32 * n)(*v)
    L.check(lib.gtav_op_gemm_dw_grouped(n, arr(xd), arr(wd), arr(outs), ints([g[0] for g in groups]), ints([g[1] for g in groups]), ints([g[1] for g in groups]), K, stream()))
    for i in range(n):
        ref = base[i].double() + xs[i].double() @ ws[i].double().t()
        _rel(f"gemm_dw_grouped group {i} {groups[i]}", dtype, outs[i], ref, 2e-5)
        _within(f"gemm_dw_grouped group {i} {groups[i]}", dtype, outs[i], ref, PB.acc_term(K, base[i].double().abs() + xs[i].double().abs() @ ws[i].double().abs().t()))


# ---- h. convert_pad, bit for bit -----------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("tiled", [1, 0])
def test_convert_pad_bit_for_bit(tiled, dtype):
    """fp32 -> the operand type with zero padding, against torch.clamp(x, +-max).to(dtype): ties of both parities, subnormals of the type, signed zeros, values
    beyond fp16 (7e4 and 1e30 survive in bf16, fp16 stops at 65504) and FLT_MAX (the largest finite value of the type, never inf)."""
    lib = _use(dtype)
    R, Cc = 100, 72
    Rp, Cp = (128, 128) if tiled else (104, 80)
    x = PB.rand(R, Cc, seed=11)
    ulp = 4 * PB.U[dtype]                                          # spacing of the type in [2, 4)
    special = [2.0 + 0.5 * ulp, 2.0 + 1.5 * ulp, -2.0 - 0.5 * ulp, -2.0 - 1.5 * ulp,            # exact ties: to the even neighbour below / above
               2.0 + 0.5 * ulp + 2.0 ** -22, 2.0 + 0.5 * ulp - 2.0 ** -22,                        # just off a tie
               PB.SUBNORMAL[dtype], 3 * PB.SUBNORMAL[dtype], -5 * PB.SUBNORMAL[dtype], 0.5 * PB.SUBNORMAL[dtype], 1.5 * PB.SUBNORMAL[dtype],
               2.5 * PB.SUBNORMAL[dtype], 0.0, -0.0, 7e4, -7e4, 1e30, -1e30, 3.4028234663852886e38, -3.4028234663852886e38, 65504.0, 65520.0, 65519.0]
    x.reshape(-1)[:len(special)] = torch.tensor(special, dtype=torch.float64).float()
    x[R - 1, Cc - len(special):] = torch.tensor(special, dtype=torch.float64).float()          # the ragged corner too
    fmax = torch.finfo(dtype).max
    want = torch.clamp(x, -fmax, fmax).to(dtype)
    assert torch.isfinite(want.float()).all()
    if dtype is BF16:
        assert want.reshape(-1)[16].item() == 1e30 or abs(want.reshape(-1)[16].item() / 1e30 - 1) < 2.0 ** -8
        assert want.reshape(-1)[18].item() == fmax and want.reshape(-1)[14].item() > 65504.0
    expect = torch.zeros(Rp * Cp, dtype=torch.int16)
    idx = tiled_index(R, Cp)[:, :Cc] if tiled else (torch.arange(R)[:, None] * Cp + torch.arange(Cc)[None, :])
    expect[idx.reshape(-1)] = want.view(torch.int16).reshape(-1)
    dst = torch.full((Rp * Cp + 256,), 0x7E7E, device=dev(), dtype=torch.int16)
    xd = x.to(dev())
    L.check(lib.gtav_op_convert_f16(xd.data_ptr(), Cc, R, Cc, dst.data_ptr(), Rp, Cp, tiled, stream()))
    got = dst.cpu()
    assert (got[Rp * Cp:] == 0x7E7E).all(), "written behind the padded image"
    bad = (got[:Rp * Cp] != expect).nonzero().reshape(-1)
    print(f"[margin convert_pad tiled={tiled} {PB.NAME[dtype]}] {bad.numel()} of {Rp * Cp} elements differ from torch's rounding")
    assert bad.numel() == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), expect[bad[:8]].tolist())
