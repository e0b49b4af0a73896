"""Inputs, fp64 references, error bounds and fp32 emulations of the operand-typed kernels, shared by tests/test_gpu_ops_typed.py (the kernels, on a GPU) and
tests/test_host_parity_bounds.py (the bounds themselves, on the CPU).  Pure torch: nothing here loads the library.  The second half of the file holds the same
for the backward-only training kernels (tests/test_gpu_ops_train.py), then the deferred-residual LayerNorm (tests/test_gpu_ops_ln_pending.py), the four
attention backward kernels (tests/test_gpu_ops_attn_bwd_bounds.py), the optimizer step (tests/test_gpu_ops_optimizer.py), the skinny fp32 GEMM (tests/test_gpu_ops.py)
and last the declared launch plans of every op-level parity problem (tests/test_host_op_coverage.py), each with its own head comment.

None of the bounds is taken from the code under test.  u is the unit roundoff of the operand type, 2^-11 for fp16 and 2^-8 for bf16.

Store bound of a GEMM output element (all terms in fp64):
    |got - ref| <= u (1 + 2^-10) |ref| + 2 (K + 2) 2^-24 (|x| |w|^T + |b|) + one subnormal step
  first term: ONE round to nearest (the 2^-10 covers rounding an fp32 value that is itself off by the second term); second term: the classical forward bound
  of a K-term fp32 dot product plus bias (products of two 2-byte operands are exact in fp32, so K + 2 roundings are already generous), doubled because the
  matrix pipe's internal rounding is not documented as round to nearest.  An fp32 output has the second term only ("accumulation term").
Temporal attention (P stays fp32):
    tol = u (1 + 2^-10) |ref| + (2 delta + (T + 2) 2^-23) sum_j p_j |v_j|,   delta = 2 * 66 * 2^-24 * max_j sum_i |q_i k_ij| / 8
  delta: the error of a score (64 exact products, 66 additions at most, doubled like the GEMM's) carried through the exponential, once for the numerator and
  once for the denominator; (T + 2) 2^-23: exp2 (1 ulp), T fused multiply-adds, T additions of the denominator, the reciprocal and the final product.
Global and per-row relative L2: the project's fp16 figure of the op (2e-5 fp32 outputs, 5e-4 LayerNorm, 6e-4 temporal attention, 1.5e-3 attention with P
  rounded to 2 bytes), times u / 2^-11 = 8 for 2-byte outputs in bf16 (the precedent of tests/test_gpu_ops_attn_bwd_long.py)."""
import functools
import math

import numpy as np
import torch

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = (F16, BF16)
NAME = {F16: "fp16", BF16: "bf16"}
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
SUBNORMAL = {F16: 2.0 ** -24, BF16: 2.0 ** -133}        # one subnormal step of the type
FACTOR = {F16: 1.0, BF16: 8.0}                            # u / 2^-11
LOG2E = 1.4426950408889634


def rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def store_rne(x, dtype):
    return x.float().to(dtype)


def store_trunc(x, dtype):
    """fp32 -> 2 bytes rounding TOWARD ZERO: the wrong store the per-element bounds must catch (a dropped guard bit, a wrong pack instruction)."""
    x = x.float().contiguous()
    if dtype is BF16:
        return (x.view(torch.int32) & -65536).view(torch.float32).to(BF16)
    h = x.to(F16)
    bits = h.view(torch.int16)
    return torch.where(h.float().abs() > x.abs(), bits - 1, bits).view(F16)    # sign-magnitude: one step down in the low 15 bits is one step toward zero


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def row_rel_l2(a, b):
    """relative L2 of every row (last dimension) -> the worst one"""
    a, b = a.double(), b.double()
    return ((a - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-30)).max().item()


def outside(err, tol):
    """(fraction of elements outside the bound, worst ratio error / bound)"""
    r = err.double() / tol.double()
    return (r > 1).double().mean().item(), r.max().item()


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------------------------
GEMM_STORE_SHAPES = [(100, 256, 64), (97, 100, 128), (300, 512, 256)]
GEMM_SHAPE_SIZES = [(96, 96, 64), (97, 100, 128), (257, 384, 192), (700, 384, 192), (1300, 256, 256)]
GEMM_PERSISTENT_SIZE = (11520, 1024, 64)     # 540 tiles of 128 x 192 on 256 CUs, one K step


class GemmCase:
    def __init__(self, M, N, K, dtype):
        self.M, self.N, self.K, self.dtype = M, N, K, dtype
        self.x = rand(M, K, seed=1).to(dtype)
        self.w = rand(N, K, seed=2, scale=1 / math.sqrt(K)).to(dtype)
        self.b = rand(N, seed=3)
        x, w = self.x.double(), self.w.double()
        self.ref_nb = x @ w.t()                                  # without the bias (split-K slabs)
        self.absdot_nb = x.abs() @ w.abs().t()
        self.ref = self.ref_nb + self.b.double()
        self.absdot = self.absdot_nb + self.b.double().abs()

    def emulate(self):
        """the pre-activation in fp32 arithmetic"""
        return self.x.float() @ self.w.float().t() + self.b


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, dtype):
    return GemmCase(M, N, K, dtype)


def acc_term(K, absdot):
    return 2.0 * (K + 2) * 2.0 ** -24 * absdot


def store_bound(ref, acc, dtype):
    return U[dtype] * (1 + 2.0 ** -10) * ref.abs() + acc + SUBNORMAL[dtype]


def gelu_tanh64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_erf64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_tanh_bound(ref, dtype):
    """EPI_GELU_TANH on an exact pre-activation: exp2 + rcp, 1 ulp each, then the 2-byte store (tests/test_gpu_ops.py, with u in place of 2^-11)"""
    return 2e-6 + ref.abs() * U[dtype] * math.sqrt(2.0) + 0.5 * SUBNORMAL[dtype]


def gelu_erf_bound(ref, dtype):
    """EPI_GELU_ERF: the polynomial's absolute contract + half an ulp of the store + half a subnormal step"""
    return 3.2e-5 + ref.abs() * U[dtype] + 0.5 * SUBNORMAL[dtype]


GELU_TANH_MAX_SLOPE = 1.13     # max |d/dx GELU_tanh| = 1.129 (at x = 1.41): what an error of the pre-activation becomes behind the activation


def gelu_tanh_gemm_bound(case):
    """EPI_GELU_TANH behind a GEMM: the store bound, its accumulation term carried through the activation (slope) plus the activation's own fp32 error — the
    absolute 2e-6 of the sweep's bound and 8 roundings of the value (exp2 and rcp 1 ulp each, five multiplies / adds)"""
    ref = gelu_tanh64(case.ref)
    return ref, store_bound(ref, GELU_TANH_MAX_SLOPE * acc_term(case.K, case.absdot) + 2e-6 + 8 * 2.0 ** -24 * ref.abs(), case.dtype)


def gelu_sweep(dtype):
    """One non-zero operand per row: pre[m][n] = v_m + bias_n exactly, v over [-9, 9] in the operand type, bias = multiples of 2^-10 up to +-1/16."""
    M, N, K = 1152, 128, 64
    v = torch.linspace(-9.0, 9.0, M).to(dtype).float()
    x = torch.zeros(M, K)
    x[:, 0] = v
    w = torch.zeros(N, K)
    w[:, 0] = 1.0
    b = (torch.arange(N, dtype=torch.float32) - N / 2) * (1.0 / 1024)
    return M, N, K, x.to(dtype), w.to(dtype), b, (v[:, None] + b[None, :]).double()


def gelu_tanh_emulate(pre):
    """common.h gelu_tanh_f in fp32 arithmetic"""
    x = pre.float()
    a = torch.tensor(-2.0 * LOG2E * 0.7978845608028654, dtype=torch.float32)
    b = a * torch.tensor(0.044715, dtype=torch.float32)
    return x / (1.0 + torch.exp2(x * (x * x * b + a)))


# ---- QKV + RoPE scatter -------------------------------------------------------------------------------------------------------------------------------
class QkvCase:
    """y = x w^T + bias of a to_qkv projection, q / k rotated pair-wise by the table row `pos[m]` of token m.  ref / mag: [M][3 D] in token order — the
    tests scatter both to the layout of the launch with the same permutation.  mag = |a| |cos| + |b| |sin| of the accumulation magnitudes of the pair."""

    def __init__(self, M, D, npos, pos, dtype, bias):
        self.M, self.D, self.dtype = M, D, dtype
        self.x = rand(M, D, seed=1).to(dtype)
        self.w = rand(3 * D, D, seed=2, scale=1 / math.sqrt(D)).to(dtype)
        self.b = rand(3 * D, seed=7) if bias else None
        ang = rand(npos, 32, seed=3) * 3
        self.cos, self.sin = ang.cos(), ang.sin()                 # fp32 [npos][32]: the values the launch's table holds
        x, w = self.x.double(), self.w.double()
        y = x @ w.t()
        A = x.abs() @ w.abs().t()
        if bias:
            y, A = y + self.b.double(), A + self.b.double().abs()
        self.pos = pos
        self.ref, self.mag = self._rotate(y, A, torch.float64)
        self.tol = store_bound(self.ref, acc_term(D, self.mag), dtype)

    def _rotate(self, y, A, ft):
        M, D = self.M, self.D
        c, s = self.cos[self.pos].to(ft)[:, None, :], self.sin[self.pos].to(ft)[:, None, :]     # [M][1][32]
        out, mag = y.clone(), (A.clone() if A is not None else None)
        for part in (0, 1):
            sl = slice(part * D, (part + 1) * D)
            yp = y[:, sl].reshape(M, D // 64, 32, 2)
            a, b = yp[..., 0], yp[..., 1]
            out[:, sl] = torch.stack((a * c - b * s, b * c + a * s), dim=-1).reshape(M, D)
            if A is not None:
                Ap = A[:, sl].reshape(M, D // 64, 32, 2)
                Aa, Ab = Ap[..., 0], Ap[..., 1]
                mag[:, sl] = torch.stack((Aa * c.abs() + Ab * s.abs(), Ab * c.abs() + Aa * s.abs()), dim=-1).reshape(M, D)
        return out, mag

    def emulate(self):
        y = self.x.float() @ self.w.float().t()
        if self.b is not None:
            y = y + self.b
        return self._rotate(y, None, torch.float32)[0]


QKV_SPATIAL = dict(NB=3, S=48, D=256)                        # tests/test_gpu_ops.py test_gemm_qkv_spatial_layout_and_rope
QKV_TEMPORAL = dict(B=2, Tq=2, t0=1, Tmax=4, P=16, D=256)    # tests/test_gpu_ops.py test_gemm_qkv_temporal_layout


@functools.lru_cache(maxsize=None)
def qkv_spatial_case(dtype):
    g = QKV_SPATIAL
    M = g["NB"] * g["S"]
    return QkvCase(M, g["D"], g["S"], torch.arange(M) % g["S"], dtype, bias=True)


@functools.lru_cache(maxsize=None)
def qkv_temporal_case(dtype):
    g = QKV_TEMPORAL
    M = g["B"] * g["Tq"] * g["P"]
    pos = g["t0"] + (torch.arange(M) // g["P"]) % g["Tq"]
    return QkvCase(M, g["D"], g["Tmax"], pos, dtype, bias=False)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(128, 96), (256, 96), (1024, 1027), (2048, 160), (1280, 96), (1792, 33)]      # (D, M); the last two: blocks of 5 and 7 waves
LN_TOL = 5e-4


def ln64(x, eps=1e-6):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps)


class LnCase:
    def __init__(self, D, M):
        self.D, self.M = D, M
        self.P = 32 if M % 32 == 0 else 1
        self.x = rand(M, D, seed=1) * 3 + 0.5
        self.mod = rand(M // self.P, 2 * D, seed=2)               # [shift | scale]
        self.g, self.beta = rand(D, seed=3) * 0.1 + 1, rand(D, seed=4) * 0.1
        xh = ln64(self.x)
        shift, scale = (self.mod[:, i * D:(i + 1) * D].double().repeat_interleave(self.P, 0) for i in range(2))
        self.ref_modulate = xh * (1 + (scale + 1e-6)) + shift
        self.ref_affine = xh * self.g.double() + self.beta.double()


@functools.lru_cache(maxsize=None)
def ln_case(D, M):
    return LnCase(D, M)


@functools.lru_cache(maxsize=None)
def ln_large_mean_case(D):
    M = 64
    x = 300.0 + 0.02 * rand(M, D, seed=5)
    g, b = rand(D, seed=3) * 0.1 + 1, rand(D, seed=4) * 0.1
    return x, g, b, ln64(x) * g.double() + b.double()


@functools.lru_cache(maxsize=None)
def splitk_ln_case(M, N, K, dtype):
    """split-K slabs + the LayerNorm's pending update resid += gate (x w^T + bias), then LN + modulate -> (P, resid, mod [gate | shift | scale], the updated
    residual fp64, the 2-byte operand's reference fp64)"""
    P = 36 if M % 36 == 0 else M
    c = gemm_case(M, N, K, dtype)
    resid, mod = rand(M, N, seed=4), rand(M // P, 3 * N, seed=5)
    gate, shift, scale = (mod[:, i * N:(i + 1) * N].double().repeat_interleave(P, 0) for i in range(3))
    new = resid.double() + gate * c.ref
    return P, resid, mod, new, ln64(new) * (1 + (scale + 1e-6)) + shift


# ---- spatial attention --------------------------------------------------------------------------------------------------------------------------------
ATTN_TOL, ATTN_DOMINATED_TOL = 1.5e-3, 2e-3
ATTN_S = [32, 72, 144, 200, 256, 576]
ATTN_NB, ATTN_HEADS = 2, 3


class AttnCase:
    """q, k, v [NB][heads][S][64] in the operand type; ref [NB S][heads 64] fp64.  jump: the two dominating keys of test_attention_flash_running_max_jump.
    prescaled: q_ps = q * log2 e / 8 rounded on the host, and the reference is the base-2 softmax of THAT q.  The fp64 softmax is formed one item at a time;
    the probabilities p (what control() needs) are kept only at the default 2 x 3 items — at 256 items of S = 256 they would be 130 MB."""

    def __init__(self, S, dtype, jump=None, prescaled=False, NB=ATTN_NB, heads=ATTN_HEADS):
        self.S, self.dtype, self.NB, self.heads = S, dtype, NB, heads
        q, k, v = (rand(NB, heads, S, 64, seed=i).to(dtype) for i in (1, 2, 3))
        if jump is None:
            q = (q.float() * 1.5).to(dtype)
        else:
            k[1, 2, S - 9] = (q[1, 2, 7].float() * jump).to(dtype)         # a key of the last key block against query 7
            k[0, 1, 70] = (q[0, 1, 150].float() * jump).to(dtype)          # and one in the second key block
            self.dominated = ((1, 2, 7), (0, 1, 150))
        self.k, self.v = k, v
        self.q = (q.double() * (LOG2E / 8)).to(dtype) if prescaled else q
        keep_p = (NB, heads) == (ATTN_NB, ATTN_HEADS)
        ps, refs = [], []
        for b in range(NB):
            if prescaled:
                s = self.q[b].double() @ k[b].double().transpose(-1, -2)
                p = torch.exp2(s - s.max(-1, keepdim=True).values)
            else:
                s = q[b].double() @ k[b].double().transpose(-1, -2) / 8.0
                p = torch.exp(s - s.max(-1, keepdim=True).values)
            p = p / p.sum(-1, keepdim=True)
            refs.append(p @ v[b].double())
            if keep_p:
                ps.append(p)
        self.p = torch.stack(ps) if keep_p else None
        self.ref4 = torch.stack(refs)                                          # NB heads S 64
        self.ref = self.ref4.permute(0, 2, 1, 3).reshape(NB * S, heads * 64)

    def control(self, requantized_q=False):
        """the fp64 result with P (unnormalised, as the kernels hold it) and the output rounded to the operand type: what a perfect kernel of this design returns.
        requantized_q: the scores of q * (log2 e / 8) rounded to the operand type AGAIN — what the flash kernel's plain-q form did on both operand types before
        the bf16 twin moved its scores to the natural logarithm's unit (csrc/attention.hip kPlainQNaturalUnit; the fp16 objects still do)"""
        p = self.p
        if requantized_q:
            q2 = (self.q.float() * torch.tensor(LOG2E / 8, dtype=torch.float32)).to(self.dtype).double()
            s = q2 @ self.k.double().transpose(-1, -2)
            p = torch.exp2(s - s.max(-1, keepdim=True).values)
            p = p / p.sum(-1, keepdim=True)
        pm = p / p.max(-1, keepdim=True).values
        pr = pm.to(self.dtype).double()
        o = (pr @ self.v.double()) / pm.sum(-1, keepdim=True)
        return o.to(self.dtype).double()


@functools.lru_cache(maxsize=None)
def _attn_case_cached(S, dtype, jump, prescaled, NB, heads):
    return AttnCase(S, dtype, jump, prescaled, NB, heads)


def attn_case(S, dtype, jump=None, prescaled=False, NB=ATTN_NB, heads=ATTN_HEADS):
    """(the cases of hundreds of items are used by one test each and hold tens of MB: built, not kept)"""
    if NB * heads > 64:
        return AttnCase(S, dtype, jump, prescaled, NB, heads)
    return _attn_case_cached(S, dtype, jump, prescaled, NB, heads)


def attn_rows(x4):
    """[NB][heads][S][64] -> one row per (item, head, query): the 64 features a single softmax produces"""
    return x4.reshape(-1, 64)


# ---- temporal attention -------------------------------------------------------------------------------------------------------------------------------
TEMPORAL_TOL = 6e-4
# (B, P, D, Tq, t0, Tmax)
TEMPORAL_CASES = [(2, 24, 256, Tq, t0, Tmax) for (Tq, t0, Tmax) in ((5, 0, 5), (1, 4, 5), (3, 5, 8), (1, 7, 32), (1, 8, 32), (9, 3, 16), (32, 0, 32), (1, 31, 32))] + \
                 [(2, 3, 256, 12, 0, 12)] + \
                 [(8, 128, 256, 3, 2, 8), (8, 128, 256, 3, 5, 8)]        # 6 columns: a partial block; 1024 columns: the query frames of a window in ONE block, at 5 and 8 visible frames


class TemporalCase:
    def __init__(self, B, P, D, Tq, t0, Tmax, dtype):
        self.args, self.dtype = (B, P, D, Tq, t0, Tmax), dtype
        h, Tk = D // 64, t0 + Tq
        self.q = rand(B, Tq, P, D, seed=1).to(dtype)
        self.kv = rand(B, Tmax, P, 2, D, seed=2).to(dtype)
        self.item = lambda x, T: x.reshape(B, T, P, h, 64).permute(0, 2, 3, 1, 4)              # B P h T 64
        self.rows = lambda o: o.permute(0, 3, 1, 2, 4).reshape(B * Tq * P, D)
        qf, kf, vf = self.item(self.q.double(), Tq), self.item(self.kv[:, :Tk, :, 0].double(), Tk), self.item(self.kv[:, :Tk, :, 1].double(), Tk)
        self.mask = torch.arange(Tk)[None, :] > (t0 + torch.arange(Tq))[:, None]              # Tq Tk
        s = (qf @ kf.transpose(-1, -2) / 8.0).masked_fill(self.mask, float("-inf"))
        p = s.softmax(-1)
        self.ref = self.rows(p @ vf)
        abs_s = (qf.abs() @ kf.abs().transpose(-1, -2) / 8.0).masked_fill(self.mask, 0.0)       # sum_i |q_i k_ij| / 8
        delta = 2 * 66 * 2.0 ** -24 * abs_s.max(-1, keepdim=True).values                        # B P h Tq 1
        visible = (t0 + torch.arange(Tq) + 1).double()[:, None]                                 # keys query tl sees
        pv = self.rows(p @ vf.abs())                                                            # sum_j p_j |v_j|
        coef = self.rows((2 * delta + (visible + 2) * 2.0 ** -23).expand(B, P, h, Tq, 64))
        self.tol = U[dtype] * (1 + 2.0 ** -10) * self.ref.abs() + coef * pv + SUBNORMAL[dtype]

    def emulate(self):
        """the kernels' arithmetic in fp32: scores, exp2 of the scaled difference to the maximum, sequential fused accumulation, one reciprocal"""
        B, P, D, Tq, t0, Tmax = self.args
        Tk = t0 + Tq
        qf, kf, vf = self.item(self.q.float(), Tq), self.item(self.kv[:, :Tk, :, 0].float(), Tk), self.item(self.kv[:, :Tk, :, 1].float(), Tk)
        s = ((qf @ kf.transpose(-1, -2)) * 0.125).masked_fill(self.mask, float("-inf"))
        p = torch.exp2((s - s.max(-1, keepdim=True).values) * torch.tensor(LOG2E, dtype=torch.float32))
        den = torch.zeros_like(p[..., 0])
        acc = torch.zeros_like(qf)
        for t in range(Tk):
            den = den + p[..., t]
            acc = acc + p[..., t:t + 1] * vf[..., t:t + 1, :]
        return self.rows(acc * (1.0 / den)[..., None])


@functools.lru_cache(maxsize=None)
def temporal_case(B, P, D, Tq, t0, Tmax, dtype):
    return TemporalCase(B, P, D, Tq, t0, Tmax, dtype)


# =======================================================================================================================================================
# The backward-only training kernels (csrc/train.hip): inputs, fp64 references, bounds and fp32 emulations shared by tests/test_gpu_ops_train.py (GPU) and
# tests/test_host_parity_bounds.py (CPU).  eps = 2^-24 is the unit roundoff of fp32.  Every figure below is a count of roundings or a project constant.
#
# An fp32 sum of n terms (frame sums, bias sums, column sums, the fp32 conditioning GEMMs):
#     |got - ref| <= (n + 2) eps sum |term|          (acc_term's convention: n terms added in ANY order pass n - 1 additions, + the rounding of the product in
#   front and of the `+=` behind; doubled where an fp32 MFMA adds, whose internal rounding is not documented).  |term| includes the old value of an
#   accumulating output.
# Bias sums: the FUSED launches (gate_bwd_fused, gelu_bwd_tiled_colsum) add the UNROUNDED fp32 products; the unfused forms add the 2-byte dy / du the first
#   launch stored, each off by u |term| (one round to nearest) + half a subnormal step — an intended difference of the two forms, so the unfused bound is the
#   fused one + u sum |term| + n subnormal steps.
# A value rounded once to 2 bytes from a short fp32 expression: store_bound(ref, acc, dtype), acc = the fp32 roundings of the expression (2 eps |ref| for a
#   product of two or three factors) and, for GELU', the error of its own fp32 evaluation (gelu_grad_eval_error).
# =======================================================================================================================================================
EPS32 = 2.0 ** -24
ERR_F16_SAT = 2               # csrc/common.h
F16_MAX = 65504.0


def sum_bound(n, mag, mfma=False):
    return (2.0 if mfma else 1.0) * (n + 2) * EPS32 * mag


def frame_sum(v, frames, P, drop_last=False):
    """[frames P][D] -> [frames][D], the sum over a frame's tokens.  drop_last: the WRONG sum that leaves out the last token of every frame (the last row of the
    last, partial 16-row chunk of the fused kernels)"""
    v = v.reshape(frames, P, -1)
    return (v[:, :P - 1] if drop_last else v).sum(1)


# ---- LayerNorm + modulate backward (fp32 only) -----------------------------------------------------------------------------------------------------------
LN_BWD_SHAPES = [(256, 3, 24), (512, 2, 16), (1024, 2, 40), (2048, 1, 17), (384, 2, 24), (100, 1, 5), (1792, 1, 17)]      # (D, frames, P); the last three: no fused kernel
LN_BWD_FUSED_D = (256, 512, 1024, 2048)


class LnBwdCase:
    """dres = (accumulate ? old : 0) + rstd (g - mean g - xhat mean(g xhat)), g = dxn (1 + scale + 1e-6); dshift = sum_t dxn, dscale = sum_t dxn xhat.
    scale / dshift / dscale live in tables of row length 3 D + 64 at the column offsets SC / SH / DS (multiples of 4: the kernels read scale as 16-byte vectors).

    Forward error of the fp32 evaluation, per element (first order in eps; every count is the number of roundings the value passes, + 2 as in sum_bound):
      a = x - K, K = the row's first element (what the kernels centre on, like the forward LayerNorm): eps |a|
      mean a   e_m  = (D + 3) eps mean|a|
      d = a - mean a:  e_d = e_m + eps (|a| + |d|)
      variance e_v  = e_m^2 + (D + 4) eps var        (the mean's error enters at second order only: sum d = 0)
      rstd     rho  = e_v / (2 (var + 1e-6)) + 3 eps   (relative: the addition, the square root, the division)
      xhat     e_xh = e_d rstd + |xhat| (rho + eps)
      g        3 eps |g|;   s1 = mean g: e_s1 = (D + 5) eps mean|g|;   s2 = mean(g xhat): e_s2 = (D + 6) eps mean|g xhat| + mean(|g| e_xh)
      dx       e_dx = rstd (6 eps |g| + e_s1 + 3 eps |s1| + e_xh |s2| + |xhat| (e_s2 + 3 eps |s2|)) + (rho + eps) rstd (|g| + |s1| + |xhat s2|)
      dres     e_dx + eps (|old| + |dx|)  with accumulate
      dshift   sum_bound(P, sum_t |dxn|);   dscale: sum_bound(P, sum_t |dxn xhat|) + sum_t |dxn| e_xh
    large_mean (rows of 300 +- 0.02, as ln_large_mean_case): because the bound follows the CENTRED arithmetic it stays sharp there (|a| is 0.03, not 300); a kernel
    that forms x - fl(mean x) instead is off by half an ulp of 300 = 1.5e-5 in the mean at least, 7.6e-4 of the standard deviation, and leaves it.  The tests hold
    dres and dscale of that set to the per-ROW relative L2 LN_TOL (the project's LayerNorm figure) as well."""

    def __init__(self, D, frames, P, large_mean=False):
        self.D, self.frames, self.P, self.M = D, frames, P, frames * P
        M = self.M
        self.stride, self.SC, self.SH, self.DS = 3 * D + 64, D + 32, 32, 2 * D + 64
        self.x = (300.0 + 0.02 * rand(M, D, seed=5)) if large_mean else rand(M, D, seed=1) * 3 + 0.5
        self.dxn = rand(M, D, seed=2)
        self.mod = rand(frames, self.stride, seed=3)
        self.old = rand(M, D, seed=4)
        x, dxn = self.x.double(), self.dxn.double()
        sc = self.mod[:, self.SC:self.SC + D].double().repeat_interleave(P, 0)
        mu = x.mean(-1, keepdim=True)
        d = x - mu
        var = (d * d).mean(-1, keepdim=True)
        r = 1.0 / torch.sqrt(var + 1e-6)
        xh = d * r
        g = dxn * (1.0 + (sc + 1e-6))
        s1, s2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
        self.ref_dx = r * (g - s1 - xh * s2)
        self.ref_dshift, self.ref_dscale = frame_sum(dxn, frames, P), frame_sum(dxn * xh, frames, P)
        e = EPS32
        a = x - x[:, :1]
        e_m = (D + 3) * e * a.abs().mean(-1, keepdim=True)
        e_d = e_m + e * (a.abs() + d.abs())
        e_v = e_m ** 2 + (D + 4) * e * var
        rho = e_v / (2 * (var + 1e-6)) + 3 * e
        e_xh = e_d * r + xh.abs() * (rho + e)
        e_s1 = (D + 5) * e * g.abs().mean(-1, keepdim=True)
        e_s2 = (D + 6) * e * (g * xh).abs().mean(-1, keepdim=True) + (g.abs() * e_xh).mean(-1, keepdim=True)
        self.tol_dx = r * (6 * e * g.abs() + e_s1 + 3 * e * s1.abs() + e_xh * s2.abs() + xh.abs() * (e_s2 + 3 * e * s2.abs())) + \
            (rho + e) * r * (g.abs() + s1.abs() + (xh * s2).abs())
        self.tol_dshift = sum_bound(P, frame_sum(dxn.abs(), frames, P))
        self.tol_dscale = sum_bound(P, frame_sum((dxn * xh).abs(), frames, P)) + frame_sum(dxn.abs() * e_xh, frames, P)

    def ref_dres(self, accumulate):
        return self.ref_dx + self.old.double() if accumulate else self.ref_dx

    def tol_dres(self, accumulate):
        return self.tol_dx + EPS32 * (self.old.double().abs() + self.ref_dx.abs()) if accumulate else self.tol_dx

    def emulate(self, accumulate, wrong=None):
        """the kernels' arithmetic in fp32 (sums in torch's order) -> dres, dshift, dscale.  wrong: "scale0" = the scale row of frame 0 for every frame,
        "noacc" = accumulate ignored, "var" = variance over D - 1, "drop" = the frame sums without the last token, "plain" = x - fl(mean x) without the
        centring on the row's first element"""
        D, P, frames = self.D, self.P, self.frames
        x, dxn = self.x, self.dxn
        sc = self.mod[:, self.SC:self.SC + D]
        sc = sc[:1].expand(frames, D) if wrong == "scale0" else sc
        sc = sc.repeat_interleave(P, 0)
        a = x if wrong == "plain" else x - x[:, :1]
        d = a - a.sum(-1, keepdim=True) / D
        var = (d * d).sum(-1, keepdim=True) / (D - 1 if wrong == "var" else D)
        r = 1.0 / torch.sqrt(var + 1e-6)
        xh = d * r
        g = dxn * (1.0 + (sc + 1e-6))
        s1, s2 = g.sum(-1, keepdim=True) / D, (g * xh).sum(-1, keepdim=True) / D
        dx = r * (g - s1 - xh * s2)
        if accumulate and wrong != "noacc":
            dx = dx + self.old
        return dx, frame_sum(dxn, frames, P, wrong == "drop"), frame_sum(dxn * xh, frames, P, wrong == "drop")


@functools.lru_cache(maxsize=None)
def ln_bwd_case(D, frames, P, large_mean=False):
    return LnBwdCase(D, frames, P, large_mean)


# ---- gate backward (2-byte dy, fp32 dgate and bias sums) ------------------------------------------------------------------------------------------------------
GATE_BWD_SHAPES = [(256, 3, 24), (128, 2, 5), (1024, 1, 144)]      # (D, frames, P)


class GateBwdCase:
    """dy = gate dres rounded to 2 bytes (gate None: 1); dgate[f] = sum_t dres y; db += sum_m dy.  gate sits at column offset G of a table of row length 3 D + 64,
    dgate goes to the same columns of a table of its own.  sat: ONE product is 70000, beyond fp16 — fp16 stores +-65504 there and raises ERR_F16_SAT, bf16 stores
    the rounded value.
      dy      store_bound(ref, 2 eps |ref|)            one product (no product at all without a gate)
      dgate   sum_bound(P, sum_t |dres y|)
      db      fused: sum_bound(M, sum_m |dy| + |old|);  unfused: + u sum_m |dy| + M subnormal steps (see the head of this section)"""

    def __init__(self, D, frames, P, dtype, gated=True, sat=False):
        self.D, self.frames, self.P, self.M, self.dtype = D, frames, P, frames * P, dtype
        M = self.M
        self.stride, self.G = 3 * D + 64, 2 * D + 32
        self.dres = rand(M, D, seed=1)
        self.y = rand(M, D, seed=2).to(dtype)
        self.mod = rand(frames, self.stride, seed=3)
        self.db0 = rand(D, seed=4)
        self.sat_at = None
        if sat:
            m0, d0 = M - 2, D - 3
            gv = self.mod[m0 // P, self.G + d0].item() if gated else 1.0
            self.dres[m0, d0] = 70000.0 / gv
            self.sat_at = (m0, d0)
        self.gate = self.mod[:, self.G:self.G + D] if gated else None
        gr = self.gate.double().repeat_interleave(P, 0) if gated else torch.ones(M, D, dtype=torch.float64)
        dres, y = self.dres.double(), self.y.double()
        self.ref_dy = gr * dres
        self.tol_dy = store_bound(self.ref_dy, 2 * EPS32 * self.ref_dy.abs(), dtype)
        self.ref_dgate = frame_sum(dres * y, frames, P)
        self.tol_dgate = sum_bound(P, frame_sum((dres * y).abs(), frames, P))
        mag = self.ref_dy.abs().sum(0)
        self.ref_db = self.db0.double() + self.ref_dy.sum(0)
        self.tol_db_fused = sum_bound(M, mag + self.db0.double().abs())
        self.tol_db_unfused = self.tol_db_fused + U[dtype] * mag + M * SUBNORMAL[dtype]

    def tol_db(self, fused):
        return self.tol_db_fused if fused else self.tol_db_unfused

    def emulate(self, fused, store=store_rne, drop=False, assign=False):
        """fp32 arithmetic -> dy (2 bytes), dgate, db.  drop: frame sums without the last token; assign: db = in place of db +="""
        D, P, frames = self.D, self.P, self.frames
        gr = self.gate.repeat_interleave(P, 0) if self.gate is not None else None
        dy32 = self.dres * gr if gr is not None else self.dres.clone()
        dy = store(dy32, self.dtype)
        dgate = frame_sum(self.dres * self.y.float(), frames, P, drop)
        if fused:
            parts = frame_sum(self.dres, frames, P, drop)
            s = (parts * self.gate if self.gate is not None else parts).sum(0)
        else:
            s = dy.float().sum(0)
        return dy, dgate, (s if assign else self.db0 + s)


@functools.lru_cache(maxsize=None)
def gate_bwd_case(D, frames, P, dtype, gated=True, sat=False):
    return GateBwdCase(D, frames, P, dtype, gated, sat)


# ---- GELU(tanh) backward with the fc1 bias sums ------------------------------------------------------------------------------------------------------------
GELU_BWD_SHAPES = [(100, 128), (512, 64), (513, 256), (1100, 128)]     # (M, N): 1, 1, 2 and 3 row splits of the 128-padded image
GELU_K, GELU_C = math.sqrt(2.0 / math.pi), 0.044715


def gelu_grad64(u):
    """d/du GELU_tanh(u) = s + T (1 - s), s = sigmoid(2 k (u + c u^3)), T = u s 2 k (1 + 3 c u^2) -> (value, s, 1 - s, T), 1 - s without cancellation"""
    u = u.double()
    w = 2.0 * GELU_K * (u + GELU_C * u ** 3)
    s, s1 = torch.sigmoid(w), torch.sigmoid(-w)
    T = u * s * 2.0 * GELU_K * (1.0 + 3.0 * GELU_C * u * u)
    return s + T * s1, s, s1, T


def gelu_grad_eval_error(u):
    """Error of common.h gelu_tanh_grad_f2 in fp32, first order (eps = 2^-24), over the magnitudes of its terms:
      arg = u fma(u^2, b, a), a = -2 log2(e) k, b = a c (constants rounded to fp32, a few roundings each): |d arg| <= 6 eps A, A = |u| (|a| + |b| u^2)
      e = exp2(arg) (1 ulp = 2 eps), s = rcp(1 + e) (eps + 2 eps):  relative error of s  rho = (1 - s) (6 ln2 A + 2) eps + 3 eps
      T = (u s) fma(u^2, 6 k c, 2 k): rho + 6 eps;  1 - s is formed from the ROUNDED s: absolute error s rho + eps (1 - s)
      value = fma(T, 1 - s, s):  |T| (1 - s) (rho + 7 eps) + (1 + |T|) s rho + eps (s + |T| (1 - s))
    The middle term is the cancellation in 1 - s where s is close to 1 (u > 3): |T| reaches 170 at u = 9."""
    u = u.double()
    _, s, s1, T = gelu_grad64(u)
    a = 2.0 * LOG2E * GELU_K
    A = u.abs() * (a + a * GELU_C * u * u)
    rho = s1 * (6 * math.log(2.0) * A + 2) * EPS32 + 3 * EPS32
    return T.abs() * s1 * (rho + 7 * EPS32) + (1 + T.abs()) * s * rho + EPS32 * (s + T.abs() * s1)


def gelu_grad_emulate(u):
    """gelu_tanh_grad_f2 in fp32 arithmetic (the fused multiply-adds as a multiply and an add)"""
    v = u.float()
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    k, c = f(0.7978845608028654), f(0.044715)
    a = f(-2.0) * f(1.4426950408889634) * k
    b, k2, k6 = a * c, f(2.0) * k, f(6.0) * k * c
    z = v * v
    s = 1.0 / (torch.exp2(v * (z * b + a)) + 1.0)
    t = (v * s) * (z * k6 + k2)
    return t * (1.0 - s) + s


class GeluBwdCase:
    """du = dh gelu'(u) rounded to 2 bytes, db += sum over the M real rows of du.  sweep: u covers [-9, 9] in the operand type (row m: the gelu_sweep value, column
    n: + a multiple of 2^-10); else u = 2 N(0, 1).  sat: one product beyond fp16 (dh = 65000 at u = 3, gelu' = 1.012).
      du   store_bound(ref, |dh| gelu_grad_eval_error(u) + 2 eps |ref|)
      db   fused: sum_bound(M, sum |du| + |old|) + sum_m |dh| eval error (the terms are the unrounded fp32 products);  unfused: + u sum |du| + M subnormal steps"""

    def __init__(self, M, N, dtype, sweep, sat=False):
        self.M, self.N, self.dtype = M, N, dtype
        if sweep:
            u = torch.linspace(-9.0, 9.0, M)[:, None] + ((torch.arange(N, dtype=torch.float32) - N / 2) / 1024)[None, :]
        else:
            u = rand(M, N, seed=1, scale=2.0)
        self.u = u.to(dtype)
        self.dh = rand(M, N, seed=2).to(dtype)
        self.db0 = rand(N, seed=3)
        self.sat_at = None
        if sat:
            self.sat_at = (M - 1, N - 5)
            self.u[self.sat_at] = 3.0
            self.dh[self.sat_at] = 65000.0
        dh, g = self.dh.double(), gelu_grad64(self.u)[0]
        self.ref_du = dh * g
        ev = dh.abs() * gelu_grad_eval_error(self.u)
        self.tol_du = store_bound(self.ref_du, ev + 2 * EPS32 * self.ref_du.abs(), dtype)
        mag = self.ref_du.abs().sum(0)
        self.ref_db = self.db0.double() + self.ref_du.sum(0)
        self.tol_db_fused = sum_bound(M, mag + self.db0.double().abs()) + ev.sum(0)
        self.tol_db_unfused = self.tol_db_fused + U[dtype] * mag + M * SUBNORMAL[dtype]

    def tol_db(self, fused):
        return self.tol_db_fused if fused else self.tol_db_unfused

    def emulate(self, fused, store=store_rne, pad_row=None, assign=False):
        """fp32 arithmetic -> du (2 bytes), db.  pad_row: a row of fp32 products behind row M that the WRONG sum includes; assign: db = in place of db +="""
        du32 = self.dh.float() * gelu_grad_emulate(self.u)
        du = store(du32, self.dtype)
        terms = du32 if fused else du.float()
        s = terms.sum(0)
        if pad_row is not None:
            s = s + pad_row
        return du, (s if assign else self.db0 + s)


@functools.lru_cache(maxsize=None)
def gelu_bwd_case(M, N, dtype, sweep, sat=False):
    return GeluBwdCase(M, N, dtype, sweep, sat)


# ---- column sums ----------------------------------------------------------------------------------------------------------------------------------------------
COLSUM_TILED_M, COLSUM_TILED_N = (1, 511, 512, 513, 1300), (64, 192)
COLSUM_F32_M, COLSUM_F32_N = (1, 255, 256, 257, 700), (50, 300)
COLSUM_MULTI_SPLITS = (1, 7, 8, 9, 17)


class ColsumCase:
    """db += sum_m a[m][n], launched `launches` times on the same a: ref = old + launches sum, bound sum_bound(launches M, |old| + launches sum |a|)"""

    def __init__(self, M, N, dtype=None, launches=1):
        self.M, self.N, self.launches = M, N, launches
        self.a = rand(M, N, seed=1) if dtype is None else rand(M, N, seed=1).to(dtype)
        self.db0 = rand(N, seed=2)
        a = self.a.double()
        self.ref = self.db0.double() + launches * a.sum(0)
        self.tol = sum_bound(launches * M, self.db0.double().abs() + launches * a.abs().sum(0))

    def emulate(self, assign=False):
        db = self.db0.clone()
        for _ in range(self.launches):
            s = self.a.float().sum(0)
            db = s if assign else db + s
        return db


@functools.lru_cache(maxsize=None)
def colsum_case(M, N, dtype=None, launches=1):
    return ColsumCase(M, N, dtype, launches)


# ---- the loss gradient ----------------------------------------------------------------------------------------------------------------------------------------
MSE_BWD_SHAPES = [(2, 3, 16, 8, 16, 2, 64), (1, 1, 3, 4, 6, 2, 64)]      # (B, T, C, H, W, p, ldf): F = C p p = 64 = ldf and 12 < ldf


class MseBwdCase:
    """dv[b][T - 1] = scale (vpred[b][T - 1] - vtarget[b]) as an image, zero in every other frame; the launch stores its patch tokens dfo[m][(ph, pw, c)] —
    the inverse of DiT.unpatchify — rounded to 2 bytes.  Two fp32 roundings (the difference, the product): store_bound(ref, 2 eps |ref|).  sat: one difference
    that `scale` carries beyond fp16."""

    def __init__(self, B, T, C, H, W, p, ldf, dtype, sat=False):
        self.shape, self.dtype, self.ldf = (B, T, C, H, W, p), dtype, ldf
        self.vpred, self.vtarget = rand(B, T, C, H, W, seed=1), rand(B, C, H, W, seed=2)
        self.scale = 3.0
        self.sat_at = None
        if sat:
            self.sat_at = (B - 1, C - 1, H - 1, W - 2)
            self.vpred[B - 1, T - 1, C - 1, H - 1, W - 2] = self.vtarget[self.sat_at] + 30000.0
        self.ref = torch.zeros(B, T, C, H, W, dtype=torch.float64)
        self.ref[:, T - 1] = float(self.scale) * (self.vpred[:, T - 1].double() - self.vtarget.double())
        self.tol = store_bound(self.ref, 2 * EPS32 * self.ref.abs(), dtype)

    def emulate(self, store=store_rne, every_frame=False):
        """fp32 arithmetic -> the gradient image (B, T, C, H, W) in 2 bytes.  every_frame: the WRONG kernel that writes the gradient for the frame in front of the
        last as well"""
        B, T = self.shape[:2]
        out = torch.zeros(self.vpred.shape)
        for t in ([T - 1] if not every_frame else range(max(T - 2, 0), T)):
            out[:, t] = torch.tensor(self.scale, dtype=torch.float32) * (self.vpred[:, t] - self.vtarget)
        return store(out, self.dtype)


@functools.lru_cache(maxsize=None)
def mse_bwd_case(B, T, C, H, W, p, ldf, dtype, sat=False):
    return MseBwdCase(B, T, C, H, W, p, ldf, dtype, sat)


# ---- the fp32 conditioning path -------------------------------------------------------------------------------------------------------------------------------
SILU_SPECIAL = (0.0, 20.0, -20.0, 90.0, -90.0)
# expf(-v) overflows at -v > 88.73: the kernels then return 0 where the true value is as large as 88.73 x 2^-128 (SiLU) or |dy| 87.73 x 2^-128 (its derivative),
# both below 2^-121
SILU_ABS = 2.0 ** -121


class SiluCase:
    """y = x sigmoid(x); dx = dy s (1 + x (1 - s)), s = sigmoid(x).  s from expf (2 ulp), an addition and a division: 8 eps relative, generous.
      silu      10 eps |ref| + SILU_ABS
      silu_bwd  16 eps |dy| s (1 + |x|) + SILU_ABS max(1, |dy|)      (magnitudes, not the value: 1 + x (1 - s) cancels at x = -1.28, and 1 - s is formed from the
                rounded s, an absolute error of 8 eps s that x multiplies)"""

    def __init__(self, R=7, C=100):
        self.R, self.C = R, C
        self.x = rand(R, C, seed=1, scale=4.0)
        self.x[0, :len(SILU_SPECIAL)] = torch.tensor(SILU_SPECIAL)
        self.dy = rand(R, C, seed=2)
        x, dy = self.x.double(), self.dy.double()
        s, s1 = torch.sigmoid(x), torch.sigmoid(-x)
        self.ref_y = x * s
        self.tol_y = 10 * EPS32 * self.ref_y.abs() + SILU_ABS
        self.ref_dx = dy * s * (1.0 + x * s1)
        self.tol_dx = 16 * EPS32 * dy.abs() * s * (1.0 + x.abs()) + SILU_ABS * dy.abs().clamp_min(1.0)

    def emulate(self):
        x, dy = self.x, self.dy
        s = 1.0 / (1.0 + torch.exp(-x))
        return x / (1.0 + torch.exp(-x)), dy * s * (1.0 + x * (1.0 - s))


@functools.lru_cache(maxsize=None)
def silu_case():
    return SiluCase()


class GemmF32Case:
    """out[i][j] (+)= sum_t a[t][i] b[t][j] over `n` terms in fp32: a [n][I], b [n][J], old [I][J] (None: the output is overwritten).
    gemm_tn_f32: a = dY [R][N], b = X [R][K], n = R, accumulating.  gemm_nn_f32: a = dY^T [N][R], b = W [N][K], n = N.  ada_bwd_dx: a = dmod^T [MODW][R],
    b = W_ada [MODW][D], n = MODW.  Bound: sum_bound(n, sum |a b| + |old|), doubled on the fp32 matrix cores."""

    def __init__(self, n, I, J, accumulate, mfma, seed=0, scale=1.0):
        self.n, self.I, self.J = n, I, J
        self.a, self.b = rand(n, I, seed=seed + 1), rand(n, J, seed=seed + 2, scale=scale)
        self.old = rand(I, J, seed=seed + 3) if accumulate else None
        a, b = self.a.double(), self.b.double()
        self.ref, mag = a.t() @ b, a.abs().t() @ b.abs()
        if accumulate:
            self.ref, mag = self.ref + self.old.double(), mag + self.old.double().abs()
        self.tol = sum_bound(n, mag, mfma)

    def emulate(self, assign=False):
        s = self.a.t() @ self.b
        return s if (self.old is None or assign) else self.old + s


@functools.lru_cache(maxsize=None)
def gemm_f32_case(n, I, J, accumulate, mfma, seed=0, scale=1.0):
    return GemmF32Case(n, I, J, accumulate, mfma, seed, scale)


GEMM_TN_F32_MFMA = [(5, 64, 64), (17, 256, 128), (80, 128, 64)]                 # (R, N, K)
GEMM_TN_F32_VALU = [(16, 64, 25, "full"), (5, 30, 25, "odd lddy"), (5, 64, 25, "dY offset")]
GEMM_NN_F32 = [(R, N, K) for N in (256, 2048, 4096) for R in (1, 17) for K in (64, 100)]
ADA_BWD_MFMA = [(3584, 256, 6), (1024 + 192, 64, 80), (2048, 1024, 17)]         # (MODW, D, R)
ADA_BWD_VALU = [(3584, 256, 81), (1024 + 192, 100, 6), (14 * 2048, 2048, 6)]        # more than 80 conditioning rows; D % 64 != 0; what a depth-1 hidden-2048 handle calls


# =======================================================================================================================================================
# The deferred-residual LayerNorm (csrc/elementwise.hip ln_row_block_kernel, csrc/ops_typed.inc LnPending): x += gate[frame] (bias + sum_k slab_k), then
# LayerNorm + modulate / affine of the updated row into the 2-byte operand.  Shared by tests/test_gpu_ops_ln_pending.py and tests/test_host_parity_bounds.py.
#
#   1  updated residual, per element:  |got - ref| <= (nsplit + 2) eps (|x| + |g| (|b| + sum_k |s_k|))  = sum_bound(nsplit, ..): nsplit additions (the bias
#      and the slabs), one product and one addition, each off by eps relative at most (a fused multiply-add only drops one of them)
#   2  the branch image y_save / launch_branch_rows: bit for bit the operand-type store (round to nearest even, clamped to the largest finite fp16 in fp16) of
#      the fp32 sum bias + s_0 + s_1 + .. in THAT order — additions only, so no contraction can move a bit
#   3  the 2-byte operand: relative L2 LN_TOL FACTOR[dtype] against the fp64 LayerNorm of the fp64-updated row, per row and globally (the criterion of the
#      LayerNorm cases above)
# Slabs, bias and gates are N(0, 1), so a dropped slab, a slab added twice, another frame's gate or a bias behind the gate move the residual by the order of 1,
# 2^20 times the bound.  Rows 0 .. 63 of the D = 1024, M = 300 case hold ln_large_mean_case's 300 +- 0.02 with slabs of 1 / 32 the size.
# =======================================================================================================================================================
class LnPendCase:
    """mode 0: modulate with a table [R][3 D] = [gate | shift | scale] (stride 3 D), frame f of P rows -> table row rows[f] (LayerNorm) / gate_rows[f] (gate),
    the identity without `indirect`;  mode 1: affine (gamma, beta), never gated.  nsplit 0: a descriptor without slabs.  tperm (T, P16): the output row order of
    the fused temporal launch.  ld: row length of the slabs and of y_save (>= D)."""

    def __init__(self, name, D, M, nsplit, mode, gate=True, bias=True, P=1, indirect=False, tperm=None, large_mean=0, ld=None):
        self.name, self.D, self.M, self.nsplit, self.mode, self.P, self.tperm = name, D, M, nsplit, mode, P, tperm
        self.ld = ld or D
        frames = M // P
        assert frames * P == M and not (mode == 1 and gate)
        self.frames = frames
        self.x = rand(M, D, seed=11) * 3 + 0.5
        self.slabs = rand(max(nsplit, 1), M, self.ld, seed=12)[:nsplit]
        if large_mean:
            self.x[:large_mean] = ln_large_mean_case(D)[0][:large_mean]
            self.slabs[:, :large_mean] *= 1.0 / 32
        self.bias = rand(D, seed=13) if bias and nsplit else None
        self.R = frames + 2 if indirect else frames
        self.mod = rand(self.R, 3 * D, seed=14)
        self.gamma, self.beta = rand(D, seed=15) * 0.1 + 1, rand(D, seed=16) * 0.1
        if indirect:     # non-monotone, one table row used by two frames, two table rows unused; the gate's list is another one
            self.rows = torch.tensor([(7 * f + 3) % self.R for f in range(frames)], dtype=torch.int32)
            self.rows[frames - 1] = self.rows[1]
            self.gate_rows = torch.tensor([(5 * f + 1) % self.R for f in range(frames)], dtype=torch.int32)
            self.gate_rows[frames - 2] = self.gate_rows[0]
        else:
            self.rows = self.gate_rows = None
        self.gated = gate and nsplit > 0
        # ---- fp64 references ----
        x = self.x.double()
        self.ref_new, self.tol_new = x, torch.zeros_like(x)
        if nsplit:
            y = self.slabs[:, :, :D].double().sum(0)
            mag = self.slabs[:, :, :D].double().abs().sum(0)
            if self.bias is not None:
                y, mag = y + self.bias.double(), mag + self.bias.double().abs()
            if self.gated:
                g = self._table(self.gate_rows, 0, torch.float64)
                y, mag = g * y, g.abs() * mag
            self.ref_new = x + y
            self.tol_new = sum_bound(nsplit, x.abs() + mag)
        xh = ln64(self.ref_new)
        if mode == 0:
            shift, scale = self._table(self.rows, 1, torch.float64), self._table(self.rows, 2, torch.float64)
            self.ref_operand = xh * (1 + (scale + 1e-6)) + shift
        else:
            self.ref_operand = xh * self.gamma.double() + self.beta.double()

    def _table(self, rows, part, ft, shift_frames=0):
        """[M][D]: columns part D .. of the table row of every token's frame"""
        f = (torch.arange(self.frames) + shift_frames) % self.frames
        r = rows.long()[f] if rows is not None else f
        D = self.D
        return self.mod[r, part * D:(part + 1) * D].to(ft).repeat_interleave(self.P, 0)

    def out_rows(self, swapped=False):
        """row of the 2-byte operand that token row m is written to (LnPending::tperm_*): (b, t, p) -> (b, p / 16, t, p % 16).  swapped: the WRONG order
        with the two parts of p exchanged, (b, p % (P / 16), t, p / (P / 16))"""
        m = torch.arange(self.M)
        if not self.tperm:
            return m
        T, P = self.tperm
        fr, pp = m // P, m % P
        bb, tt = fr // T, fr % T
        hi, lo = (pp % (P // 16), pp // (P // 16)) if swapped else (pp // 16, pp % 16)
        return ((bb * (P // 16) + hi) * T + tt) * 16 + lo

    def branch32(self, wrong=None):
        """bias + s_0 + s_1 + .. in fp32, in the kernels' order.  wrong: "drop" = without the last slab, "again" = slab 0 once more where the load chunk
        (1 / 2 / 4 / 8 slots) has an unused slot"""
        D = self.D
        y = self.bias.clone().expand(self.M, D) if self.bias is not None else torch.zeros(self.M, D)
        n = self.nsplit - 1 if wrong == "drop" else self.nsplit
        for k in range(n):
            y = y + self.slabs[k, :, :D]
        if wrong == "again" and self.nsplit not in (1, 2, 4, 8):
            y = y + self.slabs[0, :, :D]
        return y

    def y_save(self, dtype):
        return store_clamped(self.branch32(), dtype)

    def emulate(self, dtype, wrong=None):
        """the row-block kernel's arithmetic in fp32 -> (updated residual, the 2-byte operand in the launch's OUTPUT row order).  wrong: branch32's, "gate" = the
        gate of the next frame, "bias" = the bias added behind the gate, "tperm" = out_rows(swapped)"""
        D, x = self.D, self.x
        v = x
        if self.nsplit:
            if wrong == "bias" and self.bias is not None:
                y = torch.zeros(self.M, D)
                for k in range(self.nsplit):
                    y = y + self.slabs[k, :, :D]
            else:
                y = self.branch32(wrong)
            if self.gated:
                y = y * self._table(self.gate_rows, 0, torch.float32, 1 if wrong == "gate" else 0)
            if wrong == "bias" and self.bias is not None:
                y = y + self.bias
            v = x + y
        a = v - x[:, :1]                                  # K = the row's first element BEFORE the update
        m1 = a.sum(-1, keepdim=True) / D
        var = ((a * a).sum(-1, keepdim=True) / D - m1 * m1).clamp_min(0.0)
        xh = (a - m1) * (1.0 / torch.sqrt(var + 1e-6))
        if self.mode == 0:
            o = xh * (1.0 + (self._table(self.rows, 2, torch.float32) + 1e-6)) + self._table(self.rows, 1, torch.float32)
        else:
            o = xh * self.gamma + self.beta
        out = torch.empty(self.M, D, dtype=dtype)
        out[self.out_rows(wrong == "tperm")] = store_rne(o, dtype)
        return v, out


def store_clamped(x, dtype):
    """common.h sat4: fp32 -> 2 bytes, round to nearest even behind a clamp to the largest finite fp16 (bf16: fp32's own range, no clamp)"""
    x = x.float()
    return store_rne(x.clamp(-F16_MAX, F16_MAX) if dtype is F16 else x, dtype)


# name -> constructor arguments; tests/test_gpu_ops_ln_pending.py says which buffers (x_out, y_save, k_save) each launch gets
LN_PEND_CASES = {
    "d64": dict(D=64, M=40, nsplit=1, mode=0, P=8),                                               # one wave, nw = 1
    "d192": dict(D=192, M=33, nsplit=2, mode=1, gate=False, bias=False, ld=200),                  # the VAE's form; 48 of 64 threads active; ld > D
    "d256_rows": dict(D=256, M=160, nsplit=3, mode=0, P=16, indirect=True, tperm=(5, 16)),        # B 2, T 5, P 16
    "d256_tperm": dict(D=256, M=144, nsplit=0, mode=0, P=48, tperm=(3, 48)),                      # a descriptor without slabs
    "d1024_train": dict(D=1024, M=300, nsplit=4, mode=0, P=60, large_mean=64),                    # x_out + y_save + k_save, then the k_load re-run
    "d1280": dict(D=1280, M=96, nsplit=5, mode=0, P=32),                                          # 5 waves
    "d1280_tperm": dict(D=1280, M=96, nsplit=5, mode=0, P=32, tperm=(3, 32)),                     # (P = 16 above makes the order the identity: here it is not)
    "d1792": dict(D=1792, M=33, nsplit=8, mode=1, gate=False),                                    # 7 waves
    "d2048": dict(D=2048, M=130, nsplit=8, mode=0, P=26),
    "d1024_step": dict(D=1024, M=720, nsplit=4, mode=0, P=144),                                   # the batch-1 step's launch, in place, repeated
    "d192_train": dict(D=192, M=33, nsplit=2, mode=1, gate=False, ld=200),                        # the affine form with k_save, then its k_load re-run: no product caller, the hook launches it
}
LN_PEND_WRONG = ("drop", "again", "gate", "bias", "tperm")


@functools.lru_cache(maxsize=None)
def ln_pend_case(name):
    return LnPendCase(name, **LN_PEND_CASES[name])


@functools.lru_cache(maxsize=None)
def ln_pend_sat_case():
    """D = 64, 8 rows, two slabs whose sum leaves fp16 in two elements (+80000, -70000.5): fp16 stores +-65504 and raises ERR_F16_SAT, bf16 rounds the value."""
    c = LnPendCase("sat", D=64, M=8, nsplit=2, mode=0, P=8)
    c.bias = torch.zeros(64)
    c.slabs[0, 3, 5], c.slabs[1, 3, 5] = 40000.0, 40000.0
    c.slabs[0, 6, 60], c.slabs[1, 6, 60] = -30000.5, -40000.0
    return c


# =======================================================================================================================================================
# The attention backward kernels (csrc/train.hip attn_spatial_bwd_mfma_kernel / attn_spatial_bwd_stream_kernel, attn_temporal_bwd_kernel /
# attn_temporal_bwd_stream_kernel): inputs, fp64 references, ONE bound per output element and the "perfect kernel of the design" with its wrong variants, shared
# by tests/test_gpu_ops_attn_bwd_bounds.py (GPU) and tests/test_host_parity_bounds.py (CPU).
#
# The operation, per (item, head), n keys (S, or the t + 1 visible frames of query t), all in fp64 on the operands as rounded to the operand type:
#     s = q k^T / 8,  P = softmax(s),  dP = dO v^T,  Dq_i = sum_j P_ij dP_ij,  dS = P (dP - Dq) / 8,  dv = P^T dO,  dq = dS k,  dk = dS^T q,
#   then dq / dk rotated back through the launch's OWN fp32 table (RoPE^T: (a, b) -> (a cos + b sin, b cos - a sin) per pair).
#
# Inputs.  flat: unit normal.  sharp: q x 6 (the largest probability of a row has a median of about 0.65).  Planted keys (spatial `jump`; temporal `diagonal`,
#   `first`, `ladder`): see attn_bwd_inputs / temporal_bwd_inputs.  dO x 2^e is exact in both types but for fp16 subnormals, and the reference uses the rounded dO.
#
# Why an ABSOLUTE per-element bound: a query dominated by one key has dS ~ 0 and a dq row that is nearly zero, so the rounded fp64 reference itself has a per-row
#   relative L2 error of up to 1.0 there.  The forward tests' per-row instrument cannot be used on backward outputs.
#
# The bound counts roundings, first order; u = unit roundoff of the operand type x (1 + 2^-10), eps = 2^-24, sub = one subnormal step of the type.
#   score       e_ij = 2 * 66 eps sum_d |q k| / 8   (64 exact products, 66 additions at most, doubled: the matrix pipe's rounding is not documented — acc_term)
#   exponent    spatial: the argument is formed in base-2 units, s2 - lse2 with s2 = s log2 e: the constant, the product and the subtraction, three roundings of
#                 at most eps (|s2| + |lse2|) each, and exp2 itself (1 ulp = 2 eps) -> as a relative error of P (x ln 2 < 1, not taken)
#                 x_ij = 4 eps (|s_ij| + max(|lse_i|, |max_i|)) log2 e      (the statistics pass subtracts the row maximum, not lse: whichever is larger)
#               temporal: __expf(s - max) is a base-2 evaluation whose argument is scaled in fp32: subtraction, constant, product (eps |s - max| each) + 2 eps of
#                 exp2 = (3 |s - max| + 2) eps  <=  x_ij = (|s_ij - max_i| + 2) 2^-22
#   rho_ij      relative error of the fp32 P_ij:  e_ij + x_ij  (numerator)  +  sum_j P_ij (e_ij + x_ij)  (the denominator is a sum of such terms: its relative error
#               is their P-weighted mean)  +  (n + 4) 2^-23  (n exponentials of 1 ulp, n additions, the logarithm or the reciprocal and the product; a streaming
#               sweep also rescales its running sum by exp2 of the maximum's rise, at most once per 64-key chunk: three roundings each, inside the n + 4)
#   P           spatial, rounded to the operand type as an MFMA operand:  |dP_ij| <= (u + rho_ij) P + sub / 2 + 2^-126  (an fp32 exponential may flush below the
#               smallest normal);  temporal, kept in fp32: rho_ij P + 2^-126
#   dP          |d dP_ij| <= 2 * 66 eps sum_d |dO v|
#   Dq          |d Dq_i| <= sum_j P |d dP| + sum_j rho_ij P |dP| + (n + 2) 2^-23 sum_j P |dP|      (n fused multiply-adds, the shuffles' additions, one division)
#   dS          spatial: (u + rho_ij + 4 eps) |dS| + P (|d dP| + |d Dq|) / 8 + sub / 2   (subtraction, product, the exact / 8, then the 2-byte rounding);
#               temporal: the same without u and sub / 2
#   dv_jd       sum_i |dP_ij| |dO_id| + 2 (n + 2) eps sum_i P |dO|       (an fp32 sum of n terms, doubled on the matrix pipe — kept for the temporal kernels' fused
#   dq_id       sum_j |d dS_ij| |k_jd| + 2 (n + 2) eps sum_j |dS| |k|     multiply-adds as well);  dk likewise with q
#   rotation    (a, b) -> a cos + b sin: |d a| |cos| + |d b| |sin| + 3 eps (|a cos| + |b sin|)  (two products, one addition; the table is exact: both sides read it)
#   store       + u |ref| + sub: ONE round to nearest of every output element (store_bound's first and last term)
# Nothing above is taken from what a kernel returned.  If a kernel exceeds the bound on a term this derivation missed, the term is ADDED here with its derivation
# (and the control below gets the matching rounding): never a factor.
#
# The control (AttnBwdCase.control / TemporalBwdCase.control): fp64 math with exactly the design's 2-byte roundings — spatial P, dS and the outputs, temporal the
# outputs only — is "what a perfect kernel of this design returns" and must have NO element outside; each WRONG variant must leave the bound somewhere:
#   "drop_last"   the last (visible) key left out of the row statistics lse and Dq — a wrong tail mask
#   "rope_sign"   RoPE^T with the sign of the sine reversed (dq, dk)
#   "stale_max"   the running sum not rescaled when a later 64-key chunk (temporal: a later key) raises the maximum
#   "dq_chunk"    Dq without the terms of its last 64-key chunk
#   "mask_plus" / "mask_minus"   temporal: query t sees keys s <= t + 1 / s <= t - 1 (query 0 keeps key 0)
# Limit: because P and dS are rounded to 2 bytes BY DESIGN, the spatial bound carries u-sized terms of its own, and a truncating output store or a truncated dS
# (errors of 2 u where u is allowed) stays around the bound (0.4 .. 1.1 of it): the host test prints those ratios and does not require them caught.  The temporal
# bound has no such term, and a truncating store is caught there.
# =======================================================================================================================================================
FLUSH32 = 2.0 ** -126
ATTN_BWD_RESIDENT = [(2, 2, 32), (1, 2, 144), (1, 1, 160)]                   # (NB, heads, S): two tiles and idle waves; production, one tile per wave; a wave with two tiles
ATTN_BWD_STREAM = [(1, 1, 8), (2, 2, 72), (1, 2, 200), (1, 1, 576)]           # one half-empty tile; a chunk + half a tile; 4 chunks, 2 groups, ragged; 9 chunks, 5 groups
ATTN_BWD_SHAPES = ATTN_BWD_RESIDENT + ATTN_BWD_STREAM
ATTN_BWD_KINDS = ("flat", "sharp", "jump")
ATTN_BWD_SCALED_SHAPES = [(2, 2, 72), (1, 2, 144)]                            # the shapes that also run dO x 2^-10 (fp16 subnormals) and x 2^8 (loss-scaled)
ATTN_BWD_SCALES = (-10, 8)
ATTN_BWD_SAT = [(2, 2, 32), (2, 2, 72)]                                       # fp16, sharp, dO x 2^13: dk leaves fp16, dS does not
ATTN_BWD_SAT_SCALE = 13
ATTN_BWD_MUTANT_MAX_S = 200
TEMPORAL_BWD_RESIDENT = [(2, 3, 128, 1, 1), (2, 3, 128, 5, 8), (1, 3, 128, 8, 32)] + \
                        [(2, 3, 128, T, 8) for T in (2, 3, 4, 6, 7)]      # (B, P, D, T, Tmax); P = 3: a partial block of clamped lanes; attn_temporal_bwd_kernel<TT> has one instantiation per T
TEMPORAL_BWD_STREAM = [(2, 3, 128, 9, 9), (1, 3, 128, 17, 32), (1, 5, 256, 32, 32)]
TEMPORAL_BWD_SHAPES = TEMPORAL_BWD_RESIDENT + TEMPORAL_BWD_STREAM
TEMPORAL_BWD_KINDS = ("flat", "sharp", "diagonal", "first", "ladder")


def unrope(g, co, si, sign=1.0):
    """RoPE^T of [..][pos][64] with the angles' cos / sin [pos][32]: the rotation by the negative angle.  sign = -1: the WRONG rotation by the positive one"""
    a, b = g[..., 0::2], g[..., 1::2]
    return torch.stack([a * co + sign * b * si, b * co - sign * a * si], dim=-1).reshape(g.shape)


def unrope_bound(e, g, co, si):
    """the rotation's line of the derivation: e = bound of the value in front of it, g = that value"""
    ea, eb, a, b = e[..., 0::2], e[..., 1::2], g[..., 0::2].abs(), g[..., 1::2].abs()
    co, si = co.abs(), si.abs()
    return torch.stack([ea * co + eb * si + 3 * EPS32 * (a * co + b * si), eb * co + ea * si + 3 * EPS32 * (b * co + a * si)], dim=-1).reshape(g.shape)


def rope_cs(ang):
    """the launch's table: fp32 [pos][pair][cos, sin]"""
    return torch.stack([ang.cos(), ang.sin()], dim=-1).reshape(ang.shape[0], 64).contiguous()


def temporal_rope_angles(n):
    """the `temporal` table of tests/test_gpu_ops_attn_temporal_bwd.py: position t x the language frequencies 10000^(-2 i / 64)"""
    return torch.arange(n, dtype=torch.float32)[:, None] * (1.0 / (10000.0 ** (torch.arange(0, 64, 2).float() / 64)))[None, :]


class _AttnBwdMath:
    """The chain above on [..][n queries][64] q / dO and [..][n keys][64] k / v in fp64; mask [n][n] True = hidden (None: full attention); chunk = keys per
    chunk of the streaming statistics (64 spatial, 1 temporal).  p_dtype: the type P and dS are rounded to (None: they stay as they are)."""

    def __init__(self, q, k, v, g, mask, chunk):
        self.q, self.k, self.v, self.g, self.mask, self.chunk = q, k, v, g, mask, chunk
        self.n = q.shape[-2]

    def scores(self, mask=None):
        mask = self.mask if mask is None else mask
        s = self.q @ self.k.transpose(-1, -2) / 8.0
        return s if mask is None else s.masked_fill(mask, float("-inf"))

    def reference(self):
        s = self.scores()
        mx = s.max(-1, keepdim=True).values
        pu = torch.exp(s - mx)
        Z = pu.sum(-1, keepdim=True)
        P = pu / Z
        dP = self.g @ self.v.transpose(-1, -2)
        Dq = (P * dP).sum(-1, keepdim=True)
        dS = P * (dP - Dq) / 8.0
        return dict(s=s, mx=mx, lse=mx + torch.log(Z), P=P, dP=dP, Dq=Dq, dS=dS, dv=P.transpose(-1, -2) @ self.g, dq=dS @ self.k, dk=dS.transpose(-1, -2) @ self.q)

    def bounds(self, r, dtype, spatial):
        """bounds of dq, dk (in front of the rotation) and dv, per element: the derivation above, line by line"""
        n, e = self.n, EPS32
        nvis = float(n) if self.mask is None else (~self.mask).sum(-1, keepdim=True).double()         # keys a query sees
        ncol = float(n) if self.mask is None else (~self.mask).sum(0)[:, None].double()               # queries that see a key (rows of dk / dv)
        u, sub = (U[dtype] * (1 + 2.0 ** -10), SUBNORMAL[dtype]) if spatial else (0.0, 0.0)
        q, k, v, g = self.q.abs(), self.k.abs(), self.v.abs(), self.g.abs()
        P, dP, dS = r["P"], r["dP"].abs(), r["dS"].abs()
        s = r["s"].masked_fill(self.mask, 0.0) if self.mask is not None else r["s"]
        e_s = 2 * 66 * e * (q @ k.transpose(-1, -2)) / 8.0
        if spatial:
            x = 4 * e * (s.abs() + torch.maximum(r["lse"].abs(), r["mx"].abs())) * LOG2E
        else:
            x = ((s - r["mx"]).abs() + 2) * 2.0 ** -22
        num = e_s + x
        if self.mask is not None:
            num = num.masked_fill(self.mask, 0.0)
        rho = num + (P * num).sum(-1, keepdim=True) + (nvis + 4) * 2.0 ** -23
        eP = (u + rho) * P + 0.5 * sub + FLUSH32
        edP = 2 * 66 * e * (g @ v.transpose(-1, -2))
        if self.mask is not None:
            eP, edP = eP.masked_fill(self.mask, 0.0), edP.masked_fill(self.mask, 0.0)
        eDq = (P * edP).sum(-1, keepdim=True) + (rho * P * dP).sum(-1, keepdim=True) + (nvis + 2) * 2.0 ** -23 * (P * dP).sum(-1, keepdim=True)
        edS = (u + rho + 4 * e) * dS + P * (edP + eDq) / 8.0 + 0.5 * sub
        if self.mask is not None:
            edS = edS.masked_fill(self.mask, 0.0)
        t = lambda m: m.transpose(-1, -2)
        return dict(dv=t(eP) @ g + 2 * (ncol + 2) * e * (t(P) @ g), dq=edS @ k + 2 * (nvis + 2) * e * (dS @ k), dk=t(edS) @ q + 2 * (ncol + 2) * e * (t(dS) @ q))

    def design(self, p_dtype, wrong=None, trunc_ds=False):
        """dq, dk (in front of the rotation), dv and dS of a perfect kernel of the design (fp64 math, P and dS rounded to p_dtype where given), or of a WRONG one"""
        n, C = self.n, self.chunk
        mask = self.mask
        if wrong == "mask_plus":
            mask = torch.arange(n)[None, :] > torch.arange(n)[:, None] + 1
        elif wrong == "mask_minus":
            mask = torch.arange(n)[None, :] > (torch.arange(n)[:, None] - 1).clamp_min(0)
        s = self.scores(mask)
        vis = torch.ones(n, n, dtype=torch.bool) if mask is None else ~mask
        last = (vis * torch.arange(n)[None, :]).max(-1).values
        stat = vis.clone()                                   # the keys the row statistics include
        if wrong == "drop_last":
            stat[torch.arange(n), last] = False
            stat[:, 0] |= ~stat.any(-1)                      # (a query with one visible key keeps it)
        ss = s.masked_fill(~stat, float("-inf"))
        mx = ss.max(-1, keepdim=True).values
        if wrong == "stale_max":
            run = torch.full_like(mx, float("-inf"))
            Z = torch.zeros_like(mx)
            for c0 in range(0, n, C):
                blk = ss[..., c0:c0 + C]
                run = torch.maximum(run, blk.max(-1, keepdim=True).values)
                Z = Z + torch.exp(blk - run.masked_fill(run == float("-inf"), 0.0)).sum(-1, keepdim=True)      # the old sum is NOT rescaled to the new maximum
        else:
            Z = torch.exp(ss - mx).sum(-1, keepdim=True)
        lse = mx + torch.log(Z)
        P = torch.exp(s - lse)                               # every visible key, the one the statistics left out included
        dP = self.g @ self.v.transpose(-1, -2)
        dqm = stat.clone()
        if wrong == "dq_chunk":
            dqm[:, (n - 1) // C * C:] = False
        Dq = (torch.exp(ss - lse).masked_fill(~dqm, 0.0) * dP).sum(-1, keepdim=True)
        dS = P * (dP - Dq) / 8.0
        if p_dtype is not None:
            P = store_clamped(P, p_dtype).double()
            dS = (store_trunc(dS.clamp(-F16_MAX, F16_MAX) if p_dtype is F16 else dS, p_dtype) if trunc_ds else store_clamped(dS, p_dtype)).double()
        return dS @ self.k, dS.transpose(-1, -2) @ self.q, P.transpose(-1, -2) @ self.g, dS


def attn_bwd_inputs(NB, heads, S, kind, scale_log2, dtype):
    """q, k, v [NB][heads][S][64], dO [NB S][heads 64] in the operand type, the angles [S][32] of the launch's table.
    jump: per (item, head), key 5 + 64 n = (0.5 + 0.5 n) q[7] for every n (a maximum that RISES in every 64-key chunk: the rescale path of the streaming sweep and of
    every per-lane running maximum), then key S - 1 = 3 q[S - 1] (a dominant key in the last tile, which may be partial), then key 3 = 4 q[S / 2] (the maximum is met in
    the first chunk and nothing later moves it)."""
    q, k, v = (rand(NB, heads, S, 64, seed=i) for i in (1, 2, 3))
    do = rand(NB * S, heads * 64, seed=4) * 2.0 ** scale_log2
    if kind == "sharp":
        q = q * 6.0
    q = q.to(dtype)
    if kind == "jump":
        for n in range((S - 6) // 64 + 1):
            k[:, :, 5 + 64 * n] = (0.5 + 0.5 * n) * q[:, :, 7].float()
        k[:, :, S - 1] = 3.0 * q[:, :, S - 1].float()
        k[:, :, 3] = 4.0 * q[:, :, S // 2].float()
    return q, k.to(dtype), v.to(dtype), do.to(dtype), rand(S, 32, seed=5) * 3


class AttnBwdCase:
    """ref / tol [NB S][3 D] fp64: dq | dk | dv as the launch lays them out (column head 64 + d of each third).  peak: the largest |dS|, |dq|, |dk|, |dv| of the
    fp64 reference (dq / dk rotated) — the error word must stay 0 while it is below a quarter of the type's largest finite value."""

    def __init__(self, NB, heads, S, kind, scale_log2, dtype):
        self.NB, self.heads, self.S, self.kind, self.scale_log2, self.dtype = NB, heads, S, kind, scale_log2, dtype
        self.q, self.k, self.v, self.do, self.ang = attn_bwd_inputs(NB, heads, S, kind, scale_log2, dtype)
        self.cs = rope_cs(self.ang)
        self.co, self.si = self.cs[:, 0::2].double(), self.cs[:, 1::2].double()         # the fp32 table values: what the launch multiplies by
        g4 = self.do.double().reshape(NB, S, heads, 64).permute(0, 2, 1, 3)
        self.math = _AttnBwdMath(self.q.double(), self.k.double(), self.v.double(), g4, None, 64)
        r = self.math.reference()
        b = self.math.bounds(r, dtype, spatial=True)
        u, sub = U[dtype] * (1 + 2.0 ** -10), SUBNORMAL[dtype]
        outs = (unrope(r["dq"], self.co, self.si), unrope(r["dk"], self.co, self.si), r["dv"])
        tols = (unrope_bound(b["dq"], r["dq"], self.co, self.si), unrope_bound(b["dk"], r["dk"], self.co, self.si), b["dv"])
        self.ref = self.rows(*outs)
        self.tol = self.rows(*tols) + u * self.ref.abs() + sub
        self.max_ds = r["dS"].abs().max().item()
        self.peak = max(self.max_ds, self.ref.abs().max().item())
        self.pmax_median = r["P"].max(-1).values.median().item()

    def rows(self, dq, dk, dv):
        NB, heads, S = self.NB, self.heads, self.S
        return torch.cat([x.permute(0, 2, 1, 3).reshape(NB * S, heads * 64) for x in (dq, dk, dv)], dim=1).contiguous()

    def control(self, wrong=None, store=store_clamped, trunc_ds=False):
        """[NB S][3 D] in the operand type: the perfect kernel of the design (or a wrong one), see the head of this section"""
        dq, dk, dv, _ = self.math.design(self.dtype, wrong, trunc_ds)
        sign = -1.0 if wrong == "rope_sign" else 1.0
        out = self.rows(unrope(dq, self.co, self.si, sign), unrope(dk, self.co, self.si, sign), dv)
        return store(out.clamp(-F16_MAX, F16_MAX) if self.dtype is F16 else out, self.dtype)


@functools.lru_cache(maxsize=None)
def attn_bwd_case(NB, heads, S, kind, scale_log2, dtype):
    return AttnBwdCase(NB, heads, S, kind, scale_log2, dtype)


def temporal_bwd_inputs(B, P, D, T, Tmax, kind, dtype):
    """q [B][T][P][D], kv [B][Tmax][P][2][D], dO [B T P][D] in the operand type.  Per (sample, position, head): diagonal k_t = 3 q_t (every query is dominated by
    its own frame); first k_0 = 3 q_{T-1} (the last query's maximum is met at once and stays); ladder k_s = (0.5 + 0.25 s) q_{T-1} (its maximum rises with every
    key).  Cache frames from T on hold ordinary values no kernel reads."""
    q = rand(B, T, P, D, seed=1)
    kv = rand(B, Tmax, P, 2, D, seed=2)
    do = rand(B * T * P, D, seed=3)
    if kind == "sharp":
        q = q * 6.0
    q = q.to(dtype)
    qf = q.float()
    if kind == "diagonal":
        kv[:, :T, :, 0] = 3.0 * qf
    elif kind == "first":
        kv[:, 0, :, 0] = 3.0 * qf[:, T - 1]
    elif kind == "ladder":
        for s in range(T):
            kv[:, s, :, 0] = (0.5 + 0.25 * s) * qf[:, T - 1]
    return q, kv.to(dtype), do.to(dtype)


class TemporalBwdCase:
    """ref / tol [B T P][3 D] fp64, as AttnBwdCase; the table is temporal_rope_angles(Tmax), of which rows 0 .. T - 1 are used"""

    def __init__(self, B, P, D, T, Tmax, kind, dtype):
        self.args, self.kind, self.dtype = (B, P, D, T, Tmax), kind, dtype
        self.q, self.kv, self.do = temporal_bwd_inputs(B, P, D, T, Tmax, kind, dtype)
        self.cs = rope_cs(temporal_rope_angles(Tmax))
        self.co, self.si = self.cs[:T, 0::2].double(), self.cs[:T, 1::2].double()
        h = D // 64
        item = lambda x: x.double().reshape(B, T, P, h, 64).permute(0, 2, 3, 1, 4)             # B P h T 64
        mask = torch.arange(T)[None, :] > torch.arange(T)[:, None]
        self.math = _AttnBwdMath(item(self.q), item(self.kv[:, :T, :, 0]), item(self.kv[:, :T, :, 1]), item(self.do.reshape(B, T, P, D)), mask, 1)
        r = self.math.reference()
        b = self.math.bounds(r, dtype, spatial=False)
        u, sub = U[dtype] * (1 + 2.0 ** -10), SUBNORMAL[dtype]
        self.ref = self.rows(unrope(r["dq"], self.co, self.si), unrope(r["dk"], self.co, self.si), r["dv"])
        self.tol = self.rows(unrope_bound(b["dq"], r["dq"], self.co, self.si), unrope_bound(b["dk"], r["dk"], self.co, self.si), b["dv"]) + u * self.ref.abs() + sub
        self.max_ds = r["dS"].abs().max().item()
        self.peak = max(self.max_ds, self.ref.abs().max().item())

    def rows(self, dq, dk, dv):
        B, P, D, T, _ = self.args
        return torch.cat([x.permute(0, 3, 1, 2, 4).reshape(B * T * P, D) for x in (dq, dk, dv)], dim=1).contiguous()

    def control(self, wrong=None, store=store_clamped):
        dq, dk, dv, _ = self.math.design(None, wrong)
        sign = -1.0 if wrong == "rope_sign" else 1.0
        out = self.rows(unrope(dq, self.co, self.si, sign), unrope(dk, self.co, self.si, sign), dv)
        return store(out.clamp(-F16_MAX, F16_MAX) if self.dtype is F16 else out, self.dtype)


@functools.lru_cache(maxsize=None)
def temporal_bwd_case(B, P, D, T, Tmax, kind, dtype):
    return TemporalBwdCase(B, P, D, T, Tmax, kind, dtype)


# =======================================================================================================================================================
# The optimizer step (tests/test_gpu_ops_optimizer.py): sumsq_kernel, clip_coef_kernel and the three modes of adamw_multi_kernel (csrc/train.hip), through the
# hooks gtav_op_train_sumsq / _clip_coef / _adamw_multi.  Everything is fp32; u = EPS32 = 2^-24 is the unit roundoff, and every bound below is a COUNT of
# roundings times u times the magnitude the rounding acts on, to first order, times (1 + 2^-10) for the second-order terms (the largest first-order sum in
# this section is a few thousand u, whose square is far below 2^-10 of it).  Nothing here was fitted to what a GPU returned.
#
# Reference: fp64 AdamW with torch.optim.AdamW's semantics on the fp32 inputs, every hyperparameter and the coefficient c rounded to fp32 first (the C ABI passes
# floats):  gc = g c;  m = b1 m0 + (1 - b1) gc;  v = b2 v0 + (1 - b2) gc^2;  w = w0 (1 - lr wd) - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps).
#
# The kernel (one text for its three code paths):  gr = g * coef;  mm = beta1 * m + (1 - beta1) * gr;  vv = beta2 * v + (1 - beta2) * gr * gr;
#   decay = 1 - lr * wd;  step = lr / ctl[5];  rs2 = 1 / sqrtf(ctl[6]);  w = w * decay - step * mm / (sqrtf(vv) * rs2 + eps).  Division and square root are
#   correctly rounded; the compiler may contract any product into the following sum (one rounding fewer, never more).
#   m   gr, 1 - b1, two products, the sum: 4 roundings, and m0 and gc may cancel, so the magnitude is |b1 m0| + |(1 - b1) gc|, not |m|
#   v   gr (twice: it is squared), 1 - b2, two products of the second term, the sum: 6 roundings on non-negative terms, so 6 u v
#   w   first term: decay (the inner product lr wd is below 2^-6, its rounding does not reach decay's last bit: 1, counted as 2), the product, the final
#       subtraction: 4 u |w0 decay|.  Update q = step mm / den: step 1 (+ rho1, below), the product 1, the quotient 1, the final subtraction 1, and den =
#       sqrt(vv) rs2 + eps, a sum of positive terms: half of v's 6, sqrtf 1, rs2 2 (+ rho2 / 2), the product 1, the sum 1 = 8: (12 u + rho1 + rho2 / 2) |q|.
#       And the error already in mm, an ABSOLUTE one because of the cancellation: (lr / bc1) / den times m's bound.
#
# The bias corrections are a documented property of the design: clip_coef_kernel computes 1 - powf(beta, t) in fp32.  powf may be off by POWF_ULPS = 2 units in
# the last place of beta^t (the HIP math tables give powf 1 ulp; 2 allows for one more, as the file doubles every undocumented rounding), the subtraction
# rounds once more, so |ctl[5 | 6] - (1 - beta^t)| <= bc_allowed(beta, t) = 2 ulp(beta^t) + u (1 - beta^t), and rho = bc_allowed / (1 - beta^t) is what the
# step size (rho1) and, through the square root, the denominator (rho2 / 2) inherit.  At t = 2, 3 and beta2 = 0.999 the cancellation makes rho2 about 2000 u
# (1 - beta2^2 = 0.002, ulp(0.998) = 2^-24 = 2 u), at t >= 1000 it is below 8 u.  The GPU test holds ctl[5] and ctl[6] themselves to bc_allowed.
#
# Averaged weights (mode 1): e = fmaf(d, e0, (1 - d) * w) on the master the launch wrote: EMA_ROUNDINGS = 3 (1 - d, the product, the fma), each of a value no
# larger than max(|e0|, |w|) — the recurrence bound tests/test_gpu_train_ema.py sums over its steps (ema_step_bound, moved here from there).
#
# Sum of squares: every term is >= 0, so the bound is relative: (the longest chain of roundings a term passes) u.  sumsq_kernel: the square 1, the per-thread
# loop ceil(n / 4 / threads) adds, the folds of the four accumulators and of the four lanes 2 + 2, the n % 4 tail 3 more adds on thread 0, block_sum 6 + 4
# (a 64-lane tree, then the four waves in order); clip_coef_kernel: ceil(parts / 256) adds and block_sum again: sumsq_depth(n).  The norm takes half of that
# (the square root) + sqrtf + the product with inv_scale; the clipped coefficient the norm's + the sum with 1e-6, the quotient and the product.
# =======================================================================================================================================================
SECOND_ORDER = 1.0 + 2.0 ** -10
F32_MIN_SUB = 2.0 ** -149
POWF_ULPS = 2
EMA_ROUNDINGS = 3             # DESIGN.md 7 "Averaged weights"
ERR_NONFINITE = 4             # csrc/common.h
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-7                      # oracle/ref_cpu.py adamw_reference
ADAM_SETTINGS = {"base": dict(lr=1e-3, wd=0.01), "nowd": dict(lr=1e-2, wd=0.0)}
ADAM_INV_SCALE = 2.0 ** -16                                    # loss scale 2^16, folded into the coefficient
ADAM_COEFS = ("unclipped", "clipped")                          # max_norm = 0 (ctl[1] = inv_scale bit for bit) / max_norm = 0.9 of the norm (coefficient near 0.9 inv_scale)
ADAM_STARTS = ("fresh", 1000, 100000)                          # zero moments and t = 1, 2, 3 in sequence / non-trivial moments and ctl[4] = t - 1
ADAM_FRESH_STEPS = 3
# (kind, R, C): "gemm" has both images, "gemm_nowt" no W^T (the patch embedding's form), "f32" trains in place (w16 null), "f32_strided" is a view with ldp = 1024
# whose 24-float gaps hold NaN.  GEMM and fp32 parameters alternate, so an item's parameter index is never its position in a sorted list.
ADAM_PARAMS = [("gemm", 64, 64), ("f32", 1, 1), ("gemm", 128, 192), ("f32", 1, 4095), ("gemm", 65, 64), ("f32", 1, 4096), ("gemm", 16, 64), ("f32", 1, 4097),
               ("gemm", 64, 68), ("f32", 1, 8193), ("gemm", 256, 100), ("f32_strided", 3, 1000), ("gemm", 70, 66), ("gemm_nowt", 65, 64)]
ADAM_STRIDED_LDP = 1024
# "one arithmetic": the same 16 x 64 values in an interior tile (parameter 2, tile (1, 1)), an element-wise tile (parameter 12: C % 4 != 0) and an fp32 run
# (parameter 7, elements 0 .. 1023) of the same launch
ADAM_PROBE = {"interior": (2, slice(64, 80), slice(64, 128)), "edge": (12, slice(0, 16), slice(0, 64)), "run": (7, slice(0, 1), slice(0, 1024))}
ADAM_BEYOND_F16 = (70000.0, -100000.0, 65520.0, -65504.0)      # masters at elements 3 .. 6 of every GEMM weight: clamped in the fp16 image, never inf


def f32(x):
    return float(np.float32(x))


def round_up(a, b):
    return (a + b - 1) // b * b


def ulp32(x):
    """one unit in the last place of the fp32 number nearest to x > 0 (0 where x underflows fp32 altogether)"""
    return 2.0 ** max(math.floor(math.log2(x)) - 23, -149) if x > 0.0 else 0.0


def bc_ref(beta, t):
    return 1.0 - f32(beta) ** t


def bc_allowed(beta, t):
    return POWF_ULPS * ulp32(f32(beta) ** t) + EPS32 * bc_ref(beta, t)


def bc_emulate(beta, t, ulps=0):
    """1 - powf(beta, t) in fp32 with the powf that is as far above (ulps > 0) or below (ulps < 0) the true power as |ulps| units in the last place allow"""
    true = f32(beta) ** t
    p = np.float32(true)
    while ulps:
        q = np.nextafter(p, np.float32(2.0 if ulps > 0 else -1.0), dtype=np.float32)
        if abs(float(q) - true) > abs(ulps) * ulp32(true):
            break
        p = q
    return float(np.float32(1.0) - p)


def ema_step_bound(e_prev, w):
    """one applied step of e = fmaf(d, e_prev, (1 - d) w) against the fp64 recurrence on the same fp32 masters"""
    return EMA_ROUNDINGS * EPS32 * torch.maximum(e_prev.double().abs(), w.double().abs())


def adam_reference(w0, g, m0, v0, coef, t, lr, wd):
    """-> dict of fp64 tensors: the references w, m, v and the bounds tol_w, tol_m, tol_v (the head comment of this section)"""
    b1, b2, eps, lr, wd, coef = f32(ADAM_BETAS[0]), f32(ADAM_BETAS[1]), f32(ADAM_EPS), f32(lr), f32(wd), f32(coef)
    w0, g, m0, v0 = (x.double() for x in (w0, g, m0, v0))
    gc = g * coef
    m = b1 * m0 + (1.0 - b1) * gc
    v = b2 * v0 + (1.0 - b2) * gc * gc
    bc1, bc2 = bc_ref(b1, t), bc_ref(b2, t)
    den = v.sqrt() / math.sqrt(bc2) + eps
    q = (lr / bc1) * m / den
    decay = 1.0 - lr * wd
    u = EPS32 * SECOND_ORDER
    tol_m = 4 * u * ((b1 * m0).abs() + ((1.0 - b1) * gc).abs()) + F32_MIN_SUB
    tol_v = 6 * u * v + F32_MIN_SUB
    rho1, rho2 = bc_allowed(b1, t) / bc1, bc_allowed(b2, t) / bc2
    tol_w = SECOND_ORDER * (4 * EPS32 * (w0 * decay).abs() + (12 * EPS32 + rho1 + 0.5 * rho2) * q.abs() + (lr / bc1) / den * tol_m) + F32_MIN_SUB
    return dict(w=w0 * decay - q, m=m, v=v, tol_w=tol_w, tol_m=tol_m, tol_v=tol_v)


ADAM_WRONG = ("eps_in_sqrt", "no_sqrt_bc2", "bc_t_minus_1", "decay_after", "m_unclipped", "v_unsquared", "no_decay_f32", "run_start")


def _fma(a, b, c):
    """a * b + c rounded once (the product of two fp32 numbers is exact in fp64; the double rounding of the sum moves a tie in one case in 2^29)"""
    return (a.double() * b.double() + c.double()).float()


def adam_emulate(w0, g, m0, v0, coef, t, lr, wd, contract, pow_ulps=0, wrong=None, is_f32=False, inv_scale=ADAM_INV_SCALE):
    """The kernel as designed, in float32 torch arithmetic (every operation rounded once; contract: every product the source leaves to the compiler fused into
    the following sum) -> (w, m, v) fp32.  wrong: one of ADAM_WRONG, a kernel that is subtly not the design."""
    F = lambda x: torch.tensor(x, dtype=torch.float32)
    b1, b2, eps, lr, wd, c = (F(x) for x in (ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, lr, wd, coef))
    tt = t - 1 if wrong == "bc_t_minus_1" else t
    bc1, bc2 = F(bc_emulate(ADAM_BETAS[0], tt, pow_ulps)), F(bc_emulate(ADAM_BETAS[1], tt, pow_ulps))
    one = F(1.0)
    gr = g * c
    gm = g * F(inv_scale) if wrong == "m_unclipped" else gr
    if contract:
        mm = _fma(b1, m0, (one - b1) * gm)
        vv = _fma(b2, v0, (one - b2) * gr) if wrong == "v_unsquared" else _fma((one - b2) * gr, gr, b2 * v0)
    else:
        mm = b1 * m0 + (one - b1) * gm
        vv = b2 * v0 + ((one - b2) * gr if wrong == "v_unsquared" else (one - b2) * gr * gr)
    decay = one - lr * wd
    if wrong == "no_decay_f32" and is_f32:
        decay = one
    step = lr / bc1
    rs2 = one / bc2 if wrong == "no_sqrt_bc2" else one / torch.sqrt(bc2)
    if wrong == "eps_in_sqrt":
        den = torch.sqrt(vv * (rs2 * rs2) + eps)
    else:
        den = _fma(torch.sqrt(vv), rs2, eps) if contract else torch.sqrt(vv) * rs2 + eps
    q = step * mm / den
    if wrong == "decay_after":
        w = (w0 - q) * decay
    else:
        w = _fma(w0, decay, -q) if contract else w0 * decay - q
    if wrong == "run_start" and is_f32 and w.numel() > 4096:          # every run but the first starts one element late: elements 4096, 8192, .. are never visited
        w, mm, vv = w.clone(), mm.clone(), vv.clone()
        for x, x0 in ((w, w0), (mm, m0), (vv, v0)):
            x.reshape(-1)[4096::4096] = x0.reshape(-1)[4096::4096]
    return w, mm, vv


def ema_emulate(e0, w, d):
    d = torch.tensor(d, dtype=torch.float32)
    return _fma(d, e0, (torch.tensor(1.0) - d) * w)


class AdamParamSpec:
    """shape and image geometry of one parameter, as gtav_dit_train_enable computes them: Cp16 = Slot::Cp = round_up(C, 64), the W image round_up(R, 128) rows
    of it, RpT = round_up(R, 64), the W^T image round_up(C, 128) * round_up(R, 64) elements"""

    def __init__(self, kind, R, C):
        self.kind, self.R, self.C = kind, R, C
        self.gemm, self.has_wT = kind.startswith("gemm"), kind == "gemm"
        self.ldp = ADAM_STRIDED_LDP if kind == "f32_strided" else C
        self.Cp16, self.RpT = (round_up(C, 64), round_up(R, 64)) if self.gemm else (0, 0)
        self.w16_elems = round_up(R, 128) * self.Cp16
        self.wT_elems = round_up(C, 128) * self.RpT if self.has_wT else 0


class AdamCase:
    """One launch over ADAM_PARAMS.  g is the SCALED gradient (what the arena holds): g inv_scale is sign x log-uniform over 1e-13 .. 1e3 (1e-12 .. 1e2 and more
    after either coefficient), 5 % exact zeros, 10 % within a decade of eps; weights N(0, 0.02) and ADAM_BEYOND_F16; the shadow e0 = w0 + N(0, 0.01).
    start "fresh": zero moments (a zero gradient there is the exact-zero case).  Otherwise m0 about gc (a fifth of them of the opposite sign: cancellation),
    v0 about gc^2, and small non-zero moments under the zero gradients."""

    def __init__(self, setting, coef_kind, start):
        self.setting, self.coef_kind, self.start = setting, coef_kind, start
        self.lr, self.wd = ADAM_SETTINGS[setting]["lr"], ADAM_SETTINGS[setting]["wd"]
        self.params = [AdamParamSpec(*p) for p in ADAM_PARAMS]
        self.steps = list(range(1, ADAM_FRESH_STEPS + 1)) if start == "fresh" else [start]
        self.w0, self.g, self.m0, self.v0, self.e0 = [], [], [], [], []
        for i, p in enumerate(self.params):
            gen = torch.Generator().manual_seed(1000 + i)
            n = p.R * p.C
            r = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
            mag = 10.0 ** (r() * 16.0 - 13.0)
            pick = r()
            mag = torch.where(pick < 0.10, ADAM_EPS * 10.0 ** (r() - 0.5), mag)
            mag = torch.where(pick > 0.95, torch.zeros_like(mag), mag)
            sign = torch.where(r() < 0.5, -1.0, 1.0)
            gc = (sign * mag).float()
            w0 = torch.randn(n, generator=gen) * 0.02
            if p.gemm:
                w0[3:3 + len(ADAM_BEYOND_F16)] = torch.tensor(ADAM_BEYOND_F16)
            if start == "fresh":
                m0, v0 = torch.zeros(n), torch.zeros(n)
            else:
                flip = torch.where(r() < 0.2, -1.0, 1.0)
                m0 = (gc.double() * (0.5 + r()) * flip).float()
                v0 = (gc.double() ** 2 * (0.5 + 1.5 * r())).float()
                zero = gc == 0
                m0 = torch.where(zero, (torch.randn(n, generator=gen) * 1e-3), m0)
                v0 = torch.where(zero, (1e-6 * (0.5 + r())).float(), v0)
            e0 = w0 + torch.randn(n, generator=gen) * 0.01
            g = gc * (1.0 / ADAM_INV_SCALE)                                      # (a power of two: exact)
            for lst, x in zip((self.w0, self.g, self.m0, self.v0, self.e0), (w0, g, m0, v0, e0)):
                lst.append(x.reshape(p.R, p.C).clone())
        for lst in (self.w0, self.g, self.m0, self.v0, self.e0):
            pi, rs, cs = ADAM_PROBE["interior"]
            probe = lst[pi][rs, cs].clone()
            for where in ("edge", "run"):
                pj, rs2, cs2 = ADAM_PROBE[where]
                lst[pj][rs2, cs2] = probe.reshape(lst[pj][rs2, cs2].shape)
        for i, p in enumerate(self.params):                                      # a run boundary is never a zero gradient: the off-by-one run must show
            if not p.gemm and p.R * p.C > 4096:
                self.g[i].reshape(-1)[4095::4096] = 1e-3 / ADAM_INV_SCALE
                self.g[i].reshape(-1)[4096::4096] = -2e-3 / ADAM_INV_SCALE
        self.g_flat = torch.cat([x.reshape(-1) for x in self.g])                 # the gradient arena, parameter after parameter
        self.norm64 = math.sqrt((self.g_flat.double() ** 2).sum().item()) * ADAM_INV_SCALE
        self.max_norm = 0.0 if coef_kind == "unclipped" else f32(0.9 * self.norm64)

    def probe(self, tensors, where):
        pi, rs, cs = ADAM_PROBE[where]
        return tensors[pi][rs, cs].reshape(-1)


@functools.lru_cache(maxsize=None)
def adam_case(setting, coef_kind, start):
    return AdamCase(setting, coef_kind, start)


# ---- the sum of squares ---------------------------------------------------------------------------------------------------------------------------------------
SUMSQ_N = (1, 3, 4, 5, 2047, 2048, 2049, 8 * 2048 + 3, 2 ** 20 + 1)
SUMSQ_SPECIAL_N = (2049 + 2, 8 * 2048 + 3)                     # n % 4 == 3: the tail is elements n - 3 .. n - 1
SUMSQ_SPECIALS = tuple((v, where) for v in ("inf", "nan") for where in ("tail", "body"))


def sumsq_parts(n):
    return min(max((n + 2047) // 2048, 1), 4096)                # csrc/train.hip sumsq_parts


def sumsq_depth(n, parts=None):
    """the longest chain of roundings between a term and ctl[0] (the head comment of this section)"""
    parts = sumsq_parts(n) if parts is None else parts
    per_thread = -(-(n // 4) // (parts * 256)) if n >= 4 else 0
    return 1 + per_thread + 4 + 3 + 10 + -(-parts // 256) + 10


def _tree64(x):
    """[.., 64] -> [..]: wave_sum_dpp, a balanced tree (lanes, quads, half rows, rows, row pairs, all)"""
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _block_sum(x):
    """[blocks, 256] -> [blocks]: the 64-lane tree of every wave, then the four waves in order from 0"""
    wv = _tree64(x.reshape(-1, 4, 64))
    t = torch.zeros(wv.shape[0])
    for i in range(4):
        t = t + wv[:, i]
    return t


def parts_sum_emulate(part):
    """clip_coef_kernel's sum of the partial sums: thread j adds parts j, j + 256, .. in order, then block_sum"""
    n = part.numel()
    pad = torch.zeros(round_up(n, 256))
    pad[:n] = part
    a = torch.zeros(256)
    for row in pad.reshape(-1, 256):
        a = a + row
    return _block_sum(a[None])[0]


class SumsqCase:
    """n values, sign x log-uniform over 12 decades (1e-6 .. 1e6); ref: the fp64 sum of squares; tol: sumsq_depth(n) u ref.  special (value, where): ONE element is
    inf or NaN, in the n % 4 tail (the last element) or in the body (element 5)"""

    def __init__(self, n, special=None):
        self.n, self.special = n, special
        gen = torch.Generator().manual_seed(n)
        mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 12.0 - 6.0)
        self.g = (mag * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)).float()
        if special:
            assert n % 4 and n > 8
            self.g[n - 1 if special[1] == "tail" else 5] = float(special[0])
        self.parts = sumsq_parts(n)
        self.ref = (self.g.double() ** 2).sum().item()
        self.tol = sumsq_depth(n) * EPS32 * SECOND_ORDER * self.ref

    def emulate(self, contract=False, wrong=None):
        """sumsq_kernel, then clip_coef_kernel's sum -> ctl[0] as a float.  wrong: "tail_dropped" / "tail_twice" """
        n, n4, threads = self.n, self.n // 4, self.parts * 256
        rows = -(-n4 // threads) if n4 else 0
        g4 = torch.zeros(max(rows, 1) * threads, 4)
        g4.reshape(-1)[:n4 * 4] = self.g[:n4 * 4]
        g4 = g4.reshape(max(rows, 1), threads, 4)
        idx = torch.arange(threads)
        cnt = torch.where(idx < n4, (n4 - 1 - idx) // threads + 1, torch.zeros_like(idx))            # float4 rows of thread idx: idx, idx + threads, ..
        acc = [torch.zeros(threads, 4) for _ in range(4)]
        add = (lambda a, v: _fma(v, v, a)) if contract else (lambda a, v: a + v * v)
        for k in range(rows):
            # the unrolled loop runs while four rows are left (row k goes to accumulator k % 4 of that group), the remainder loop adds into a0
            in_group = (k // 4 * 4 + 3 < cnt)[:, None]
            live = (k < cnt)[:, None]
            for j in range(4):
                tgt = (in_group & (k % 4 == j)) | (~in_group & (j == 0))
                acc[j] = torch.where(live & tgt, add(acc[j], g4[k]), acc[j])
        q = (acc[0] + acc[1]) + (acc[2] + acc[3])
        a = (q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])
        tail = self.g[n4 * 4:]
        for rep in range({"tail_dropped": 0, "tail_twice": 2}.get(wrong, 1)):
            for x in tail:
                a[0] = _fma(x, x, a[0]) if contract else a[0] + x * x
        return parts_sum_emulate(_block_sum(a.reshape(self.parts, 256))).item()


@functools.lru_cache(maxsize=None)
def sumsq_case(n, special=None):
    return SumsqCase(n, special)


# ---- the coefficient ------------------------------------------------------------------------------------------------------------------------------------------
class ClipCase:
    """One launch of clip_coef_kernel on caller-made partial sums.  expect(): what every word must hold afterwards.
      skip        a non-finite sum, or ERR_F16_SAT / ERR_NONFINITE in the error word: ctl[1] = 0, ctl[2] one higher, ctl[4 .. 7] keep their bits, the two bits
                  are cleared and every other bit of the word survives
      applied     ctl[1] = inv_scale BIT FOR BIT when max_norm = 0 or the norm is below it, else inv_scale max_norm / (norm + 1e-6) within coef_tol; ctl[4] one
                  higher, ctl[5] / ctl[6] within bc_allowed of 1 - beta^t, ctl[7] = train.ema_decay_at(t) bit for bit with ema_decay > 0 and untouched without
      both        ctl[0] the sum within (chain of the parts' sum) u, ctl[3] the unscaled norm (or non-finite as the sum is)"""
    CTL_IN = (-1.0, -2.0, 7.0, -3.0, 41.0, 0.25, 0.125, 0.0625)      # what ctl holds before: every word recognisable, 41 applied and 7 skipped steps
    OTHER_BIT = 1                                                    # ERR_TIMESTEP: not the optimizer's to clear

    def __init__(self, name, ssq, nparts, inv_scale, max_norm, err_bits=None, ema_decay=0.0, warmup=False, special=None):
        self.name, self.inv_scale, self.max_norm, self.ema_decay, self.warmup = name, f32(inv_scale), f32(max_norm), f32(ema_decay), warmup
        gen = torch.Generator().manual_seed(nparts)
        share = torch.rand(nparts, generator=gen, dtype=torch.float64) + 0.1
        self.part = (share / share.sum() * ssq).float()
        if special:
            self.part[nparts // 2] = float(special)
        self.err_in = None if err_bits is None else (err_bits | self.OTHER_BIT)
        self.ssq = self.part.double().sum().item()
        self.finite = math.isfinite(self.ssq)
        self.depth = -(-nparts // 256) + 10
        self.norm = math.sqrt(self.ssq) * self.inv_scale if self.finite else self.ssq
        self.skip = not self.finite or bool((self.err_in or 0) & (ERR_F16_SAT | ERR_NONFINITE))
        self.t = self.CTL_IN[4] + 1
        u = EPS32 * SECOND_ORDER
        self.ssq_tol = self.depth * u * self.ssq if self.finite else None
        self.norm_tol = (self.depth / 2 + 2) * u * self.norm if self.finite else None
        self.clipped = self.finite and self.max_norm > 0.0 and self.norm + 1e-6 > self.max_norm
        if self.clipped:
            self.coef = self.inv_scale * self.max_norm / (self.norm + f32(1e-6))
            self.coef_tol = (self.depth / 2 + 5) * u * self.coef
            assert self.norm * (1 - 1e-3) > self.max_norm                    # (never a norm so close to the threshold that a rounding decides)
        else:
            self.coef = self.inv_scale
            assert self.max_norm == 0.0 or not self.finite or self.norm * (1 + 1e-3) < self.max_norm

    def emulate(self, wrong=None):
        """ctl[1] of an applied step in fp32.  wrong: "no_1e-6" """
        F = lambda x: torch.tensor(x, dtype=torch.float32)
        norm = torch.sqrt(parts_sum_emulate(self.part)) * F(self.inv_scale)
        if not self.max_norm > 0.0:
            return self.inv_scale
        den = norm if wrong == "no_1e-6" else norm + F(1e-6)
        return (F(self.inv_scale) * torch.minimum(F(1.0), F(self.max_norm) / den)).item()


S, N = ERR_F16_SAT, ERR_NONFINITE
CLIP_CASES = {c.name: c for c in (
    ClipCase("no clipping", 3.0e9, 9, 2.0 ** -16, 0.0),
    ClipCase("below max_norm", 3.0e9, 300, 2.0 ** -16, 2.0, err_bits=0),
    ClipCase("above max_norm", 3.0e9, 257, 2.0 ** -16, 0.25, err_bits=0, ema_decay=0.999),
    ClipCase("above max_norm, warm-up", 3.0e9, 1, 2.0 ** -16, 0.25, ema_decay=0.9999, warmup=True),
    ClipCase("warm-up past its end", 3.0e9, 8, 2.0 ** -16, 0.0, ema_decay=0.5, warmup=True),
    ClipCase("small norm", 1.0e-6, 5, 1.0, 1.0e-4),                          # norm 1e-3: the one place where the 1e-6 of the denominator is a part in a thousand
    ClipCase("inf sum", 3.0e9, 300, 2.0 ** -16, 1.0, err_bits=0, ema_decay=0.999, special="inf"),
    ClipCase("nan sum", 3.0e9, 9, 2.0 ** -16, 0.0, special="nan"),
    ClipCase("saturation bit", 3.0e9, 9, 2.0 ** -16, 1.0, err_bits=S, ema_decay=0.999),
    ClipCase("non-finite bit", 3.0e9, 9, 2.0 ** -16, 0.0, err_bits=N),
    ClipCase("both bits", 3.0e9, 9, 2.0 ** -16, 1.0, err_bits=S | N, ema_decay=0.999, warmup=True),
)}
del S, N


# =======================================================================================================================================================
# The skinny fp32 GEMM (csrc/skinny.hip): Y = act(X W^T + bias) on v_mfma_f32_16x16x4_f32, shared by tests/test_gpu_ops.py test_skinny_f32 and
# tests/test_host_parity_bounds.py.  Two assertions per case:
#   per element against fp64:  |pre - ref| <= sum_bound(K, sum_k |x w|, mfma=True)  +  eps (sum_k |x w| + |b|)   (the one rounding of the bias add; no bias, no term)
#     act = 1 (SiLU): that bound times the slope s (1 + |x| (1 - s)) >= |d/dx x sigmoid(x)| (the magnitudes SiluCase's derivative bound uses), plus SiluCase's
#     evaluation error 10 eps |ref| + SILU_ABS.  First order, like every bound of this file.
#   bit for bit across instantiations:  Y[m][n] depends on row m of X and row n of W only, and skinny.hip promises the same fp32 fma chain in the same order for every
#     (FT, RT, KC) — so 64 output columns of any case equal the output of the 64-feature problem on those rows of W, which plans to (act, 1, 1, 0).
# The chain, which skinny_emulate follows: per 32 columns of K, eight MFMAs; MFMA (h, e) adds the four products at k = kb + 16 h + 4 g + e, g = 0 .. 3, to the accumulator.
# =======================================================================================================================================================
# (M, N, K, act, call): call "" = contiguous rows and a bias; "ld" = ldx = K + 4 and ldy = N + 4 with NaN guard columns; "nobias" = bias == NULL (and "ld")
SKINNY_CASES = [
    (5, 1024, 256, 1, ""), (16, 6144, 1056, 0, "ld"), (37, 192, 1024, 1, "nobias"), (808, 6144, 1024, 0, ""), (131, 320, 1024, 1, "ld"),   # 808: the adaLN rows of a batch-8 frame; 131: a ragged last slab
    (16, 262148, 32, 0, "ld"),        # (0, 4, 1, 0); N % 16 == 4: a partly live last wave
    (20, 131076, 64, 1, ""),          # (1, 4, 1, 0)
    (48, 87556, 32, 1, "ld"),         # (1, 4, 2, 0): a ragged second slab
    (1000, 16388, 96, 0, "nobias"),   # (0, 8, 2, 0): K % 128 != 0 keeps it off the chunked path
    (40, 65540, 256, 0, "ld"),        # (0, 4, 5, 128): two K chunks; N = 65540: the last block has one live wave and three that only stage
    (90, 65540, 128, 0, "nobias"),    # (0, 4, 6, 128)
    (101, 65540, 256, 0, ""),         # (0, 4, 7, 128): the batch-1 frame's row count
    (200, 65540, 128, 0, "ld"),       # (0, 4, 6, 128): three row blocks, the last with 8 live rows
]
SKINNY_HOST_CASES = [(40, 68, 256, 0, True), (20, 68, 64, 1, True), (37, 132, 128, 0, False), (5, 64, 96, 1, False)]      # (M, N, K, act, bias): the CPU control's sizes


class SkinnyCase:
    def __init__(self, M, N, K, act, bias=True):
        self.M, self.N, self.K, self.act = M, N, K, act
        self.x, self.w = rand(M, K, seed=1), rand(N, K, seed=2, scale=1 / math.sqrt(K))
        self.b = rand(N, seed=3) if bias else None
        x, w = self.x.double(), self.w.double()
        pre, mag = x @ w.t(), x.abs() @ w.abs().t()
        tol = sum_bound(K, mag, mfma=True)
        if bias:
            pre = pre + self.b.double()
            tol = tol + EPS32 * (mag + self.b.double().abs())
        del mag
        if act:
            s, s1 = torch.sigmoid(pre), torch.sigmoid(-pre)
            self.ref = pre * s
            self.tol = s * (1.0 + pre.abs() * s1) * tol + 10 * EPS32 * self.ref.abs() + SILU_ABS
        else:
            self.ref, self.tol = pre, tol

    def windows(self, ft):
        """first columns of the three 64-column windows of the bit-equality check: the first block, a block boundary inside N (blocks are 64 FT features wide; the
        middle of N where there is one block only), the last 64 columns with the ragged tail"""
        N = self.N
        mid = 64 * ft - 32 if N >= 64 * ft + 32 else max(0, (N // 2 - 32) // 4 * 4)
        return sorted({0, mid, N - 64})


def skinny_emulate(x, w, b, act, wrong=None):
    """the kernel's chain in fp32 arithmetic.  wrong: "chunk" = the last 128 columns of K left out (a dropped last K chunk), "bias2" = the bias added twice"""
    M, K = x.shape
    N = w.shape[0]
    if wrong == "chunk":
        K -= 128
    xr, wr = x[:, :K].reshape(M, K // 32, 2, 4, 4), w[:, :K].reshape(N, K // 32, 2, 4, 4)      # [..][kb][h][g][e]
    acc = torch.zeros(M, N)
    for kb in range(K // 32):
        for h in range(2):
            for e in range(4):
                p = xr[:, None, kb, h, :, e] * wr[None, :, kb, h, :, e]
                acc = acc + (((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3])
    if b is not None:
        acc = acc + b
        if wrong == "bias2":
            acc = acc + b
    return acc / (1.0 + torch.exp(-acc)) if act else acc


def skinny_case(M, N, K, act, bias=True):
    """(not kept: the large cases hold hundreds of MB of fp64)"""
    return SkinnyCase(M, N, K, act, bias)


# =======================================================================================================================================================
# The declared launch plans.  Every instantiation a non-GEMM launcher can pick computes the same result, so a parity test cannot see which one it ran; and a
# kernel that no parity test ever runs is compared with nothing.  op_rows() lists every op-level parity problem of the families of csrc/launch_plan.h — the
# tables above as they are, and the lists that stood inline in tests/test_gpu_ops.py — each with the arguments of gtav_op_launch_plan and the plan it is
# DECLARED to produce: the instantiation (family number of LaunchFamily, a, b, c, d) and, for spatial and temporal attention, the launch form.
#   tests/test_host_op_coverage.py (CPU): the library returns the declared plan for every row; per family the declared instantiations are the product list of
#     launch_plan.h but for a literal list of exceptions; every launch form occurs on every instantiation that can take it.
#   The GPU tests take their problems from these tables only and call helpers.assert_declared_plan before a launch: a problem that is not declared fails there,
#     and so does a library on the GPU machine that plans otherwise than the CPU test proved.
# Launch forms.  One-pass spatial kernel: "qsplit=1" (one block per (frame, head): from 512 pairs on) / "qsplit>1" (the query tiles split over grid y); NK = 2 and 4
# have at most four query tiles and never split.  Register-resident temporal kernel: "one" (Tq = 1), "split" (one block per query frame: fewer than 1024
# columns), "loop" (Tq > 1 in one block: 1024 columns or more).  Every other kernel has one form, None.
# =======================================================================================================================================================
LN_OPS_SHAPES = [(128, 96), (256, 96), (512, 96), (1024, 96), (2048, 160), (1024, 2304), (1024, 1027), (1024, 46080)]      # tests/test_gpu_ops.py test_layernorm_kernels: (D, M); 46 080: the batched VAE's rows
LN_LARGE_MEAN_D, LN_LARGE_MEAN_M = (128, 1024), 64
# every descriptor tests/test_gpu_ops_ln_pending.py launches: (case, slabs, output row permutation, k_save, k_load)
LN_PEND_LAUNCHES = [(n, 1, 0, 0, 0) for n in ("d64", "d192", "d1280", "d1792", "d2048", "d1024_step", "d1024_train")] + \
                   [("d256_rows", 1, 1, 0, 0), ("d256_rows", 1, 0, 0, 0), ("d1280_tperm", 1, 1, 0, 0), ("d1280_tperm", 1, 0, 0, 0), ("d256_tperm", 0, 1, 0, 0), ("d256_tperm", 0, 0, 0, 0),
                    ("d1024_train", 1, 0, 1, 0), ("d1024_train", 0, 0, 0, 1), ("d192_train", 1, 0, 1, 0), ("d192_train", 1, 0, 0, 0), ("d192_train", 0, 0, 0, 1), ("sat", 1, 0, 0, 0)]
ATTN_PRESCALED_S = [200, 576]
# (NB, heads, S, prescaled) beyond ATTN_S at 2 x 3: what each selects is declared below
ATTN_EXTRA = [(2, 3, 40, 0), (2, 3, 104, 0), (2, 3, 184, 0), (2, 3, 184, 1), (2, 3, 256, 1),                # NK = 4, NK = 8, <3,3,1,*>, <2,3,0,1>
              (64, 4, 256, 0), (64, 4, 256, 1), (64, 4, 200, 0), (64, 4, 200, 1),                           # NQT = 4: a padding tie once NB heads nqb >= 512
              (128, 4, 72, 0), (128, 4, 104, 0), (128, 4, 144, 0)]                                          # qsplit == 1: 512 (frame, head) pairs, the batch-8 launch
ATTN_OPS_SHAPES = [(5, 16, 144), (2, 16, 576), (3, 4, 32), (1, 2, 72), (1, 2, 200), (3, 8, 256), (1, 3, 328), (5, 16, 576), (1, 2, 1152)]    # tests/test_gpu_ops.py test_attention_spatial
ATTN_OPS_SPIKE = (1, 1, 144)
ATTN_OPS_JUMP = [(576, 4.0), (576, 0.45), (200, 4.0)]                                                        # (S, jump) at 2 x 3
TEMPORAL_OPS_GEOMETRY, TEMPORAL_OPS_WINDOWS = (2, 24, 256, 5), [(5, 0), (1, 4), (2, 1), (1, 0)]             # tests/test_gpu_ops.py test_attention_temporal: (B, P, D, Tmax), (Tq, t0)
ATTN_BWD_OPS_SHAPES = [(3, 2, 144), (2, 4, 32), (1, 1, 160)]                                                 # tests/test_gpu_ops.py test_attention_spatial_backward_mfma
LN_BWD_LARGE_MEAN = [(256, 2, 24), (1024, 2, 24)]

OP_KIND = {"layernorm": 0, "attn_spatial": 1, "attn_temporal": 2, "attn_spatial_bwd": 3, "attn_temporal_bwd": 4, "skinny": 5, "gemm_tn_f32": 6, "gemm_nn_f32": 7,
           "ada_bwd_dx": 8, "ln_mod_bwd_fused": 9}
LF_ATTN_1P, LF_ATTN_T = 2, 4            # csrc/launch_plan.h LaunchFamily: the two kernels with more than one launch form


def op_problems():
    """(family, arguments of gtav_op_launch_plan, the table the problem comes from), one per problem and table"""
    out = []
    for D, M in LN_SHAPES + LN_OPS_SHAPES:
        out += [("layernorm", (mode, M, D, 0, 0, 0, 0), "LN_SHAPES / LN_OPS_SHAPES") for mode in (0, 1)]
    out += [("layernorm", (1, LN_LARGE_MEAN_M, D, 0, 0, 0, 0), "LN_LARGE_MEAN_D") for D in LN_LARGE_MEAN_D]
    for name, slabs, perm, k_save, k_load in LN_PEND_LAUNCHES:
        c = dict(D=64, M=8, mode=0) if name == "sat" else LN_PEND_CASES[name]
        out.append(("layernorm", (c["mode"], c["M"], c["D"], slabs, perm, k_save, k_load), "LN_PEND_LAUNCHES"))
    out += [("attn_spatial", (ATTN_NB, ATTN_HEADS, S, 0), "ATTN_S") for S in ATTN_S]
    out += [("attn_spatial", (ATTN_NB, ATTN_HEADS, S, 1), "ATTN_PRESCALED_S") for S in ATTN_PRESCALED_S]
    out += [("attn_spatial", a, "ATTN_EXTRA") for a in ATTN_EXTRA]
    out += [("attn_spatial", a + (0,), "ATTN_OPS_SHAPES") for a in ATTN_OPS_SHAPES + [ATTN_OPS_SPIKE]]
    out += [("attn_spatial", (ATTN_NB, ATTN_HEADS, S, 0), "ATTN_OPS_JUMP") for S in sorted({s for s, _ in ATTN_OPS_JUMP})]
    out += [("attn_temporal", a, "TEMPORAL_CASES") for a in TEMPORAL_CASES]
    B, P, D, Tmax = TEMPORAL_OPS_GEOMETRY
    out += [("attn_temporal", (B, P, D, Tq, t0, Tmax), "TEMPORAL_OPS_WINDOWS") for Tq, t0 in TEMPORAL_OPS_WINDOWS]
    out += [("attn_spatial_bwd", a, "ATTN_BWD_SHAPES / ATTN_BWD_OPS_SHAPES") for a in ATTN_BWD_SHAPES + ATTN_BWD_OPS_SHAPES]
    out += [("attn_temporal_bwd", (B, P, D, T), "TEMPORAL_BWD_SHAPES") for B, P, D, T, _ in TEMPORAL_BWD_SHAPES]
    out += [("skinny", (M, N, K, act), "SKINNY_CASES") for M, N, K, act, _ in SKINNY_CASES]
    out += [("gemm_tn_f32", a[:3], "GEMM_TN_F32_*") for a in GEMM_TN_F32_MFMA + GEMM_TN_F32_VALU]
    out += [("gemm_nn_f32", a, "GEMM_NN_F32") for a in GEMM_NN_F32]
    out += [("ada_bwd_dx", a, "ADA_BWD_*") for a in ADA_BWD_MFMA + ADA_BWD_VALU]
    out += [("ln_mod_bwd_fused", (f, P, D), "LN_BWD_SHAPES / LN_BWD_LARGE_MEAN") for D, f, P in LN_BWD_SHAPES + LN_BWD_LARGE_MEAN if D in LN_BWD_FUSED_D]
    seen, rows = set(), []
    for r in out:
        if r[:2] not in seen:
            seen.add(r[:2])
            rows.append(r)
    return rows


def plan_form(family, args, plan12):
    """the launch form of a plan (the twelve integers of gtav_op_launch_plan), None for a kernel that has one form only"""
    if family == "attn_spatial" and plan12[0] == LF_ATTN_1P:
        return "qsplit=1" if plan12[9] == 1 else "qsplit>1"
    if family == "attn_temporal" and plan12[0] == LF_ATTN_T:
        return "one" if args[3] == 1 else "split" if plan12[9] == 1 else "loop"
    return None


def query_plan(lib, family, args):
    """gtav_op_launch_plan of `lib` (a ctypes library that exports it) -> ((family number, a, b, c, d), form)"""
    import ctypes
    out = (ctypes.c_int32 * 12)()
    rc = lib.gtav_op_launch_plan(OP_KIND[family], *(tuple(args) + (0,) * (7 - len(args))), out)
    assert rc == 0, (family, args, "refused")
    return tuple(out[:5]), plan_form(family, args, list(out))


# (family, arguments) -> ((family number, a, b, c, d), form).  Written down, not computed: a planner rule that moves shows here, in a row that names what it
# was meant to run.  The comments name the kernel of each group.
DECLARED_PLANS = {
    # ---- layernorm
    ("layernorm", (0, 96, 128, 0, 0, 0, 0)): ((1, 0, 0, 0, 0), None),
    ("layernorm", (1, 96, 128, 0, 0, 0, 0)): ((1, 1, 0, 0, 0), None),
    ("layernorm", (0, 96, 256, 0, 0, 0, 0)): ((0, 0, 1, 0, 0), None),
    ("layernorm", (1, 96, 256, 0, 0, 0, 0)): ((0, 1, 1, 0, 0), None),
    ("layernorm", (0, 1027, 1024, 0, 0, 0, 0)): ((0, 0, 4, 0, 0), None),
    ("layernorm", (1, 1027, 1024, 0, 0, 0, 0)): ((0, 1, 4, 0, 0), None),
    ("layernorm", (0, 160, 2048, 0, 0, 0, 0)): ((0, 0, 8, 0, 0), None),
    ("layernorm", (1, 160, 2048, 0, 0, 0, 0)): ((0, 1, 8, 0, 0), None),
    ("layernorm", (0, 96, 1280, 0, 0, 0, 0)): ((1, 0, 0, 0, 0), None),
    ("layernorm", (1, 96, 1280, 0, 0, 0, 0)): ((1, 1, 0, 0, 0), None),
    ("layernorm", (0, 33, 1792, 0, 0, 0, 0)): ((1, 0, 0, 0, 0), None),
    ("layernorm", (1, 33, 1792, 0, 0, 0, 0)): ((1, 1, 0, 0, 0), None),
    ("layernorm", (0, 96, 512, 0, 0, 0, 0)): ((0, 0, 2, 0, 0), None),
    ("layernorm", (1, 96, 512, 0, 0, 0, 0)): ((0, 1, 2, 0, 0), None),
    ("layernorm", (0, 96, 1024, 0, 0, 0, 0)): ((0, 0, 4, 0, 0), None),
    ("layernorm", (1, 96, 1024, 0, 0, 0, 0)): ((0, 1, 4, 0, 0), None),
    ("layernorm", (0, 2304, 1024, 0, 0, 0, 0)): ((0, 0, 4, 0, 0), None),
    ("layernorm", (1, 2304, 1024, 0, 0, 0, 0)): ((0, 1, 4, 0, 0), None),
    ("layernorm", (0, 46080, 1024, 0, 0, 0, 0)): ((0, 0, 4, 0, 0), None),
    ("layernorm", (1, 46080, 1024, 0, 0, 0, 0)): ((0, 1, 4, 0, 0), None),
    ("layernorm", (1, 64, 128, 0, 0, 0, 0)): ((1, 1, 0, 0, 0), None),
    ("layernorm", (1, 64, 1024, 0, 0, 0, 0)): ((0, 1, 4, 0, 0), None),
    ("layernorm", (0, 40, 64, 1, 0, 0, 0)): ((1, 0, 1, 0, 0), None),
    ("layernorm", (1, 33, 192, 1, 0, 0, 0)): ((1, 1, 1, 0, 0), None),
    ("layernorm", (0, 96, 1280, 1, 0, 0, 0)): ((1, 0, 1, 0, 0), None),
    ("layernorm", (1, 33, 1792, 1, 0, 0, 0)): ((1, 1, 1, 0, 0), None),
    ("layernorm", (0, 130, 2048, 1, 0, 0, 0)): ((1, 0, 1, 0, 0), None),
    ("layernorm", (0, 720, 1024, 1, 0, 0, 0)): ((1, 0, 1, 0, 0), None),
    ("layernorm", (0, 300, 1024, 1, 0, 0, 0)): ((1, 0, 1, 0, 0), None),
    ("layernorm", (0, 160, 256, 1, 1, 0, 0)): ((1, 0, 1, 0, 0), None),
    ("layernorm", (0, 160, 256, 1, 0, 0, 0)): ((1, 0, 1, 0, 0), None),
    ("layernorm", (0, 96, 1280, 1, 1, 0, 0)): ((1, 0, 1, 0, 0), None),
    ("layernorm", (0, 144, 256, 0, 1, 0, 0)): ((1, 0, 0, 0, 0), None),
    ("layernorm", (0, 144, 256, 0, 0, 0, 0)): ((0, 0, 1, 0, 0), None),
    ("layernorm", (0, 300, 1024, 1, 0, 1, 0)): ((1, 0, 1, 1, 0), None),
    ("layernorm", (0, 300, 1024, 0, 0, 0, 1)): ((1, 0, 0, 2, 0), None),
    ("layernorm", (1, 33, 192, 1, 0, 1, 0)): ((1, 1, 1, 1, 0), None),
    ("layernorm", (1, 33, 192, 0, 0, 0, 1)): ((1, 1, 0, 2, 0), None),
    ("layernorm", (0, 8, 64, 1, 0, 0, 0)): ((1, 0, 1, 0, 0), None),
    # ---- attn_spatial
    ("attn_spatial", (2, 3, 32, 0)): ((2, 4, 2, 0, 0), 'qsplit=1'),
    ("attn_spatial", (2, 3, 72, 0)): ((2, 4, 6, 0, 0), 'qsplit>1'),
    ("attn_spatial", (2, 3, 144, 0)): ((2, 4, 10, 0, 0), 'qsplit>1'),
    ("attn_spatial", (2, 3, 200, 0)): ((3, 2, 3, 1, 0), None),
    ("attn_spatial", (2, 3, 256, 0)): ((3, 2, 3, 0, 0), None),
    ("attn_spatial", (2, 3, 576, 0)): ((3, 3, 3, 0, 0), None),
    ("attn_spatial", (2, 3, 200, 1)): ((3, 2, 3, 1, 1), None),
    ("attn_spatial", (2, 3, 576, 1)): ((3, 3, 3, 0, 1), None),
    ("attn_spatial", (2, 3, 40, 0)): ((2, 4, 4, 0, 0), 'qsplit=1'),
    ("attn_spatial", (2, 3, 104, 0)): ((2, 4, 8, 0, 0), 'qsplit>1'),
    ("attn_spatial", (2, 3, 184, 0)): ((3, 3, 3, 1, 0), None),
    ("attn_spatial", (2, 3, 184, 1)): ((3, 3, 3, 1, 1), None),
    ("attn_spatial", (2, 3, 256, 1)): ((3, 2, 3, 0, 1), None),
    ("attn_spatial", (64, 4, 256, 0)): ((3, 4, 2, 0, 0), None),
    ("attn_spatial", (64, 4, 256, 1)): ((3, 4, 2, 0, 1), None),
    ("attn_spatial", (64, 4, 200, 0)): ((3, 4, 2, 1, 0), None),
    ("attn_spatial", (64, 4, 200, 1)): ((3, 4, 2, 1, 1), None),
    ("attn_spatial", (128, 4, 72, 0)): ((2, 4, 6, 0, 0), 'qsplit=1'),
    ("attn_spatial", (128, 4, 104, 0)): ((2, 4, 8, 0, 0), 'qsplit=1'),
    ("attn_spatial", (128, 4, 144, 0)): ((2, 4, 10, 0, 0), 'qsplit=1'),
    ("attn_spatial", (5, 16, 144, 0)): ((2, 4, 10, 0, 0), 'qsplit>1'),
    ("attn_spatial", (2, 16, 576, 0)): ((3, 3, 3, 0, 0), None),
    ("attn_spatial", (3, 4, 32, 0)): ((2, 4, 2, 0, 0), 'qsplit=1'),
    ("attn_spatial", (1, 2, 72, 0)): ((2, 4, 6, 0, 0), 'qsplit>1'),
    ("attn_spatial", (1, 2, 200, 0)): ((3, 2, 3, 1, 0), None),
    ("attn_spatial", (3, 8, 256, 0)): ((3, 2, 3, 0, 0), None),
    ("attn_spatial", (1, 3, 328, 0)): ((3, 2, 3, 1, 0), None),
    ("attn_spatial", (5, 16, 576, 0)): ((3, 3, 3, 0, 0), None),
    ("attn_spatial", (1, 2, 1152, 0)): ((3, 2, 3, 0, 0), None),
    ("attn_spatial", (1, 1, 144, 0)): ((2, 4, 10, 0, 0), 'qsplit>1'),
    # ---- attn_temporal
    ("attn_temporal", (2, 24, 256, 5, 0, 5)): ((4, 5, 0, 0, 0), 'split'),
    ("attn_temporal", (2, 24, 256, 1, 4, 5)): ((4, 5, 0, 0, 0), 'one'),
    ("attn_temporal", (2, 24, 256, 3, 5, 8)): ((4, 8, 0, 0, 0), 'split'),
    ("attn_temporal", (2, 24, 256, 1, 7, 32)): ((4, 8, 0, 0, 0), 'one'),
    ("attn_temporal", (2, 24, 256, 1, 8, 32)): ((5, 1, 8, 0, 0), None),
    ("attn_temporal", (2, 24, 256, 9, 3, 16)): ((5, 8, 4, 0, 0), None),
    ("attn_temporal", (2, 24, 256, 32, 0, 32)): ((5, 8, 4, 0, 0), None),
    ("attn_temporal", (2, 24, 256, 1, 31, 32)): ((5, 1, 8, 0, 0), None),
    ("attn_temporal", (2, 3, 256, 12, 0, 12)): ((5, 8, 4, 0, 0), None),
    ("attn_temporal", (8, 128, 256, 3, 2, 8)): ((4, 5, 0, 0, 0), 'loop'),
    ("attn_temporal", (8, 128, 256, 3, 5, 8)): ((4, 8, 0, 0, 0), 'loop'),
    ("attn_temporal", (2, 24, 256, 2, 1, 5)): ((4, 5, 0, 0, 0), 'split'),
    ("attn_temporal", (2, 24, 256, 1, 0, 5)): ((4, 5, 0, 0, 0), 'one'),
    # ---- attn_spatial_bwd
    ("attn_spatial_bwd", (2, 2, 32)): ((6, 0, 0, 0, 0), None),
    ("attn_spatial_bwd", (1, 2, 144)): ((6, 0, 0, 0, 0), None),
    ("attn_spatial_bwd", (1, 1, 160)): ((6, 0, 0, 0, 0), None),
    ("attn_spatial_bwd", (1, 1, 8)): ((7, 0, 0, 0, 0), None),
    ("attn_spatial_bwd", (2, 2, 72)): ((7, 0, 0, 0, 0), None),
    ("attn_spatial_bwd", (1, 2, 200)): ((7, 0, 0, 0, 0), None),
    ("attn_spatial_bwd", (1, 1, 576)): ((7, 0, 0, 0, 0), None),
    ("attn_spatial_bwd", (3, 2, 144)): ((6, 0, 0, 0, 0), None),
    ("attn_spatial_bwd", (2, 4, 32)): ((6, 0, 0, 0, 0), None),
    # ---- attn_temporal_bwd
    ("attn_temporal_bwd", (2, 3, 128, 1)): ((8, 1, 0, 0, 0), None),
    ("attn_temporal_bwd", (2, 3, 128, 5)): ((8, 5, 0, 0, 0), None),
    ("attn_temporal_bwd", (1, 3, 128, 8)): ((8, 8, 0, 0, 0), None),
    ("attn_temporal_bwd", (2, 3, 128, 2)): ((8, 2, 0, 0, 0), None),
    ("attn_temporal_bwd", (2, 3, 128, 3)): ((8, 3, 0, 0, 0), None),
    ("attn_temporal_bwd", (2, 3, 128, 4)): ((8, 4, 0, 0, 0), None),
    ("attn_temporal_bwd", (2, 3, 128, 6)): ((8, 6, 0, 0, 0), None),
    ("attn_temporal_bwd", (2, 3, 128, 7)): ((8, 7, 0, 0, 0), None),
    ("attn_temporal_bwd", (2, 3, 128, 9)): ((9, 0, 0, 0, 0), None),
    ("attn_temporal_bwd", (1, 3, 128, 17)): ((9, 0, 0, 0, 0), None),
    ("attn_temporal_bwd", (1, 5, 256, 32)): ((9, 0, 0, 0, 0), None),
    # ---- skinny
    ("skinny", (5, 1024, 256, 1)): ((10, 1, 1, 1, 0), None),
    ("skinny", (16, 6144, 1056, 0)): ((10, 0, 1, 1, 0), None),
    ("skinny", (37, 192, 1024, 1)): ((10, 1, 1, 1, 0), None),
    ("skinny", (808, 6144, 1024, 0)): ((10, 0, 4, 2, 0), None),
    ("skinny", (131, 320, 1024, 1)): ((10, 1, 1, 1, 0), None),
    ("skinny", (16, 262148, 32, 0)): ((10, 0, 4, 1, 0), None),
    ("skinny", (20, 131076, 64, 1)): ((10, 1, 4, 1, 0), None),
    ("skinny", (48, 87556, 32, 1)): ((10, 1, 4, 2, 0), None),
    ("skinny", (1000, 16388, 96, 0)): ((10, 0, 8, 2, 0), None),
    ("skinny", (40, 65540, 256, 0)): ((10, 0, 4, 5, 128), None),
    ("skinny", (90, 65540, 128, 0)): ((10, 0, 4, 6, 128), None),
    ("skinny", (101, 65540, 256, 0)): ((10, 0, 4, 7, 128), None),
    ("skinny", (200, 65540, 128, 0)): ((10, 0, 4, 6, 128), None),
    # ---- gemm_tn_f32
    ("gemm_tn_f32", (5, 64, 64)): ((11, 0, 0, 0, 0), None),
    ("gemm_tn_f32", (17, 256, 128)): ((11, 0, 0, 0, 0), None),
    ("gemm_tn_f32", (80, 128, 64)): ((11, 0, 0, 0, 0), None),
    ("gemm_tn_f32", (16, 64, 25)): ((12, 0, 0, 0, 0), None),
    ("gemm_tn_f32", (5, 30, 25)): ((12, 0, 0, 0, 0), None),
    ("gemm_tn_f32", (5, 64, 25)): ((12, 0, 0, 0, 0), None),
    # ---- gemm_nn_f32
    ("gemm_nn_f32", (1, 256, 64)): ((13, 16, 0, 0, 0), None),
    ("gemm_nn_f32", (1, 256, 100)): ((13, 16, 0, 0, 0), None),
    ("gemm_nn_f32", (17, 256, 64)): ((13, 16, 0, 0, 0), None),
    ("gemm_nn_f32", (17, 256, 100)): ((13, 16, 0, 0, 0), None),
    ("gemm_nn_f32", (1, 2048, 64)): ((13, 8, 0, 0, 0), None),
    ("gemm_nn_f32", (1, 2048, 100)): ((13, 8, 0, 0, 0), None),
    ("gemm_nn_f32", (17, 2048, 64)): ((13, 8, 0, 0, 0), None),
    ("gemm_nn_f32", (17, 2048, 100)): ((13, 8, 0, 0, 0), None),
    ("gemm_nn_f32", (1, 4096, 64)): ((13, 4, 0, 0, 0), None),
    ("gemm_nn_f32", (1, 4096, 100)): ((13, 4, 0, 0, 0), None),
    ("gemm_nn_f32", (17, 4096, 64)): ((13, 4, 0, 0, 0), None),
    ("gemm_nn_f32", (17, 4096, 100)): ((13, 4, 0, 0, 0), None),
    # ---- ada_bwd_dx
    ("ada_bwd_dx", (3584, 256, 6)): ((14, 0, 0, 0, 0), None),
    ("ada_bwd_dx", (1216, 64, 80)): ((14, 0, 0, 0, 0), None),
    ("ada_bwd_dx", (2048, 1024, 17)): ((14, 0, 0, 0, 0), None),
    ("ada_bwd_dx", (3584, 256, 81)): ((15, 0, 0, 0, 0), None),
    ("ada_bwd_dx", (1216, 100, 6)): ((15, 0, 0, 0, 0), None),
    ("ada_bwd_dx", (28672, 2048, 6)): ((15, 0, 0, 0, 0), None),
    # ---- ln_mod_bwd_fused
    ("ln_mod_bwd_fused", (3, 24, 256)): ((16, 1, 0, 0, 0), None),
    ("ln_mod_bwd_fused", (2, 16, 512)): ((16, 2, 0, 0, 0), None),
    ("ln_mod_bwd_fused", (2, 40, 1024)): ((16, 4, 0, 0, 0), None),
    ("ln_mod_bwd_fused", (1, 17, 2048)): ((16, 8, 0, 0, 0), None),
    ("ln_mod_bwd_fused", (2, 24, 256)): ((16, 1, 0, 0, 0), None),
    ("ln_mod_bwd_fused", (2, 24, 1024)): ((16, 4, 0, 0, 0), None),
}


def op_rows():
    """[(family, arguments, (instantiation, form), table)]: op_problems() with the declared plans; a problem without one is a KeyError that names it"""
    return [(f, a, DECLARED_PLANS[(f, a)], src) for f, a, src in op_problems()]


def declared_plan(family, args):
    return DECLARED_PLANS[(family, tuple(args))]
