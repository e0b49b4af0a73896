"""Inputs, fp64 references, error bounds and fp32 emulations of the operand-typed kernels, shared by tests/test_gpu_ops_typed.py (the kernels, on a GPU) and
tests/test_host_parity_bounds.py (the bounds themselves, on the CPU).  Pure torch: nothing here loads the library.

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
LN_SHAPES = [(128, 96), (256, 96), (1024, 1027), (2048, 160)]      # (D, M)
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
    prescaled: q_ps = q * log2 e / 8 rounded on the host, and the reference is the base-2 softmax of THAT q."""

    def __init__(self, S, dtype, jump=None, prescaled=False):
        NB, heads = ATTN_NB, ATTN_HEADS
        self.S, self.dtype = S, dtype
        q, k, v = (rand(NB, heads, S, 64, seed=i).to(dtype) for i in (1, 2, 3))
        if jump is None:
            q = (q.float() * 1.5).to(dtype)
        else:
            k[1, 2, S - 9] = (q[1, 2, 7].float() * jump).to(dtype)         # a key of the last key block against query 7
            k[0, 1, 70] = (q[0, 1, 150].float() * jump).to(dtype)          # and one in the second key block
            self.dominated = ((1, 2, 7), (0, 1, 150))
        self.k, self.v = k, v
        if prescaled:
            self.q = (q.double() * (LOG2E / 8)).to(dtype)
            s = self.q.double() @ k.double().transpose(-1, -2)
            p = torch.exp2(s - s.max(-1, keepdim=True).values)
        else:
            self.q = q
            s = q.double() @ k.double().transpose(-1, -2) / 8.0
            p = torch.exp(s - s.max(-1, keepdim=True).values)
        self.p = p / p.sum(-1, keepdim=True)
        self.ref4 = self.p @ v.double()                                        # NB heads S 64
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
def attn_case(S, dtype, jump=None, prescaled=False):
    return AttnCase(S, dtype, jump, prescaled)


def attn_rows(x4):
    """[NB][heads][S][64] -> one row per (item, head, query): the 64 features a single softmax produces"""
    return x4.reshape(-1, 64)


# ---- temporal attention -------------------------------------------------------------------------------------------------------------------------------
TEMPORAL_TOL = 6e-4
# (B, P, D, Tq, t0, Tmax)
TEMPORAL_CASES = [(2, 24, 256, Tq, t0, Tmax) for (Tq, t0, Tmax) in ((5, 0, 5), (1, 4, 5), (3, 5, 8), (1, 7, 32), (1, 8, 32), (9, 3, 16), (32, 0, 32), (1, 31, 32))] + \
                 [(2, 3, 256, 12, 0, 12)]        # 6 columns: a partial block


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
