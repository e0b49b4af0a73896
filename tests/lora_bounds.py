"""Inputs, fp64 references, error bounds and fp32 emulations of the low-rank adapter kernels (csrc/train.hip lora_*), shared by tests/test_gpu_ops_lora.py (the
kernels, on a GPU) and tests/test_host_lora.py (the bounds themselves, on the CPU).  Pure torch: nothing here loads the library.  Conventions as in the head of
parity_bounds.py: u is the unit roundoff of the operand type, every term is fp64 math on the operands the kernel reads, none comes from the code under test.

Merge, W = W0 + s B A with fp32 W0 [N][K], A [r][K], B [N][r] (r fmaf's and one more, all fp32):
    image   |got - ref| <= u (1 + 2^-10) |ref| + (r + 2) 2^-24 (|W0| + s |B| |A|) + one subnormal step      fp32 export: the middle term alone
    the W^T image holds the bits of the transposed W image.
Gradients of one Linear, from the 2-byte X [M][K], dY [M][N] and the adapters rounded to the operand type (A^, B^): t = X A^^T, u = dY B^ exact in fp64,
    dB = s dY^T t    |got - ref| <= s |dY|^T (u (1 + 2^-10) |t| + 2 (K + 2) 2^-24 |X| |A^|^T) + 2 (M + 2) 2^-24 s |dY|^T |t|
    dA = s u^T X     |got - ref| <= s (u (1 + 2^-10) |u| + 2 (N + 2) 2^-24 |dY| |B^|)^T |X| + 2 (M + 2) 2^-24 s |u|^T |X|
  first term: the ONE 2-byte store of t (u), off by its own K-term (N-term) fp32 dot product, carried through the second contraction; last term: that contraction's
  own M-term fp32 accumulation (the partial sums per row split and their fixed-order addition are M + splits roundings at most), doubled like every matrix-pipe bound.
Global relative L2 of dA and dB: not derivable, so measured HERE on the CPU, per operand type: the fp32 emulation below with t and u stored by store_rne (what
  the kernel must do) and the same with store_trunc (the wrong store), each against fp64 on every shape and rank; the threshold is the geometric mean of the
  worst round-to-nearest figure and the best truncating one (GLOBAL_TOL; both figures in its comment, tests/test_host_lora.py re-measures them)."""
import functools
import math

import torch

from parity_bounds import BF16, F16, NAME, SUBNORMAL, U, outside, rand, rel_l2, store_rne, store_trunc  # noqa: F401  (re-exported for the two test files)

SHAPES = [(96, 256, 256), (192, 768, 256), (300, 256, 1024), (384, 1024, 256)]      # (M token rows, N outputs, K inputs)
RANKS = (16, 64)
SCALE = 2.0                                                                          # s = alpha / r

# measured by tests/test_host_lora.py::test_emulation_controls (relative L2 against fp64 over SHAPES x RANKS x {dA, dB}):
#   fp16: store_rne 2.010e-04 .. 2.152e-04, store_trunc 4.040e-04 .. 4.406e-04        bf16: store_rne 1.629e-03 .. 1.727e-03, store_trunc 3.228e-03 .. 3.404e-03
# threshold = sqrt(worst store_rne x best store_trunc): 2.949e-04 (fp16), 2.361e-03 (bf16)
GLOBAL_TOL = {F16: math.sqrt(2.152e-4 * 4.040e-4), BF16: math.sqrt(1.727e-3 * 3.228e-3)}


class LoraCase:
    def __init__(self, M, N, K, r, dtype):
        self.M, self.N, self.K, self.r, self.dtype, self.s = M, N, K, r, dtype, SCALE
        seed = 1000 * r + M
        self.x = rand(M, K, seed=seed + 1).to(dtype)
        self.dy = rand(M, N, seed=seed + 2, scale=0.5).to(dtype)
        g = torch.Generator().manual_seed(seed + 3)
        self.a = (torch.rand(r, K, generator=g) * 2 - 1) / math.sqrt(K)              # init_lora's distribution
        self.b = rand(N, r, seed=seed + 4, scale=0.02)
        self.w0 = rand(N, K, seed=seed + 5, scale=1 / math.sqrt(K))
        self.a_hat, self.b_hat = self.a.to(dtype), self.b.to(dtype)
        x, dy, ah, bh = self.x.double(), self.dy.double(), self.a_hat.double(), self.b_hat.double()
        # ---- gradients ----
        self.t, self.u = x @ ah.t(), dy @ bh
        self.dB, self.dA = self.s * dy.t() @ self.t, self.s * self.u.t() @ x
        uu, e = U[dtype] * (1 + 2.0 ** -10), 2.0 ** -24
        t_err = uu * self.t.abs() + 2 * (K + 2) * e * (x.abs() @ ah.abs().t())
        u_err = uu * self.u.abs() + 2 * (N + 2) * e * (dy.abs() @ bh.abs())
        self.dB_tol = self.s * dy.abs().t() @ t_err + 2 * (M + 2) * e * self.s * dy.abs().t() @ self.t.abs()
        self.dA_tol = self.s * u_err.t() @ x.abs() + 2 * (M + 2) * e * self.s * self.u.abs().t() @ x.abs()
        # ---- merge (the fp32 adapters themselves) ----
        w0, a, b = self.w0.double(), self.a.double(), self.b.double()
        self.w = w0 + self.s * b @ a
        self.w_acc = (r + 2) * e * (w0.abs() + self.s * b.abs() @ a.abs())
        self.w_tol = uu * self.w.abs() + self.w_acc + SUBNORMAL[dtype]

    def emulate(self, store):
        """(dA, dB) in fp32 arithmetic with t and u stored once by `store`"""
        x, dy = self.x.float(), self.dy.float()
        t = store(x @ self.a_hat.float().t(), self.dtype).float()
        u = store(dy @ self.b_hat.float(), self.dtype).float()
        return self.s * u.t() @ x, self.s * dy.t() @ t

    def emulate_merge(self):
        """the fp32 sum as the contract orders it: acc = fma over k ascending from 0, then fma(s, acc, W0)"""
        acc = torch.zeros(self.N, self.K, dtype=torch.float64)
        for k in range(self.r):     # fp64 products of fp32 values are exact; rounding each step to fp32 is the fused multiply-add
            acc = (acc + self.b[:, k:k + 1].double() * self.a[k:k + 1, :].double()).float().double()
        return (self.s * acc + self.w0.double()).float()


@functools.lru_cache(maxsize=None)
def lora_case(M, N, K, r, dtype):
    return LoraCase(M, N, K, r, dtype)


def grad_errors(case, dA, dB):
    """{name: (relative L2, worst error / bound)} of a (dA, dB) pair against the case's fp64 reference; everything must be finite"""
    out = {}
    for name, got, ref, tol in (("dA", dA, case.dA, case.dA_tol), ("dB", dB, case.dB, case.dB_tol)):
        got = got.double().cpu()
        assert torch.isfinite(got).all(), name
        out[name] = (rel_l2(got, ref), outside((got - ref).abs(), tol)[1])
    return out
