"""The one launch the patch geometries add to the training step, at kernel level: the patch embedding's weight gradient where the patch has F < Kpe =
round_up(F, 64) features (csrc/api_train.hip TrainBackward::gemm_dw, Kv < K).  dW [D][F] += dY^T X is the accumulating GEMM (EPI_RESID, no gate, no bias) on the
transposed operands dY^T [D][Mp] and X^T [Kpe][Mp] with N = F and ldo = F, straight into the contiguous gradient: no pad column may reach the arena.
The rows F .. Kpe of X^T (zeros in a step: the transposed pad columns of xp) hold NaN here and the gradient sits between NaN guards, so a store behind column F
of any row, or a pad row that leaks into a sum, shows.  Bound: fp32-accumulated GEMM on identical operands, 2e-5 relative L2 (tests/test_gpu_ops.py)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import dev, rel_l2, stream, to_tiled  # noqa: E402
from gtav_amd import lib as L  # noqa: E402

EPI_RESID = 4   # tests/test_gpu_ops.py test_gemm_residual_gate_epilogue


# D (rows of dW), F (its columns), tokens: the toy step (B T P = 192), a ragged token count, the widths of a 576-token step of the full-size model
@pytest.mark.parametrize("D,F,M", [(256, 16, 192), (256, 32, 192), (256, 4, 200), (1024, 16, 11520)])
def test_patch_embedding_weight_gradient_at_its_valid_width(D, F, M):
    g = torch.Generator().manual_seed(3)
    Mp = (M + 63) // 64 * 64
    dy = torch.zeros(D, Mp)
    dy[:, :M] = torch.randn(D, M, generator=g)
    xt = torch.full((256, Mp), float("nan"))        # (the widest feature tile of the GEMM: in a step the operand buffer is wider still)
    xt[:F] = 0
    xt[:F, :M] = torch.randn(F, M, generator=g) / math.sqrt(M)
    a, w = to_tiled(dy, torch.float16), to_tiled(xt, torch.float16)
    init = torch.randn(D, F, generator=g)
    guard = 256
    buf = torch.full((guard + D * F + guard,), float("nan"), device=dev())
    out = buf[guard: guard + D * F]
    out.copy_(init.reshape(-1).to(dev()))
    L.check(L.load().gtav_op_gemm_f16(a.data_ptr(), Mp, w.data_ptr(), 0, out.data_ptr(), F, D, F, Mp, EPI_RESID, 0, 0, 1, stream()))
    torch.cuda.synchronize()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + D * F:]).all(), "a store outside the gradient"
    got = out.reshape(D, F).cpu()
    assert torch.isfinite(got).all(), "a pad row of the operand reached a sum"
    ref = init.double() + dy.half().double() @ xt[:F].half().double().t()
    e = rel_l2(got - init, ref - init.double())
    print(f"[geometry dW {D}x{F} over {M} tokens] {e:.3e}")
    assert e < 2e-5
