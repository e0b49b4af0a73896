"""Kernel-level parity of the low-rank adapter kernels (csrc/train.hip lora_*) on the GPU, through the kernel-level entry points gtav_op_lora_grads and gtav_op_lora_merge
(include/gtav_amd.h), in both operand types (gtav_op_set_operand_dtype).  References are fp64 math on the operands the kernels read; inputs, references and bounds come from
tests/lora_bounds.py, where every bound is derived (tests/test_host_lora.py holds them against fp32 emulations on the CPU).  Operands are laid out on the host;
every buffer a launch writes starts as NaNs with spare space behind it, which must come back bit for bit.  `pytest -s` prints each margin
(profiles/lora/op_margins.txt is such a printout)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import lora_bounds as LB  # noqa: E402
from helpers import dev, stream, tiled_index  # noqa: E402
from gtav_amd import lib as L  # noqa: E402

F16, BF16 = LB.F16, LB.BF16
DTYPES = pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
SHAPES = pytest.mark.parametrize("shape", LB.SHAPES, ids=["x".join(map(str, s)) for s in LB.SHAPES])
RANKS = pytest.mark.parametrize("r", LB.RANKS)
NAN16, NAN32 = 0x7FA5, 0x7FC00123
MAX_SPLITS = 16                           # csrc/ops.h LORA_MAX_SPLITS


@pytest.fixture(autouse=True)
def _restore_hooks():
    yield
    L.load().gtav_op_set_operand_dtype(0)


def _use(dtype):
    L.load().gtav_op_set_operand_dtype(1 if dtype is BF16 else 0)
    return L.load()


def _up(n, m):
    return (n + m - 1) // m * m


def _cdiv(a, b):
    return (a + b - 1) // b


def _ws_floats(M, N, K, r):
    """csrc/ops.h lora_grads_workspace, restated: t^T and u^T as 2-byte [r][round_up(M, 128)], the adapters as 2-byte [r][K] and [r][N], then one [N + K][r]
    partial per run of 128-row tiles"""
    tiles = _cdiv(M, 128)
    splits = _cdiv(tiles, _cdiv(tiles, min(tiles, MAX_SPLITS)))
    return r * _up(M, 128) + r * (N + K) // 2 + splits * (N + K) * r


def _tiled(x, dtype, pad_bits):
    """(R, K) -> tile-major 2-byte image of round_up(R, 128) x K on the GPU, laid out on the host; every pad row holds `pad_bits`"""
    R, K = x.shape
    flat = torch.full((_up(R, 128) * K,), pad_bits, dtype=torch.int16)
    flat[tiled_index(R, K).reshape(-1)] = x.to(dtype).contiguous().view(torch.int16).reshape(-1)
    return flat.view(dtype).to(dev())


def _nan32(n):
    return torch.full((n,), NAN32, dtype=torch.int32, device=dev()).view(torch.float32)


def _grads(lib, c, pad_bits, spare=4096):
    """one launch from zeroed gradients: (dA, dB, ws, error word); the workspace is exactly the documented size with a NaN sentinel run behind it"""
    M, N, K, r = c.M, c.N, c.K, c.r
    x, dy = _tiled(c.x, c.dtype, pad_bits), _tiled(c.dy, c.dtype, pad_bits)
    a, b = c.a.to(dev()).contiguous(), c.b.to(dev()).contiguous()
    dA, dB = torch.zeros(r, K, device=dev()), torch.zeros(N, r, device=dev())
    n = _ws_floats(M, N, K, r)
    ws = _nan32(n + spare)
    err = torch.zeros(1, dtype=torch.int32, device=dev())
    L.check(lib.gtav_op_lora_grads(x.data_ptr(), dy.data_ptr(), a.data_ptr(), b.data_ptr(), M, N, K, r, c.s, dA.data_ptr(), dB.data_ptr(), ws.data_ptr(), n,
                                   err.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert (ws[n:].view(torch.int32) == NAN32).all(), "the launch wrote behind its workspace"
    return dA, dB, ws, int(err.item()), (x, dy, a, b, n)


@DTYPES
@RANKS
@SHAPES
def test_lora_grads(shape, r, dtype):
    M, N, K = shape
    c = LB.lora_case(M, N, K, r, dtype)
    lib = _use(dtype)
    dA, dB, ws, err, (x, dy, a, b, n) = _grads(lib, c, NAN16)
    assert err == 0
    e = LB.grad_errors(c, dA, dB)
    for name, (l2, worst) in e.items():
        print(f"[margin lora_grads {LB.NAME[dtype]} {M}x{N}x{K} r{r}] {name}: rel-L2 {l2:.3e} = {l2 / LB.GLOBAL_TOL[dtype]:.3f} of the threshold, per element: worst error / bound {worst:.3f}")
    for name, (l2, worst) in e.items():
        assert worst <= 1.0, (name, worst)
        assert l2 < LB.GLOBAL_TOL[dtype], (name, l2, LB.GLOBAL_TOL[dtype])
    # padding: the rows >= M of the tile-major inputs are never used — zeros there give the same bits as NaNs
    if M % 128:
        dA0, dB0, _, err0, _ = _grads(lib, c, 0)
        assert err0 == 0 and torch.equal(dA0, dA) and torch.equal(dB0, dB)
    # the gradients ACCUMULATE, in a fixed order: a second launch on the same buffers doubles every element exactly
    first = (dA.clone(), dB.clone())
    L.check(lib.gtav_op_lora_grads(x.data_ptr(), dy.data_ptr(), a.data_ptr(), b.data_ptr(), M, N, K, r, c.s, dA.data_ptr(), dB.data_ptr(), ws.data_ptr(), n, 0, stream()))
    torch.cuda.synchronize()
    assert torch.equal(dA, 2 * first[0]) and torch.equal(dB, 2 * first[1])


def test_lora_grads_refusals():
    lib = _use(F16)
    c = LB.lora_case(96, 256, 256, 16, F16)
    x, dy = _tiled(c.x, F16, 0), _tiled(c.dy, F16, 0)
    a, b = c.a.to(dev()), c.b.to(dev())
    dA, dB, ws = torch.zeros(16, 256, device=dev()), torch.zeros(256, 16, device=dev()), torch.zeros(1 << 20, device=dev())

    def call(M=96, N=256, K=256, r=16, n=1 << 20):
        return lib.gtav_op_lora_grads(x.data_ptr(), dy.data_ptr(), a.data_ptr(), b.data_ptr(), M, N, K, r, 1.0, dA.data_ptr(), dB.data_ptr(), ws.data_ptr(), n, 0, stream())
    assert call(n=_ws_floats(96, 256, 256, 16) - 1) != 0 and b"workspace" in lib.gtav_last_error()
    assert call(r=24) != 0 and b"rank 24" in lib.gtav_last_error()
    assert call(N=200) != 0 and b"multiples of 64" in lib.gtav_last_error()
    assert call(n=_ws_floats(96, 256, 256, 16)) == 0
    torch.cuda.synchronize()


@DTYPES
@RANKS
@SHAPES
def test_lora_merge(shape, r, dtype):
    _, N, K = shape
    c = LB.lora_case(*shape, r, dtype)
    lib = _use(dtype)
    n_img, n_t, spare = _up(N, 128) * K, _up(K, 128) * _up(N, 64), 8192
    img = torch.full((n_img + spare,), NAN16, dtype=torch.int16, device=dev())
    imgT = torch.full((n_t + spare,), NAN16, dtype=torch.int16, device=dev())
    w32 = _nan32(N * K + spare)
    w0, a, b = c.w0.to(dev()).contiguous(), c.a.to(dev()).contiguous(), c.b.to(dev()).contiguous()
    L.check(lib.gtav_op_lora_merge(w0.data_ptr(), a.data_ptr(), b.data_ptr(), N, K, r, c.s, img.data_ptr(), imgT.data_ptr(), w32.data_ptr(), stream()))
    torch.cuda.synchronize()
    for name, buf, n in (("image", img, n_img), ("transposed image", imgT, n_t)):
        assert (buf[n:] == NAN16).all(), f"the launch wrote behind the {name}"
    assert (w32[N * K:].view(torch.int32) == NAN32).all(), "the launch wrote behind the fp32 export"
    got = img.cpu()[tiled_index(N, K).reshape(-1)].reshape(N, K)
    gotT = imgT.cpu()[tiled_index(K, _up(N, 64)).reshape(-1)].reshape(K, _up(N, 64))[:, :N]
    exp = w32[: N * K].reshape(N, K).cpu()
    assert torch.isfinite(exp).all() and torch.isfinite(got.view(dtype).float()).all()
    worst32 = LB.outside((exp.double() - c.w).abs(), c.w_acc)[1]
    worst16 = LB.outside((got.view(dtype).double() - c.w).abs(), c.w_tol)[1]
    print(f"[margin lora_merge {LB.NAME[dtype]} {N}x{K} r{r}] per element: worst error / bound, image {worst16:.3f}, fp32 export {worst32:.3f}")
    assert worst32 <= 1.0 and worst16 <= 1.0
    assert torch.equal(gotT, got.t()), "W^T holds the bits of the transposed image"
    assert torch.equal(got, LB.store_rne(exp, dtype).view(torch.int16)), "the image is the round-to-nearest cast of the exported fp32 sum"
    # without the optional outputs
    img2 = torch.full((n_img,), NAN16, dtype=torch.int16, device=dev())
    L.check(lib.gtav_op_lora_merge(w0.data_ptr(), a.data_ptr(), b.data_ptr(), N, K, r, c.s, img2.data_ptr(), 0, 0, stream()))
    torch.cuda.synchronize()
    assert torch.equal(img2, img[:n_img])
