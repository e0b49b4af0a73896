"""Per-element fp64 parity of the four attention backward kernels (csrc/train.hip attn_spatial_bwd_mfma_kernel, attn_spatial_bwd_stream_kernel,
attn_temporal_bwd_kernel, attn_temporal_bwd_stream_kernel) on the GPU, in both operand types, on flat AND peaked softmax rows, through the test hooks
gtav_op_train_attn_spatial_bwd / gtav_op_train_attn_temporal_bwd (include/gtav_amd_testing.h): the launch a training handle makes, with its error word.

Inputs, fp64 references and ONE derived bound per output element come from tests/parity_bounds.py (last section); tests/test_host_parity_bounds.py holds "a
perfect kernel of the design" inside that bound for every case below and a list of wrong kernels (a dropped key, a stale running maximum, Dq short of a chunk,
RoPE^T with the wrong sign, a causal mask off by one) outside.  None is taken from what a kernel returned.  Every case launches twice into NaN-filled buffers:
equal bits, nothing written behind the M token rows (the pad rows of the last 128-row tile and a spare tile stay NaN), every element of dq / dk / dv inside its
bound, and the error word 0 unless the case is built to saturate.  `pytest -s` prints, per case, the worst ratio error / bound
(profiles/op_parity_attn_bwd/margins.txt is such a printout)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import parity_bounds as PB  # noqa: E402
from helpers import assert_declared_plan, dev, stream, tiled_index  # noqa: E402
from gtav_amd import lib as L  # noqa: E402

F16, BF16 = PB.F16, PB.BF16
DTYPES = pytest.mark.parametrize("dtype", PB.DTYPES, ids=[PB.NAME[d] for d in PB.DTYPES])
NAN16 = 0x7FA5                 # a NaN in fp16 and in bf16: what every output buffer holds before a launch
THIRDS = ("dq", "dk", "dv")

SPATIAL_CASES = [(s, k, 0) for s in PB.ATTN_BWD_SHAPES for k in PB.ATTN_BWD_KINDS] + \
                [(s, k, e) for s in PB.ATTN_BWD_SCALED_SHAPES for k in PB.ATTN_BWD_KINDS for e in PB.ATTN_BWD_SCALES]
SPATIAL_IDS = [f"{s[0]}x{s[1]}x{s[2]}-{k}-2^{e}" for s, k, e in SPATIAL_CASES]
TEMPORAL_CASES = [(s, k) for s in PB.TEMPORAL_BWD_SHAPES for k in PB.TEMPORAL_BWD_KINDS]
TEMPORAL_IDS = ["x".join(map(str, s)) + "-" + k for s, k in TEMPORAL_CASES]


@pytest.fixture(autouse=True)
def _restore_hooks():
    yield
    L.load().gtav_op_set_operand_dtype(0)


def _use(dtype):
    L.load().gtav_op_set_operand_dtype(1 if dtype is BF16 else 0)
    return L.load()


def _within(name, got, ref, tol, dtype):
    """every element of dq, dk and dv against its bound"""
    got = got.double()
    assert torch.isfinite(got).all(), name
    D = ref.shape[1] // 3
    for i, third in enumerate(THIRDS):
        sl = slice(i * D, (i + 1) * D)
        frac, worst = PB.outside((got[:, sl] - ref[:, sl]).abs(), tol[:, sl])
        print(f"[margin {name} {third} {PB.NAME[dtype]}] per element: worst error / bound {worst:.3f}")
        assert worst <= 1.0, (name, third, worst, frac)


class _Err:
    """the caller's device error word between three sentinel words"""

    def __init__(self):
        self.buf = torch.tensor([0x1234, 0, 0x5678, 0x9ABC], dtype=torch.int32, device=dev())

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4

    def expect(self, name, bits):
        assert self.buf.cpu().tolist() == [0x1234, bits, 0x5678, 0x9ABC], (name, self.buf.cpu().tolist())


class _Out:
    """the tile-major [M][3 D] gradient inside a NaN-filled buffer of round_up(M, 128) + 128 rows"""

    def __init__(self, M, K, dtype):
        self.M, self.K, self.dtype = M, K, dtype
        self.n = ((M + 127) // 128 * 128 + 128) * K
        self.buf = torch.full((self.n,), NAN16, dtype=torch.int16, device=dev()).view(dtype)
        self.idx = tiled_index(M, K).reshape(-1)

    def values(self, name):
        """the M token rows (CPU, bit patterns carried through), after checking that every other element still holds the NaN it held"""
        flat = self.buf.view(torch.int16).cpu()
        keep = torch.ones(self.n, dtype=torch.bool)
        keep[self.idx] = False
        assert (flat[keep] == NAN16).all(), f"{name}: the launch wrote behind its {self.M} token rows ({int((flat[keep] != NAN16).sum())} elements)"
        return flat[self.idx].reshape(self.M, self.K).view(self.dtype)


def _tail(t, fill, pad):
    """t flattened with `pad` elements of `fill` behind it, on the GPU (fill None: no tail)"""
    flat = t.contiguous().reshape(-1)
    if fill is None:
        return flat.to(dev())
    buf = torch.full((flat.numel() + pad,), fill, dtype=t.dtype)
    buf[: flat.numel()] = flat
    return buf.to(dev())


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---- spatial --------------------------------------------------------------------------------------------------------------------------------------------------
def _launch_spatial(c, err, fill=None):
    """one launch of case c -> the rows [NB S][3 D] (CPU).  fill: what 64 rows behind q / k / dO / the table and 4096 elements behind V^T hold"""
    lib = _use(c.dtype)
    NB, heads, S = c.NB, c.heads, c.S
    assert_declared_plan("attn_spatial_bwd", NB, heads, S)
    pad = 64 * 64 * heads
    qd, kd, vtd, dod, csd = (_tail(t, fill, pad) for t in (c.q, c.k, c.v.transpose(-1, -2), c.do, c.cs))
    out = _Out(NB * S, 3 * heads * 64, c.dtype)
    L.check(lib.gtav_op_train_attn_spatial_bwd(qd.data_ptr(), kd.data_ptr(), vtd.data_ptr(), dod.data_ptr(), NB, heads, S, csd.data_ptr(), out.buf.data_ptr(),
                                                err.ptr if err is not None else 0, stream()))
    torch.cuda.synchronize()
    return out.values(f"attn_spatial_bwd {NB}x{heads}x{S}")


def _expect_clear(c):
    """the issue of the error word: 0 whenever the fp64 |dS|, |dq|, |dk|, |dv| all stay below a quarter of the type's largest finite value (bf16 never raises it)"""
    assert c.dtype is BF16 or c.peak < 0.25 * PB.F16_MAX, c.peak


@DTYPES
@pytest.mark.parametrize("shape,kind,e", SPATIAL_CASES, ids=SPATIAL_IDS)
def test_attention_spatial_backward_within_bounds(shape, kind, e, dtype):
    """S <= 160 with S % 16 == 0: the resident kernel (on bf16 operands as well); every other S: the streaming kernel"""
    c = PB.attn_bwd_case(*shape, kind, e, dtype)
    name = f"attn_spatial_bwd {shape[0]}x{shape[1]}x{shape[2]} {kind} dO x 2^{e}"
    err = _Err()
    got = _launch_spatial(c, err)
    again = _launch_spatial(c, err)
    assert _bits_equal(got, again), name                          # no atomics: launches are bitwise reproducible
    _within(name, got, c.ref, c.tol, dtype)
    _expect_clear(c)
    err.expect(name, 0)


@pytest.mark.parametrize("shape", PB.ATTN_BWD_SAT, ids=lambda s: "x".join(map(str, s)))
def test_attention_spatial_backward_saturation_raises_the_bit(shape):
    """fp16, sharp, dO x 2^13: dk leaves fp16 by a factor of 2 while dS stays below a quarter of it (tests/test_host_parity_bounds.py holds both at these inputs).
    The outputs are finite and within the bound of the CLAMPED reference (clamping cannot increase an error), and the word carries ERR_F16_SAT — the bit on which a
    training step skips its optimizer step.  Without an error word the same bits come back."""
    c = PB.attn_bwd_case(*shape, "sharp", PB.ATTN_BWD_SAT_SCALE, F16)
    assert c.ref.abs().max().item() > PB.F16_MAX and c.max_ds < 0.25 * PB.F16_MAX
    name = f"attn_spatial_bwd saturation {shape[0]}x{shape[1]}x{shape[2]}"
    err = _Err()
    got = _launch_spatial(c, err)
    err.expect(name, PB.ERR_F16_SAT)
    again = _launch_spatial(c, None)
    assert _bits_equal(got, again), name
    assert (got.float().abs() <= PB.F16_MAX).all()
    assert (got.float().abs() == PB.F16_MAX).any()
    _within(name, got, c.ref.clamp(-PB.F16_MAX, PB.F16_MAX), c.tol, F16)


@DTYPES
def test_attention_spatial_backward_reads_nothing_behind_the_frame(dtype):
    """`jump` at S = 200 (a ragged last tile, a dominant key in it): NaN bit patterns behind the last row of q / k / dO / the table and behind V^T, against zeros
    there: finite, equal bit for bit, and inside the bound."""
    c = PB.attn_bwd_case(1, 2, 200, "jump", 0, dtype)
    err = _Err()
    with_nan = _launch_spatial(c, err, float("nan"))
    with_zero = _launch_spatial(c, err, 0.0)
    assert torch.isfinite(with_nan.float()).all()
    assert _bits_equal(with_nan, with_zero)
    _within("attn_spatial_bwd 1x2x200 jump NaN tails", with_nan, c.ref, c.tol, dtype)
    err.expect("NaN tails", 0)


# ---- temporal -------------------------------------------------------------------------------------------------------------------------------------------------
def _launch_temporal(c, err, fill=None):
    """fill: what the cache frames from T on, the table rows from T on and 64 rows behind q / dO hold"""
    lib = _use(c.dtype)
    B, P, D, T, Tmax = c.args
    assert_declared_plan("attn_temporal_bwd", B, P, D, T)
    kv, cs = c.kv, c.cs
    if fill is not None:
        kv, cs = kv.clone(), cs.clone()
        kv[:, T:] = fill
        cs[T:] = fill
    qd, kvd, dod, csd = (_tail(t, fill, 64 * D) for t in (c.q, kv, c.do, cs))
    out = _Out(B * T * P, 3 * D, c.dtype)
    L.check(lib.gtav_op_train_attn_temporal_bwd(qd.data_ptr(), kvd.data_ptr(), dod.data_ptr(), B, P, D, T, Tmax, csd.data_ptr(), out.buf.data_ptr(),
                                                 err.ptr if err is not None else 0, stream()))
    torch.cuda.synchronize()
    return out.values(f"attn_temporal_bwd {c.args}")


@DTYPES
@pytest.mark.parametrize("shape,kind", TEMPORAL_CASES, ids=TEMPORAL_IDS)
def test_attention_temporal_backward_within_bounds(shape, kind, dtype):
    """T <= 8: the register-resident kernel; 9 .. 32: the streaming kernel"""
    c = PB.temporal_bwd_case(*shape, kind, dtype)
    name = f"attn_temporal_bwd {'x'.join(map(str, shape))} {kind}"
    err = _Err()
    got = _launch_temporal(c, err)
    again = _launch_temporal(c, None)                             # (and the error word may be null)
    assert _bits_equal(got, again), name
    _within(name, got, c.ref, c.tol, dtype)
    _expect_clear(c)
    err.expect(name, 0)


@DTYPES
def test_attention_temporal_backward_reads_nothing_beyond_the_window(dtype):
    """`ladder` at T = 17 in a cache of 32 frames: NaN bit patterns in frames 17 .. 31, in the table rows from 17 on and behind q / dO, against zeros there"""
    c = PB.temporal_bwd_case(1, 3, 128, 17, 32, "ladder", dtype)
    err = _Err()
    with_nan = _launch_temporal(c, err, float("nan"))
    with_zero = _launch_temporal(c, err, 0.0)
    assert torch.isfinite(with_nan.float()).all()
    assert _bits_equal(with_nan, with_zero)
    _within("attn_temporal_bwd 1x3x128x17x32 ladder NaN tails", with_nan, c.ref, c.tol, dtype)
    err.expect("NaN tails", 0)
