"""Backward of the causal temporal attention through gtav_op_attn_temporal_bwd / gtav_op_attn_temporal_bwd_bf16 (csrc/train.hip): the streaming kernel
attn_temporal_bwd_stream_kernel on windows of 9 .. 32 frames, and the register-resident kernel (T <= 8) through the same entry.

Reference: torch fp64 autograd of softmax(q k^T / 8 + causal mask) v per (sample, position, head) on the SAME 2-byte-rounded q / k / v / dO, dq / dk rotated
back through the launch's own rope table.  Bound: the project's bound for the spatial backward op (tests/test_gpu_ops_attn_bwd_long.py): 2e-3 relative L2 per
dq / dk / dv on fp16 operands, 8 x that on bf16.  (The temporal kernels keep P and dS in fp32, so the only rounding is the 2-byte store.)  `pytest -s` prints
every measured error."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import dev, rel_l2, stream, untile  # noqa: E402
from gtav_amd import lib as L  # noqa: E402
import gtav_amd.weights as W  # noqa: E402

TOL = {torch.float16: 2e-3, torch.bfloat16: 8 * 2e-3}   # tests/test_gpu_ops_attn_bwd_long.py
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])

# (B, P, D, T, Tmax)
STREAM = [(2, 8, 256, 9, 9), (2, 8, 256, 12, 32), (2, 8, 256, 17, 32), (2, 8, 256, 31, 32), (2, 8, 256, 32, 32),
          (1, 3, 256, 16, 16),                                     # 12 items: a partial block, clamped lanes
          (1, 144, 1024, 9, 32), (1, 144, 1024, 32, 32)]           # production width
RESIDENT = [(2, 8, 256, 5, 5), (2, 8, 256, 8, 32)]


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _table(kind, n):
    """Angles [n][32] of the rope table: zeros (identity) or the model's temporal table (position t x the language frequencies)."""
    if kind == "identity":
        return torch.zeros(n, 32)
    return torch.arange(n, dtype=torch.float32)[:, None] * W.rope_freqs_lang(64)[None, :]


def _cs(ang):
    return torch.stack([ang.cos(), ang.sin()], dim=-1).reshape(ang.shape[0], 64).contiguous()      # [pos][pair][cos, sin]


def _inputs(B, P, D, T, Tmax, dtype):
    q = _rand(B, T, P, D, seed=1).to(dtype)
    kv = _rand(B, Tmax, P, 2, D, seed=2).to(dtype)
    do = _rand(B * T * P, D, seed=3).to(dtype)
    return q, kv, do


_REF = {}


def _reference(B, P, D, T, Tmax, dtype, kind):
    """[B T P][3 D] fp64: dq | dk | dv of the fp64 causal attention on the rounded operands, dq / dk rotated back (computed once per case, never modified)."""
    key = (B, P, D, T, Tmax, dtype, kind)
    if key not in _REF:
        h = D // 64
        q, kv, do = _inputs(B, P, D, T, Tmax, dtype)
        item = lambda x: x.double().reshape(B, T, P, h, 64).permute(0, 2, 3, 1, 4)             # B P h T 64
        qf, kf, vf = (item(x).clone().requires_grad_(True) for x in (q, kv[:, :T, :, 0], kv[:, :T, :, 1]))
        s = qf @ kf.transpose(-1, -2) / 8.0
        s = s.masked_fill(torch.arange(T)[None, :] > torch.arange(T)[:, None], float("-inf"))
        (s.softmax(-1) @ vf).backward(item(do.reshape(B, T, P, D)))
        ang = _table(kind, T).double()
        co, si = ang.cos(), ang.sin()                                                           # [T][32], broadcast over B P h

        def unrope(g):                                                                          # RoPE^T: rotation by the negative angle
            a, b = g[..., 0::2], g[..., 1::2]
            return torch.stack([a * co + b * si, b * co - a * si], dim=-1).reshape(g.shape)

        rows = lambda g: g.permute(0, 3, 1, 2, 4).reshape(B * T * P, D)
        _REF[key] = torch.cat([rows(unrope(qf.grad)), rows(unrope(kf.grad)), rows(vf.grad)], dim=1).contiguous()
    return _REF[key]


def _op(dtype):
    lib = L.load()
    return lib.gtav_op_attn_temporal_bwd if dtype == torch.float16 else lib.gtav_op_attn_temporal_bwd_bf16


def _launch(dtype, qd, kvd, dod, csd, B, P, D, T, Tmax):
    """-> the launch's rows [B T P][3 D] as a CPU tensor of the operand type (bit patterns carried through)."""
    M = B * T * P
    out = torch.zeros((M + 127) // 128 * 128, 3 * D, device=dev(), dtype=dtype)
    L.check(_op(dtype)(qd.data_ptr(), kvd.data_ptr(), dod.data_ptr(), B, P, D, T, Tmax, csd.data_ptr(), out.data_ptr(), stream()))
    torch.cuda.synchronize()
    return untile(out.view(torch.int16), M, 3 * D).view(dtype)


def _run(B, P, D, T, Tmax, dtype, kind):
    q, kv, do = _inputs(B, P, D, T, Tmax, dtype)
    qd, kvd, dod, csd = (x.to(dev()).contiguous() for x in (q, kv, do, _cs(_table(kind, Tmax))))
    return _launch(dtype, qd, kvd, dod, csd, B, P, D, T, Tmax)


def _check(got, B, P, D, T, Tmax, dtype, kind):
    ref = _reference(B, P, D, T, Tmax, dtype, kind)
    assert torch.isfinite(got.float()).all()
    errs = {n: rel_l2(got[:, sl].double(), ref[:, sl]) for n, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D)))}
    print(f"[attn_temporal_bwd {dtype} B={B} P={P} D={D} T={T} Tmax={Tmax} {kind}] " + " ".join(f"{n} {e:.3e}" for n, e in errs.items())
          + f" (bound {TOL[dtype]:.1e})")
    for n, e in errs.items():
        assert e < TOL[dtype], (n, e)


@DTYPES
@pytest.mark.parametrize("kind", ["identity", "temporal"])
@pytest.mark.parametrize("B,P,D,T,Tmax", STREAM)
def test_streaming_kernel_matches_fp64_autograd(B, P, D, T, Tmax, kind, dtype):
    _check(_run(B, P, D, T, Tmax, dtype, kind), B, P, D, T, Tmax, dtype, kind)


@DTYPES
@pytest.mark.parametrize("kind", ["identity", "temporal"])
@pytest.mark.parametrize("B,P,D,T,Tmax", RESIDENT)
def test_resident_kernel_through_the_same_entry(B, P, D, T, Tmax, kind, dtype):
    _check(_run(B, P, D, T, Tmax, dtype, kind), B, P, D, T, Tmax, dtype, kind)


@DTYPES
def test_nothing_beyond_the_window_or_behind_the_rows_is_read(dtype):
    """Tmax = 32, T = 12: cache frames 12 .. 31, the rows behind row B T P of q / dO and the table rows from T on hold NaN bit patterns in one set of buffers and
    zeros in the other: both outputs are finite and equal bit for bit."""
    B, P, D, T, Tmax = 2, 8, 256, 12, 32
    q, kv, do = _inputs(B, P, D, T, Tmax, dtype)
    pad = 64 * D                                            # 64 rows behind the last one: more than any lane group could over-read
    outs = []
    for fill in (float("nan"), 0.0):
        def tail(x):
            flat = x.contiguous().reshape(-1)
            buf = torch.full((flat.numel() + pad,), fill, dtype=dtype)
            buf[: flat.numel()] = flat
            return buf.to(dev())
        kvp = kv.clone()
        kvp[:, T:] = fill
        cs = _cs(_table("temporal", Tmax))
        cs[T:] = fill
        outs.append(_launch(dtype, tail(q), tail(kvp), tail(do), cs.to(dev()), B, P, D, T, Tmax))
        assert torch.isfinite(outs[-1].float()).all()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    _check(outs[0], B, P, D, T, Tmax, dtype, "temporal")


@DTYPES
@pytest.mark.parametrize("B,P,D,T,Tmax", [(2, 8, 256, 17, 32), (2, 3, 256, 9, 9)])
def test_launches_are_repeatable_and_independent_of_the_batch(B, P, D, T, Tmax, dtype):
    """No atomics and one fixed summation order per output element: two launches give the same bits, and sample 0 of the B = 2 launch equals the B = 1 launch."""
    q, kv, do = _inputs(B, P, D, T, Tmax, dtype)
    csd = _cs(_table("temporal", Tmax)).to(dev())
    qd, kvd, dod = (x.to(dev()).contiguous() for x in (q, kv, do))
    a = _launch(dtype, qd, kvd, dod, csd, B, P, D, T, Tmax)
    b = _launch(dtype, qd, kvd, dod, csd, B, P, D, T, Tmax)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    one = _launch(dtype, q[:1].contiguous().to(dev()), kv[:1].contiguous().to(dev()), do[: T * P].contiguous().to(dev()), csd, 1, P, D, T, Tmax)
    assert torch.equal(one.view(torch.int16), a[: T * P].view(torch.int16))


def test_windows_outside_the_range_are_refused_by_name():
    lib = L.load()
    z = torch.zeros(1 << 20, device=dev(), dtype=torch.float16)
    cs = torch.zeros(64 * 64, device=dev())
    for T, Tmax in ((33, 40), (12, 9), (0, 8)):
        rc = lib.gtav_op_attn_temporal_bwd(z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 8, 256, T, Tmax, cs.data_ptr(), z.data_ptr(), stream())
        assert rc != 0
        msg = lib.gtav_last_error().decode()
        assert "attn_temporal_bwd" in msg and f"T={T}" in msg and "32" in msg, msg
    _check(_run(2, 8, 256, 9, 9, torch.float16, "temporal"), 2, 8, 256, 9, 9, torch.float16, "temporal")     # the next valid call works
