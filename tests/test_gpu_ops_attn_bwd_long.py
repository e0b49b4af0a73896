"""Spatial attention backward on frames of more than 160 tokens and on S % 16 == 8 (csrc/train.hip attn_spatial_bwd_stream_kernel), fp16 and bf16 operands,
through gtav_op_attn_spatial_bwd / gtav_op_attn_spatial_bwd_bf16.

Reference: torch autograd of softmax(q k^T / 8) v in fp32 on the SAME 2-byte-rounded q / k / v / dO, un-rotated through the RoPE — the pattern of
tests/test_gpu_ops.py::test_attention_spatial_backward_mfma.  Tolerances: fp16 2e-3 relative L2 per dq / dk / dv (that test's bound: the kernel's only
extra rounding is P and dS to the operand type); bf16 8 x that, the ratio tests/test_gpu_train_bf16.py keeps between its two gradient bounds.  `pytest -s`
prints every measured error."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import dev, rel_l2, stream, untile  # noqa: E402
from gtav_amd import lib as L  # noqa: E402

TOL = {torch.float16: 2e-3, torch.bfloat16: 8 * 2e-3}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_spatial_bwd_resident.safetensors")

LONG = [(2, 4, 576), (1, 2, 288), (1, 1, 1024)]
RAGGED = [(2, 2, 200), (1, 1, 168)]
SHORT8 = [(2, 2, 152), (1, 1, 8)]


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _inputs(NB, heads, S, dtype):
    D = heads * 64
    q = _rand(NB, heads, S, 64, seed=1).to(dtype)
    k = _rand(NB, heads, S, 64, seed=2).to(dtype)
    v = _rand(NB, heads, S, 64, seed=3).to(dtype)
    do = _rand(NB * S, D, seed=4).to(dtype)
    ang = _rand(S, 32, seed=5) * 3
    cs = torch.stack([ang.cos(), ang.sin()], dim=-1).reshape(S, 64).contiguous()          # [pos][pair][cos, sin]
    return q, k, v, do, ang, cs


_REF = {}


def _reference(NB, heads, S, dtype):
    """[NB S][3 D] fp32: dq | dk | dv of the fp32 attention on the rounded operands, dq / dk rotated back (computed once per case, never modified)."""
    key = (NB, heads, S, dtype)
    if key not in _REF:
        D = heads * 64
        q, k, v, do, ang, _ = _inputs(NB, heads, S, dtype)
        qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
        o = torch.softmax(qf @ kf.transpose(-1, -2) / 8.0, dim=-1) @ vf                            # NB h S 64
        o.backward(do.float().reshape(NB, S, heads, 64).permute(0, 2, 1, 3))
        co, si = ang.cos()[None, None], ang.sin()[None, None]                                      # RoPE^T: rotation by the negative angle

        def unrope(gr):
            a, b = gr[..., 0::2], gr[..., 1::2]
            return torch.stack([a * co + b * si, b * co - a * si], dim=-1).reshape(gr.shape)

        ref = torch.cat([unrope(qf.grad), unrope(kf.grad), vf.grad], dim=1)                        # NB (3 h) S 64
        _REF[key] = ref.reshape(NB, 3, heads, S, 64).permute(0, 3, 1, 2, 4).reshape(NB * S, 3 * D).contiguous()
    return _REF[key]


def _op(dtype):
    lib = L.load()
    return lib.gtav_op_attn_spatial_bwd if dtype == torch.float16 else lib.gtav_op_attn_spatial_bwd_bf16


def _launch(dtype, qd, kd, vtd, dod, csd, NB, heads, S):
    Mp = (NB * S + 127) // 128 * 128
    out = torch.zeros(Mp, 3 * heads * 64, device=dev(), dtype=dtype)
    L.check(_op(dtype)(qd.data_ptr(), kd.data_ptr(), vtd.data_ptr(), dod.data_ptr(), NB, heads, S, csd.data_ptr(), out.data_ptr(), stream()))
    torch.cuda.synchronize()
    return out


def _untile(out, R, K):
    return untile(out.view(torch.int16), R, K).view(out.dtype)     # (indexing only: the 2-byte pattern is carried through)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("NB,heads,S", LONG + RAGGED + SHORT8)
def test_attention_spatial_backward_streaming(NB, heads, S, dtype):
    """Long sequences (several key / query chunks and groups), a half-empty last 16-row tile, and S % 16 == 8 below the resident kernel's bound:
    two launches bitwise equal, dq / dk / dv within the bound."""
    D = heads * 64
    q, k, v, do, _, cs = _inputs(NB, heads, S, dtype)
    ref = _reference(NB, heads, S, dtype)
    qd, kd, vtd, dod, csd = (t.to(dev()).contiguous() for t in (q, k, v.transpose(-1, -2), do, cs))
    out = _launch(dtype, qd, kd, vtd, dod, csd, NB, heads, S)
    out2 = _launch(dtype, qd, kd, vtd, dod, csd, NB, heads, S)
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))          # no atomics: launches are bitwise reproducible
    got = _untile(out, NB * S, 3 * D).float()
    assert torch.isfinite(got).all()
    errs = {name: rel_l2(got[:, sl], ref[:, sl]) for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D)))}
    print(f"[attn_spatial_bwd {dtype} NB={NB} heads={heads} S={S}] " + " ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    for name, e in errs.items():
        assert e < TOL[dtype], (name, e)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_nothing_behind_the_frame_leaks_in(dtype):
    """The buffers are not padded per frame.  S = 200 (last tile half empty), one (frame, head): the rows behind the item in q / k / dO and the elements behind
    the last V^T row are NaN bit patterns (as tests/test_gpu_long_window.py does for the temporal cache); a second set of buffers holds the same frame followed by
    zeros.  Both outputs must be finite and equal bit for bit.  With two items, the neighbour of a V^T row past column S is the next row — covered by the parity
    test: a leak would show as an error."""
    NB, heads, S = 1, 1, 200
    D = 64
    q, k, v, do, _, cs = _inputs(NB, heads, S, dtype)
    pad = 64                                    # rows / columns of tail: more than any tile or chunk could over-read

    def tail(t, fill):                          # t flattened + `pad` rows of `fill` behind it
        flat = t.contiguous().reshape(-1)
        buf = torch.full((flat.numel() + pad * 64,), fill, dtype=dtype)
        buf[: flat.numel()] = flat
        return buf.to(dev())
    outs = []
    for fill in (float("nan"), 0.0):
        qd, kd, vtd, dod = (tail(t, fill) for t in (q, k, v.transpose(-1, -2), do))
        csd = torch.full((S * 64 + pad * 64,), fill)
        csd[: S * 64] = cs.reshape(-1)
        csd = csd.to(dev())
        out = _launch(dtype, qd, kd, vtd, dod, csd, NB, heads, S)
        got = _untile(out, NB * S, 3 * D)
        assert torch.isfinite(got.float()).all()
        outs.append(got)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    assert rel_l2(outs[0].float(), _reference(NB, heads, S, dtype)) < TOL[dtype]


def test_sequence_lengths_that_are_no_multiple_of_8_are_refused_by_name():
    lib = L.load()
    z = torch.zeros(1 << 16, device=dev(), dtype=torch.float16)
    cs = torch.zeros(1 << 14, device=dev())
    for S in (0, 4, 148, 180):
        rc = lib.gtav_op_attn_spatial_bwd(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 1, S, cs.data_ptr(), z.data_ptr(), stream())
        assert rc != 0
        assert "multiple of 8" in lib.gtav_last_error().decode()


@pytest.mark.parametrize("NB,heads,S", [(3, 2, 144), (1, 1, 160)])
def test_resident_shapes_keep_their_bits(NB, heads, S):
    """S <= 160 with S % 16 == 0 still runs attn_spatial_bwd_mfma_kernel: the output equals, bit for bit, what this repository's kernel gave before the
    streaming kernel existed (tests/golden/attn_spatial_bwd_resident.safetensors, written by tools/make_attn_bwd_fixture.py: a checksum pair and a strided
    sample of the fp16 output per shape)."""
    from safetensors.torch import load_file
    gold = load_file(GOLDEN)
    D = heads * 64
    q, k, v, do, _, cs = _inputs(NB, heads, S, torch.float16)
    qd, kd, vtd, dod, csd = (t.to(dev()).contiguous() for t in (q, k, v.transpose(-1, -2), do, cs))
    out = _launch(torch.float16, qd, kd, vtd, dod, csd, NB, heads, S)
    bits = _untile(out, NB * S, 3 * D).view(torch.int16).reshape(-1).to(torch.int64) & 0xFFFF
    w = torch.arange(bits.numel(), dtype=torch.int64) % 65521 + 1
    sums = torch.stack([bits.sum(), (bits * w).sum() % ((1 << 61) - 1)])
    tag = f"{NB}x{heads}x{S}"
    assert torch.equal(bits[::7].to(torch.int32), gold[f"sample.{tag}"])
    assert torch.equal(sums, gold[f"sums.{tag}"])
