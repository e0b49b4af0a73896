#!/usr/bin/env python3
"""Writes tests/golden/attn_spatial_bwd_resident.safetensors: the bits of gtav_op_attn_spatial_bwd at the shapes the resident kernel
(attn_spatial_bwd_mfma_kernel, S <= 160 and S % 16 == 0) serves, from a given build of the library — the commit before the streaming kernel was added, so
that tests/test_gpu_ops_attn_bwd_long.py::test_resident_shapes_keep_their_bits pins "those shapes keep their bits".  Needs a GPU.
usage: tools/make_attn_bwd_fixture.py [--lib path/to/libgtav_amd.so] [--out file]
Per shape NB x heads x S: `sample.<tag>` = every 7th 2-byte pattern of the row-major [NB S][3 D] output, `sums.<tag>` = (sum, weighted sum) of all patterns."""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(3, 2, 144), (1, 1, 160)]


def tiled_index(R, K):
    r = torch.arange(R)[:, None]
    k = torch.arange(K)[None, :]
    return ((r >> 7) * (K >> 6) + (k >> 6)) * 8192 + (r & 127) * 64 + ((((k >> 3) & 7) ^ (r & 7)) << 3) + (k & 7)


def rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "ai-generated-gtav_amd", "libgtav_amd.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "attn_spatial_bwd_resident.safetensors"))
    a = ap.parse_args()
    from safetensors.torch import save_file
    lib = C.CDLL(a.lib)
    fn = lib.gtav_op_attn_spatial_bwd
    fn.argtypes = [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_void_p] * 3
    fn.restype = C.c_int
    lib.gtav_last_error.restype = C.c_char_p
    dev = torch.device("cuda", 0)
    out = {}
    for NB, heads, S in SHAPES:
        D = heads * 64
        # the inputs of tests/test_gpu_ops_attn_bwd_long.py::_inputs
        q, k, v = (rand(NB, heads, S, 64, seed=s).half() for s in (1, 2, 3))
        do = rand(NB * S, D, seed=4).half()
        ang = rand(S, 32, seed=5) * 3
        cs = torch.stack([ang.cos(), ang.sin()], dim=-1).reshape(S, 64).contiguous()
        qd, kd, vtd, dod, csd = (t.to(dev).contiguous() for t in (q, k, v.transpose(-1, -2), do, cs))
        Mp = (NB * S + 127) // 128 * 128
        o = torch.zeros(Mp, 3 * D, device=dev, dtype=torch.float16)
        rc = fn(qd.data_ptr(), kd.data_ptr(), vtd.data_ptr(), dod.data_ptr(), NB, heads, S, csd.data_ptr(), o.data_ptr(), None)
        if rc:
            raise SystemExit(lib.gtav_last_error().decode())
        torch.cuda.synchronize()
        flat = o.view(torch.int16).reshape(-1).cpu()
        bits = flat[tiled_index(NB * S, 3 * D).reshape(-1)].to(torch.int64) & 0xFFFF
        w = torch.arange(bits.numel(), dtype=torch.int64) % 65521 + 1
        tag = f"{NB}x{heads}x{S}"
        out[f"sample.{tag}"] = bits[::7].to(torch.int32).contiguous()
        out[f"sums.{tag}"] = torch.stack([bits.sum(), (bits * w).sum() % ((1 << 61) - 1)])
        print(tag, out[f"sums.{tag}"].tolist())
    save_file(out, a.out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
