"""Micro-benchmark of the spatial attention backward through the C-ABI (GPU), with the forward flash kernel as a yardstick:
    python tools/attn_bwd_bench.py [--cases bwd,1280,576 bwd,1280,288 bwd,1280,144 fwd,1280,576] [--bf16] [--iters 20]
A case is kind,items,S with items = frames x heads (16 heads).  S <= 160 with S % 16 == 0 runs the resident kernel (attn_spatial_bwd_mfma_kernel), every other S the
streaming kernel (attn_spatial_bwd_stream_kernel).  FLOPs: 10 S^2 64 per item for the backward (five tile products), 4 S^2 64 for the forward.
Times are event pairs around `--iters` back-to-back launches rotating over two buffer sets, median of `--rounds`; under `rocprofv3 --kernel-trace --stats`
the same launches give the per-kernel device times (profiles/long_frames/).
A case tbwd,B,P,T is the TEMPORAL attention backward (gtav_op_attn_temporal_bwd) of B samples x P positions x 16 heads on a window of T frames in a cache of
T frames: T <= 8 runs attn_temporal_bwd_kernel<T>, 9 <= T <= 32 attn_temporal_bwd_stream_kernel (profiles/long_window_train/); FLOPs: 5 T (T + 1) 64 per item
(the causal half of the five products)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gtav_amd import lib as L  # noqa: E402


def temporal_case(lib, a, case, dev, st):
    _, B, P, T = case.split(",")
    B, P, T, H = int(B), int(P), int(T), 16
    D = H * 64
    dt = torch.bfloat16 if a.bf16 else torch.float16
    bwd = lib.gtav_op_attn_temporal_bwd_bf16 if a.bf16 else lib.gtav_op_attn_temporal_bwd
    ang = torch.arange(T, device=dev, dtype=torch.float32)[:, None] * torch.rand(32, device=dev)[None, :]
    cs = torch.stack([ang.cos(), ang.sin()], dim=-1).reshape(T, 64).contiguous()
    M = B * T * P
    sets = [(torch.randn(M, D, device=dev).to(dt), torch.randn(B, T, P, 2, D, device=dev).to(dt), torch.randn(M, D, device=dev).to(dt),
             torch.zeros((M + 127) // 128 * 128, 3 * D, device=dev, dtype=dt)) for _ in range(2)]

    def run(i):
        q, kv, do, out = sets[i % 2]
        L.check(bwd(q.data_ptr(), kv.data_ptr(), do.data_ptr(), B, P, D, T, T, cs.data_ptr(), out.data_ptr(), st))
    for i in range(4):
        run(i)
    times = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(a.iters):
            run(i)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / a.iters)
    times.sort()
    us = times[len(times) // 2]
    flop = 5.0 * T * (T + 1) * 64 * B * P * H
    print(f"attn_temporal bwd {'bf16' if a.bf16 else 'fp16'} B={B} P={P} T={T} ({M} tokens, {B * P * H} items): median {us:9.2f} us (min {times[0]:9.2f}, "
          f"max {times[-1]:9.2f})   {flop / us / 1e6:7.2f} TFLOP/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["bwd,1280,576", "bwd,1280,288", "bwd,1280,144", "fwd,1280,576"])
    ap.add_argument("--bf16", action="store_true", help="the bf16-operand twin of the backward (the forward yardstick stays fp16)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of libgtav_amd.so (A/B of two builds, one per process)")
    a = ap.parse_args()
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)
    lib = L.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    H = 16
    for case in a.cases:
        if case.startswith("tbwd,"):
            temporal_case(lib, a, case, dev, st)
            continue
        kind, items, S = case.split(",")
        items, S = int(items), int(S)
        NB = items // H
        assert NB * H == items, "items must be a multiple of 16 heads"
        dt = torch.bfloat16 if (a.bf16 and kind == "bwd") else torch.float16
        sets = []
        for _ in range(2):
            q = (torch.randn(NB, H, S, 64, device=dev)).to(dt)
            k = (torch.randn(NB, H, S, 64, device=dev)).to(dt)
            vt = torch.randn(NB, H, 64, S, device=dev).to(dt)
            do = torch.randn(NB * S, H * 64, device=dev).to(dt)
            ang = torch.randn(S, 32, device=dev) * 3
            cs = torch.stack([ang.cos(), ang.sin()], dim=-1).reshape(S, 64).contiguous()
            out = torch.zeros((NB * S + 127) // 128 * 128, (3 if kind == "bwd" else 1) * H * 64, device=dev, dtype=dt)
            sets.append((q, k, vt, do, cs, out))
        bwd = lib.gtav_op_attn_spatial_bwd_bf16 if dt == torch.bfloat16 else lib.gtav_op_attn_spatial_bwd

        def run(i):
            q, k, vt, do, cs, out = sets[i % 2]
            if kind == "bwd":
                L.check(bwd(q.data_ptr(), k.data_ptr(), vt.data_ptr(), do.data_ptr(), NB, H, S, cs.data_ptr(), out.data_ptr(), st))
            else:
                L.check(lib.gtav_op_attn_spatial(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), NB, H, S, st))
        for i in range(4):
            run(i)
        times = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(a.iters):
                run(i)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        times.sort()
        us = times[len(times) // 2]
        flop = (10.0 if kind == "bwd" else 4.0) * items * S * S * 64
        print(f"attn_spatial {kind} {'bf16' if dt == torch.bfloat16 else 'fp16'} items={items} S={S}: median {us:9.2f} us (min {times[0]:9.2f}, max {times[-1]:9.2f})   "
              f"{flop / us / 1e6:7.1f} TFLOP/s", flush=True)
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
