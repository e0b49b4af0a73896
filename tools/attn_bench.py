"""Micro-benchmark of the attention kernels through the C-ABI (GPU):
    python tools/attn_bench.py [--nb 5 40 80]                       spatial attention
    python tools/attn_bench.py --temporal [--bf16] [--cases B,Tq,t0 ...]   temporal attention: the streaming kernel of windows above 8 frames and, as the
                                                                    yardstick, the register-resident kernel at (B, 8, 0) / (B, 5, 0)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gtav_amd import lib as L  # noqa: E402


TEMPORAL_CASES = ["1,32,0", "8,32,0", "8,16,0", "1,1,31", "8,1,31", "1,8,0", "8,8,0", "1,5,0", "8,5,0", "1,1,7", "8,1,7"]


def temporal(a, lib, dev, st):
    """Per case: median / min / max over `--rounds` timed batches of `--iters` launches (one event pair per batch), after 8 warm-up launches; the launches
    rotate over buffer sets whose total size exceeds the 256 MB Infinity Cache, so no launch finds its operands cached by the one before.
    Bytes moved: window launches touch every q / k / v / o element once (4 M D 2); a context-cached launch reads 2 (t0 + 1) cache rows and one q row and
    writes one o row per column ((2 (t0 + 1) + 2) B P D 2)."""
    P, D = a.p, a.d
    dt = torch.bfloat16 if a.bf16 else torch.float16
    op = lib.gtav_op_attn_temporal_bf16 if a.bf16 else lib.gtav_op_attn_temporal
    print(f"attn_temporal P={P} D={D} {'bf16' if a.bf16 else 'fp16'} operands; {a.rounds} rounds x {a.iters} launches, us per launch")
    for case in a.cases:
        B, Tq, t0 = (int(v) for v in case.split(","))
        Tmax = t0 + Tq
        M = B * Tq * P
        nbytes = 4 * M * D * 2 if t0 == 0 else (2 * (t0 + 1) + 2) * B * P * D * 2
        per_set = (B * Tmax * P * 2 * D + 2 * M * D) * 2
        nsets = max(4, min(16, int(300e6 // per_set) + 1))
        sets = []
        for _ in range(nsets):
            q = (torch.randn(B, Tq, P, D, device=dev) * 0.5).to(dt)
            kv = (torch.randn(B, Tmax, P, 2, D, device=dev) * 0.5).to(dt)
            out = torch.zeros((M + 127) // 128 * 128, D, device=dev, dtype=dt)
            sets.append((q, kv, out))

        def run(i):
            q, kv, out = sets[i % nsets]
            L.check(op(q.data_ptr(), kv.data_ptr(), out.data_ptr(), B, P, D, Tq, t0, Tmax, st))
        for i in range(8):
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
        med = times[len(times) // 2]
        kern = "stream" if t0 + Tq > 8 else "registers"
        print(f"  B={B} Tq={Tq:2d} t0={t0:2d} ({kern:9s}): median {med:8.2f}  min {times[0]:8.2f}  max {times[-1]:8.2f} us   {nbytes / 1e6:7.2f} MB -> "
              f"{nbytes / med / 1e3:7.1f} GB/s   {med * 1e3 / (nbytes / 1e6):7.2f} ns/MB   ({nsets} buffer sets)")
        del sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--temporal", action="store_true", help="time gtav_op_attn_temporal instead of the spatial kernel")
    ap.add_argument("--cases", nargs="+", default=TEMPORAL_CASES, help="--temporal: B,Tq,t0 triples")
    ap.add_argument("--p", type=int, default=144, help="--temporal: tokens per frame")
    ap.add_argument("--d", type=int, default=1024, help="--temporal: model width")
    ap.add_argument("--rounds", type=int, default=7, help="--temporal: timed batches per case")
    ap.add_argument("--bf16", action="store_true", help="--temporal: the bf16-operand twin (gtav_op_attn_temporal_bf16)")
    ap.add_argument("--nb", type=int, nargs="+", default=[5, 40, 80])
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--s", type=int, default=144)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--exp", action="store_true", help="experiments build (libgtav_amd_exp.so): honours GTAV_ATTN_FLASH_NQT / GTAV_ATTN_FLASH_OCC3")
    a = ap.parse_args()
    lib = L.load_experiments() if a.exp else L.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    if a.temporal:
        return temporal(a, lib, dev, st)
    for NB in a.nb:
        S, H = a.s, a.heads
        # rotate over several buffer sets so inputs are not L2-resident from the previous launch
        sets = []
        for _ in range(4):
            q = (torch.randn(NB, H, S, 64, device=dev) * 0.5).half()
            k = (torch.randn(NB, H, S, 64, device=dev) * 0.5).half()
            vt = torch.randn(NB, H, 64, S, device=dev).half()
            out = torch.zeros((NB * S + 127) // 128 * 128, H * 64, device=dev, dtype=torch.float16)
            sets.append((q, k, vt, out))

        def run(i):
            q, k, vt, out = sets[i % 4]
            L.check(lib.gtav_op_attn_spatial(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), NB, H, S, st))
        for i in range(8):
            run(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(a.iters):
            run(i)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.iters
        mb = NB * H * S * 64 * 2 * 4 / 1e6
        print(f"attn_spatial NB={NB:4d} heads={H} S={S}: {us:8.2f} us   {mb:7.1f} MB moved -> {mb / us:5.2f} TB/s   "
              f"{4.0 * NB * H * S * S * 64 / us / 1e6:7.1f} TFLOP/s")


if __name__ == "__main__":
    main()
