"""Time of the training window's noising at the shipped geometry (B = 16, W = 5, n = 16 x 18 x 32 = 9 216): the one launch of the rng= path
(gtav_noise_window_rng) against the sequence the explicit-draw path of train._frame_step runs on draws that already sit on the device (two slice copies into
all_noise, gtav_add_noise, three .contiguous() copies, gtav_vtarget).  Device events around `--reps` repetitions after a warm-up, the two alternating for
`--rounds` rounds.  Both are a handful of microsecond-sized launches: what the events see is mostly how fast the host enqueues them.
    python tools/noise_window_time.py [--out profiles/rng/noise_window_time.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtav_amd import lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    lib = L.load()
    B, W, shape = 16, 5, (16, 18, 32)
    n = 16 * 18 * 32
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, W, *shape, generator=g) * 0.5).to(dev)
    alpha = torch.rand(B, W, generator=g).to(dev)
    ctx_noise, noise = torch.randn(B, W - 1, *shape, generator=g).to(dev), torch.randn(B, 1, *shape, generator=g).to(dev)
    x_noisy = torch.empty_like(x)
    v_target = torch.empty((B, *shape), device=dev)
    s = L.current_stream()

    def fused(k):
        L.check(lib.gtav_noise_window_rng(x.data_ptr(), alpha.data_ptr(), x_noisy.data_ptr(), v_target.data_ptr(), B, W, n, 0x1234, k, 0, 20.0, s))

    def sequence(k):
        all_noise = torch.empty_like(x)
        all_noise[:, :-1] = ctx_noise
        all_noise[:, -1:] = noise
        L.check(lib.gtav_add_noise(x.data_ptr(), all_noise.data_ptr(), alpha.data_ptr(), x_noisy.data_ptr(), B * W, n, 20.0, s))
        x_last, nz_last, a_last = x[:, -1].contiguous(), all_noise[:, -1].contiguous(), alpha[:, -1].contiguous()
        vt = torch.empty_like(x_last)
        L.check(lib.gtav_vtarget(x_last.data_ptr(), nz_last.data_ptr(), a_last.data_ptr(), vt.data_ptr(), B, n, 20.0, s))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(args.reps):
            fn(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps * 1e3

    for fn in (fused, sequence):
        for k in range(20):
            fn(k)
    torch.cuda.synchronize()
    res = {"fused": [], "sequence": []}
    for _ in range(args.rounds):
        res["fused"].append(timed(fused))
        res["sequence"].append(timed(sequence))
    lines = [f"noise of the training window, B={B} W={W} n={n}, {args.reps} repetitions per reading, {args.rounds} alternating rounds, device events, "
             f"{torch.cuda.get_device_name(0)}",
             "microseconds per repetition (median, min .. max):"]
    for name, what in (("fused", "gtav_noise_window_rng, one launch"),
                       ("sequence", "2 slice copies + gtav_add_noise + 3 .contiguous() + gtav_vtarget (7 launches, 2 allocations)")):
        v = res[name]
        lines.append(f"  {name:9s} {statistics.median(v):8.2f}  ({min(v):.2f} .. {max(v):.2f})   {what}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
