"""A/B of the weight-fill cache policy (gtav_dit_set_weight_fill_policy) on the CAPTURED batch-1 window step of the product library, in ONE process on ONE GPU:
one DiT-S/2 handle, the policy words alternating round by round (each switch drops the graphs: eager warm-up, capture, first replay, then `--steps` timed
replays), under the next-weight prefetch as the library ships it, as generate.tune_weight_prefetch leaves it (`--tuned`) and off.  Prints ms per step, best
and median of the rounds, and the difference to the default policy in the same prefetch setting.
Usage (GPU box): python tools/fill_policy_ab.py [--steps 48] [--rounds 5] [--tuned]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import gtav_amd  # noqa: E402,F401


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tuned", action="store_true", help="also under the prefetch mode and fused switches generate.tune_weight_prefetch picks on this GPU")
    a = ap.parse_args()
    import gtav_amd.weights as W
    from gtav_amd.generate import PREFETCH_CLASSES, fill_policy_mode, tune_weight_prefetch
    from gtav_amd.model.dit import DiT_models
    from gtav_amd.utils import alphas_cumprod
    dev = torch.device("cuda", 0)
    m = DiT_models["DiT-S/2"](init_weights=False, max_batch=1)
    m.load_state_dict(W.synth_state_dict(W.dit_param_shapes(depth=16), seed=0))
    m.set_schedule(alphas_cumprod(1e-4))
    x0 = (torch.randn(1, 5, 16, 18, 32, generator=torch.Generator().manual_seed(11)) * 0.5).to(dev)
    ts = [999 - 7 * k for k in range(a.steps + 3)]

    def timed(word):
        m.set_weight_fill_policy(word)
        x = x0.clone()
        m.prepare_frame_(1, 5, 0, 4, 15, ts, None)
        for k in range(3):
            m.denoise_step_(x, 0, 4, 15, ts[k], ts[k + 1], False, None, cond_step=k)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for k in range(3, a.steps + 3):
            m.denoise_step_(x, 0, 4, 15, ts[k], ts[min(k + 1, a.steps + 2)], False, None, cond_step=k)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / a.steps * 1e3, x

    words = [("default", 0)] + [(c, fill_policy_mode(tuple(int(i == j) for j in range(4)))) for i, c in enumerate(PREFETCH_CLASSES)] + [("all", 0x1111)]
    settings = [("prefetch as shipped", lambda: m.set_weight_prefetch(0x11441)), ("prefetch off", lambda: m.set_weight_prefetch(0))]
    if a.tuned:
        r = tune_weight_prefetch(m, 1, fill_policy=False)
        m.set_schedule(alphas_cumprod(1e-4))
        print("tuner (fill policy left out):", r, flush=True)
        settings.insert(0, (f"prefetch tuned ({r['mode']:#x})", lambda: m.set_weight_prefetch(r["mode"])))
    for name, apply in settings:
        apply()
        ms = {w: [] for w, _ in words}
        ref = None
        for _ in range(a.rounds):
            for w, word in words:
                t, x = timed(word)
                ms[w].append(t)
                ref = x if ref is None else ref
                assert torch.equal(x, ref), f"{w}: the latents differ"
        base = statistics.median(ms["default"])
        print(f"{name}: ms per captured step over {a.rounds} rounds of {a.steps} replays (best / median / median vs default)")
        for w, _ in words:
            med = statistics.median(ms[w])
            print(f"  nt fills: {w:8s} {min(ms[w]):.4f} / {med:.4f} / {(med / base - 1) * 100:+.2f} %", flush=True)
    m.set_weight_fill_policy(0)
    m.check()


if __name__ == "__main__":
    main()
