"""Time per generated frame of a play session (gtav_amd.play.PlaySession) against generate_latents on the same GPU: DiT-S/2 on 18 x 32 latents and the
production ViT-L/20 VAE at 360 x 640, synthetic weights, a window of 5 frames, batch 1, ctx_cache=True, hoisted conditioning, actions on, device-side noise.
Four legs per noise-step count, interleaved a, b, c, d, a, b, ... for `--rounds` rounds of `--frames` frames each, a host clock around a device synchronise
per round:
    (a) generate_latents, per generated frame (a 4-frame prompt, so every frame runs the full window): the path before play sessions, the baseline
    (b) a session with decode=None          — the launches of (a) plus one gtav_rng_normal per frame instead of one per clip
    (c) a session with decode="sync"        — plus latents_to_tokens + vae.decode + frames_to_u8 of the finished frame on the same stream
    (d) the decode on a second stream       — OverlapSession below: the same three calls on a stream of its own, beside the next frame's steps.  This is
                                              the experiment that decided the feature: it made every frame slower than (c), so PlaySession offers "sync" only
Warm-up is window + 2 frames per leg, so that every step is captured before the first reading.  Medians and min .. max per leg; the two comparisons the
numbers are read for are printed under them as they come out, whichever way.
    python tools/play_frame_time.py [--out profiles/play/frame_time.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtav_amd import lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--noise-steps", type=int, nargs="*", default=[10, 50, 100])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.frames >= 20 and args.rounds >= 5, "at least 5 rounds of at least 20 frames"
    L.load()
    import gtav_amd.weights as W
    from gtav_amd.generate import generate_latents
    from gtav_amd.model.dit import DiT_models
    from gtav_amd.model.vae import VAE_models
    from gtav_amd.generate import vae_decode_frames
    from gtav_amd.play import PlaySession
    from gtav_amd.rng import NoiseSource

    class OverlapSession(PlaySession):
        """Leg (d): decode="sync" with the decode moved to a second stream.  The finished latent frame is copied to the staging buffer on the compute stream
        and an event recorded; the decode stream waits for it, runs the three calls and records its own event, which the compute stream waits for only before
        it overwrites the staging buffer a frame later.  The returned frame is ordered on the decode stream."""

        def __init__(self, *a, **kw):
            super().__init__(*a, decode="sync", **kw)
            self._dec_stream, self._staged, self._decoded = torch.cuda.Stream(self._x.device), torch.cuda.Event(), torch.cuda.Event()

        def _decode_frame(self, lat):
            compute = torch.cuda.current_stream(lat.device)
            compute.wait_event(self._decoded)
            self._stage[:, 0].copy_(lat)
            self._staged.record(compute)
            with torch.cuda.stream(self._dec_stream):
                self._dec_stream.wait_event(self._staged)
                out = vae_decode_frames(self._stage, self.vae)
                self._decoded.record(self._dec_stream)
            return out[:, 0]

    dev = torch.device("cuda", 0)
    F, B, n_prompt = 5, 1, 4
    dit = DiT_models["DiT-S/2"](init_weights=False, max_batch=B)
    dit.load_state_dict(W.synth_state_dict(W.dit_param_shapes(depth=16), seed=0))
    vae = VAE_models["vit-l-20-shallow-encoder"](init_weights=False, max_frames_per_call=B)
    vae.load_state_dict(W.synth_state_dict(W.vae_param_shapes(), seed=1))
    dit.reserve(B, F, noise_steps=max(args.noise_steps))          # one handle for every leg and step count
    g = torch.Generator().manual_seed(11)
    x_prompt = (torch.randn(B, n_prompt, 16, 18, 32, generator=g) * 0.5).to(dev)
    total = n_prompt + args.frames
    acts = torch.zeros(B, total, 25, device=dev)
    acts[:, torch.arange(total), torch.randint(0, 25, (total,), generator=g)] = 1
    lines = [f"play session against generate_latents: DiT-S/2 on 18 x 32 latents (144 tokens per frame), ViT-L/20 VAE at 360 x 640, window {F}, batch {B}, ctx_cache, "
             f"hoisted conditioning, actions, device-side noise; {args.rounds} interleaved rounds of {args.frames} frames per leg, host clock around a device "
             f"synchronise per round, {torch.cuda.get_device_name(0)}",
             "ms per generated frame: median (min .. max)"]
    for ns in args.noise_steps:
        kw = lambda: dict(prompt_latents=x_prompt, prompt_actions=acts[:, :n_prompt], noise_steps=ns, rng=NoiseSource(7))
        sessions = {"b": PlaySession(dit, vae, decode=None, **kw()), "c": PlaySession(dit, vae, decode="sync", **kw()), "d": OverlapSession(dit, vae, **kw())}
        rng_a = NoiseSource(7)

        def run(leg, frames):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            if leg == "a":
                generate_latents(dit, x_prompt, n_prompt + frames, ns, actions=acts[:, :n_prompt + frames], ctx_cache=True, rng=rng_a)
            else:
                s = sessions[leg]
                for k in range(frames):
                    s.step(acts[:, (n_prompt + k) % total])
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) / frames * 1e3

        for leg in "abcd":
            run(leg, F + 2)                                       # warm-up: every step of the leg captured
            if leg == "a":
                run(leg, args.frames)                             # (generate_latents' buffers, and with them its captured steps, depend on the clip length)
        res = {leg: [] for leg in "abcd"}
        for _ in range(args.rounds):
            for leg in "abcd":
                res[leg].append(run(leg, args.frames))
        for s in sessions.values():
            s.check()
            s.close()
        med = {leg: statistics.median(r) for leg, r in res.items()}
        lines.append(f"noise_steps {ns}")
        names = {"a": "generate_latents", "b": "session, decode=None", "c": 'session, decode="sync"', "d": "decode on a second stream"}
        for leg in "abcd":
            lines.append(f"  ({leg}) {names[leg]:27s} {med[leg]:9.3f} ({min(res[leg]):.3f} .. {max(res[leg]):.3f})")
        inside = min(res["a"]) <= med["b"] <= max(res["a"])
        lines.append(f"      (b) median is {'inside' if inside else 'OUTSIDE'} (a)'s min .. max; (b) - (a) = {med['b'] - med['a']:+.3f} ms per frame")
        slower = med["d"] > max(res["c"])
        lines.append(f"      (d) median is {'ABOVE' if slower else 'not above'} (c)'s max; (c) - (d) = {med['c'] - med['d']:+.3f} ms per frame")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
