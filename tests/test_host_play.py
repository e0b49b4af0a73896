"""CPU (no GPU): the host side of gtav_amd.play — the ring addressing, the slot and noise-stream numbering, the argument rules, and that PlaySession and
generate_latents run the one per-frame body generate.denoise_frame.  Sessions are built against the recording stand-in for the library of
tools/model_call_trace.py (every C call is recorded and returns 0), with denoise_frame replaced by a recorder."""
import contextlib
import importlib.util
import os

import pytest
import torch

from gtav_amd import generate, play
from gtav_amd.play import PlaySession, check_session_args, check_step_args, ring_slot, ring_window
from gtav_amd.rng import NoiseSource

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def tool():
    """tools/model_call_trace.py, its stand_in() wrapped so that every model of the block gives its (stand-in) handle back while the stand-in is still the
    library: the test's own variables keep the models alive beyond the block, and the real library must never be handed such a handle."""
    spec = importlib.util.spec_from_file_location("model_call_trace", os.path.join(ROOT, "tools", "model_call_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    inner = mod.stand_in

    @contextlib.contextmanager
    def stand_in():
        with inner() as sim:
            try:
                yield sim
            finally:
                for m in mod.ALIVE:
                    m._free()
                del mod.ALIVE[:]
    mod.stand_in = stand_in
    return mod


@pytest.fixture()
def frames(monkeypatch):
    """generate.denoise_frame replaced by a recorder of (F, start, cur, ctx_cache, hoist_cond, action rows of the window in temporal order)."""
    seen = []

    def recorder(model, x, start, cur, t_of, order, act, stabilization_level, ctx_cache, hoist_cond):
        F = x.shape[1]
        T = cur - start + 1 + (F if cur < start else 0)
        rows = None if act is None else torch.stack([act[:, (start + j) % F] for j in range(T)], dim=1).clone()
        seen.append(dict(F=F, start=start, cur=cur, T=T, t_of=list(t_of), order=list(order), ctx_cache=ctx_cache, hoist_cond=hoist_cond, act=rows,
                         level=stabilization_level))
    monkeypatch.setattr(generate, "denoise_frame", recorder)
    return seen


# ---- ring addressing ------------------------------------------------------------------------------------------------------------------------------
def test_ring_window_is_the_linear_window_modulo_F():
    for F in range(1, 33):
        for n in range(0, 3 * F + 1):
            lin = max(0, n + 1 - F)                                   # generate_latents: start = max(0, i + 1 - max_frames), cur = i
            start, cur, T = ring_window(n, F)
            assert (start, cur, T) == (lin % F, n % F, n - lin + 1) and 1 <= T <= F and 0 <= start < F and 0 <= cur < F
            assert T == cur - start + 1 + (F if cur < start else 0)    # the T the C entry points compute
            assert [(start + j) % F for j in range(T)] == [ring_slot(f, F) for f in range(lin, n + 1)]     # the window's frames, in temporal order
            if n < F:
                assert (start, cur) == (0, n)                          # not wrapped yet: the linear call, argument for argument
    with pytest.raises(ValueError):
        ring_window(3, 0)
    with pytest.raises(ValueError):
        ring_window(-1, 4)


def test_the_factored_frame_body_is_one_function_object():
    assert play._gen is generate and play._gen.denoise_frame is generate.denoise_frame
    assert "denoise_frame" in generate.generate_latents.__wrapped__.__code__.co_names
    assert not hasattr(play, "denoise_frame") and "denoise_step_" not in PlaySession.step.__wrapped__.__code__.co_names


# ---- sessions against the stand-in ----------------------------------------------------------------------------------------------------------------------
def _prompt(B, n, A=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, 16, 4, 4, generator=g), torch.randn(B, n, A, generator=g)


@pytest.mark.parametrize("n_prompt", [1, 3, 7])
def test_slots_noise_stream_and_windows(tool, frames, n_prompt):
    """Absolute frame f lives in slot f % F and is drawn from stream slot f of the ONE draw number the session took; its window is generate_latents' window,
    frame for frame and action row for action row.  F = 4; the prompt of 7 frames is longer than the ring."""
    F, B, n_new, fsz = 4, 2, 11, 16 * 4 * 4
    xp, ap = _prompt(B, n_prompt)
    acts = torch.randn(B, n_new, 3, generator=torch.Generator().manual_seed(5))
    with tool.stand_in() as sim:
        m = tool.dit(max_frames=F, max_batch=B)
        rng = NoiseSource(77, sample0=10)
        rng.next_draw()
        s = PlaySession(m, prompt_latents=xp, prompt_actions=ap, noise_steps=3, rng=rng, decode=None, ctx_cache=False, stabilization_level=9)
        assert rng.draw == 2 and s.frame_index == n_prompt - 1 and s.F == F
        keep = min(n_prompt, F - 1)
        assert torch.equal(s.window(), xp[:, n_prompt - keep:])
        for k in range(n_new):
            s.step(acts[:, k])
            assert s.frame_index == n_prompt + k
        draws = [c for c in sim.calls if c[0] == "gtav_rng_normal"]
        s.close()
    assert len(draws) == n_new and len(frames) == n_new
    all_act = torch.cat([ap, acts], dim=1)
    for k, (c, fr) in enumerate(zip(draws, frames)):
        f = n_prompt + k
        # gtav_rng_normal(out, sample_stride, rows, n, seed, draw, sample0, slot0, slots_per_sample, clamp_abs, stream)
        assert c[2:10] == [F * fsz, B, fsz, 77, 1, 10, f, 1], (k, c)
        lin = max(0, f + 1 - F)
        assert (fr["F"], fr["start"], fr["cur"], fr["T"]) == (F, lin % F, f % F, f - lin + 1)
        assert torch.equal(fr["act"], all_act[:, lin:f + 1]), k
        assert (fr["ctx_cache"], fr["hoist_cond"], fr["level"]) == (False, True, 9)
        assert (fr["t_of"], fr["order"]) == generate.noise_schedule(3) == ([0, 333, 666, 999], [3, 2, 1, 0])


def test_generate_latents_runs_the_same_body_on_the_same_windows(tool, frames):
    """generate_latents and a session over the same clip call generate.denoise_frame once per generated frame with the same schedule, switches and action
    rows; the windows differ only in being taken modulo F."""
    F, B, n_prompt, n_new = 3, 1, 2, 7
    xp, acts = _prompt(B, n_prompt + n_new)
    with tool.stand_in():
        m = tool.dit(max_frames=F, max_batch=B)
        generate.generate_latents(m, xp[:, :n_prompt], n_prompt + n_new, 3, actions=acts, ctx_cache=True, rng=NoiseSource(1))
        lin, frames[:] = list(frames), []
        with PlaySession(m, prompt_latents=xp[:, :n_prompt], prompt_actions=acts[:, :n_prompt], noise_steps=3, rng=NoiseSource(1), decode=None) as s:
            for k in range(n_new):
                s.step(acts[:, n_prompt + k])
    assert len(lin) == len(frames) == n_new
    for a, b in zip(lin, frames):
        assert (a["F"], b["F"]) == (n_prompt + n_new, F)
        assert (b["start"], b["cur"], b["T"]) == (a["start"] % F, a["cur"] % F, a["T"])
        assert torch.equal(a["act"], b["act"])
        assert all(a[k] == b[k] for k in ("t_of", "order", "ctx_cache", "hoist_cond", "level"))


def test_explicit_noise_is_copied_and_clamped(tool, frames):
    with tool.stand_in() as sim:
        m = tool.dit(max_frames=3)
        with PlaySession(m, prompt_latents=_prompt(1, 1)[0], noise_steps=2, decode=None, noise_abs_max=1.5) as s:
            nz = torch.randn(1, 16, 4, 4)
            out = s.step(noise=nz)
            assert torch.equal(out, nz)                                # (the stand-in's clamp does nothing: the draw reached slot 1 as given)
        clamps = [c for c in sim.calls if c[0] == "gtav_clamp_frames"]
        assert [c[2:8] for c in clamps] == [[1, 1, 0, 256, -1.5, 1.5]] and not any(c[0] == "gtav_rng_normal" for c in sim.calls)


# ---- argument rules ---------------------------------------------------------------------------------------------------------------------------------
def test_step_argument_errors(tool, frames):
    rng = NoiseSource(1)
    with pytest.raises(ValueError, match="rng= makes the draws itself; noise must be None"):
        check_step_args(rng=rng, has_actions=False, action=None, noise=torch.zeros(1))
    with pytest.raises(TypeError, match="noise missing"):
        check_step_args(rng=None, has_actions=False, action=None, noise=None)
    with pytest.raises(ValueError, match="every step needs an action"):
        check_step_args(rng=rng, has_actions=True, action=None, noise=None)
    with pytest.raises(ValueError, match="action must be None"):
        check_step_args(rng=rng, has_actions=False, action=torch.zeros(1, 3), noise=None)
    check_step_args(rng=rng, has_actions=True, action=torch.zeros(1, 3), noise=None)
    check_step_args(rng=None, has_actions=False, action=None, noise=torch.zeros(1))
    xp, ap = _prompt(1, 2)
    with tool.stand_in():
        m = tool.dit(max_frames=3)
        with PlaySession(m, prompt_latents=xp, prompt_actions=ap, noise_steps=2, rng=NoiseSource(3), decode=None) as s:
            with pytest.raises(ValueError, match="every step needs an action"):
                s.step()
            with pytest.raises(ValueError, match="noise must be None"):
                s.step(ap[:, 0], noise=xp[:, 0])
            assert s.frame_index == 1 and not frames                   # a refused step leaves the session where it was
            s.step(ap[:, 0])
        with pytest.raises(RuntimeError, match="closed"):
            s.step(ap[:, 0])
        with PlaySession(m, prompt_latents=xp, noise_steps=2, decode=None) as s:
            with pytest.raises(TypeError, match="noise missing"):
                s.step()
            with pytest.raises(ValueError, match="action must be None"):
                s.step(ap[:, 0], noise=xp[:, 0])


def test_session_argument_errors(tool):
    ok = dict(n_latents=2, n_frames=None, has_vae=False, has_prompt_actions=True, guidance_scale=None, decode=None)
    check_session_args(**ok)
    for change, text in [(dict(n_latents=None), "exactly one of prompt_latents and prompt_frames"),
                         (dict(n_frames=2), "exactly one of prompt_latents and prompt_frames"),
                         (dict(n_latents=0), "the prompt is empty"),
                         (dict(n_latents=None, n_frames=0, has_vae=True), "the prompt is empty"),
                         (dict(n_latents=None, n_frames=2), "prompt_frames needs a vae"),
                         (dict(decode="sync"), "decode='sync' needs a vae"),
                         (dict(decode="overlap", has_vae=True), "one of 'sync', None; a decode on a second stream was measured slower"),
                         (dict(decode="async", has_vae=True), "one of 'sync', None"),
                         (dict(guidance_scale=2.0, has_prompt_actions=False), "guidance_scale needs actions")]:
        with pytest.raises(ValueError, match=text):
            check_session_args(**dict(ok, **change))
    xp, ap = _prompt(1, 2)
    with tool.stand_in() as sim:
        m = tool.dit(max_frames=3, max_batch=2)
        for kw, text in [(dict(prompt_latents=xp), "decode='sync' needs a vae"),                     # decode defaults to "sync"
                         (dict(prompt_latents=xp, decode=None, guidance_scale=3.0), "guidance_scale needs actions"),
                         (dict(prompt_latents=xp[:, :0], decode=None), "the prompt is empty"),
                         (dict(decode=None), "exactly one of prompt_latents and prompt_frames"),
                         (dict(prompt_latents=xp, prompt_actions=ap[:, :1], decode=None), "prompt_actions")]:
            with pytest.raises(ValueError, match=text):
                PlaySession(m, noise_steps=2, rng=NoiseSource(1), **kw)
        assert m._guidance is None and not sim.calls                   # a refused session has touched neither the model nor the library
        # guidance: set for the session's life, the model's own setting back at close()
        m.set_guidance(1.5)
        with PlaySession(m, prompt_latents=xp, prompt_actions=ap, noise_steps=2, rng=NoiseSource(1), decode=None, guidance_scale=3.0):
            assert m._guidance == 3.0
        assert m._guidance == 1.5
        small = tool.dit(max_frames=3, max_batch=1)
        with pytest.raises(ValueError, match="2 B = 2 internal samples"):
            PlaySession(small, prompt_latents=xp, prompt_actions=ap, noise_steps=2, rng=NoiseSource(1), decode=None, guidance_scale=3.0)
        assert small._guidance is None
