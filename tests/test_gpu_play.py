"""gtav_amd.play.PlaySession on the GPU: frame k of a session is, bit for bit, generated frame k of the clip generate_latents makes from the same prompt,
actions and noise — over rollouts that wrap the ring twice — plus snapshot / restore, constant memory, the decode and range_policy="auto".

Both sides run generate.denoise_frame on the same windows: the session on the ring form of the sampler step (tests/test_gpu_ring_window.py), generate_latents
on the linear one; the noise of frame f is stream slot f of one draw on both.  Every comparison is torch.equal.  The toy model of
tests/test_gpu_geometry_models.py (32 tokens per frame), noise_steps = 3, synthetic weights."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import dev  # noqa: E402
import gtav_amd.weights as W  # noqa: E402
from gtav_amd.generate import generate_latents, vae_decode_frames  # noqa: E402
from gtav_amd.model.dit import DiT  # noqa: E402
from gtav_amd.model.vae import AutoencoderKL  # noqa: E402
from gtav_amd.play import PlaySession  # noqa: E402
from gtav_amd.rng import NoiseSource  # noqa: E402
from test_gpu_geometry_models import SMALL_VAE  # noqa: E402

TOY = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)
NOISE_STEPS, SEED, SAMPLE0 = 3, 0x5EED1234ABCD, 6


@functools.lru_cache(maxsize=None)
def _state_dict(input_w=16):
    return W.synth_state_dict(W.dit_param_shapes(**dict(TOY, input_w=input_w)), seed=7)


def _mk(F, max_batch, input_w=16, sd=None, **extra):
    m = DiT(**dict(TOY, input_w=input_w), max_frames=F, max_batch=max_batch, init_weights=False, **extra)
    m.load_state_dict(sd or _state_dict(input_w))
    return m


def _prompt(B, n_prompt, n_new, seed=3, input_w=16):
    """Prompt latents (B, n_prompt, ...), one-hot actions of the whole clip (B, n_prompt + n_new, 25) and explicit noise (B, n_new, ...), on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, n_prompt, 16, 8, input_w, generator=g) * 0.5
    total = n_prompt + n_new
    a = torch.zeros(B, total, 25)
    a[torch.arange(B)[:, None], torch.arange(total)[None], torch.randint(0, 25, (B, total), generator=g)] = 1
    return x, a, torch.randn(B, n_new, 16, 8, input_w, generator=g)


# (F, n_prompt as a function of F, B, ctx_cache, hoist_cond, actions, guidance, bf16, explicit noise)
CASES = {
    "F3_p1_B1": (3, lambda F: 1, 1, True, True, True, None, False, False),
    "F3_pFm1_B2": (3, lambda F: F - 1, 2, True, True, True, None, False, False),
    "F3_pFp2_B1": (3, lambda F: F + 2, 1, True, True, True, None, False, False),
    "F5_p1_B2": (5, lambda F: 1, 2, True, True, True, None, False, False),
    "F5_pFm1_B1": (5, lambda F: F - 1, 1, True, True, True, None, False, False),
    "F5_pFp2_B2": (5, lambda F: F + 2, 2, True, True, True, None, False, False),
    "F5_no_ctx_cache": (5, lambda F: 1, 1, False, True, True, None, False, False),
    "F5_no_hoist": (5, lambda F: F - 1, 2, True, False, True, None, False, False),
    "F3_neither": (3, lambda F: F + 2, 2, False, False, True, None, False, False),
    "F5_no_actions": (5, lambda F: 1, 2, True, True, False, None, False, False),
    "F3_no_actions_no_hoist": (3, lambda F: F - 1, 1, True, False, False, None, False, False),
    "F5_guided": (5, lambda F: F + 2, 2, True, True, True, 3.0, False, False),
    "F3_guided_no_hoist": (3, lambda F: 1, 1, True, False, True, 3.0, False, False),
    "F5_bf16": (5, lambda F: F - 1, 2, True, True, True, None, True, False),
    "F5_explicit_noise": (5, lambda F: 1, 2, True, True, True, None, False, True),
    "F3_explicit_noise_no_actions": (3, lambda F: F + 2, 1, False, True, False, None, False, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_session_frames_are_the_clip_generate_latents_makes(case):
    """Item 5.  n_new = 2 F + 1 generated frames: the ring wraps twice.  One session call per frame; the reference clip is generated once.  Fails on the commit
    before gtav_amd.play."""
    F, n_prompt, B, ctx_cache, hoist_cond, actions, scale, bf16, explicit = CASES[case]
    n_prompt, n_new = n_prompt(F), 2 * F + 1
    m = _mk(F, max_batch=2 * B if scale is not None else B)
    if bf16:
        m.set_operand_dtype(torch.bfloat16)
    x_prompt, a, nz = _prompt(B, n_prompt, n_new)
    act = a if actions else None
    kw = dict(ctx_cache=ctx_cache, hoist_cond=hoist_cond, guidance_scale=scale)
    noise = dict(noise_chunks=nz) if explicit else dict(rng=NoiseSource(SEED, SAMPLE0))
    ref = generate_latents(m, x_prompt, n_prompt + n_new, NOISE_STEPS, actions=act, **noise, **kw)
    assert torch.equal(ref[:, :n_prompt].cpu(), x_prompt) and torch.isfinite(ref).all()
    with PlaySession(m, prompt_latents=x_prompt, prompt_actions=a[:, :n_prompt] if actions else None, noise_steps=NOISE_STEPS,
                     rng=None if explicit else NoiseSource(SEED, SAMPLE0), decode=None, **kw) as s:
        assert s.frame_index == n_prompt - 1 and s.window().shape[1] == min(n_prompt, F - 1)
        assert (m._guidance is not None) == (scale is not None)
        for k in range(1, n_new + 1):
            f = n_prompt + k - 1
            out = s.step(action=a[:, f] if actions else None, noise=nz[:, k - 1] if explicit else None)
            assert s.frame_index == f
            assert torch.equal(out, ref[:, f]), f"generated frame {k} (absolute {f}, ring slot {f % F})"
            lo = max(0, f + 1 - F)
            assert torch.equal(s.window(), ref[:, lo:f + 1]), f"the window after frame {k}"
    assert m._guidance is None
    m.check()


def _session(F=3, B=2, seed=SEED, **kw):
    m = _mk(F, max_batch=B)
    x_prompt, a, _ = _prompt(B, 2, 64)
    return m, a, PlaySession(m, prompt_latents=x_prompt, prompt_actions=a[:, :2], noise_steps=NOISE_STEPS, rng=NoiseSource(seed, SAMPLE0), decode=None, **kw)


def test_snapshot_and_restore():
    """Item 6: after restore, two further steps reproduce the original continuation bit for bit (the ring has wrapped in between, so every slot was
    overwritten); a different action after restore gives a different frame."""
    F = 3
    m, a, s = _session(F)
    with s:
        for f in range(2, 4):
            s.step(a[:, f])
        snap = s.snapshot()
        ptrs = (s._x.data_ptr(), s._act.data_ptr())
        want = [s.step(a[:, f]) for f in range(4, 4 + F + 2)]
        s.restore(snap)
        assert s.frame_index == 3 and (s._x.data_ptr(), s._act.data_ptr()) == ptrs
        for j in range(2):
            assert torch.equal(s.step(a[:, 4 + j]), want[j])
        s.restore(snap)
        other = a[:, 4].roll(1, dims=-1)
        assert not torch.equal(other, a[:, 4])
        assert not torch.equal(s.step(other), want[0])
        assert torch.equal(snap["x"], s.snapshot()["x"]) is False      # (the snapshot is a copy: the session went on)
    m.check()


def test_steps_allocate_nothing_on_the_device():
    """Item 7: from the third step on, memory_allocated() and the two rings' addresses stay over 2 F more steps (the handle was sized and every step captured
    during the warm-up; the returned frame is dropped before the next reading)."""
    F = 3
    m, a, s = _session(F)
    with s:
        for f in range(2, 5):
            s.step(a[:, f])
        torch.cuda.synchronize()
        ptrs, handle = (s._x.data_ptr(), s._act.data_ptr()), m._handle.value
        base = torch.cuda.memory_allocated()
        for f in range(5, 5 + 2 * F):
            out = s.step(a[:, f])
            del out
            assert torch.cuda.memory_allocated() == base, f
            assert (s._x.data_ptr(), s._act.data_ptr()) == ptrs and m._handle.value == handle


@functools.lru_cache(maxsize=None)
def _vae():
    kw = dict(SMALL_VAE, latent_dim=16)
    v = AutoencoderKL(**kw, init_weights=False, max_frames_per_call=4)
    v.load_state_dict(W.synth_state_dict(W.vae_param_shapes(**kw), seed=5))
    return v


def test_decode_sync():
    """Item 8: SMALL_VAE on 64 x 96 frames with 16 latent channels feeding a DiT on 8 x 12 latents (24 tokens per frame).  The "sync" frame is
    vae_decode_frames of the same latent, uint8, over 2 F + 1 steps.  (decode="overlap" is not offered: the measurement the feature was conditional on came out
    against it, profiles/play/frame_time.txt; the refusal is in tests/test_host_play.py.)"""
    F, B = 3, 2
    v = _vae()
    m = _mk(F, max_batch=B, input_w=12)
    x_prompt, a, _ = _prompt(B, 2, 2 * F + 1, input_w=12)
    shown = []
    with PlaySession(m, v, prompt_latents=x_prompt, prompt_actions=a[:, :2], noise_steps=NOISE_STEPS, rng=NoiseSource(SEED, SAMPLE0), decode="sync") as s:
        for k in range(2 * F + 1):
            out = s.step(a[:, 2 + k])
            assert out.dtype == torch.uint8 and tuple(out.shape) == (B, 64, 96, 3)
            want = vae_decode_frames(s.window()[:, -1:], v)[:, 0]
            assert torch.equal(out, want), k
            shown.append(out.clone())
        s.check()
    assert not torch.equal(shown[0], shown[1])
    with pytest.raises(ValueError, match="measured slower"):
        PlaySession(m, v, prompt_latents=x_prompt, noise_steps=NOISE_STEPS, rng=NoiseSource(SEED), decode="overlap")
    # prompt_frames: the session encodes them with the same vae
    g = torch.Generator().manual_seed(1)
    pf = torch.rand(B, 2, 3, 64, 96, generator=g)
    from gtav_amd.generate import vae_encode
    lat = vae_encode(pf.to(dev()), v, 2)
    with PlaySession(m, v, prompt_frames=pf, noise_steps=NOISE_STEPS, rng=NoiseSource(SEED), decode=None) as s1, \
            PlaySession(m, prompt_latents=lat, noise_steps=NOISE_STEPS, rng=NoiseSource(SEED), decode=None) as s2:
        assert torch.equal(s1.window(), lat) and torch.equal(s1.step(), s2.step())


def test_range_policy_auto_redoes_the_saturated_frame_only():
    """Item 9, with the outlier state dict of tests/test_gpu_range.py (fc1 of block 0's spatial MLP x 3e5: fp16 stores saturate).  The first step saturates,
    the saturated operand groups move to bf16 and that frame is made again from its own noise; no later frame is redone, and every frame of the session
    equals the one of a session on a model whose switched groups were bf16 from the start."""
    from test_gpu_range import _outlier_case
    _, big, *_ = _outlier_case()
    F, B = 3, 1
    x_prompt, a, _ = _prompt(B, 2, 8)
    frames, switched = {}, None
    for policy in ("auto", "report"):
        m = _mk(F, max_batch=B, sd=big, range_policy=policy)
        if policy == "report":
            m.set_operand_dtype(torch.bfloat16, switched)
        checks = []
        real_check = m.check
        m.check = lambda: (checks.append(1), real_check())[1]
        with PlaySession(m, prompt_latents=x_prompt, prompt_actions=a[:, :2], noise_steps=NOISE_STEPS, rng=NoiseSource(SEED, SAMPLE0), decode=None) as s:
            frames[policy] = []
            for k in range(F + 2):
                before = len(checks)
                frames[policy].append(s.step(a[:, 2 + k]))
                assert torch.isfinite(frames[policy][-1]).all()
                groups = [g for g, d in enumerate(m.operand_dtypes()) if d == torch.bfloat16]
                if policy == "report":
                    assert len(checks) == 0                                     # "report": the session never synchronises for a check
                elif k == 0:
                    switched = groups
                    assert 0 in switched and len(checks) >= 2                   # the frame was made again (once per round of switches)
                else:
                    assert len(checks) - before == 1 and groups == switched, k   # no later frame is redone
        real_check()
    assert all(torch.equal(p, q) for p, q in zip(frames["auto"], frames["report"]))
