"""The ring window of the fused sampler step (include/gtav_amd.h: 0 <= cur < start < F), through DiT.prepare_frame_ / DiT.denoise_step_.

A ring step on a buffer rolled by r frames reads the same frames, action rows and conditioning rows in the same order as the linear step on the buffer as
it was, launches the same kernels on them and differs only in the frame indices step_setup_kernel and the two conditioning-input kernels compute: every
comparison here is torch.equal.  The toy model of tests/test_gpu_geometry_models.py (hidden 256, depth 2, 4 heads, 25 actions, 8 x 16 latents, patch 2,
16 channels: 32 tokens per frame), synthetic weights."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import dev  # noqa: E402
import gtav_amd.weights as W  # noqa: E402
from gtav_amd import lib as L  # noqa: E402
from gtav_amd.lib import GtavError  # noqa: E402
from gtav_amd.model.dit import DiT  # noqa: E402
from gtav_amd.utils import alphas_cumprod  # noqa: E402

TOY = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)
T_CTX, TS = 15, [999, 666, 333]          # timesteps of the context frames and of two successive steps of frame `cur` (noise_steps = 3)


@functools.lru_cache(maxsize=None)
def _state_dict():
    return W.synth_state_dict(W.dit_param_shapes(**TOY), seed=7)


def _mk(max_frames, max_batch=4):
    m = DiT(**TOY, max_frames=max_frames, max_batch=max_batch, init_weights=False)
    m.load_state_dict(_state_dict())
    m.set_schedule(alphas_cumprod(1e-4))
    return m


@functools.lru_cache(maxsize=None)
def _model5():
    """Windows of up to 5 frames, max_batch 4 (a guided step of batch 2), sized once for the largest table of these tests (set_graph is not a recorded
    setting: a handle rebuilt by growth would come back with graphs on).  Every test leaves it unguided, with graphs on."""
    m = _mk(5)
    m.reserve(4, 5, noise_steps=len(TS) - 1)
    return m


@functools.lru_cache(maxsize=None)
def _inputs(B, F, seed=5):
    g = torch.Generator().manual_seed(seed + 100 * B + F)
    x = torch.randn(B, F, 16, 8, 16, generator=g) * 0.7
    a = torch.zeros(B, F, 25)
    a[torch.arange(B)[:, None], torch.arange(F)[None], torch.randint(0, 25, (B, F), generator=g)] = 1
    return x.to(dev()), a.to(dev())


class _Buffers:
    """One latent buffer, one action buffer and one v_out per side, allocated once: the captured steps are keyed by these pointers, so every rotation of one
    (B, F) replays the graphs the first one captured."""

    def __init__(self, B, F):
        self.x = torch.empty(B, F, 16, 8, 16, device=dev())
        self.a = torch.empty(B, F, 25, device=dev())
        self.v = torch.empty(B, 16, 8, 16, device=dev())


def _two_steps(m, buf, x0, a0, start, cur, *, prepared, actions, reps):
    """A full-window step and then a context-cached step of frame `cur` on buf.x <- x0, `reps` times over (with graphs on, the third time replays both
    captured steps).  Returns (x after mode 0, v_out of mode 0, x after mode 1, v_out of mode 1) and asserts that every repetition gave the same bits."""
    B, F = x0.shape[:2]
    buf.a.copy_(a0)
    act = buf.a if actions else None
    outs = []
    for _ in range(reps):
        buf.x.copy_(x0)
        buf.v.fill_(float("nan"))
        if prepared:
            m.prepare_frame_(B, F, start, cur, T_CTX, TS, act)
        m.denoise_step_(buf.x, start, cur, T_CTX, TS[0], TS[1], False, act, cached=False, v_out=buf.v, cond_step=0 if prepared else -1)
        x_a, v_a = buf.x.clone(), buf.v.clone()
        m.denoise_step_(buf.x, start, cur, T_CTX, TS[1], TS[2], False, act, cached=True, v_out=buf.v, cond_step=1 if prepared else -1)
        outs.append((x_a, v_a, buf.x.clone(), buf.v.clone()))
    for o in outs[1:]:
        assert all(torch.equal(p, q) for p, q in zip(o, outs[0])), "eager, captured and replayed steps differ"
    assert all(torch.isfinite(t).all() for t in outs[0])
    return outs[0]


def _assert_rotation(lin, ring, x0, r, lin_cur, ring_cur):
    """lin / ring: _two_steps' results on x0 and on roll(x0, r, dim=1)."""
    x0r = torch.roll(x0, r, dims=1)
    for k in (0, 2):                                        # x after the mode-0 step, x after the mode-1 step
        assert torch.equal(ring[k][:, ring_cur], lin[k][:, lin_cur]), ("frame cur", k)
        assert torch.equal(ring[k + 1], lin[k + 1]), ("v_out", k)
        keep_r = [f for f in range(x0.shape[1]) if f != ring_cur]
        keep_l = [f for f in range(x0.shape[1]) if f != lin_cur]
        assert torch.equal(ring[k][:, keep_r], x0r[:, keep_r]) and torch.equal(lin[k][:, keep_l], x0[:, keep_l]), ("another frame changed", k)
    assert not torch.equal(lin[0][:, lin_cur], x0[:, lin_cur]) and not torch.equal(lin[2][:, lin_cur], lin[0][:, lin_cur])     # (both steps did step)


VARIANTS = [("actions", True, None), ("no actions", False, None), ("guided", True, 3.0)]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("F", [2, 3, 5])
def test_a_ring_step_on_the_rolled_buffer_is_the_linear_step(F, B, graph):
    """Item 1: every rotation r of a full window, inline and prepared conditioning, mode 0 and mode 0 + mode 1, with actions, without, and guided (s = 3 over
    2 B internal samples); eager, or captured (each key is called three times: eager, capture, replay — and the later rotations replay the first one's graphs
    with other (start, cur) in StepParams).  This test fails on the commit before the ring window, which refuses start > cur."""
    m = _model5()
    handle = m._handle.value
    x0, a0 = _inputs(B, F)
    lin_buf, ring_buf = _Buffers(B, F), _Buffers(B, F)
    try:
        m.set_graph(graph)
        for name, actions, scale in VARIANTS:
            m.set_guidance(scale)
            for prepared in (False, True):
                kw = dict(prepared=prepared, actions=actions, reps=3 if graph else 1)
                lin = _two_steps(m, lin_buf, x0, a0, 0, F - 1, **kw)
                for r in range(1, F):
                    ring = _two_steps(m, ring_buf, torch.roll(x0, r, dims=1), torch.roll(a0, r, dims=1), r, (r - 1) % F, **kw)
                    _assert_rotation(lin, ring, x0, r, F - 1, (r - 1) % F)
        m.set_guidance(None)
        m.check()
        assert m._handle.value == handle                    # (no growth in between: `graph` held for every step above)
    finally:
        m.set_guidance(None)
        m.set_graph(True)
    if F == 5 and B == 1:                                   # actions matter to the result: the rotation of the action ring is really under test
        with_a = _two_steps(m, lin_buf, x0, a0, 0, F - 1, prepared=False, actions=True, reps=1)
        without = _two_steps(m, lin_buf, x0, a0, 0, F - 1, prepared=False, actions=False, reps=1)
        other = _two_steps(m, lin_buf, x0, torch.roll(a0, 1, dims=1), 0, F - 1, prepared=False, actions=True, reps=1)
        assert not torch.equal(with_a[1], without[1]) and not torch.equal(with_a[1], other[1])


def test_a_wrapped_window_of_nine_frames_runs_the_streaming_temporal_kernel():
    """Item 1, F = 9, B = 1: more than 8 visible frames, so the streaming temporal attention runs on a wrapped window."""
    F, r = 9, 4
    m = _mk(9, max_batch=1)
    x0, a0 = _inputs(1, F)
    lin_buf, ring_buf = _Buffers(1, F), _Buffers(1, F)
    for prepared in (False, True):
        lin = _two_steps(m, lin_buf, x0, a0, 0, F - 1, prepared=prepared, actions=True, reps=3)
        ring = _two_steps(m, ring_buf, torch.roll(x0, r, dims=1), torch.roll(a0, r, dims=1), r, r - 1, prepared=prepared, actions=True, reps=3)
        _assert_rotation(lin, ring, x0, r, F - 1, r - 1)
    m.check()


@pytest.mark.parametrize("F,start,cur,T", [(5, 4, 1, 3), (7, 5, 2, 5)], ids=["F5_T3", "F7_beyond_max_frames_T5"])
@pytest.mark.parametrize("B", [1, 2])
def test_a_partial_wrapped_window(F, start, cur, T, B):
    """Item 2: a wrapped window shorter than the buffer, also in a buffer of more frames than max_frames = 5, against the linear window [0, T - 1] of the
    buffer rolled so that frame `start` comes first.  The frames outside the window hold other values on the two sides and must not matter."""
    m = _model5()
    x0, a0 = _inputs(B, F, seed=9)                          # the ring side
    r = F - start                                           # ring slot f is linear frame (f + r) % F
    xl, al = torch.roll(x0, r, dims=1).clone(), torch.roll(a0, r, dims=1).clone()
    xl[:, T:] = 3.0                                         # outside the linear window [0, T - 1]
    al[:, T:] = 0.5
    lin_buf, ring_buf = _Buffers(B, F), _Buffers(B, F)
    for prepared in (False, True):
        lin = _two_steps(m, lin_buf, xl, al, 0, T - 1, prepared=prepared, actions=True, reps=3)
        ring = _two_steps(m, ring_buf, x0, a0, start, cur, prepared=prepared, actions=True, reps=3)
        for k in (0, 2):
            assert torch.equal(ring[k][:, cur], lin[k][:, T - 1]) and torch.equal(ring[k + 1], lin[k + 1])
            keep = [f for f in range(F) if f != cur]
            assert torch.equal(ring[k][:, keep], x0[:, keep])
    m.check()


def test_refusals():
    """Item 3: windows outside 0 <= start, cur < F, a wrapped window longer than max_frames, and a mode-1 / cond_step >= 0 step whose (start, cur) is not the
    recorded one, ring or not."""
    m = _mk(5, max_batch=1)
    F = 7
    x0, a0 = _inputs(1, F)
    x, a = x0.clone(), a0.clone()
    step = lambda start, cur, **kw: m.denoise_step_(x, start, cur, T_CTX, TS[0], TS[1], False, a, **kw)
    prep = lambda start, cur: m.prepare_frame_(1, F, start, cur, T_CTX, TS, a)
    step(0, 2)                                              # (the handle exists from here on)
    for start, cur in [(F, 0), (F + 3, 2), (-1, 2), (-2, -1), (2, -1), (5, F), (6, F)]:
        with pytest.raises(GtavError, match="denoise_step: bad window"):
            step(start, cur)
        with pytest.raises(GtavError, match="prepare_frame: bad window"):
            prep(start, cur)
    # a wrapped window of 6 frames on a handle of max_frames 5.  (DiT's methods grow the handle for an inline step or a prepare_frame_ of a longer window, as they
    # do for a linear one: the C calls are made directly where they would.)
    prep(5, 2)
    with pytest.raises(GtavError, match="denoise_step: bad window"):
        step(4, 2, cond_step=0)
    h, h_was = m._handle, m._handle.value
    ts = (ctypes.c_int32 * 3)(*TS)
    with torch.cuda.device(dev()):
        assert L.load().gtav_dit_prepare_frame(h, 1, F, 4, 2, T_CTX, ts, 3, a.data_ptr(), L.current_stream()) != 0
        assert "prepare_frame: bad window" in L.load().gtav_last_error().decode()
        assert L.load().gtav_dit_denoise_step(h, x.data_ptr(), 1, F, 4, 2, T_CTX, TS[0], TS[1], 0, a.data_ptr(), 0, -1, 0, L.current_stream()) != 0
        assert "denoise_step: bad window" in L.load().gtav_last_error().decode()
        assert L.load().gtav_dit_denoise_step(h, x.data_ptr(), 1, F, 5, 2, T_CTX, TS[0], TS[1], 0, a.data_ptr(), 0, -1, 0, L.current_stream()) == 0   # T = 5
    assert m._handle.value == h_was                         # (nothing above rebuilt the handle)
    # mode 1 needs the full-window step of the same (start, cur)
    step(5, 2)
    step(5, 2, cached=True)
    for start, cur in [(6, 3), (5, 1), (0, 2), (2, 5)]:
        with pytest.raises(GtavError, match="without a preceding full-window step.*stale"):
            step(start, cur, cached=True)
    step(1, 5)
    with pytest.raises(GtavError, match="without a preceding full-window step.*stale"):
        step(5, 2, cached=True)
    # cond_step >= 0 needs prepare_frame on the same (start, cur)
    prep(5, 2)
    step(5, 2, cond_step=0)
    for start, cur in [(6, 3), (5, 1), (0, 2)]:
        with pytest.raises(GtavError, match="gtav_dit_prepare_frame was not called for this window"):
            step(start, cur, cond_step=0)
    prep(0, 2)
    with pytest.raises(GtavError, match="gtav_dit_prepare_frame was not called for this window"):
        step(5, 2, cond_step=0)
    m.check()
    assert torch.equal(x[:, [0, 1, 3, 4, 6]], x0[:, [0, 1, 3, 4, 6]])       # only frames 2 and 5 were ever `cur` of an accepted step


@pytest.mark.parametrize("B", [1, 2])
def test_a_linear_window_is_the_rotation_by_zero(B):
    """Item 4: start <= cur keeps its meaning — the step on window [0, F - 1] of a second buffer (other pointers: other captured steps) gives the bits of the
    first, and a linear window inside a longer buffer those of the same frames at the head of a shorter one."""
    F = 5
    m = _model5()
    x0, a0 = _inputs(B, F)
    one, two = _Buffers(B, F), _Buffers(B, F)
    for prepared in (False, True):
        a = _two_steps(m, one, x0, a0, 0, F - 1, prepared=prepared, actions=True, reps=3)
        b = _two_steps(m, two, x0, a0, 0, F - 1, prepared=prepared, actions=True, reps=3)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        x7, a7 = _inputs(B, 7)
        long_buf, short_buf = _Buffers(B, 7), _Buffers(B, 4)
        c = _two_steps(m, long_buf, x7, a7, 2, 5, prepared=prepared, actions=True, reps=1)
        d = _two_steps(m, short_buf, x7[:, 2:6].contiguous(), a7[:, 2:6].contiguous(), 0, 3, prepared=prepared, actions=True, reps=1)
        assert torch.equal(c[2][:, 5], d[2][:, 3]) and torch.equal(c[3], d[3]) and torch.equal(c[1], d[1])
    m.check()
