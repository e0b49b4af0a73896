"""The DiT training step on frames of more than 160 tokens, and on token counts that are a multiple of 8 but not of 16 (the spatial attention backward
streams such frames: csrc/train.hip attn_spatial_bwd_stream_kernel), against torch autograd on the CPU oracle, for fp16 and bf16 training handles.

Bounds are those of tests/train_cases.py (FWD_TOL for the forward, GRAD_TOL relative L2 per gradient tensor, for fp16 and for bf16 operands).  Every gradient
tensor is compared; `pytest -s` prints every measured margin."""
import math

import pytest
import torch

import train_cases as TC
from helpers import rel_l2_logged as rel_l2       # (-s shows the measured margins)
from train_cases import DTYPES, FWD_TOL, GRAD_TOL

pytestmark = pytest.mark.gpu

GEOMETRIES = [(24, 48), (36, 64), (20, 40)]          # 288, 576 and 200 tokens per frame (200 = 12.5 tiles of 16)


def _kw(h, w, **over):
    return dict(TC.TOY_KW, input_h=h, input_w=w, **over)


def _compare(kw, dtype, actions, sd_seed=1):
    sd, inp, _, v_ref, grads = TC.oracle(kw, 2, 3, actions, sd_seed)
    m = TC.model(kw, 2, 3, dtype, sd)
    v = TC.forward_backward(m, inp)
    assert rel_l2(v, v_ref) < FWD_TOL[dtype]
    worst = TC.grad_errors(m, grads, log=True)
    print(f"worst gradient error ({dtype}): {max(worst.values()):.3e} (bound {GRAD_TOL[dtype]:.1e})")
    bad = {k: e for k, e in worst.items() if e > GRAD_TOL[dtype]}
    assert not bad, f"gradient mismatch: {bad}"


@DTYPES
@pytest.mark.parametrize("actions", [True, False], ids=["actions", "noactions"])
@pytest.mark.parametrize("hw", GEOMETRIES, ids=["288tok", "576tok", "200tok"])
def test_gradients_match_autograd_on_long_frames(hw, actions, dtype):
    _compare(_kw(*hw), dtype, actions)


@DTYPES
def test_gradients_at_the_real_widths_576_tokens(dtype):
    """hidden 1024, 16 heads, depth 2, 36 x 64 latents (576 tokens per frame), B = 2, T = 3: D = 1024 and M = 3 456 tokens = 27 whole 128-token row tiles, the
    grouped weight-gradient launch."""
    _compare(_kw(36, 64, hidden_size=1024, num_heads=16), dtype, True, sd_seed=0)


def test_training_steps_reduce_the_loss_at_288_tokens():
    from gtav_amd.train import training_step
    kw = _kw(24, 48)
    m = TC.model(kw, 2, 5)
    lat, a, tgt, ctx, cn, nz = TC.clip(kw)
    losses = [float(training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)) for _ in range(3)]
    print("losses:", losses)
    m.check()
    assert all(math.isfinite(l) for l in losses)
    assert losses[-1] < losses[0], losses


def test_phased_backward_equals_monolithic_at_288_tokens():
    kw = _kw(24, 48)
    m = TC.model(kw, 2, 3)
    x, t, a, vt = TC.inputs(kw)
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    whole = m.grad_arena.clone()
    m.zero_grad()
    for phase in range(m.depth + 2):
        m.backward_phases_(v, vt, phase, phase + 1)
    assert rel_l2(m.grad_arena, whole) < 1e-6


def test_save_state_load_state_resumes_bit_exactly_at_288_tokens(tmp_path):
    """Three steps straight == two steps, save_state, a fresh model, load_state, one more step: weights equal bit for bit (the streaming attention backward is
    reproducible from launch to launch)."""
    from gtav_amd.model.dit import DiT
    from gtav_amd.train import load_state, save_state, training_step
    kw = _kw(24, 48)
    lat, a, tgt, ctx, cn, nz = TC.clip(kw)
    skw = dict(lr=3e-4, weight_decay=0.01, max_grad_norm=1.0)
    m1 = TC.model(kw, 2, 5)
    for _ in range(3):
        training_step(m1, lat, a, tgt, ctx, cn, nz, **skw)
    m1.pull_weights()
    straight = {k: v.clone() for k, v in m1._sd.items()}
    del m1
    m2 = TC.model(kw, 2, 5)
    for _ in range(2):
        training_step(m2, lat, a, tgt, ctx, cn, nz, **skw)
    ck = str(tmp_path / "train_checkpoints" / "dit_last")
    save_state(m2, ck, global_step=2, epoch=0)
    del m2
    m3 = DiT(**kw, max_batch=2, max_frames=5, init_weights=True, trainable=True)               # other weights until load_state
    st = load_state(m3, ck, steps_per_epoch=7, gradient_accumulation_steps=4)
    assert st["step"] == 2
    training_step(m3, lat, a, tgt, ctx, cn, nz, **skw)
    m3.pull_weights()
    for k in straight:
        assert torch.equal(m3._sd[k], straight[k]), k
    applied, skipped, _ = m3.train_stats()
    assert applied and skipped == 0
