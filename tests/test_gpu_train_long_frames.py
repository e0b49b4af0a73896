"""The DiT training step on frames of more than 160 tokens, and on token counts that are a multiple of 8 but not of 16 (the spatial attention backward
streams such frames: csrc/train.hip attn_spatial_bwd_stream_kernel), against torch autograd on the CPU oracle, for fp16 and bf16 training handles.

Bounds are those of tests/test_gpu_train.py (fp16: forward 2e-3, gradients 4.5e-3 relative L2 per tensor) and tests/test_gpu_train_bf16.py (bf16: forward
1.5e-2, gradients 8 x the fp16 bound).  Every gradient tensor is compared; `pytest -s` prints every measured margin."""
import math
import os

import pytest
import torch

from helpers import rel_l2 as _rel_l2

pytestmark = pytest.mark.gpu

TOL_FWD = {torch.float16: 2e-3, torch.bfloat16: 1.5e-2}
GRAD_TOL = {torch.float16: 4.5e-3, torch.bfloat16: 8 * 4.5e-3}

KW = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)   # tests/test_gpu_train.py KW
GEOMETRIES = [(24, 48), (36, 64), (20, 40)]          # 288, 576 and 200 tokens per frame (200 = 12.5 tiles of 16)
DTYPES = [torch.float16, torch.bfloat16]


def rel_l2(a, b):
    v = _rel_l2(a, b)
    print(f"[rel_l2 {os.environ.get('PYTEST_CURRENT_TEST', '').split('::')[-1].split(' ')[0]}] {v:.3e}")   # (-s shows the measured margins)
    return v


def _kw(h, w, **over):
    kw = dict(KW, input_h=h, input_w=w)
    kw.update(over)
    return kw


def _inputs(h, w, B=2, T=3, actions=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, 16, h, w, generator=g)
    t = torch.randint(0, 1000, (B, T), generator=g)
    a = None
    if actions:
        a = torch.zeros(B, T, 25)
        a[:, :, 3] = 1
        a[0, T - 1, 7] = 1
    vt = torch.randn(B, 1, 16, h, w, generator=g)
    return x, t, a, vt


def _model(kw, sd, B, T, dtype):
    from gtav_amd.model.dit import DiT
    m = DiT(**kw, max_batch=B, max_frames=T, init_weights=False, trainable=True, train_dtype=dtype)
    m.load_state_dict(sd)
    return m


_ORACLE = {}


def _oracle(kw, sd_seed, h, w, B, T, actions):
    """(state dict, inputs, oracle loss / v / gradients) of one case: computed once, shared by the fp16 and the bf16 test, never modified."""
    key = (tuple(sorted(kw.items())), sd_seed, B, T, actions)
    if key not in _ORACLE:
        import gtav_amd.weights as W
        from oracle import ref_cpu as O
        sd = W.synth_state_dict(W.dit_param_shapes(**kw), seed=sd_seed)
        x, t, a, vt = _inputs(h, w, B, T, actions)
        torch.set_num_threads(16)
        _, v_ref, grads = O.dit_loss_and_grads(sd, O.DiTConfig(**kw), x, t, a, vt)
        assert all(torch.isfinite(g).all() for g in grads.values())
        _ORACLE[key] = (sd, (x, t, a, vt), v_ref, grads)
    return _ORACLE[key]


def _compare(m, dtype, x, t, a, vt, v_ref, grads):
    v = m.forward_train(x, t, a)
    assert rel_l2(v, v_ref) < TOL_FWD[dtype]
    m.zero_grad()
    m.backward_(v, vt)
    m.check()
    worst = {}
    for k, gref in grads.items():
        g = m.grad(k).cpu()
        assert torch.isfinite(g).all(), k
        if gref.norm() == 0:
            assert g.abs().max() == 0, k                 # external_cond.* without actions: unused, gradient None upstream
            continue
        worst[k] = rel_l2(g, gref)
    print(f"worst gradient error ({dtype}): {max(worst.values()):.3e} (bound {GRAD_TOL[dtype]:.1e})")
    bad = {k: e for k, e in worst.items() if e > GRAD_TOL[dtype]}
    assert not bad, f"gradient mismatch: {bad}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("actions", [True, False], ids=["actions", "noactions"])
@pytest.mark.parametrize("hw", GEOMETRIES, ids=["288tok", "576tok", "200tok"])
def test_gradients_match_autograd_on_long_frames(hw, actions, dtype):
    h, w = hw
    kw = _kw(h, w)
    sd, (x, t, a, vt), v_ref, grads = _oracle(kw, 1, h, w, 2, 3, actions)
    _compare(_model(kw, sd, 2, 3, dtype), dtype, x, t, a, vt, v_ref, grads)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_gradients_at_the_real_widths_576_tokens(dtype):
    """hidden 1024, 16 heads, depth 2, 36 x 64 latents (576 tokens per frame), B = 2, T = 3: D = 1024 and M = 3 456 tokens = 27 whole 128-token row tiles, the
    grouped weight-gradient launch."""
    kw = _kw(36, 64, hidden_size=1024, num_heads=16)
    sd, (x, t, a, vt), v_ref, grads = _oracle(kw, 0, 36, 64, 2, 3, True)
    _compare(_model(kw, sd, 2, 3, dtype), dtype, x, t, a, vt, v_ref, grads)


def _step_inputs(h, w, B=2, seed=5):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B, 5, 16, h, w, generator=g) * 0.5
    a = torch.zeros(B, 5, 25)
    a[:, :, 3] = 1
    tgt, ctx = torch.tensor([30, 10][:B]), torch.tensor([5, 20][:B])
    cn = torch.randn(B, 4, 16, h, w, generator=g)
    nz = torch.randn(B, 1, 16, h, w, generator=g)
    return lat, a, tgt, ctx, cn, nz


def _fresh(kw, sd, **over):
    from gtav_amd.model.dit import DiT
    m = DiT(**kw, max_batch=2, max_frames=5, trainable=True, **dict(dict(init_weights=False), **over))
    if not over.get("init_weights"):
        m.load_state_dict(sd)
    return m


def test_training_steps_reduce_the_loss_at_288_tokens():
    import gtav_amd.weights as W
    from gtav_amd.train import training_step
    kw = _kw(24, 48)
    m = _fresh(kw, W.synth_state_dict(W.dit_param_shapes(**kw), seed=1))
    lat, a, tgt, ctx, cn, nz = _step_inputs(24, 48)
    losses = [float(training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)) for _ in range(3)]
    print("losses:", losses)
    m.check()
    assert all(math.isfinite(l) for l in losses)
    assert losses[-1] < losses[0], losses


def test_phased_backward_equals_monolithic_at_288_tokens():
    import gtav_amd.weights as W
    kw = _kw(24, 48)
    m = _model(kw, W.synth_state_dict(W.dit_param_shapes(**kw), seed=1), 2, 3, torch.float16)
    x, t, a, vt = _inputs(24, 48)
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
    import gtav_amd.weights as W
    from gtav_amd.train import load_state, save_state, training_step
    kw = _kw(24, 48)
    sd = W.synth_state_dict(W.dit_param_shapes(**kw), seed=1)
    lat, a, tgt, ctx, cn, nz = _step_inputs(24, 48)
    skw = dict(lr=3e-4, weight_decay=0.01, max_grad_norm=1.0)
    m1 = _fresh(kw, sd)
    for _ in range(3):
        training_step(m1, lat, a, tgt, ctx, cn, nz, **skw)
    m1.pull_weights()
    straight = {k: v.clone() for k, v in m1._sd.items()}
    del m1
    m2 = _fresh(kw, sd)
    for _ in range(2):
        training_step(m2, lat, a, tgt, ctx, cn, nz, **skw)
    ck = str(tmp_path / "train_checkpoints" / "dit_last")
    save_state(m2, ck, global_step=2, epoch=0)
    del m2
    m3 = _fresh(kw, sd, init_weights=True)               # other weights until load_state
    st = load_state(m3, ck, steps_per_epoch=7, gradient_accumulation_steps=4)
    assert st["step"] == 2
    training_step(m3, lat, a, tgt, ctx, cn, nz, **skw)
    m3.pull_weights()
    for k in straight:
        assert torch.equal(m3._sd[k], straight[k]), k
    applied, skipped, _ = m3.train_stats()
    assert applied and skipped == 0
