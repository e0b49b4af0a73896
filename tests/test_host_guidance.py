"""Classifier-free guidance without a GPU: the CPU control of the GPU test's bound, argument validation of the new entry point, and the exactness of the
three-operation combine at scale 1 (tests/guidance_cases.py holds the cases and the oracle)."""
import ctypes

import numpy as np
import pytest
import torch

import guidance_cases as G
from gtav_amd import lib as L
from gtav_amd.sampler import guided_combine


@pytest.mark.parametrize("noise_idx", (6,) + G.NOISE_IDX)
def test_guided_bound_cannot_hide_an_unguided_or_wrongly_scaled_step(noise_idx):
    """tests/test_gpu_guidance.py bounds rel_l2(v_out, v_g) by TOL_SMALL amp(s).  That bound only means something if a step that ignored the guidance (returned
    v_c) would miss it by far: TOL_SMALL amp(s) must stay below a tenth of |v_g(s) - v_c| / |v_g(s)| for s = 0 and s = 3.  Noise index 6 of 10 is t = 599
    (there, on frame `cur`: |v_c - v_u| / |v_c| = 0.45, amp(3) = 3.27, amp(0) = amp(1) = 1.00; over the four indices amp(3) is 3.27 .. 3.63 and the
    bound stays 60 to 200 times below the distance to v_c); the others are the GPU test's own."""
    v_c, v_u = G.oracle_branches(noise_idx)
    sep = ((v_c - v_u).double().norm() / v_c.double().norm()).item()
    print(f"[guidance noise_idx={noise_idx}] |v_c - v_u| / |v_c| = {sep:.3f}, amp(0) = {G.amp(v_c, v_u, 0.0):.3f}, amp(1) = {G.amp(v_c, v_u, 1.0):.3f}, "
          f"amp(3) = {G.amp(v_c, v_u, 3.0):.3f}")
    assert abs(G.amp(v_c, v_u, 1.0) - 1.0) < 1e-6 and abs(G.amp(v_c, v_u, 0.0) - 1.0) < 1e-6
    for s in (0.0, 3.0):
        v_g = G.combine(v_c, v_u, s)
        moved = ((v_g - v_c).double().norm() / v_g.double().norm()).item()
        print(f"[guidance noise_idx={noise_idx}] s = {s}: bound {G.TOL_SMALL * G.amp(v_c, v_u, s):.2e}, |v_g - v_c| / |v_g| = {moved:.3f}")
        assert G.TOL_SMALL * G.amp(v_c, v_u, s) < 0.1 * moved, (noise_idx, s)


def test_set_guidance_argument_validation_without_gpu():
    """The new entry point rejects a null handle before touching the device; the Python switch refuses a non-finite scale and a model without actions
    before a handle exists."""
    lib = L.load()
    assert lib.gtav_dit_set_guidance(None, 1, ctypes.c_float(3.0)) != 0
    assert b"dit_set_guidance: null handle" in lib.gtav_last_error()
    from gtav_amd.model.dit import DiT
    m = DiT(**G.SMALL_DIT, max_batch=2, init_weights=False)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="not finite"):
            m.set_guidance(bad)
    assert m._guidance is None
    m.set_guidance(2.5)
    assert m._guidance == 2.5 and m._internal_batch(1) == 2
    with pytest.raises(ValueError, match="max_batch=4"):       # the message names the value the model needs
        m._internal_batch(2)
    m.set_guidance(None)
    assert m._internal_batch(2) == 2
    kw = dict(G.SMALL_DIT, external_cond_dim=0)
    with pytest.raises(ValueError, match="no external_cond"):
        DiT(**kw, init_weights=False).set_guidance(2.0)
    from gtav_amd.generate import generate_latents
    with pytest.raises(ValueError, match="guidance_scale needs actions"):
        generate_latents(None, torch.zeros(1, 1, 16, 8, 16), 3, 2, torch.zeros(1, 2, 16, 8, 16), None, guidance_scale=2.0)


def test_train_forward_keep_argument_validation_and_the_host_draw():
    lib = L.load()
    assert lib.gtav_dit_train_forward_keep(None, None, None, None, None, None, 2, 3, None) != 0
    assert b"train_forward: null argument" in lib.gtav_last_error()
    from gtav_amd.train import draw_action_keep, forward_loss
    a, b = (draw_action_keep(64, 0.1, torch.Generator().manual_seed(5)) for _ in range(2))
    assert torch.equal(a, b) and a.dtype == torch.int32 and a.shape == (64,) and set(a.tolist()) <= {0, 1} and 0 < int(a.sum()) < 64
    assert int(draw_action_keep(8, 0.0).sum()) == 8 and int(draw_action_keep(8, 1.0).sum()) == 0
    with pytest.raises(ValueError, match="not a probability"):
        draw_action_keep(4, 1.5)
    with pytest.raises(ValueError, match="action_keep needs keep_activations=True"):
        forward_loss(None, torch.zeros(2, 5, 16, 8, 16), torch.zeros(2, 5, 25), action_keep=[1, 0])


def test_three_operation_combine_is_exact_at_scale_one():
    """d = v_c - v_u, m = (s - 1) d, v_g = v_c + m in numpy float32: s = 1 gives v_c bit for bit (m is a signed zero), s = 0 gives v_c - d, and the torch
    form the oracle uses agrees with the numpy form the product's mirror uses."""
    v_c, v_u = G.oracle_branches(4)
    c, u = v_c.numpy(), v_u.numpy()
    assert np.array_equal(guided_combine(c, u, 1.0), c)
    assert np.array_equal(guided_combine(c, u, 0.0), c + np.float32(-1.0) * (c - u))
    for s in G.SCALES + (1.5,):
        got = guided_combine(v_c, v_u, s)
        assert got.dtype == torch.float32 and torch.equal(got, G.combine(v_c, v_u, s))
        assert np.array_equal(guided_combine(c, u, s), got.numpy())
