"""CPU: temporal windows of 9 .. 32 frames (DiT max_frames up to 32) — the oracle and the product's host tables against fixtures recorded from the
ACTUAL reference with `max_frames` up to 32 (tools/make_golden.py g12_long_window -> tests/golden/g12_long_window.safetensors,
g13_long_window_steps.safetensors), and the window limits that need no GPU.  Tolerances are tests/test_oracle_golden.py's: 2e-5 per forward / step,
1e-4 for a rollout of chained forwards (fp32 vs fp32; the oracle runs the same ATen kernels, most tensors are bit-equal)."""
import ctypes as C
import os

import pytest
import torch
from safetensors.torch import load_file

from oracle import ref_cpu as O
import gtav_amd.weights as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL_DIT = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)
TOL = 2e-5            # tests/test_oracle_golden.py TOL (G2, G4)
TOL_ROLLOUT = 1e-4    # tests/test_oracle_golden.py test_g5_rollout (33 chained fp32 forwards; here 40)
SEED = 21             # tools/make_golden.py g12_long_window


def rel(a, b):
    v = ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()
    print(f"[rel {os.environ.get('PYTEST_CURRENT_TEST', '').split('::')[-1].split(' ')[0]}] {v:.3e}")
    return v


def gold(name):
    return load_file(os.path.join(GOLD, name))


def _oracle():
    sd = W.synth_state_dict(W.dit_param_shapes(**SMALL_DIT), seed=SEED)
    cfg = O.DiTConfig(**SMALL_DIT)
    return sd, cfg, (lambda x, t, a: O.dit_forward(sd, cfg, x, t, a))


def test_g12_temporal_rope_table_of_32_positions():
    """The table the product uploads for a 32-frame handle equals the reference's angles' cos / sin bit for bit, as the T = 5 table does."""
    from gtav_amd.model.dit import _rope_tables_temporal
    ang = gold("g12_long_window.safetensors")["rope_temporal_angles_T32"]
    assert ang.shape == (32, 64)
    assert torch.equal(O.rope_angles_temporal(32, O.rope_freqs_lang(64)), ang)
    c, s = _rope_tables_temporal(W.rope_freqs_lang(64), 32)
    assert torch.equal(c, ang.cos()) and torch.equal(s, ang.sin())
    # a shorter table is a prefix of the longer one: positions do not depend on the handle's capacity
    c5, s5 = _rope_tables_temporal(W.rope_freqs_lang(64), 5)
    assert torch.equal(c5, c[:5]) and torch.equal(s5, s[:5])


def test_g12_oracle_forwards_of_32_and_12_frames():
    g = gold("g12_long_window.safetensors")
    sd, cfg, _ = _oracle()
    with torch.no_grad():
        assert rel(O.dit_forward(sd, cfg, g["x_b1t32"], g["t_b1t32"], g["a_b1t32"]), g["out_b1t32"]) < TOL
        assert rel(O.dit_forward(sd, cfg, g["x_b2t12"], g["t_b2t12"], None), g["out_b2t12"]) < TOL


def test_g13_oracle_denoise_step_on_a_16_frame_window():
    g = gold("g13_long_window_steps.safetensors")
    _, _, fn = _oracle()
    ac = O.alphas_cumprod_table(1e-4)[:, None, None, None]
    nr = torch.linspace(0, 999, 11)
    assert g["x"].shape[1] == 20
    with torch.no_grad():
        for idx in (4, 0):
            xp, vp = O.denoise_step(fn, g["x"], g["actions"], idx, 15, nr, ac, start_frame=4)
            assert vp.shape[1] == 16
            assert rel(vp, g[f"v_pred_{idx}"]) < TOL and rel(xp[:, -1:], g[f"x_pred_last_{idx}"]) < TOL


def test_g13_oracle_rollout_with_a_9_frame_window():
    """1 prompt frame -> 11 frames, 3 noise steps: 40 chained forwards on windows of 2 .. 9 frames, the last two after the window slid."""
    g = gold("g13_long_window_steps.safetensors")
    _, _, fn = _oracle()
    with torch.no_grad():
        out = O.generate_latents(fn, g["roll_x_prompt"], 11, 3, g["roll_noise"], g["roll_actions"], max_frames=9)
    assert out.shape == g["roll_latents"].shape
    assert rel(out, g["roll_latents"]) < TOL_ROLLOUT


def test_window_limits_of_the_python_mirror_need_no_gpu():
    """max_frames above 32 is refused by name before any handle exists; a trainable model keeps the reference's attribute but refuses a window above 8."""
    from gtav_amd.model.dit import DiT, MAX_FRAMES, TRAIN_MAX_FRAMES
    assert (MAX_FRAMES, TRAIN_MAX_FRAMES) == (32, 8)
    for n in (9, 16, 32):
        assert DiT(**SMALL_DIT, init_weights=False, max_frames=n).max_frames == n
    with pytest.raises(ValueError, match="32"):
        DiT(**SMALL_DIT, init_weights=False, max_frames=33)
    m = DiT(**SMALL_DIT, init_weights=False)
    m.max_frames = 32
    assert m.max_frames == 32
    with pytest.raises(ValueError, match="32"):
        m.max_frames = 33
    assert m.max_frames == 32                       # unchanged by the refused assignment
    with pytest.raises(ValueError, match="32"):
        m(torch.zeros(1, 33, 16, 8, 16), torch.zeros(1, 33, dtype=torch.long))
    with pytest.raises(ValueError, match="32"):
        m.reserve(1, max_frames=40)
    tr = DiT(**SMALL_DIT, init_weights=False, max_frames=12, trainable=True)
    assert tr.max_frames == 12
    with pytest.raises(ValueError, match="8 frames"):
        tr.forward_train(torch.zeros(1, 12, 16, 8, 16), torch.zeros(1, 12, dtype=torch.long))


def test_library_create_range_names_32():
    """gtav_dit_create validates its configuration before it touches a device."""
    from gtav_amd import lib as L
    lib = L.load()
    h = C.c_void_p()
    cfg = L.DitConfig(max_frames=33, max_batch=1, max_cond_rows=33, mlp_ratio=4.0, **SMALL_DIT)
    assert lib.gtav_dit_create(C.byref(cfg), C.byref(h)) != 0
    msg = lib.gtav_last_error().decode()
    assert "max_frames=33" in msg and "[1, 32]" in msg
    assert not h.value
