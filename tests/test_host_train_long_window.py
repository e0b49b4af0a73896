"""CPU: the opt-in to training windows of 9 .. 32 frames (DiT(train_max_frames=n), gtav_dit_train_allow_window) — what needs no GPU: the constructor's
validation before any handle exists, the Python mirror's constants, and the C-ABI's new symbols."""
import os
import re

import pytest

SMALL_DIT = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gtav_dit_train_allow_window", "gtav_op_attn_temporal_bwd", "gtav_op_attn_temporal_bwd_bf16")


def test_constructor_validates_train_max_frames_without_a_handle():
    from gtav_amd.model.dit import DiT
    with pytest.raises(ValueError, match="32"):
        DiT(**SMALL_DIT, init_weights=False, trainable=True, train_max_frames=33)
    with pytest.raises(ValueError, match="8 to 32"):
        DiT(**SMALL_DIT, init_weights=False, trainable=True, train_max_frames=7)
    with pytest.raises(ValueError, match="trainable=True"):
        DiT(**SMALL_DIT, init_weights=False, train_max_frames=16)


def test_python_mirror_keeps_the_default_window_and_the_reference_attribute():
    from gtav_amd.model.dit import DiT, MAX_FRAMES, TRAIN_MAX_FRAMES
    assert (MAX_FRAMES, TRAIN_MAX_FRAMES) == (32, 8)
    m = DiT(**SMALL_DIT, init_weights=False, max_frames=12, trainable=True, train_max_frames=16)
    assert m.max_frames == 12 and not m._handle
    m.max_frames = 32                      # the attribute follows the caller; the handle will be sized for min(max_frames, train_max_frames)
    assert m.max_frames == 32 and m._capacity_t == 16
    # no opt-in: today's cap and today's refusal
    d = DiT(**SMALL_DIT, init_weights=False, max_frames=12, trainable=True)
    assert d.max_frames == 12 and d._capacity_t == 8
    import torch
    with pytest.raises(ValueError, match="8 frames"):
        d.forward_train(torch.zeros(1, 12, 16, 8, 16), torch.zeros(1, 12, dtype=torch.long))
    # opted in: a window above train_max_frames is refused by name before a handle exists
    with pytest.raises(ValueError, match="train_max_frames=16"):
        m.forward_train(torch.zeros(1, 17, 16, 8, 16), torch.zeros(1, 17, dtype=torch.long))
    assert not m._handle


def test_cabi_declares_and_exports_the_new_symbols():
    from gtav_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "gtav_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gtav_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.gtav_abi_version() == 4
    # argument validation that touches no device
    assert lib.gtav_dit_train_allow_window(None, 16) != 0 and b"null handle" in lib.gtav_last_error()
    assert lib.gtav_op_attn_temporal_bwd(None, None, None, 1, 8, 256, 9, 9, None, None, None) != 0 and b"null argument" in lib.gtav_last_error()
