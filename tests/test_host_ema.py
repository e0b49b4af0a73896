"""Averaged weights (DiT(train_ema_decay=...), DESIGN.md 7 "Averaged weights"): everything that is decided before a GPU is touched — the constructor's rules, the
host mirror of the per-step decay, the four C-ABI symbols and their refusals by name."""
import ctypes
import os
import re

import numpy as np
import pytest

from gtav_amd import lib as L
from gtav_amd import train as TR
from gtav_amd.model.dit import DiT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25, init_weights=False)
SYMBOLS = ("gtav_dit_train_set_ema", "gtav_dit_get_ema", "gtav_dit_set_ema", "gtav_dit_train_swap_ema")


def test_constructor_rules():
    """Validated before any handle exists: the option needs trainable=True and a decay inside (0, 1); the decay is read-only afterwards."""
    with pytest.raises(ValueError, match="trainable=True"):
        DiT(**KW, train_ema_decay=0.9)
    for bad in (0.0, 1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match=r"\(0, 1\)"):
            DiT(**KW, trainable=True, train_ema_decay=bad)
    with pytest.raises(ValueError, match="train_ema_decay"):
        DiT(**KW, trainable=True, train_ema_warmup=True)
    m = DiT(**KW, trainable=True, train_ema_decay=0.9, train_ema_warmup=True)
    assert m.ema_decay == 0.9 and m.ema_warmup is True and not m._handle
    with pytest.raises(AttributeError):
        m.ema_decay = 0.5
    plain = DiT(**KW, trainable=True)
    assert plain.ema_decay is None
    for call in (plain.ema_state_dict, lambda: plain.load_ema_state_dict({}), lambda: plain.ema_weights().__enter__()):
        with pytest.raises(L.GtavError, match="no averaged weights"):
            call()


def test_ema_decay_at_hand_values():
    f32 = np.float32
    # without warm-up: the decay itself, rounded to float32 once
    for n in (1, 2, 1000):
        assert TR.ema_decay_at(n, 0.9) == float(f32(0.9))
    assert TR.ema_decay_at(1, 0.9) != 0.9                      # (0.9 is not a float32)
    # warm-up: (1 + n) / (10 + n) until it reaches the decay
    assert TR.ema_decay_at(1, 0.25, True) == float(f32(2) / f32(11))
    assert TR.ema_decay_at(2, 0.25, True) == 0.25              # 3 / 12 = the decay exactly
    assert TR.ema_decay_at(3, 0.25, True) == 0.25              # 4 / 13 > 0.25
    assert TR.ema_decay_at(1, 0.9999, True) == float(f32(2) / f32(11))
    assert TR.ema_decay_at(90, 0.9999, True) == float(f32(91) / f32(100))
    assert TR.ema_decay_at(89990, 0.9999, True) == float(min(f32(0.9999), f32(89991) / f32(90000)))   # equal in exact arithmetic: the smaller float32
    assert TR.ema_decay_at(10 ** 6, 0.9999, True) == float(f32(0.9999))
    # monotone, never above the decay
    seq = [TR.ema_decay_at(n, 0.999, True) for n in range(1, 20000, 7)]
    assert all(a <= b for a, b in zip(seq, seq[1:])) and max(seq) == float(f32(0.999))
    for bad in (0, -1, 1 << 24):
        with pytest.raises(ValueError, match="applied step"):
            TR.ema_decay_at(bad, 0.9)
    for bad in (0.0, 1.0, 1.5):
        with pytest.raises(ValueError, match=r"\(0, 1\)"):
            TR.ema_decay_at(1, bad)


def test_symbols_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gtav_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"^int {name}\(gtav_dit\* h[,)]", code, flags=re.M), f"{name}: not declared in gtav_amd.h"
        assert hasattr(dll, name), f"{name}: not exported"
        assert name in L.SIGNATURES, f"{name}: not bound in lib.SIGNATURES"
    assert L.SIGNATURES["gtav_dit_get_ema"] == L.SIGNATURES["gtav_dit_get_weight"] == L.SIGNATURES["gtav_dit_set_ema"]
    # additive: the version stays
    assert L.load().gtav_abi_version() == 4


def test_set_ema_refusals_without_a_gpu():
    """A bad decay and a null handle are refused by name before anything is touched."""
    lib = L.load()
    assert lib.gtav_dit_train_set_ema(None, 0.9, 0) != 0
    assert b"train_set_ema: null handle" in lib.gtav_last_error()
    for bad in (0.0, 1.0, 1.5, -0.5, float("nan")):
        assert lib.gtav_dit_train_set_ema(None, bad, 0) != 0
        err = lib.gtav_last_error()
        assert b"train_set_ema: decay=" in err and b"outside (0, 1)" in err, err
    assert lib.gtav_dit_train_swap_ema(None, None) != 0
    assert b"train_swap_ema" in lib.gtav_last_error()
    assert lib.gtav_dit_get_ema(None, b"x", None, 0, None) != 0
    assert b"get_ema" in lib.gtav_last_error()
    assert lib.gtav_dit_set_ema(None, b"x", None, 0, None) != 0
    assert b"set_ema" in lib.gtav_last_error()
