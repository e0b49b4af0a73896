"""CPU (no GPU): the opt-in activation recomputation of the DiT training step (DiT(trainable=True, train_recompute=True) ->
gtav_dit_train_set_recompute) at the Python and the C-ABI boundary: constructor rules, the read-only attribute, the two new symbols in the header and the
ctypes table, and argument validation before anything touches a device."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=3, num_heads=4, external_cond_dim=25, init_weights=False)


def test_constructor_rules():
    from gtav_amd.model.dit import DiT
    assert inspect.signature(DiT.__init__).parameters["train_recompute"].default is False
    assert inspect.signature(DiT.__init__).parameters["train_recompute"].kind is inspect.Parameter.KEYWORD_ONLY
    assert DiT(**KW).train_recompute is False
    assert DiT(**KW, trainable=True).train_recompute is False
    m = DiT(**KW, trainable=True, train_recompute=True)
    assert m.train_recompute is True
    with pytest.raises(ValueError, match="train_recompute=True needs trainable=True"):
        DiT(**KW, train_recompute=True)
    with pytest.raises(ValueError, match="train_recompute=True needs trainable=True"):
        DiT(**KW, trainable=False, train_recompute=True)
    with pytest.raises(AttributeError):
        m.train_recompute = False
    assert m.train_recompute is True


def test_recompute_combines_with_the_other_training_options():
    import torch
    from gtav_amd.model.dit import DiT
    m = DiT(**KW, max_frames=12, trainable=True, train_recompute=True, train_dtype=torch.bfloat16, train_max_frames=12)
    assert m.train_recompute and m.train_dtype == torch.bfloat16 and m._train_window == 12
    assert callable(m.train_saved_bytes)


def test_new_symbols_are_declared_bound_and_exported():
    import ctypes
    from gtav_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "gtav_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint gtav_dit_train_set_recompute\(gtav_dit\* h, int32_t enable\);", code)
    assert re.search(r"\bint gtav_dit_train_saved_bytes\(gtav_dit\* h, int64_t\* bytes\);", code)
    assert L.SIGNATURES["gtav_dit_train_set_recompute"] == [ctypes.c_void_p, ctypes.c_int32]
    assert L.SIGNATURES["gtav_dit_train_saved_bytes"] == [ctypes.c_void_p, ctypes.c_void_p]
    assert L.DECLARATIONS["gtav_dit_train_saved_bytes"] == ("int", [("gtav_dit*", "h"), ("int64_t*", "bytes")])     # the C types the binding was derived from
    dll = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(dll, "gtav_dit_train_set_recompute") and hasattr(dll, "gtav_dit_train_saved_bytes")
    assert L.load().gtav_abi_version() == 4          # new entry points, no changed signature


def test_argument_validation_without_gpu():
    import ctypes
    from gtav_amd import lib as L
    lib = L.load()
    assert lib.gtav_dit_train_set_recompute(None, 1) != 0
    assert b"train_set_recompute: null handle" in lib.gtav_last_error()
    n = ctypes.c_int64(-1)
    assert lib.gtav_dit_train_saved_bytes(None, ctypes.byref(n)) != 0
    assert b"train_saved_bytes: null argument" in lib.gtav_last_error() and n.value == -1


def test_the_statistics_shift_fields_are_part_of_the_pinned_struct():
    """LnPending is one text for both operand types (ops_typed.inc): the two fields the re-run's LayerNorm needs are declared there, and the size pin moved
    with them (13 x 8 bytes + 2 pointers)."""
    text = open(os.path.join(ROOT, "ai-generated-gtav_amd", "csrc", "ops_typed.inc")).read()
    body = text[text.index("struct LnPending {"):text.index("static_assert(sizeof(LnPending)")]
    assert re.search(r"\bfloat\* k_save;", body) and re.search(r"\bconst float\* k_load;", body)
    assert "static_assert(sizeof(LnPending) == 120," in text
