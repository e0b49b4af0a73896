"""bf16 training (DiT(trainable=True, train_dtype=torch.bfloat16)): the interface checks that need no GPU — constructor arguments, the operand-type rules of a
trainable model before its handle exists, the C-ABI's argument validation and the operand type a checkpoint records."""
import pytest
import torch

from gtav_amd import lib as L

KW = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)


def test_train_dtype_argument():
    from gtav_amd.model.dit import DiT, DiT_models
    m = DiT(**KW, init_weights=False, trainable=True, train_dtype=torch.bfloat16)
    assert m.train_dtype == torch.bfloat16 and m.loss_scale == 1.0
    assert m.operand_dtypes() == [torch.bfloat16] * m.n_operand_groups
    f = DiT(**KW, init_weights=False, trainable=True)
    assert f.train_dtype == torch.float16 and f.loss_scale == 65536.0
    assert f.operand_dtypes() == [torch.float16] * f.n_operand_groups
    assert DiT_models["DiT-S/2"](init_weights=False, trainable=True, train_dtype=torch.bfloat16).train_dtype == torch.bfloat16
    with pytest.raises(ValueError):
        DiT(**KW, init_weights=False, train_dtype=torch.bfloat16)         # inference models pick their type with set_operand_dtype
    with pytest.raises(ValueError):
        DiT(**KW, init_weights=False, trainable=True, train_dtype=torch.float32)


def test_operand_type_rules_of_trainable_models():
    from gtav_amd.model.dit import DiT
    m = DiT(**KW, init_weights=False, trainable=True, train_dtype=torch.bfloat16)
    m.set_operand_dtype(torch.bfloat16)                                   # nothing to do
    with pytest.raises(L.GtavError, match="bf16 operands"):
        m.set_operand_dtype(torch.float16)
    assert m.operand_dtypes() == [torch.bfloat16] * m.n_operand_groups
    f = DiT(**KW, init_weights=False, trainable=True)
    with pytest.raises(L.GtavError, match="fp16 operands"):
        f.set_operand_dtype(torch.bfloat16)


def test_train_enable_typed_rejects_bad_arguments():
    lib = L.load()
    assert lib.gtav_dit_train_enable_typed(None, None, 0, 1) != 0
    assert b"null handle" in lib.gtav_last_error()


def test_checkpoint_operand_type_name():
    from gtav_amd.model.dit import DiT
    from gtav_amd.train import _operand_dtype_name
    assert _operand_dtype_name(DiT(**KW, init_weights=False, trainable=True, train_dtype=torch.bfloat16)) == "bf16"
    assert _operand_dtype_name(DiT(**KW, init_weights=False, trainable=True)) == "fp16"
