"""The DiT training step on bf16 operands (DiT(trainable=True, train_dtype=torch.bfloat16), include/gtav_amd.h gtav_dit_train_enable_typed): the reference's
own `--mixed_precision bf16` (train_dit.py:190-198).  Forward, backward and the optimizer's operand rewrite run on the bf16 twins of the training kernels.

Tolerances: bf16 keeps 3 fewer mantissa bits than fp16, and all-bf16 forwards measure 5-7e-3 against the fp32 oracle where fp16 gives <= 1e-3
(tests/test_gpu_range.py).  The forward bound is that file's TOL_BF16 (1.5e-2); gradients are held to 8 x the fp16 GRAD_TOL (tests/train_cases.py),
3.6e-2 relative L2 per tensor.  `pytest -s` prints every measured margin."""
import json
import math
import os

import pytest
import torch

import train_cases as TC
from helpers import rel_l2 as _rel_l2
from helpers import rel_l2_logged as rel_l2       # (-s shows the measured margins)
from train_cases import BF16, F16
from train_cases import TOY_KW as KW

pytestmark = pytest.mark.gpu

TOL_FWD_BF16, GRAD_TOL_BF16 = TC.FWD_TOL[BF16], TC.GRAD_TOL[BF16]


def _model(sd, B, T, dtype=BF16, **kw):
    return TC.model(KW, B, T, dtype, sd, **kw)


def _inputs(B=2, T=3, actions=True, seed=0):
    return TC.inputs(KW, B, T, actions, seed)


def _grad_errors(m, grads, keys=None):
    return TC.grad_errors(m, grads, keys, log=True)


# ---- 1. toy DiT against the fp32 oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actions", [True, False])
def test_bf16_gradients_match_autograd(actions):
    sd, inp, _, v_ref, grads = TC.oracle(KW, 2, 3, actions)
    worst = {}
    for dtype in (F16, BF16):
        m = _model(sd, 2, 3, dtype)
        assert m.train_dtype == dtype
        v = TC.forward_backward(m, inp)
        assert rel_l2(v, v_ref) < TC.FWD_TOL[dtype]
        worst[dtype] = _grad_errors(m, grads)
        del m
    bad = {k: e for k, e in worst[BF16].items() if e > GRAD_TOL_BF16}
    assert not bad, f"bf16 gradient mismatch: {bad}"
    w16, wbf = max(worst[F16].values()), max(worst[BF16].values())
    print(f"worst gradient error: fp16 {w16:.3e}, bf16 {wbf:.3e} (bound {GRAD_TOL_BF16:.1e})")
    assert wbf > w16                                   # the bf16 mode really ran


# ---- 2. full-size DiT-S/2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(1, 5), (4, 4), (3, 5)])
def test_bf16_full_size_gradients(B, T):
    """DiT-S/2 at its real size: B = 1, T = 5 (M = 720: loader-wave GEMM, split-K residual GEMMs, 144-token spatial attention backward); B = 4, T = 4
    (M = 2304: the transpose-free grouped weight-gradient launch); B = 3, T = 5 (M = 2160: a ragged last row tile, through the transposed copies).
    The keys of the fp16 tests, and two backward passes bit-identical."""
    import gtav_amd.weights as W
    from gtav_amd.model.dit import DiT_models
    from oracle import ref_cpu as O
    sd = W.synth_state_dict(W.dit_param_shapes(depth=16), seed=0)
    g = torch.Generator().manual_seed(11 + B)
    x = torch.randn(B, T, 16, 18, 32, generator=g) * 0.7
    t = torch.full((B, T), 15, dtype=torch.long)
    t[:, -1] = torch.tensor([420, 77, 901, 333][:B])
    a = torch.zeros(B, T, 25)
    a[torch.arange(B)[:, None], torch.arange(T)[None], torch.randint(0, 25, (B, T), generator=g)] = 1
    vt = torch.randn(B, 1, 16, 18, 32, generator=g)
    torch.set_num_threads(16)
    _, v_ref, grads = O.dit_loss_and_grads(sd, O.dit_s_2(), x, t, a, vt)
    m = DiT_models["DiT-S/2"](init_weights=False, max_batch=B, trainable=True, train_dtype=BF16)
    assert all(d == BF16 for d in m.operand_dtypes())
    m.load_state_dict(sd)
    v = m.forward_train(x, t, a)
    assert rel_l2(v, v_ref) < TOL_FWD_BF16
    keys = ["x_embedder.proj.weight", "t_embedder.mlp.0.weight", "external_cond.weight", "blocks.0.s_attn.to_qkv.weight", "blocks.0.t_attn.to_out.weight",
            "blocks.7.s_mlp.fc1.weight", "blocks.7.t_mlp.fc2.weight", "blocks.7.t_adaLN_modulation.1.weight", "blocks.15.t_attn.to_qkv.weight",
            "blocks.15.s_mlp.fc2.bias", "final_layer.linear.weight", "final_layer.adaLN_modulation.1.bias"]
    keys += [f"blocks.{l}.{h}_{n}.weight" for l in (0, 7, 15) for h in "st" for n in ("attn.to_qkv", "attn.to_out", "mlp.fc1", "mlp.fc2")]
    keys += ["blocks.7.s_mlp.fc1.bias", "blocks.7.t_mlp.fc2.bias", "blocks.7.t_attn.to_out.bias", "blocks.0.s_adaLN_modulation.1.weight",
             "blocks.15.t_adaLN_modulation.1.bias"]
    keys = list(dict.fromkeys(keys))
    runs = []
    for _ in range(2):
        m.zero_grad()
        m.backward_(v, vt)
        m.check()
        runs.append(m.grad_arena.clone())
    assert torch.equal(runs[0], runs[1])
    worst = _grad_errors(m, grads, keys)
    print(f"B={B} T={T}: worst bf16 gradient error {max(worst.values()):.3e} ({max(worst, key=worst.get)})")
    assert max(worst.values()) < GRAD_TOL_BF16, worst


# ---- 3. fixture G8: autograd through the reference's own module -------------------------------------------------------------------------
def test_bf16_gradients_match_reference_fixture_g8():
    from safetensors.torch import load_file
    g = load_file(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g8_training.safetensors"))
    sd = TC.state_dict(KW, 3)
    m = _model(sd, 2, 3)
    v = m.forward_train(g["x"], g["t"], g["actions"])
    assert rel_l2(v, g["v_pred"]) < TOL_FWD_BF16
    m.zero_grad()
    m.backward_(v, g["v_target"])
    m.check()
    names = sorted(k for k in sd if not k.endswith("freqs"))
    assert len(names) == int(g["names_check"])
    sel = lambda t_: t_.reshape(-1) if t_.numel() <= 4096 else t_.reshape(-1)[::97]
    norms = torch.stack([m.grad(k).norm().cpu() for k in names])
    dn = float(((norms - g["grad_norms"]).abs() / g["grad_norms"]).max())
    print(f"worst per-parameter gradient norm deviation {dn:.3e}")
    assert dn < 0.03
    for k in names:
        assert rel_l2(sel(m.grad(k).cpu()), g["grad." + k]) < GRAD_TOL_BF16, k
    m.adamw_step(1e-3, weight_decay=0.01, max_grad_norm=1.0)
    applied, _, total = m.train_stats()
    print(f"global gradient norm {total:.6e}, reference {float(g['total_grad_norm']):.6e}")
    assert applied and abs(total - float(g["total_grad_norm"])) < 0.02 * float(g["total_grad_norm"])


# ---- 4. the outlier checkpoint: fp16 cannot train it, bf16 can --------------------------------------------------------------------------
def _outlier_sd():
    sd = TC.state_dict(KW, 3)
    big = dict(sd)
    big["blocks.0.s_mlp.fc1.weight"] = sd["blocks.0.s_mlp.fc1.weight"] * 3e5     # the x3e5 outlier of tests/test_gpu_range.py
    return big


def test_outlier_checkpoint_fp16_training_step_is_skipped():
    """The gap this mode closes: every saturating fp16 activation store raises the saturation bit, and the optimizer skips the step at any loss scale."""
    from gtav_amd.train import training_step
    m = _model(_outlier_sd(), 2, 5, F16)
    m.loss_scale = 1.0
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-4)
    applied, skipped, _ = m.train_stats()
    assert not applied and skipped == 1


def test_outlier_checkpoint_trains_on_bf16_operands():
    from gtav_amd.train import training_step
    from oracle import ref_cpu as O
    big = _outlier_sd()
    x, t, a, vt = _inputs(B=2, T=3, seed=4)
    _, v_ref, grads = O.dit_loss_and_grads(big, O.DiTConfig(**KW), x, t, a, vt)
    m = _model(big, 2, 5)
    assert m.loss_scale == 1.0
    v = m.forward_train(x, t, a)
    assert torch.isfinite(v).all()
    print(f"outlier forward: {rel_l2(v, v_ref):.3e}")
    m.zero_grad()
    m.backward_(v, vt)
    m.check()                                            # nothing saturated, nothing non-finite
    assert torch.isfinite(m.grad_arena).all()
    # the outlier layer itself and everything downstream of it: the bf16 bound
    keys = ["blocks.0.s_mlp.fc1.weight", "blocks.0.s_mlp.fc2.weight", "blocks.1.t_mlp.fc1.weight", "blocks.1.s_attn.to_out.weight", "final_layer.linear.weight",
            "t_embedder.mlp.0.weight"]
    worst = _grad_errors(m, grads, keys)
    assert max(worst.values()) < GRAD_TOL_BF16, worst
    # Upstream of it (the patch embedding, block 0's to_qkv) the gradient reaches the parameter through the x3e5 Jacobian and the LayerNorm of a residual the
    # outlier branch dominates: there the problem itself is ill-conditioned.  The fp32 oracle fed nothing but the bf16 rounding of the weights — what any bf16
    # run, the reference's autocast included, computes with — moves these gradients by 4-6e-2.  They are held to that sensitivity instead.
    rb = {k: (v.to(BF16).float() if v.dim() == 2 else v) for k, v in big.items()}
    _, _, grads_rb = O.dit_loss_and_grads(rb, O.DiTConfig(**KW), x, t, a, vt)
    for k in ("x_embedder.proj.weight", "blocks.0.s_attn.to_qkv.weight"):
        sens = _rel_l2(grads_rb[k], grads[k])
        e = rel_l2(m.grad(k), grads[k])
        print(f"{k}: bf16 training {e:.3e}, fp32 oracle on bf16-rounded weights {sens:.3e}")
        assert e < 1.5 * sens, (k, e, sens)
    # eight optimisation steps through the training loop: every one applies (the Adam step count reaches 8), the loss stays finite
    lat, a5, tgt, ctx, cn, nz = TC.clip(KW)
    losses = []
    for _ in range(8):
        losses.append(float(training_step(m, lat, a5, tgt, ctx, cn, nz, lr=1e-4)))
        applied, _, gnorm = m.train_stats()
        assert applied and math.isfinite(gnorm)
    print("outlier losses:", losses)
    assert all(math.isfinite(l) for l in losses)
    st = m.opt_state_dict()["step"]
    assert int(st[0]) == 8 and int(st[1]) == 0


def test_bf16_training_step_reduces_the_loss():
    from gtav_amd.train import training_step
    m = _model(TC.state_dict(KW, 1), 2, 5)
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    losses = [float(training_step(m, lat, a.new_zeros(2, 5, 25), tgt, ctx, cn, nz, lr=2e-4, weight_decay=0.0, max_grad_norm=1.0)) for _ in range(8)]
    print("losses:", losses)
    assert all(math.isfinite(l) for l in losses)
    assert losses[-1] < losses[0] * 0.9, losses
    assert int(m.opt_state_dict()["step"][0]) == 8


# ---- 5. the optimizer's bf16 operand rewrite ---------------------------------------------------------------------------------------------
def test_bf16_adamw_rewrites_the_operands_like_a_fresh_inference_handle():
    """After two steps the W / W^T images the optimizer wrote from the updated masters are the bf16 conversion of those masters: a fresh bf16 INFERENCE handle
    loaded with the pulled weights returns the trained handle's plain forward bit for bit."""
    from gtav_amd.model.dit import DiT
    from gtav_amd.train import training_step
    m = _model(TC.state_dict(KW, 1), 2, 5)
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    for _ in range(2):
        training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-3, weight_decay=0.01)
    assert int(m.opt_state_dict()["step"][0]) == 2
    m.pull_weights()
    x, t, a3, _ = _inputs(B=2, T=5, seed=9)
    out = m(x, t, a3).clone()
    m.check()
    mi = DiT(**KW, max_batch=2, max_frames=5, init_weights=False)
    mi.set_operand_dtype(BF16)
    mi.load_state_dict(m.state_dict())
    ref = mi(x, t, a3)
    mi.check()
    assert torch.equal(out, ref)


# ---- 6. phases, overflow ------------------------------------------------------------------------------------------------------------------
def test_bf16_phased_backward_equals_monolithic():
    m = _model(TC.state_dict(KW, 1), 2, 3)
    x, t, a, vt = _inputs()
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    whole = m.grad_arena.clone()
    m.zero_grad()
    for phase in range(m.depth + 2):
        m.backward_phases_(v, vt, phase, phase + 1)
    assert torch.equal(m.grad_arena, whole)


def test_bf16_overflow_skips_the_step():
    sd = TC.state_dict(KW, 1)
    m = _model(sd, 2, 3)
    x, t, a, vt = _inputs()
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    m.grad_arena[5] = float("inf")
    m.adamw_step(1e-3, weight_decay=0.01, max_grad_norm=1.0)
    applied, skipped, _ = m.train_stats()
    assert not applied and skipped == 1
    m.pull_weights()
    for k in ("blocks.0.s_mlp.fc1.bias", "blocks.0.s_mlp.fc1.weight", "final_layer.linear.weight"):
        assert torch.equal(m._sd[k], sd[k]), k


# ---- 7. checkpoint / resume -----------------------------------------------------------------------------------------------------------------
def test_bf16_save_state_load_state_resumes_bit_exactly(tmp_path):
    from gtav_amd.train import load_state, save_state, training_step
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    kw = dict(lr=3e-4, weight_decay=0.01, max_grad_norm=1.0)
    sd = TC.state_dict(KW, 1)
    m1 = _model(sd, 2, 5)
    for _ in range(3):
        training_step(m1, lat, a, tgt, ctx, cn, nz, **kw)
    m1.pull_weights()
    straight = {k: v.clone() for k, v in m1._sd.items()}
    del m1
    m2 = _model(sd, 2, 5)
    for _ in range(2):
        training_step(m2, lat, a, tgt, ctx, cn, nz, **kw)
    ck = str(tmp_path / "dit_last")
    save_state(m2, ck, global_step=2, epoch=0)
    del m2
    with open(os.path.join(ck, "step.json")) as f:
        step = json.load(f)
    assert step["operand_dtype"] == "bf16" and step["loss_scale"] == 1.0
    from gtav_amd.model.dit import DiT
    m3 = DiT(**KW, max_batch=2, max_frames=5, init_weights=True, trainable=True, train_dtype=BF16)
    st = load_state(m3, ck)
    assert st["step"] == 2
    training_step(m3, lat, a, tgt, ctx, cn, nz, **kw)
    m3.pull_weights()
    for k in straight:
        assert torch.equal(m3._sd[k], straight[k]), k
    assert int(m3.opt_state_dict()["step"][0]) == 3
    # into an fp16-trainable handle: the weights and moments load, the loss scale of the bf16 run does not
    m4 = DiT(**KW, max_batch=2, max_frames=5, init_weights=True, trainable=True)
    load_state(m4, ck)
    assert m4.loss_scale == 65536.0
    assert int(m4.opt_state_dict()["step"][0]) == 2


# ---- 8. interface -------------------------------------------------------------------------------------------------------------------------
def test_bf16_trainable_model_operand_dtype_interface():
    from gtav_amd.lib import GtavError
    from gtav_amd.model.dit import DiT, DiT_models
    m = _model(TC.state_dict(KW, 1), 1, 2)
    assert m.loss_scale == 1.0 and all(d == BF16 for d in m.operand_dtypes())
    m.set_operand_dtype(BF16)                            # no-op
    with pytest.raises(GtavError, match="bf16 operands"):
        m.set_operand_dtype(F16)
    x, t, a, vt = _inputs(B=1, T=2)
    m.forward_train(x, t, a)                             # builds the handle
    m.set_operand_dtype(BF16)
    with pytest.raises(GtavError, match="bf16 operands"):
        m.set_operand_dtype(F16)
    assert all(d == BF16 for d in m.operand_dtypes())
    m2 = DiT_models["DiT-S/2"](init_weights=False, trainable=True, train_dtype=BF16)
    assert m2.train_dtype == BF16 and m2.loss_scale == 1.0
    with pytest.raises(ValueError):
        DiT(**KW, train_dtype=BF16)                       # an inference model picks its type with set_operand_dtype
