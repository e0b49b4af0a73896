"""The DiT training step at every patch geometry the forward takes (include/gtav_amd.h gtav_dit_train_enable): F = in_channels * patch_size^2 features per
patch from 16 to 256, where the patch embedding contracts over Kpe = round_up(F, 64) zero-padded columns and the final projection's gradient is round_up(F, 64)
wide.  Toy model (hidden 256, depth 2, 4 heads, 25 actions), B = 2, T = 3, 32 tokens per frame at every geometry; fp16 and bf16 operands.

Bounds are the project's own for the same comparisons (tests/train_cases.py): forward within FWD_TOL, every gradient tensor within GRAD_TOL relative L2, for
fp16 and for bf16 operands.  x_embedder.proj.weight is the worst tensor of every training test of the project: where it ALONE exceeds GRAD_TOL at some
geometry it is held to 1.5 x the figure the same tensor reads at (patch 2, 16 channels, 8 x 16) with the same batch and seed in the same run — the geometry
every earlier test uses (the rule of tests/test_gpu_train_long_window.py).  `pytest -s` prints every margin (profiles/geometry/grad_errors.txt).

The training handle has no hook that seeds its workspace, so rows behind M and the pad columns of xp / dfo cannot be poisoned from here; that the pad columns
of the patch-embedding image stay exactly zero through optimizer steps is asserted through the gradients of a later step being finite and equal, bit for bit,
to those of a fresh handle loaded from the saved state (whose image set_weight builds from the master alone)."""
import functools
import math
import os

import pytest
import torch

import train_cases as TC
from helpers import dev, rel_l2_logged
from helpers import rel_l2 as _rel_l2
from train_cases import DTYPES, F16, FWD_TOL, GRAD_TOL

pytestmark = pytest.mark.gpu

PE = "x_embedder.proj.weight"

SMALL = dict(hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)
GEO = {   # id: geometry; F = C p^2, Kpe = round_up(F, 64)
    "p2c4": dict(input_h=8, input_w=16, patch_size=2, in_channels=4),        # F = 16: 48 pad columns
    "p2c8": dict(input_h=8, input_w=16, patch_size=2, in_channels=8),        # F = 32
    "p1c16": dict(input_h=4, input_w=8, patch_size=1, in_channels=16),       # F = 16, no patching
    "p4c4": dict(input_h=16, input_w=32, patch_size=4, in_channels=4),       # F = 64: the (ph, pw, c) order at a patch other than 2
    "p2c32": dict(input_h=8, input_w=16, patch_size=2, in_channels=32),      # F = 128: two column tiles of dfo
    "p4c16": dict(input_h=16, input_w=32, patch_size=4, in_channels=16),     # F = 256: four column tiles of dfo
}
DEFAULT = dict(input_h=8, input_w=16, patch_size=2, in_channels=16)          # the geometry of every other training test
GEOS = sorted(GEO)
STEP_KW = dict(lr=3e-4, weight_decay=0.01, max_grad_norm=1.0)

rel_l2 = functools.partial(rel_l2_logged, tag="geometry")       # rel_l2(a, b, what): (-s shows the measured margins)


def _kw(geo):
    return dict(SMALL, **(DEFAULT if geo == "default" else GEO[geo]))


def _sd(geo, seed=1):
    return TC.state_dict(_kw(geo), seed)


def _inputs(geo, actions=True):
    return TC.inputs(_kw(geo), 2, 3, actions)


def _ref(geo, actions):
    """The oracle's loss, v_pred and gradients of one geometry (shared: never modified)."""
    return TC.oracle(_kw(geo), 2, 3, actions)[2:]


def _model(geo, dtype=F16, sd=None, **extra):
    return TC.model(_kw(geo), 2, 3, dtype, sd, **extra)


def _backward(m, *inputs):
    return TC.forward_backward(m, inputs)


@functools.lru_cache(maxsize=None)
def _default_pe_error(actions, dtype):
    """x_embedder.proj.weight's error at the default geometry, same batch and seed: the launches every earlier training test runs."""
    x, t, a, vt = _inputs("default", actions)
    m = _model("default", dtype)
    _backward(m, x, t, a, vt)
    return _rel_l2(m.grad(PE), _ref("default", actions)[2][PE])


def _accept(errs, dtype, actions, tag):
    top = max(errs, key=errs.get)
    print(f"[geometry-grad {tag}] worst {errs[top]:.3e} ({top}), {PE} {errs[PE]:.3e}, GRAD_TOL {GRAD_TOL[dtype]:.1e}")
    over = {k: e for k, e in errs.items() if e > GRAD_TOL[dtype]}
    if not over:
        return
    assert set(over) == {PE}, f"gradient mismatch beyond GRAD_TOL {GRAD_TOL[dtype]:.1e}: {over}"
    bound = 1.5 * _default_pe_error(actions, dtype)
    print(f"[geometry-grad {tag}] above GRAD_TOL: {over[PE]:.3e} {PE}; 1.5 x the default geometry's = {bound:.3e}")
    assert over[PE] <= bound, f"{PE}: {over[PE]:.3e} beyond GRAD_TOL {GRAD_TOL[dtype]:.1e} and beyond 1.5 x the default geometry's figure {bound:.3e}"


# ---- 1. forward, loss and every gradient against autograd on the oracle ------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("actions", [True, False], ids=["actions", "noactions"])
@pytest.mark.parametrize("geo", GEOS)
def test_gradients_match_autograd(geo, actions, dtype):
    loss_ref, v_ref, grads = _ref(geo, actions)
    x, t, a, vt = _inputs(geo, actions)
    m = _model(geo, dtype)
    assert m.train_dtype == dtype
    v = _backward(m, x, t, a, vt)
    assert rel_l2(v, v_ref, "v_pred") < FWD_TOL[dtype]
    loss = torch.nn.functional.mse_loss(v[:, -1:].cpu(), vt)
    e_loss = abs(float(loss) - float(loss_ref)) / float(loss_ref)
    print(f"[geometry {geo}] loss {float(loss):.6f} oracle {float(loss_ref):.6f} rel {e_loss:.3e}")
    assert e_loss < FWD_TOL[dtype]
    _accept(TC.grad_errors(m, grads), dtype, actions, f"{geo} actions={actions} {dtype}")


def _g14_sel(name, v):
    """The elements fixture G14 keeps of a gradient (tools/make_golden.py g14_sel)."""
    if v.numel() <= 512:
        return v.reshape(-1)
    return v.reshape(-1)[::97 if name in (PE, "final_layer.linear.weight") else 997]


@DTYPES
@pytest.mark.parametrize("geo", ["p4c4", "p2c8"])
def test_gradients_match_reference_fixture_g14(geo, dtype):
    """HIP gradients against autograd through the REFERENCE's own DiT module (tests/golden/g14_geometry.safetensors), no oracle in between."""
    from safetensors.torch import load_file
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_geometry.safetensors")
    g = {k[len(geo) + 1:]: v for k, v in load_file(path).items() if k.startswith(geo + ".")}
    sd = _sd(geo, 3)
    m = _model(geo, dtype, sd)
    v = _backward(m, g["x"], g["t"], g["actions"], g["v_target"])
    assert rel_l2(v, g["v_pred"], "v_pred") < FWD_TOL[dtype]
    loss = torch.nn.functional.mse_loss(v[:, -1:].cpu(), g["v_target"])
    assert abs(float(loss) - float(g["loss"])) / float(g["loss"]) < FWD_TOL[dtype]
    names = sorted(k for k in sd if not k.endswith("freqs"))
    assert len(names) == int(g["names_check"])
    norms = torch.stack([m.grad(k).norm().cpu() for k in names])
    e_norm = (norms - g["grad_norms"]).abs() / g["grad_norms"]
    print(f"[geometry-grad {geo} {dtype} G14] worst norm error {float(e_norm.max()):.3e} ({names[int(e_norm.argmax())]})")
    assert float(e_norm.max()) < GRAD_TOL[dtype]
    errs = {k: _rel_l2(_g14_sel(k, m.grad(k).cpu()), g["grad." + k]) for k in names}
    _accept(errs, dtype, True, f"{geo} {dtype} G14")


# ---- 2. the optimizer: masters against adamw_reference, the rewritten W / W^T images against the oracle at the updated weights -------------------
@DTYPES
@pytest.mark.parametrize("geo", GEOS)
def test_adamw_step_matches_reference(geo, dtype):
    """One clip_grad_norm_ + AdamW step on IDENTICAL gradients (the oracle's, written into the arena in its documented order: parameters by name) against
    oracle adamw_reference, equal to fp32 rounding (tests/test_gpu_train.py test_adamw_step_matches_torch: 1e-4 of the update, 1e-5 of the norm); then the
    forward and the gradients at the UPDATED weights: what the rewritten operand images hold, pad columns included."""
    from oracle import ref_cpu as O
    sd = _sd(geo)
    _, _, grads = _ref(geo, True)
    x, t, a, vt = _inputs(geo)
    params = {k: v for k, v in sd.items() if not k.endswith("freqs")}
    ref, norm_ref = O.adamw_reference(params, grads, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0, steps=1)
    m = _model(geo, dtype)
    m.forward_train(x, t, a)                      # builds the handle
    flat = torch.cat([grads[k].reshape(-1) for k in sorted(params)]) * m.loss_scale
    assert flat.numel() == m.grad_arena.numel()
    m.grad_arena.copy_(flat.to(m.grad_arena.device))
    m.adamw_step(1e-3, weight_decay=0.01, max_grad_norm=1.0)
    applied, skipped, norm = m.train_stats()
    assert applied and skipped == 0
    assert abs(norm - float(norm_ref)) / float(norm_ref) < 1e-5
    m.pull_weights()
    for k in params:
        assert m._sd[k].shape == params[k].shape, k
        e = _rel_l2(m._sd[k] - params[k], ref[k] - params[k])
        assert e < 1e-4, (k, e)
    sd2 = dict(sd)
    sd2.update(ref)
    _, v2_ref, grads2 = O.dit_loss_and_grads(sd2, O.DiTConfig(**_kw(geo)), x, t, a, vt)
    v2 = _backward(m, x, t, a, vt)
    assert rel_l2(v2, v2_ref, "v_pred after the step") < FWD_TOL[dtype]
    _accept(TC.grad_errors(m, grads2), dtype, True, f"{geo} {dtype} after one AdamW step")


# ---- 3. the training modes: recompute, phases and buckets, checkpoints, mixed-capable handles, device noise ---------------------------------------
def _clip(geo):
    return TC.clip(_kw(geo), F=3)


def _masters(m):
    m.pull_weights()
    return {k: v.clone() for k, v in m._sd.items()}


@DTYPES
@pytest.mark.parametrize("geo", GEOS)
def test_recompute_handle_equals_the_plain_handle(geo, dtype):
    from gtav_amd.train import training_step
    clip = _clip(geo)
    plain, rec = _model(geo, dtype), _model(geo, dtype, train_recompute=True)
    assert rec.train_recompute and not plain.train_recompute
    for step in range(3):
        la = training_step(plain, *clip, n_prompt_frames=2, **STEP_KW)
        lb = training_step(rec, *clip, n_prompt_frames=2, **STEP_KW)
        assert torch.equal(la, lb) and math.isfinite(float(la)), step
        assert torch.equal(plain.grad_arena, rec.grad_arena), step
        assert plain.train_stats() == rec.train_stats() and plain.train_stats()[0], step
    wa, wb = _masters(plain), _masters(rec)
    for k in wa:
        assert torch.equal(wa[k], wb[k]), k
    assert not torch.equal(wa[PE], _sd(geo)[PE])


@DTYPES
@pytest.mark.parametrize("geo", GEOS)
def test_phased_backward_equals_monolithic_and_buckets_tile_the_arena(geo, dtype):
    from gtav_amd.train import gradient_buckets
    x, t, a, vt = _inputs(geo)
    m = _model(geo, dtype)
    v = _backward(m, x, t, a, vt)
    whole = m.grad_arena.clone()
    buckets = gradient_buckets(m)
    spans = sorted((off, off + cnt) for _, off, cnt in buckets)
    assert spans[0][0] == 0 and spans[-1][1] == m.grad_arena.numel() and all(a_[1] == b_[0] for a_, b_ in zip(spans, spans[1:]))
    kw = _kw(geo)
    F = kw["in_channels"] * kw["patch_size"] ** 2
    off, cnt = m.param_range("x_embedder.proj.weight")
    assert cnt == 256 * F                                   # the arena holds the gradient at its state-dict width: no pad column
    assert m.param_range("final_layer.linear.")[1] == F * 256 + F
    m.zero_grad()
    for phase in range(m.depth + 2):
        m.backward_phases_(v, vt, phase, phase + 1)
        for ph, o, c in buckets:
            if ph == phase:
                assert torch.equal(m.grad_arena[o: o + c], whole[o: o + c]), (phase, o)
    assert torch.equal(m.grad_arena, whole)


@DTYPES
@pytest.mark.parametrize("geo", ["p2c4", "p4c16"])
def test_save_state_load_state_resumes_bit_exactly(geo, dtype, tmp_path):
    """Three steps straight == two steps, save_state, a FRESH model, load_state, one more step: weights equal bit for bit (F = 16 and F = 256).  And the
    gradients of a step after two optimizer steps equal those of the fresh handle, whose patch-embedding image set_weight built from the master with zero
    pad columns: a non-zero pad column in the image the optimizer rewrote would meet xp's zeros only in the forward's product, but a NaN or an inf there
    (0 x inf) would not stay hidden, and the weight gradient is checked finite."""
    from gtav_amd.model.dit import DiT
    from gtav_amd.train import load_state, save_state, training_step
    clip = _clip(geo)
    x, t, a, vt = _inputs(geo)
    m1 = _model(geo, dtype)
    for _ in range(3):
        training_step(m1, *clip, n_prompt_frames=2, **STEP_KW)
    straight = _masters(m1)
    m2 = _model(geo, dtype)
    for _ in range(2):
        training_step(m2, *clip, n_prompt_frames=2, **STEP_KW)
    ck = str(tmp_path / "train_checkpoints" / "dit_last")
    save_state(m2, ck, global_step=2, epoch=0)
    m3 = DiT(**_kw(geo), max_batch=2, max_frames=3, init_weights=True, trainable=True, train_dtype=dtype)    # other weights until load_state
    assert load_state(m3, ck)["step"] == 2
    _backward(m2, x, t, a, vt)
    _backward(m3, x, t, a, vt)
    assert torch.isfinite(m2.grad_arena).all() and torch.equal(m2.grad_arena, m3.grad_arena)
    training_step(m3, *clip, n_prompt_frames=2, **STEP_KW)
    resumed = _masters(m3)
    for k in straight:
        assert torch.equal(resumed[k], straight[k]), k
    applied, skipped, _ = m3.train_stats()
    assert applied and skipped == 0 and int(m3.opt_state_dict()["step"][0]) == 3


@pytest.mark.parametrize("geo", ["p2c4", "p4c16"])
def test_mixed_capable_handle_with_device_noise_equals_the_plain_handle_with_materialised_draws(geo):
    """train_range_policy="auto" (no group switched) and rng= in one step: equal, bit for bit, to the plain handle fed the same draws as tensors."""
    import gtav_amd.rng as R
    from gtav_amd.train import training_step
    kw = _kw(geo)
    shape = (kw["in_channels"], kw["input_h"], kw["input_w"])
    lat, a = _clip(geo)[:2]
    src = R.NoiseSource(0x0123456789ABCDEF, sample0=6)
    ref = src.clone()
    ma, mb = _model(geo, F16, train_range_policy="auto"), _model(geo, F16)
    for step in range(2):
        la = training_step(ma, lat, a, rng=src, ctx_max_noise_idx=40, noise_steps=50, n_prompt_frames=2, **STEP_KW)
        d = ref.next_draw()
        tgt, ctx = ref.randint(1, 51, 2, R.SLOT_TARGET_IDX, d), ref.randint(1, 41, 2, R.SLOT_CTX_IDX, d)
        cn, nz = ref.normal(2, 2, shape, d, 0, dev()), ref.normal(2, 1, shape, d, 2, dev())
        lb = training_step(mb, lat, a, tgt, ctx, cn, nz, noise_steps=50, n_prompt_frames=2, **STEP_KW)
        assert torch.equal(la, lb) and math.isfinite(float(la)), step
        assert ma.train_stats() == mb.train_stats() and ma.train_stats()[0], step
    assert ma.train_autorange() == []
    wa, wb = _masters(ma), _masters(mb)
    for k in wb:
        assert torch.equal(wa[k], wb[k]), k


# ---- 4. the two refusals that remain, by name ---------------------------------------------------------------------------------------------------
def test_padded_mlp_width_is_refused_by_name():
    from gtav_amd.lib import GtavError
    from gtav_amd.model.dit import DiT
    m = DiT(**_kw("p2c4"), mlp_ratio=3.75, max_batch=2, max_frames=3, init_weights=False, trainable=True)    # 960 features, padded to 1024
    with pytest.raises(GtavError, match="padded MLP width .*960, padded to 1024.* is not implemented for training"):
        m.zero_grad()


def test_patch_width_not_a_multiple_of_4_is_refused_by_name():
    from gtav_amd.lib import GtavError
    from gtav_amd.model.dit import DiT
    m = DiT(**dict(SMALL, input_h=4, input_w=8, patch_size=1, in_channels=3), max_batch=2, max_frames=3, init_weights=False, trainable=True)
    with pytest.raises(GtavError, match=r"in_channels \* patch_size\^2 = 3 features is not implemented for training"):
        m.zero_grad()
