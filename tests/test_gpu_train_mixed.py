"""fp16 and bf16 operand groups on ONE training handle (DiT(trainable=True, train_range_policy="auto"), include/gtav_amd.h gtav_dit_train_allow_mixed):
the opt-in costs no bits, a handle with every group switched is the bf16 handle, every boundary between two groups of different types computes the right
gradients, and a checkpoint with one outlier layer — which skips every fp16 step — trains again after train_autorange() moved the saturated groups to bf16.

Toy geometry and bounds of tests/train_cases.py: hidden 256, 4 heads, 8 x 16 latents, patch 2 (32 tokens per frame); the bf16 GRAD_TOL (8 x the fp16 one) and
FWD_TOL.  `pytest -s` prints every measured margin.

Depth: the bit-for-bit tests of recompute mode and of the phased backward run at depth 3, where a middle block exists — in recompute mode it is the only block
whose re-run both starts from a stored shift and ends by re-saving the next block's.  The tests against the fp32 oracle run at depth 2, the depth GRAD_TOL_BF16 was
measured for (all-bf16 reaches 2.7e-2 of 3.6e-2 there): the gradient error of the tensors upstream grows with every half-block the gradient crosses,
and at depth 3 the ALL-bf16 handle itself sits at the bound for x_embedder.proj.weight (DESIGN.md 7 has the figures), so a depth-3 comparison would test the
bound, not the seams.  Depth 2 has every seam there is: inside a block, between two blocks, and between the last half-block and the final layer."""
import json
import math
import os

import pytest
import torch

import train_cases as TC
from helpers import rel_l2_logged as rel_l2       # (-s shows the measured margins)
from train_cases import BF16, F16
from train_cases import TOY_KW as KW

pytestmark = pytest.mark.gpu

TOL_FWD_BF16, GRAD_TOL_BF16 = TC.FWD_TOL[BF16], TC.GRAD_TOL[BF16]

KW3 = dict(KW, depth=3)
# layer groups of the depth-2 model: 0 .. 3 the half-blocks, 4 the patch embedding, 5 the final layer.  Even / odd: every boundary between two half-blocks changes
# type; the last pattern also changes type between the last half-block (3) and the final layer (5), whose LayerNorm applies that half-block's pending branch
PATTERNS = {"even_bf16": [0, 2, 4], "odd_bf16": [1, 3, 5], "final_seam": [1, 2, 5]}


def _outlier_sd():
    sd = TC.state_dict(KW, 3)
    big = dict(sd)
    big["blocks.0.s_mlp.fc1.weight"] = sd["blocks.0.s_mlp.fc1.weight"] * 3e5     # the x3e5 outlier of tests/test_gpu_range.py
    return big


def _model(sd, B, T, dtype=F16, policy="auto", kw=KW, **extra):
    return TC.model(kw, B, T, dtype, sd, train_range_policy=policy, **extra)


def _inputs(B=2, T=3, actions=True, seed=0):
    return TC.inputs(KW, B, T, actions, seed)


def _forward_backward(m, inp, v_ref, grads, keys=None):
    """One forward + backward against the oracle: (forward error, per-tensor gradient errors); nothing may be left in the error words."""
    v = TC.forward_backward(m, inp)
    return rel_l2(v, v_ref), TC.grad_errors(m, grads, keys)


def _print_table(title, cols):
    """cols: {column name: {tensor: error}}; one line per tensor (-s)."""
    names = list(cols)
    print(f"\n# {title}\n# {'tensor':<44}" + "".join(f"{n:>12}" for n in names))
    for k in next(iter(cols.values())):
        print(f"{k:<46}" + "".join(f"{cols[n].get(k, float('nan')):>12.3e}" for n in names))


def _snapshot(m, probe):
    """Everything a training run is: the forward on fixed inputs, the gradient arena it was left with, masters, AdamW state, the optimizer's words."""
    x, t, a, _ = probe
    st = m.train_stats()
    arena = m.grad_arena.clone()
    opt = m.opt_state_dict()
    m.pull_weights()
    out = {"arena": arena, "stats": torch.tensor([float(st[0]), float(st[1]), st[2]], dtype=torch.float64), "v_pred": m.forward_train(x, t, a).clone()}
    out.update({"w." + k: v.clone() for k, v in m._sd.items()})
    out.update({"opt." + k: v for k, v in opt.items()})
    return out


def _run(m, n_steps, probe, **kw):
    from gtav_amd.train import training_step
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    losses = [training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-3, weight_decay=0.01, **kw).clone() for _ in range(n_steps)]
    snap = _snapshot(m, probe)
    snap["losses"] = torch.cat(losses)
    return snap


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- 1. the opt-in costs no bits ----------------------------------------------------------------------------------------------------------
@TC.DTYPES
def test_mixed_capable_handle_with_no_group_switched_equals_the_default_handle(dtype):
    sd, probe = TC.state_dict(KW), _inputs(B=2, T=5, seed=9)
    plain = _run(_model(sd, 2, 5, dtype, "report"), 3, probe)
    m = _model(sd, 2, 5, dtype, "auto")
    opted = _run(m, 3, probe)
    assert all(d == dtype for d in m.operand_dtypes()) and m.loss_scale == (65536.0 if dtype == F16 else 1.0)
    assert int(plain["opt.step"][0]) == 3
    _assert_same(plain, opted)
    assert m.train_autorange() == []


# ---- 2. every group switched = the bf16 twin ------------------------------------------------------------------------------------------------
def test_all_groups_switched_equals_the_bf16_handle():
    """The images train_set_group_dtype remakes from the masters in the handle are set_weight's, and no launch stays on the fp16 kernels."""
    sd, probe = TC.state_dict(KW), _inputs(B=2, T=5, seed=9)
    twin = _run(_model(sd, 2, 5, BF16, "report"), 3, probe)
    m = _model(sd, 2, 5, F16, "auto")
    m.forward_train(*probe[:3])                    # the weights are in the handle as fp16 images ...
    m.train_set_group_dtype(BF16)                   # ... and are converted again in place
    m.loss_scale = 1.0
    assert all(d == BF16 for d in m.operand_dtypes())
    _assert_same(twin, _run(m, 3, probe))


# ---- 3. every seam a type change --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actions", [True, False], ids=["actions", "noactions"])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_alternating_types_match_autograd(pattern, actions):
    sd, inp, _, v_ref, grads = TC.oracle(KW, 2, 3, actions)
    m = _model(sd, 2, 3)
    m.train_set_group_dtype(BF16, PATTERNS[pattern])
    assert [d == BF16 for d in m.operand_dtypes()] == [g in PATTERNS[pattern] for g in range(6)]
    e_fwd, worst = _forward_backward(m, inp, v_ref, grads)
    _print_table(f"test 3 {pattern} actions={actions}: forward {e_fwd:.3e}", {"rel_l2": worst})
    assert e_fwd < TOL_FWD_BF16
    bad = {k: e for k, e in worst.items() if e > GRAD_TOL_BF16}
    assert not bad, f"gradient mismatch: {bad}"


# ---- 4. one group switched on an ordinary checkpoint ------------------------------------------------------------------------------------------
def test_one_group_switched_keeps_every_gradient_in_the_bf16_bound():
    """Group 1 (block 0, temporal half) on bf16, everything else fp16.  Whether the tensors of the fp16 groups stay at their fp16 error is printed per tensor
    beside the all-fp16 and the all-bf16 handle (profiles/train_mixed/grad_errors.txt is this table), not asserted."""
    sd, inp, _, v_ref, grads = TC.oracle(KW, 2, 3, True)
    cols = {}
    for name, dtype, groups in (("fp16", F16, []), ("group1", F16, [1]), ("bf16", BF16, [])):
        m = _model(sd, 2, 3, dtype)
        if groups:
            m.train_set_group_dtype(BF16, groups)
        e_fwd, cols[name] = _forward_backward(m, inp, v_ref, grads)
        cols[name] = dict(cols[name], **{"(forward)": e_fwd})
        del m
    _print_table("test 4: group 1 on bf16 against all-fp16 and all-bf16", cols)
    bad = {k: e for k, e in cols["group1"].items() if e > GRAD_TOL_BF16}
    assert not bad, f"gradient mismatch: {bad}"
    assert cols["group1"]["(forward)"] < TOL_FWD_BF16


# ---- 5. the outlier checkpoint recovers -------------------------------------------------------------------------------------------------------
OUTLIER_KEYS = ["blocks.0.s_mlp.fc1.weight", "blocks.0.s_mlp.fc2.weight", "blocks.1.t_mlp.fc1.weight", "blocks.1.s_attn.to_out.weight", "final_layer.linear.weight",
                "t_embedder.mlp.0.weight"]     # tests/test_gpu_train_bf16.py test_outlier_checkpoint_trains_on_bf16_operands


def _outlier_switch(m):
    """The skipped first step of the outlier checkpoint and the switch: returns the switched groups."""
    from gtav_amd.train import training_step
    m.loss_scale = 1.0
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-4)
    applied, skipped, _ = m.train_stats()
    assert not applied and skipped == 1
    before = m.operand_dtypes()
    switched = m.train_autorange()
    print("switched groups:", switched)
    assert switched and 0 in switched and all(before[g] == F16 for g in switched)
    assert [g for g, d in enumerate(m.operand_dtypes()) if d == BF16] == switched
    return switched


def test_outlier_checkpoint_recovers_after_train_autorange():
    from gtav_amd.train import training_step
    big = _outlier_sd()
    m = _model(big, 2, 5)
    _outlier_switch(m)
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    losses = []
    for _ in range(8):
        losses.append(float(training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-4)))
        applied, skipped, gnorm = m.train_stats()
        assert applied and skipped == 1 and math.isfinite(gnorm)
    print("outlier losses:", losses)
    assert all(math.isfinite(l) for l in losses)
    st = m.opt_state_dict()["step"]
    assert int(st[0]) == 8 and int(st[1]) == 1
    assert m.train_autorange() == []


def test_outlier_checkpoint_gradients_after_the_switch():
    big = _outlier_sd()
    from oracle import ref_cpu as O
    inp = _inputs(seed=4)
    _, v_ref, grads = O.dit_loss_and_grads(big, O.DiTConfig(**KW), *inp)
    m = _model(big, 2, 5)
    _outlier_switch(m)
    # The groups that stayed fp16 need their loss scale back: at scale 1 their gradient stores underflow (block 1's gradients come out as zeros).  Which scale is
    # the loss scaler's business, and the test does what LossScaler does: from the fp16 default down, by factors of 4, to the first at which no store saturates.
    from gtav_amd.lib import GtavError
    m.loss_scale = 65536.0
    while True:
        try:
            e_fwd, worst = _forward_backward(m, inp, v_ref, grads, OUTLIER_KEYS)
            break
        except GtavError as e:
            assert "fp16 range" in str(e) and m.loss_scale > 1.0, e
            m.loss_scale = m.loss_scale / 4
    print(f"loss scale {m.loss_scale}")
    _print_table(f"test 5: outlier checkpoint after the switch: forward {e_fwd:.3e}", {"rel_l2": worst})
    assert max(worst.values()) < GRAD_TOL_BF16, worst
    assert m.train_autorange() == []


# ---- 6. forward saturation switches, backward saturation halves the loss scale ----------------------------------------------------------------
def test_gradient_overflow_switches_nothing_and_halves_the_scale():
    from gtav_amd.train import LossScaler, training_step
    m = _model(TC.state_dict(KW), 2, 5)
    m.zero_grad()                                   # builds the handle: the scaler reads the skip counter it starts from
    sc = LossScaler(m, check_every=1)
    m.loss_scale = 2.0 ** 40                        # every fp16 gradient store saturates; the forward does not know the scale
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-4)
    applied, skipped, _ = m.train_stats()
    assert not applied and skipped == 1
    assert sc.update() == 2.0 ** 39 and sc.switched == []
    assert all(d == F16 for d in m.operand_dtypes())
    training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-4)
    assert m.train_stats()[1] == 2
    assert m.train_autorange() == []                # (called directly: nothing either)
    m.check()


def test_forward_saturation_switches_groups_and_leaves_the_scale():
    from gtav_amd.train import LossScaler, training_step
    m = _model(_outlier_sd(), 2, 5)
    m.zero_grad()
    sc = LossScaler(m, check_every=1)
    m.loss_scale = 1.0
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-4)
    assert m.train_stats()[1] == 1
    assert sc.update() == 1.0 and 0 in sc.switched
    training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-4)
    applied, skipped, _ = m.train_stats()
    assert applied and skipped == 1
    assert sc.update() == 1.0 and sc.switched == []


# ---- 7. combinations ----------------------------------------------------------------------------------------------------------------------------
def _alternating(sd, B, T, kw=KW3, **extra):
    m = _model(sd, B, T, kw=kw, **extra)
    m.train_set_group_dtype(BF16, range(0, m.n_operand_groups, 2))
    return m


def test_recompute_mode_equals_plain_mode_on_alternating_types():
    sd, probe = TC.state_dict(KW3), _inputs(B=2, T=5, seed=9)
    plain = _run(_alternating(sd, 2, 5), 2, probe)
    rc = _run(_alternating(sd, 2, 5, train_recompute=True), 2, probe)
    assert int(plain["opt.step"][0]) == 2
    _assert_same(plain, rc)


def test_phased_backward_equals_monolithic_on_alternating_types():
    m = _alternating(TC.state_dict(KW3), 2, 3)
    x, t, a, vt = _inputs()
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    whole = m.grad_arena.clone()
    m.zero_grad()
    for phase in range(m.depth + 2):
        m.backward_phases_(v, vt, phase, phase + 1)
    assert torch.equal(m.grad_arena, whole)


@pytest.mark.parametrize("case", ["9frames", "200tok"])
def test_alternating_types_on_a_long_window_and_a_long_frame(case):
    kw, B, T, extra = (KW, 2, 9, dict(train_max_frames=9)) if case == "9frames" else (dict(KW, input_h=20, input_w=40), 2, 3, {})
    sd, inp, _, v_ref, grads = TC.oracle(kw, B, T, True)
    e_fwd, worst = _forward_backward(_alternating(sd, B, T, kw, **extra), inp, v_ref, grads)
    _print_table(f"test 7 {case}: forward {e_fwd:.3e}", {"rel_l2": worst})
    assert e_fwd < TOL_FWD_BF16
    bad = {k: e for k, e in worst.items() if e > GRAD_TOL_BF16}
    assert not bad, f"gradient mismatch: {bad}"


# ---- 8. resume ------------------------------------------------------------------------------------------------------------------------------------
def test_save_state_load_state_resumes_a_switched_run_bit_exactly(tmp_path):
    from gtav_amd.lib import GtavError
    from gtav_amd.model.dit import DiT
    from gtav_amd.train import load_state, save_state, training_step
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    kw = dict(lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)
    m1 = _model(_outlier_sd(), 2, 5)
    switched = _outlier_switch(m1)
    ck = str(tmp_path / "dit_last")
    save_state(m1, ck, global_step=1, epoch=0)
    with open(os.path.join(ck, "step.json")) as f:
        step = json.load(f)
    assert step["operand_dtype"] == "fp16" and step["bf16_groups"] == switched and step["loss_scale"] == 1.0
    for _ in range(2):
        training_step(m1, lat, a, tgt, ctx, cn, nz, **kw)
    m1.pull_weights()
    straight = {k: v.clone() for k, v in m1._sd.items()}
    del m1
    m2 = DiT(**KW, max_batch=2, max_frames=5, init_weights=True, trainable=True, train_range_policy="auto")      # other weights until load_state
    load_state(m2, ck)
    assert [g for g, d in enumerate(m2.operand_dtypes()) if d == BF16] == switched and m2.loss_scale == 1.0
    for _ in range(2):
        training_step(m2, lat, a, tgt, ctx, cn, nz, **kw)
    st = m2.opt_state_dict()["step"]
    assert int(st[0]) == 2 and int(st[1]) == 1
    m2.pull_weights()
    for k in straight:
        assert torch.equal(m2._sd[k], straight[k]), k
    m3 = DiT(**KW, max_batch=2, max_frames=5, init_weights=True, trainable=True)
    with pytest.raises(GtavError, match="train_range_policy='auto'"):
        load_state(m3, ck)


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_mixed_type_calls_are_refused_by_name():
    import ctypes as C
    from gtav_amd import lib as L
    from gtav_amd.lib import GtavError
    lib = L.load()

    def err(rc):
        assert rc != 0
        return lib.gtav_last_error().decode()
    n = C.c_int32(0)
    words = (C.c_int32 * 8)()
    plain = _model(TC.state_dict(KW), 1, 2, policy="report")
    plain.zero_grad()
    h = plain._handle
    assert "already enabled" in err(lib.gtav_dit_train_allow_mixed(h, 1))
    for msg in (err(lib.gtav_dit_train_set_group_dtype(h, 0, 1, None)), err(lib.gtav_dit_train_autorange(h, None, C.byref(n), None)),
                err(lib.gtav_dit_train_range_words(h, words, None))):
        assert "gtav_dit_train_allow_mixed" in msg, msg
    for call in (plain.train_autorange, plain.train_range_words, lambda: plain.train_set_group_dtype(BF16, [0])):
        with pytest.raises(GtavError, match="train_range_policy='auto'"):
            call()
    with pytest.raises(GtavError, match="keeps fp16 operands"):       # as on every fp16 training handle
        plain.set_operand_dtype(BF16)
    m = _model(TC.state_dict(KW), 1, 2)
    m.zero_grad()
    h = m._handle
    assert "already enabled" in err(lib.gtav_dit_train_allow_mixed(h, 1))
    n_groups = m.n_operand_groups
    assert f"outside [-1, {n_groups})" in err(lib.gtav_dit_train_set_group_dtype(h, n_groups, 1, None))
    assert "dtype 2" in err(lib.gtav_dit_train_set_group_dtype(h, 0, 2, None))
    assert "keeps fp16 operands" in err(lib.gtav_dit_set_operand_dtype(h, 0, 1))
    m.train_set_group_dtype(BF16, [1])
    assert "gtav_dit_train_set_group_dtype" in err(lib.gtav_dit_set_operand_dtype(h, -1, 0))
    with pytest.raises(GtavError, match="train_set_group_dtype"):
        m.set_operand_dtype(F16)
    assert [g for g, d in enumerate(m.operand_dtypes()) if d == BF16] == [1]
    with pytest.raises(ValueError):
        from gtav_amd.model.dit import DiT
        DiT(**KW, train_range_policy="auto")            # an inference model has range_policy


def test_autorange_switches_before_it_reports():
    """A bad timestep in the same interval as a saturating forward: train_autorange raises for the timestep AFTER it switched, and the model's view of the
    types is the handle's."""
    from gtav_amd.lib import GtavError
    from gtav_amd.train import training_step
    m = _model(_outlier_sd(), 2, 5)
    m.loss_scale = 1.0
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-4)
    x, t, a3, _ = _inputs(B=2, T=3)
    m.forward_train(x, torch.full_like(t, 1000), a3)
    with pytest.raises(GtavError, match="timestep"):
        m.train_autorange()
    import ctypes as C
    from gtav_amd import lib as L
    d = C.c_int32(0)
    handle = []
    for g in range(m.n_operand_groups):
        L.check(L.load().gtav_dit_get_operand_dtype(m._handle, g, C.byref(d)))
        handle.append(BF16 if d.value else F16)
    assert handle == m.operand_dtypes() and handle[0] == BF16
    assert m.train_autorange() == []


# ---- 10. stale bits -------------------------------------------------------------------------------------------------------------------------------
def test_a_saturating_validation_forward_neither_skips_nor_switches():
    from gtav_amd.lib import GtavError
    from gtav_amd.train import training_step
    m = _model(TC.state_dict(KW), 2, 5)
    x, t, a3, _ = _inputs(B=2, T=5, seed=9)
    out = m(x * 1e7, t, a3)                         # inference forward on the training handle: the patch embedding's operand saturates
    assert torch.isfinite(out).all()
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-4)
    applied, skipped, _ = m.train_stats()
    assert applied and skipped == 0
    assert m.train_range_words() == [0] * m.n_operand_groups
    with pytest.raises(GtavError, match="fp16 range"):
        m.check()
    m.check()
    assert m.train_autorange() == [] and all(d == F16 for d in m.operand_dtypes())
