"""Per-sample action dropout in the DiT training step (DiT.forward_train(action_keep=...) -> gtav_dit_train_forward_keep), the training half of classifier-free
guidance: a sample with keep 0 is conditioned as the reference conditions external_cond=None.

Two contracts are bit for bit (torch.equal) against the code path that existed before: keep all ones is the plain step with actions, keep all zeros the plain
step with actions=None (external_cond.* gradients exactly zero).  A mixed mask is checked against the CPU oracle run per sample at B = 1 with that sample's
actions or None: the loss is a mean over samples, so the batch gradient is the mean of the per-sample gradients, exactly.  Bounds: train_cases.FWD_TOL / GRAD_TOL."""
import pytest
import torch

import train_cases as TC
from oracle import ref_cpu as O
from train_cases import DTYPES, F16

pytestmark = pytest.mark.gpu

KW = TC.TOY_KW
B, T = 2, 3
_REF = {}


def _one_pass(m, inputs, keep=None, actions=True):
    """forward (with the mask), zero_grad, monolithic backward: (v_pred, gradient arena), cloned."""
    x, t, a, vt = inputs
    v = m.forward_train(x, t, a if actions else None, action_keep=keep)
    m.zero_grad()
    m.backward_(v, vt)
    m.check()
    torch.cuda.synchronize()
    return v.clone(), m.grad_arena.clone()


def _assert_same(got, want):
    for name, g, w in zip(("v_pred", "gradient arena"), got, want):
        assert g.shape == w.shape and torch.equal(g, w), f"{name}: {int((g != w).sum())} of {g.numel()} elements differ, max |diff| {float((g - w).abs().max()):.3e}"


def _oracle(keep):
    """(v_ref, grads) for the mask `keep`: the oracle per sample at B = 1 with the sample's actions or None, v concatenated, gradients averaged.  Once per mask."""
    keep = tuple(keep)
    if keep not in _REF:
        n = len(keep)
        sd = TC.state_dict(KW)
        x, t, a, vt = TC.inputs(KW, n, T)
        vs, grads = [], None
        for b, k in enumerate(keep):
            _, v, g = O.dit_loss_and_grads(sd, O.DiTConfig(**KW), x[b:b + 1], t[b:b + 1], a[b:b + 1] if k else None, vt[b:b + 1])
            vs.append(v)
            grads = g if grads is None else {name: grads[name] + g[name] for name in g}
        _REF[keep] = (torch.cat(vs), {name: g / n for name, g in grads.items()})
    return _REF[keep]


HANDLES = pytest.mark.parametrize("kind", ["plain", "recompute", "mixed", "lora"])


def _model(dtype, kind="plain", n=B):
    kw = {"plain": {}, "recompute": dict(train_recompute=True), "mixed": dict(train_range_policy="auto"), "lora": dict(train_lora_rank=16)}[kind]
    return TC.model(KW, n, T, dtype, **kw)


@DTYPES
@HANDLES
def test_keep_all_ones_is_the_plain_step_with_actions(dtype, kind):
    m = _model(dtype, kind)
    inp = TC.inputs(KW, B, T)
    want = _one_pass(m, inp)
    _assert_same(_one_pass(m, inp, keep=[1, 1]), want)
    assert kind == "lora" or float(m.grad("external_cond.bias").abs().max()) > 0


@DTYPES
@HANDLES
def test_keep_all_zeros_is_the_plain_step_without_actions(dtype, kind):
    m = _model(dtype, kind)
    inp = TC.inputs(KW, B, T)
    want = _one_pass(m, inp, actions=False)
    _assert_same(_one_pass(m, inp, keep=[0, 0]), want)
    if kind != "lora":        # (a LoRA handle trains the adapters alone)
        assert float(m.grad("external_cond.weight").abs().max()) == 0 and float(m.grad("external_cond.bias").abs().max()) == 0


@DTYPES
@pytest.mark.parametrize("keep", [(1, 0), (0, 1, 0)], ids=["keep10", "keep010"])
def test_mixed_mask_against_the_per_sample_oracle(dtype, keep):
    n = len(keep)
    m = _model(dtype, n=n)
    v, _ = _one_pass(m, TC.inputs(KW, n, T), keep=list(keep))
    v_ref, grads = _oracle(keep)
    assert TC.rel_l2_logged(v, v_ref, "v_pred") < TC.FWD_TOL[dtype]
    errs = TC.grad_errors(m, grads)
    assert "external_cond.bias" in errs and "external_cond.weight" in errs
    worst = max(errs, key=errs.get)
    print(f"[action_keep {keep}] worst gradient {worst} {errs[worst]:.3e} ({errs[worst] / TC.GRAD_TOL[dtype]:.2f} of GRAD_TOL); external_cond.bias "
          f"{errs['external_cond.bias']:.3e}, external_cond.weight {errs['external_cond.weight']:.3e}")
    assert errs[worst] < TC.GRAD_TOL[dtype], (worst, errs[worst])
    # the kept sample alone fed external_cond: its bias gradient is not the all-kept one
    v1, g1 = _one_pass(m, TC.inputs(KW, n, T), keep=[1] * n)
    lo, cnt = m.param_range("external_cond.")
    hi = lo + cnt
    v, g = _one_pass(m, TC.inputs(KW, n, T), keep=list(keep))
    assert not torch.equal(g[lo:hi], g1[lo:hi]) and not torch.equal(v, v1)


@DTYPES
def test_mixed_mask_on_a_recompute_handle_is_bit_equal(dtype):
    inp = TC.inputs(KW, B, T)
    _assert_same(_one_pass(_model(dtype, "recompute"), inp, keep=[1, 0]), _one_pass(_model(dtype), inp, keep=[1, 0]))


def test_the_mask_needs_actions_and_one_flag_per_sample():
    m = _model(F16)
    x, t, a, vt = TC.inputs(KW, B, T)
    with pytest.raises(ValueError, match="without external_cond"):
        m.forward_train(x, t, None, action_keep=[1, 0])
    with pytest.raises(ValueError, match="3 flags for a batch of 2"):
        m.forward_train(x, t, a, action_keep=[1, 0, 1])


@DTYPES
def test_training_step_with_action_keep(dtype):
    from gtav_amd.train import draw_action_keep, training_step
    m = TC.model(KW, B, 5, dtype)
    lat, a, tgt, ctx, cn, nz = TC.clip(KW, B)
    g = torch.Generator().manual_seed(3)
    for step in range(3):
        keep = draw_action_keep(B, 0.5, g)
        loss = training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-4, weight_decay=0.01, max_grad_norm=1.0, action_keep=keep)
        assert torch.isfinite(loss).all(), step
        m.check()
    k1 = [draw_action_keep(16, 0.1, torch.Generator().manual_seed(7)) for _ in range(2)]
    assert torch.equal(k1[0], k1[1]) and k1[0].dtype == torch.int32 and set(k1[0].tolist()) <= {0, 1}
