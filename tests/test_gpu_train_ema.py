"""Averaged (EMA) weights kept inside the AdamW launch, on the GPU, in both operand types: DiT(trainable=True, train_ema_decay=d[, train_ema_warmup=True])
(include/gtav_amd.h gtav_dit_train_set_ema; DESIGN.md 7 "Averaged weights").  The toy model of tests/train_cases.py at B = 2, T = 3 throughout; the gradients
are the CPU oracle's, copied into the arena as tests/test_gpu_train.py test_adamw_step_matches_torch does, so every step moves every model alike.

The recurrence bound is derived, not tuned.  The device computes, per element and applied step, e' = fmaf(d, e, (1 - d) * w) in fp32 (train.hip ADAM_STEP_EMA):
C_ROUND = 3 roundings — 1 - d, the product, the fma — each at most 2^-24 of a value no larger than max(|e|, |w|), and an error already in e is multiplied by
d < 1.  So against the fp64 recurrence on the same fp32 masters |ema - e_K| <= C_ROUND 2^-24 sum_k max(|e_{k-1}|, |w_k|): one term per applied step, which is
tests/parity_bounds.py ema_step_bound (tests/test_gpu_ops_optimizer.py holds a single launch to the same term)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import parity_bounds as PB  # noqa: E402
import train_cases as TC  # noqa: E402
from train_cases import TOY_KW as KW  # noqa: E402

assert PB.EMA_ROUNDINGS == 3         # C_ROUND: DESIGN.md 7 "Averaged weights"
LR, WD, CLIP = 1e-3, 0.01, 1.0
GEMM_W = "blocks.0.s_mlp.fc1.weight"          # the largest GEMM weight of the toy model, [1024][256]
KW_EDGE = dict(KW, in_channels=4)             # 16 features per patch: x_embedder.proj.weight [256][16] and final_layer.linear.weight [16][256] are edge tiles


def _flat_grads(m, grads, names):
    flat = torch.cat([grads[k].reshape(-1) for k in names]) * m.loss_scale
    assert flat.numel() == m.grad_arena.numel()
    return flat.to(m.grad_arena.device)


def _step(m, flat, poison=False):
    m.grad_arena.copy_(flat)
    if poison:
        m.grad_arena[5] = float("inf")
    m.adamw_step(LR, weight_decay=WD, max_grad_norm=CLIP)


def _masters(m):
    """The fp32 masters of the trainable parameters, exact."""
    if m.lora_rank:
        return dict(m.lora_state_dict())
    m.pull_weights()
    return {k: m._sd[k] for k in m._train_shapes()}


def _ema(m):
    sd = m.ema_state_dict()
    return {k: sd[k] for k in m._train_shapes()}


def _equal(a, b):
    assert set(a) == set(b)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, bad[:5]


def _setup(kw, dtype, **dit_kwargs):
    """(model with its handle built, inputs, flat oracle gradients)"""
    sd, inp, _, _, grads = TC.oracle(kw, 2, 3, True)
    m = TC.model(kw, 2, 3, dtype, **dit_kwargs)
    m.forward_train(*inp[:3])                     # builds the handle
    names = sorted(k for k in sd if not k.endswith("freqs"))
    return m, inp, _flat_grads(m, grads, names)


def _recurrence(m, e0, flat, K, decay, warmup, big):
    """K applied steps; the shadow against the fp64 recurrence on the masters pulled after each step, within the derived per-element bound; and the bound is far
    below what a wrong update would show on the tensor `big`."""
    from gtav_amd.train import ema_decay_at
    names = list(m._train_shapes())
    e_ref = {k: e0[k].double() for k in names}
    bound = {k: torch.zeros_like(e_ref[k]) for k in names}
    _equal(_ema(m), {k: e0[k] for k in names})    # a freshly loaded model: ema = weights
    for n in range(1, K + 1):
        _step(m, flat)
        w = _masters(m)
        d = ema_decay_at(n, decay, warmup)        # float32(d_n) as a double; 1 - d below is then exact in fp64
        for k in names:
            wk = w[k].double()
            bound[k] += PB.ema_step_bound(e_ref[k], wk)
            e_ref[k] = d * e_ref[k] + (1.0 - d) * wk
    applied, skipped, _ = m.train_stats()
    assert applied and skipped == 0
    ema = _ema(m)
    worst = 0.0
    for k in names:
        err = (ema[k].double() - e_ref[k]).abs()
        over = err > bound[k]
        assert not over.any(), (k, float(err[over].max()), float(bound[k][over].min()))
        nz = bound[k] > 0
        if nz.any():
            worst = max(worst, float((err[nz] / bound[k][nz]).max()))
    print(f"[ema margin] worst |ema - ref| / bound = {worst:.3f}")
    # the test would see a wrong update: the shadow has moved from e_0 and lags the masters by far more than the bound
    bmax = float(bound[big].max())
    moved, lag = float((ema[big] - e0[big]).abs().max()), float((ema[big] - w[big]).abs().max())
    assert moved > 100 * bmax and lag > 100 * bmax, (moved, lag, bmax)
    return w, ema


# ---- 1. the recurrence -------------------------------------------------------------------------------------------------------------------------------------
@TC.DTYPES
@pytest.mark.parametrize("decay,warmup", [(0.9, False), (0.25, True)], ids=["d0.9", "warmup-d0.25"])
def test_recurrence(dtype, decay, warmup):
    m, _, flat = _setup(KW, dtype, train_ema_decay=decay, train_ema_warmup=warmup)
    assert m.ema_decay == decay
    _recurrence(m, TC.state_dict(KW), flat, 4, decay, warmup, GEMM_W)


@TC.DTYPES
def test_recurrence_edge_tiles(dtype):
    m, _, flat = _setup(KW_EDGE, dtype, train_ema_decay=0.9)
    _recurrence(m, TC.state_dict(KW_EDGE), flat, 4, 0.9, False, "x_embedder.proj.weight")


# ---- 2. the step itself is unchanged -----------------------------------------------------------------------------------------------------------------------
@TC.DTYPES
def test_the_step_is_unchanged(dtype):
    m, inp, flat = _setup(KW, dtype, train_ema_decay=0.9)
    p, _, _ = _setup(KW, dtype)
    for _ in range(4):
        _step(m, flat)
        _step(p, flat)
    assert m.train_stats() == p.train_stats()
    _equal(_masters(m), _masters(p))
    om, op = m.opt_state_dict(), p.opt_state_dict()
    _equal(om, op)
    assert int(om["step"][0]) == 4
    assert torch.equal(m.forward_train(*inp[:3]), p.forward_train(*inp[:3]))


# ---- 3. a skipped step -------------------------------------------------------------------------------------------------------------------------------------
@TC.DTYPES
def test_skipped_step_leaves_the_shadow_and_the_count(dtype):
    from gtav_amd.train import ema_decay_at
    m, _, flat = _setup(KW, dtype, train_ema_decay=0.9, train_ema_warmup=True)
    _step(m, flat)                                # n = 1
    w1, e1 = _masters(m), _ema(m)
    _step(m, flat, poison=True)
    applied, skipped, _ = m.train_stats()
    assert not applied and skipped == 1
    _equal(_ema(m), e1)
    _equal(_masters(m), w1)
    _step(m, flat)                                # n = 2: the skipped step consumed no n
    applied, skipped, _ = m.train_stats()
    assert applied and skipped == 1
    w2, e2 = _masters(m), _ema(m)
    d2, d3 = ema_decay_at(2, 0.9, True), ema_decay_at(3, 0.9, True)
    assert d2 == 0.25 and d3 > 0.3
    bmax = 0.0
    for k in e1:
        ref = d2 * e1[k].double() + (1.0 - d2) * w2[k].double()
        bound = PB.ema_step_bound(e1[k], w2[k])
        assert ((e2[k].double() - ref).abs() <= bound).all(), k
        if k == GEMM_W:
            bmax = float(bound.max())
    wrong = d3 * e1[GEMM_W].double() + (1.0 - d3) * w2[GEMM_W].double()      # what n = 3 would have given
    assert float((e2[GEMM_W].double() - wrong).abs().max()) > 100 * bmax


# ---- 4. the swap -------------------------------------------------------------------------------------------------------------------------------------------
def _plain(sd, dtype, groups=None):
    from gtav_amd.model.dit import DiT
    mi = DiT(**KW, max_batch=2, max_frames=3, init_weights=False)
    if dtype is TC.BF16:
        mi.set_operand_dtype(TC.BF16, groups)
    mi.load_state_dict(sd)
    return mi


def _swap_involution(m, inp, flat):
    """Into the context and out again: inside, the training step is refused by name; afterwards every bit is where it was."""
    from gtav_amd.lib import GtavError
    x, t, a, vt = inp
    w, e, opt = _masters(m), _ema(m), m.opt_state_dict()
    fwd = m(x, t, a).clone()
    v = m.forward_train(x, t, a)
    with m.ema_weights():
        inside = m(x, t, a).clone()
        for call in (lambda: m.forward_train(x, t, a), lambda: m.backward_(v, vt), lambda: _step(m, flat), lambda: m.ema_state_dict()):
            with pytest.raises(GtavError, match="swap"):
                call()
        with pytest.raises(GtavError, match="nest"):
            with m.ema_weights():
                pass
    _equal(_masters(m), w)
    _equal(_ema(m), e)
    _equal(m.opt_state_dict(), opt)
    assert torch.equal(m(x, t, a), fwd)
    assert not torch.equal(inside, fwd)
    m.check()
    return inside


@TC.DTYPES
def test_swap(dtype):
    m, inp, flat = _setup(KW, dtype, train_ema_decay=0.9)
    u, _, _ = _setup(KW, dtype, train_ema_decay=0.9)      # the uninterrupted run
    for _ in range(2):
        _step(m, flat)
        _step(u, flat)
    ema_sd = m.ema_state_dict()
    assert set(ema_sd) == set(m.state_dict())             # the reference's key layout
    inside = _swap_involution(m, inp, flat)
    assert torch.equal(inside, _plain(ema_sd, dtype)(*inp[:3]))
    for _ in range(2):
        _step(m, flat)
        _step(u, flat)
    _equal(_masters(m), _masters(u))
    _equal(_ema(m), _ema(u))
    _equal(m.opt_state_dict(), u.opt_state_dict())
    assert torch.equal(m.forward_train(*inp[:3]), u.forward_train(*inp[:3]))


# ---- 5. checkpoint -----------------------------------------------------------------------------------------------------------------------------------------
@TC.DTYPES
def test_checkpoint_round_trip(dtype, tmp_path):
    import json
    import os
    from gtav_amd.train import load_state, save_state
    m, _, flat = _setup(KW, dtype, train_ema_decay=0.9, train_ema_warmup=True)
    for _ in range(2):
        _step(m, flat)
    save_state(m, str(tmp_path / "ck"), 2, 0)
    assert os.path.exists(tmp_path / "ck" / "ema.safetensors")
    assert json.load(open(tmp_path / "ck" / "step.json"))["ema"] == {"decay": 0.9, "warmup": True}
    r = TC.model(KW, 2, 3, dtype, sd=TC.state_dict(KW, 2), train_ema_decay=0.9, train_ema_warmup=True)
    load_state(r, str(tmp_path / "ck"))
    _equal(_ema(r), _ema(m))
    _equal(_masters(r), _masters(m))
    _step(m, flat)
    _step(r, flat)                                # n = 3 on both: the count came with the optimizer state
    _equal(_ema(r), _ema(m))
    _equal(_masters(r), _masters(m))
    # a model without a shadow ignores the file ...
    p = TC.model(KW, 2, 3, dtype, sd=TC.state_dict(KW, 2))
    load_state(p, str(tmp_path / "ck"))
    # ... and what it writes loads into a model with one as ema = weights
    save_state(p, str(tmp_path / "plain"), 2, 0)
    assert not os.path.exists(tmp_path / "plain" / "ema.safetensors")
    r2 = TC.model(KW, 2, 3, dtype, sd=TC.state_dict(KW, 2), train_ema_decay=0.9)
    load_state(r2, str(tmp_path / "plain"))
    _equal(_ema(r2), _masters(r2))
    _equal(_masters(r2), _masters(p))


# ---- 6. LoRA: the average is over the adapters -------------------------------------------------------------------------------------------------------------
@TC.DTYPES
def test_lora_recurrence_and_swap(dtype):
    import test_gpu_train_lora as TL
    rank = 16
    inp, _, grads = TL.lora_oracle(2, 3, True, rank)
    m = TL.lora_model(2, 3, dtype, rank, train_ema_decay=0.9)
    m.forward_train(*inp[:3])
    flat = _flat_grads(m, grads, sorted(grads))
    _recurrence(m, TL.adapters(rank), flat, 4, 0.9, False, "blocks.0.s_mlp.fc1.lora_B.weight")
    ema = m.ema_state_dict()
    assert set(ema) == set(TL.adapters(rank))     # the adapter keys
    fwd = m(*inp[:3]).clone()
    with m.ema_weights():
        inside = m(*inp[:3]).clone()
        merged = m.merged_state_dict()
    assert torch.equal(inside, _plain(merged, dtype)(*inp[:3]))
    assert torch.equal(m(*inp[:3]), fwd) and not torch.equal(inside, fwd)
    _equal(_ema(m), ema)


# ---- 7. mixed operand groups -------------------------------------------------------------------------------------------------------------------------------
def test_mixed_groups_recurrence_and_swap():
    m, inp, flat = _setup(KW, TC.F16, train_range_policy="auto", train_ema_decay=0.9)
    m.train_set_group_dtype(TC.BF16, [0])
    assert m.operand_dtypes()[0] == TC.BF16 and m.operand_dtypes()[1] == TC.F16
    _recurrence(m, TC.state_dict(KW), flat, 4, 0.9, False, GEMM_W)
    _swap_involution(m, inp, flat)
