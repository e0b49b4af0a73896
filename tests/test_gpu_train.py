"""SURVEY.md 8(f)1 — DiT training step on the GPU against torch autograd / torch.optim on the CPU oracle.
Tolerances: the backward pass is mixed precision like the reference's own (fp16 operands here, bf16 autocast there, fp32 master
weights and gradients in both), so parameter gradients are compared by relative L2 per tensor: <= 6e-3 for every tensor
(measured 3e-4 .. 3.5e-3, profiles/round2/train_grad_parity.txt and `pytest -s`); AdamW updates of a step <= 2e-2 of the update's norm."""
import math

import pytest
import torch

import train_cases as TC
from helpers import dev
from helpers import rel_l2_logged as rel_l2       # (-s shows the measured margins)
from train_cases import TOY_KW as KW

pytestmark = pytest.mark.gpu

GRAD_TOL, FWD_TOL = TC.GRAD_TOL[TC.F16], TC.FWD_TOL[TC.F16]


def _setup(B=2, T=3, actions=True, seed=0):
    x, t, a, vt = TC.inputs(KW, B, T, actions, seed)
    return TC.model(KW, B, T), TC.state_dict(KW), x, t, a, vt


@pytest.mark.parametrize("actions", [True, False])
def test_gradients_match_autograd(actions):
    _, (x, t, a, vt), _, v_ref, grads = TC.oracle(KW, 2, 3, actions)
    m = TC.model(KW, 2, 3)
    v = m.forward_train(x, t, a)
    assert rel_l2(v, v_ref) < FWD_TOL
    # same function as the inference forward; the MLP's GELU is applied to the fp16-rounded pre-activation (kept for gelu') instead
    # of the fp32 accumulator, hence not bit-identical (measured 4.6e-4)
    assert rel_l2(m(x, t, a), v.cpu()) < 1.5e-3
    m.zero_grad()
    m.backward_(v, vt)
    m.check()
    worst = TC.grad_errors(m, grads, log=True)
    bad = {k: v_ for k, v_ in worst.items() if v_ > GRAD_TOL}
    assert not bad, f"gradient mismatch: {bad}"


def test_backward_accumulates_and_zero_grad_clears():
    m, sd, x, t, a, vt = _setup()
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    g1 = m.grad_arena.clone()
    m.backward_(v, vt)
    assert rel_l2(m.grad_arena, 2 * g1) < 1e-5
    m.zero_grad()
    assert float(m.grad_arena.abs().max()) == 0.0


def test_adamw_step_matches_torch():
    """clip_grad_norm_ + AdamW against torch.optim.AdamW on IDENTICAL gradients (the oracle's, written into the gradient arena in
    its documented order: parameters by lexicographic name): three steps, updates equal to fp32 rounding.  (With each side's own
    gradients the first Adam step is sign(g) * lr per element, so a single element whose tiny gradient differs in sign dominates any
    norm: that comparison says nothing about the optimizer.)"""
    from oracle import ref_cpu as O
    sd, (x, t, a, vt), _, _, grads = TC.oracle(KW, 2, 3, True)
    m = TC.model(KW, 2, 3)
    params = {k: v for k, v in sd.items() if not k.endswith("freqs")}
    steps = 3
    ref, norm_ref = O.adamw_reference(params, grads, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0, steps=steps)
    m.forward_train(x, t, a)                      # builds the handle
    flat = torch.cat([grads[k].reshape(-1) for k in sorted(params)]) * m.loss_scale
    assert flat.numel() == m.grad_arena.numel()
    for _ in range(steps):
        m.grad_arena.copy_(flat.to(m.grad_arena.device))
        m.adamw_step(1e-3, weight_decay=0.01, max_grad_norm=1.0)
    applied, skipped, norm = m.train_stats()
    assert applied and skipped == 0
    assert abs(norm - float(norm_ref)) / float(norm_ref) < 1e-5
    m.pull_weights()
    for k in params:
        upd_ref = ref[k] - params[k]
        upd = m._sd[k] - params[k]
        assert rel_l2(upd, upd_ref) < 1e-4, (k, rel_l2(upd, upd_ref))
    # the refreshed fp16 operands (W and W^T) are what the next forward / backward use: both must match the oracle at the UPDATED weights
    sd2 = dict(sd)
    sd2.update(ref)
    _, v2_ref, grads2 = O.dit_loss_and_grads(sd2, O.DiTConfig(**KW), x, t, a, vt)
    v2 = m.forward_train(x, t, a)
    assert rel_l2(v2, v2_ref) < FWD_TOL
    m.zero_grad()
    m.backward_(v2, vt)
    for k in ("blocks.1.t_mlp.fc1.weight", "blocks.0.s_attn.to_qkv.weight", "t_embedder.mlp.0.weight", "x_embedder.proj.weight"):
        assert rel_l2(m.grad(k), grads2[k]) < GRAD_TOL, k


@TC.DTYPES
def test_images_after_a_step_are_the_images_of_the_pulled_masters(dtype):
    """One applied step, pull_weights, and a FRESH training handle loaded with those masters: the same forward bits and the same gradient arena bits for the same
    batch.  The stepped handle computes with the W and W^T images the AdamW launch wrote, the fresh one with what the converters make of the masters: equal
    results tie both images of the real parameter list to their masters (kernel level: tests/test_gpu_ops_optimizer.py)."""
    sd, (x, t, a, vt), _, _, grads = TC.oracle(KW, 2, 3, True)
    m = TC.model(KW, 2, 3, dtype)
    m.forward_train(x, t, a)                      # builds the handle
    flat = torch.cat([grads[k].reshape(-1) for k in sorted(k for k in sd if not k.endswith("freqs"))]) * m.loss_scale
    m.grad_arena.copy_(flat.to(m.grad_arena.device))
    m.adamw_step(1e-3, weight_decay=0.01, max_grad_norm=1.0)
    applied, skipped, _ = m.train_stats()
    assert applied and skipped == 0
    m.pull_weights()
    stepped = {k: v.clone() for k, v in m._sd.items()}
    assert not torch.equal(stepped["blocks.0.s_mlp.fc1.weight"], sd["blocks.0.s_mlp.fc1.weight"])
    fresh = TC.model(KW, 2, 3, dtype, sd=stepped)
    out = []
    for h in (m, fresh):
        v = h.forward_train(x, t, a)
        h.zero_grad()
        h.backward_(v, vt)
        h.check()
        out.append((v.float().cpu().clone(), h.grad_arena.cpu().clone()))
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32))
    assert torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32))


def test_overflow_skips_the_step():
    m, sd, x, t, a, vt = _setup()
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    m.grad_arena[5] = float("inf")
    before = m.grad("final_layer.linear.weight")  # noqa: F841  (forces a stream sync point)
    m.adamw_step(1e-3, weight_decay=0.01, max_grad_norm=1.0)
    applied, skipped, _ = m.train_stats()
    assert not applied and skipped == 1
    m.pull_weights()
    assert torch.equal(m._sd["blocks.0.s_mlp.fc1.bias"], sd["blocks.0.s_mlp.fc1.bias"])


def test_training_step_reduces_the_loss():
    from gtav_amd.train import training_step
    m = TC.model(KW, 2, 5)
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    losses = [float(training_step(m, lat, a.new_zeros(2, 5, 25), tgt, ctx, cn, nz, lr=2e-4, weight_decay=0.0, max_grad_norm=1.0)) for _ in range(8)]
    assert all(math.isfinite(l) for l in losses)
    assert losses[-1] < losses[0] * 0.9, losses


def test_comm_c_abi_single_rank():
    """gtav_comm_* (RCCL opened at run time) on a communicator of one rank: id, init, all-reduce (sum and average are the identity),
    all-gather (rank 0's bytes at slot 0).  The multi-rank arithmetic is RCCL's; what is checked here is the binding."""
    from gtav_amd.comm import Comm
    torch.cuda.set_device(0)
    c = Comm(1, 0, Comm.unique_id())
    t = torch.arange(1000, device=dev(), dtype=torch.float32)
    ref = t.clone()
    c.all_reduce_(t)
    c.all_reduce_(t, average=True)
    g = c.all_gather(t.half())
    torch.cuda.synchronize()
    assert torch.equal(t, ref) and g.shape == (1, 1000) and torch.equal(g[0], ref.half())
    c.close()


def test_full_size_gradients_match_autograd():
    """DiT-S/2 at its real size (depth 16, hidden 1024, 18 x 32 latents; B = 1, T = 5 with actions: M = 720 tokens, the shapes the
    loader-wave GEMM, the split-K residual GEMMs and the 144-token spatial attention backward run in production)."""
    import gtav_amd.weights as W
    from gtav_amd.model.dit import DiT_models
    from oracle import ref_cpu as O
    sd = W.synth_state_dict(W.dit_param_shapes(depth=16), seed=0)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 5, 16, 18, 32, generator=g) * 0.7
    t = torch.tensor([[15, 15, 15, 15, 420]])
    a = torch.zeros(1, 5, 25)
    a[:, :, 3] = 1
    vt = torch.randn(1, 1, 16, 18, 32, generator=g)
    torch.set_num_threads(16)
    _, v_ref, grads = O.dit_loss_and_grads(sd, O.dit_s_2(), x, t, a, vt)
    m = DiT_models["DiT-S/2"](init_weights=False, max_batch=1, trainable=True)
    m.load_state_dict(sd)
    v = m.forward_train(x, t, a)
    assert rel_l2(v, v_ref) < 1e-3
    m.zero_grad()
    m.backward_(v, vt)
    m.check()
    keys = ["x_embedder.proj.weight", "t_embedder.mlp.0.weight", "external_cond.weight", "blocks.0.s_attn.to_qkv.weight", "blocks.0.t_attn.to_out.weight",
            "blocks.7.s_mlp.fc1.weight", "blocks.7.t_mlp.fc2.weight", "blocks.7.t_adaLN_modulation.1.weight", "blocks.15.t_attn.to_qkv.weight",
            "blocks.15.s_mlp.fc2.bias", "final_layer.linear.weight", "final_layer.adaLN_modulation.1.bias"]
    worst = {k: rel_l2(m.grad(k), grads[k]) for k in keys}
    assert max(worst.values()) < GRAD_TOL, worst


@pytest.mark.parametrize("B,T", [(3, 5), (4, 4)])
def test_full_size_gradients_grouped_weight_gradient_launch(B, T):
    """DiT-S/2 at its real size with B = 3 clips (M = 2160 tokens): from 2048 tokens on the four weight gradients of a half-block run as ONE
    grouped launch of 256 x 256 tiles (gemm.h launch_gemm_dw_grouped, 192 tiles) instead of four launches of 128 x 128 tiles — every Linear
    weight gradient of the first, a middle and the last block against torch autograd, and two backward passes bit-identical.
    B = 4, T = 4 (M = 2304 = 18 whole 128-token row tiles): the transpose-free form of that launch (mainloop256_tn: the contraction runs over the rows of the
    tile-major activations themselves); M = 2160 has a ragged last row tile and goes through the transposed copies."""
    import gtav_amd.weights as W
    from gtav_amd.model.dit import DiT_models
    from oracle import ref_cpu as O
    sd = W.synth_state_dict(W.dit_param_shapes(depth=16), seed=0)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, T, 16, 18, 32, generator=g) * 0.7
    t = torch.full((B, T), 15, dtype=torch.long)
    t[:, -1] = torch.tensor([420, 77, 901, 333][:B])
    a = torch.zeros(B, T, 25)
    a[torch.arange(B)[:, None], torch.arange(T)[None], torch.randint(0, 25, (B, T), generator=g)] = 1
    vt = torch.randn(B, 1, 16, 18, 32, generator=g)
    torch.set_num_threads(16)
    _, v_ref, grads = O.dit_loss_and_grads(sd, O.dit_s_2(), x, t, a, vt)
    m = DiT_models["DiT-S/2"](init_weights=False, max_batch=B, trainable=True)
    m.load_state_dict(sd)
    v = m.forward_train(x, t, a)
    assert rel_l2(v, v_ref) < 1e-3
    keys = [f"blocks.{l}.{h}_{n}.weight" for l in (0, 7, 15) for h in "st" for n in ("attn.to_qkv", "attn.to_out", "mlp.fc1", "mlp.fc2")]
    # ... and what the fused elementwise backward kernels produce at this width (bias gradients from the gate / GELU passes, adaLN gradients from the LayerNorm pass)
    keys += ["blocks.7.s_mlp.fc1.bias", "blocks.7.t_mlp.fc2.bias", "blocks.7.t_attn.to_out.bias", "blocks.0.s_adaLN_modulation.1.weight", "blocks.15.t_adaLN_modulation.1.bias"]
    runs = []
    for _ in range(2):
        m.zero_grad()
        m.backward_(v, vt)
        m.check()
        runs.append({k: m.grad(k).clone() for k in keys})
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in keys)
    worst = {k: rel_l2(runs[0][k], grads[k]) for k in keys}
    print("worst weight-gradient error:", max(worst.values()))
    assert max(worst.values()) < GRAD_TOL, worst


def test_plain_forward_of_a_trainable_handle_at_large_m_equals_the_inference_handle():
    """at M >= 3649 tokens the plain forward (gtav_dit_forward) of a TRAINABLE handle takes the in-place residual epilogue of the persistent kernel
    (EPI_RESID, csrc/api_dit.hip resid_gemm) like an inference handle does — it keeps no activations, so nothing of the training path depends on the slabs — and
    must return the same bits.  DiT-S/2, B = 8, T = 5 (M = 5 760); forward_train on the same inputs agrees to rounding (it runs the slab path)."""
    import gtav_amd.weights as W
    from gtav_amd.model.dit import DiT_models
    B, T = 8, 5
    sd = W.synth_state_dict(W.dit_param_shapes(depth=16), seed=0)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, T, 16, 18, 32, generator=g) * 0.6
    t = torch.randint(0, 1000, (B, T), generator=g)
    a = torch.zeros(B, T, 25)
    a[:, :, 3] = 1
    mi = DiT_models["DiT-S/2"](init_weights=False, max_batch=B)
    mi.load_state_dict(sd)
    ref = mi(x, t, a).clone()
    mi.check()
    del mi
    torch.cuda.empty_cache()
    mt = DiT_models["DiT-S/2"](init_weights=False, max_batch=B, trainable=True)
    mt.load_state_dict(sd)
    out = mt(x, t, a).clone()
    mt.check()
    assert torch.equal(out, ref)
    vt = mt.forward_train(x, t, a)
    assert rel_l2(vt, ref) < 1.5e-3               # (the slab path: other fp16 roundings of the stored activations than the in-place path — measured 6.2e-4; each is within 1e-3 of the oracle)
    assert torch.equal(mt(x, t, a), ref)          # the saved activations of forward_train do not disturb a later plain forward


@pytest.mark.parametrize("B,T", [(1, 1), (3, 2), (1, 5), (5, 5)])
def test_gradients_other_windows(B, T):
    """Windows of 1, 2 and 5 frames (the temporal attention backward is specialised per window length; T = 1 has one key per query);
    B = 5, T = 5 gives 25 conditioning rows: two ragged 16-row tiles in the fp32-MFMA adaLN backward kernels."""
    _, inp, _, v_ref, grads = TC.oracle(KW, B, T, True)
    m = TC.model(KW, B, T)
    v = TC.forward_backward(m, inp)
    assert rel_l2(v, v_ref) < FWD_TOL
    worst = TC.grad_errors(m, grads, log=True)
    assert max(worst.values()) < GRAD_TOL, {k: v_ for k, v_ in worst.items() if v_ > GRAD_TOL}


def test_loss_scale_is_transparent_and_micro_batches_accumulate():
    """(1) The unscaled gradients do not depend on the loss scale (256 vs 65536) beyond fp16 rounding.  (2) Two micro-batches with
    per-micro-batch mean losses accumulate to twice the gradient of... each its own loss: g(b0) + g(b1) equals the sum of separate runs
    (what gradient_accumulation_steps relies on, train_dit.py:676-680)."""
    m, sd, x, t, a, vt = _setup(B=2, T=3)
    key = "blocks.1.s_mlp.fc1.weight"
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    g_hi = m.grad(key).clone()
    m.loss_scale = 256.0
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    g_lo = m.grad(key).clone()
    assert rel_l2(g_lo, g_hi) < 5e-3
    m.loss_scale = 65536.0
    parts = []
    for b in range(2):
        vb = m.forward_train(x[b:b + 1], t[b:b + 1], a[b:b + 1])
        m.zero_grad()
        m.backward_(vb, vt[b:b + 1])
        parts.append(m.grad(key).clone())
    m.zero_grad()
    for b in range(2):
        vb = m.forward_train(x[b:b + 1], t[b:b + 1], a[b:b + 1])
        m.backward_(vb, vt[b:b + 1])
    assert rel_l2(m.grad(key), parts[0] + parts[1]) < 1e-5
    # and the batch-of-two gradient is the mean of the two single-sample gradients (mse 'mean' over B n elements)
    assert rel_l2(g_hi, 0.5 * (parts[0] + parts[1])) < 5e-3


def test_gradients_match_reference_fixture_g8():
    """HIP gradients against tests/golden/g8_training.safetensors directly — autograd through the REFERENCE's own DiT module
    (tools/make_golden.py g8_training), no oracle in between: per-parameter gradient norms within 1 %, the stored elements of every
    gradient within 1e-2 relative L2, the global (clipping) norm within 0.5 %."""
    import os
    from safetensors.torch import load_file
    g = load_file(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g8_training.safetensors"))
    sd = TC.state_dict(KW, 3)
    m = TC.model(KW, 2, 3, sd=sd)
    v = m.forward_train(g["x"], g["t"], g["actions"])
    assert rel_l2(v, g["v_pred"]) < FWD_TOL
    m.zero_grad()
    m.backward_(v, g["v_target"])
    m.check()
    names = sorted(k for k in sd if not k.endswith("freqs"))
    assert len(names) == int(g["names_check"])
    sel = lambda t_: t_.reshape(-1) if t_.numel() <= 4096 else t_.reshape(-1)[::97]
    norms = torch.stack([m.grad(k).norm().cpu() for k in names])
    assert float(((norms - g["grad_norms"]).abs() / g["grad_norms"]).max()) < GRAD_TOL
    for k in names:
        assert rel_l2(sel(m.grad(k).cpu()), g["grad." + k]) < GRAD_TOL, k
    m.adamw_step(1e-3, weight_decay=0.01, max_grad_norm=1.0)
    applied, _, total = m.train_stats()
    assert applied and abs(total - float(g["total_grad_norm"])) < 5e-3 * float(g["total_grad_norm"])


def test_per_block_residual_taps_match_reference_fixture_g2():
    """The residual stream after every block on the GPU against the reference's own block outputs (forward hooks on model.blocks[i],
    tests/golden/g2_small_dit.safetensors): per-block parity, not only end-to-end."""
    import os
    from safetensors.torch import load_file
    g = load_file(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g2_small_dit.safetensors"))
    m = TC.model(KW, 2, 3, sd=TC.state_dict(KW, 3))
    v = m.forward_train(g["x"], g["t"], g["actions"])
    assert rel_l2(v, g["out_actions"]) < 1e-3
    for i in range(2):
        assert rel_l2(m.residual_after(4 * (i + 1), 2, 3), g[f"block{i}_actions"]) < 1e-3, i


def test_phased_backward_equals_monolithic_and_buckets_cover_the_arena():
    """gtav_dit_train_backward_phases one phase at a time gives the single call's gradients (to fp32 rounding: bias gradients and the
    conditioning path accumulate with float atomics, whose order is not fixed); the all-reduce buckets
    (final layer, one per block in reverse, embedders) are disjoint, contiguous and cover the arena; each bucket's gradients are final
    after the phase it is attached to (later phases do not touch them)."""
    from gtav_amd.train import gradient_buckets
    m, sd, x, t, a, vt = _setup()
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    whole = m.grad_arena.clone()
    m.zero_grad()
    buckets = gradient_buckets(m)
    spans = sorted((off, off + cnt) for _, off, cnt in buckets)
    assert spans[0][0] == 0 and spans[-1][1] == m.grad_arena.numel() and all(a_[1] == b_[0] for a_, b_ in zip(spans, spans[1:]))
    L = m.depth
    for phase in range(L + 2):
        m.backward_phases_(v, vt, phase, phase + 1)
        for ph, off, cnt in buckets:
            if ph == phase:
                assert rel_l2(m.grad_arena[off: off + cnt], whole[off: off + cnt]) < 1e-6, (phase, off)
    assert rel_l2(m.grad_arena, whole) < 1e-6


def test_overlapped_all_reduce_path_single_rank_process_group():
    """backward_overlapped with a real process group (RCCL, world size 1 on this one-GPU box) forced through the multi-rank code path
    (world_size=2 arithmetic with an all-reduce that doubles, standing in for a second rank with identical gradients): events, the
    communication stream, bucket slicing and the final averaging; result = the plain backward's gradients."""
    import os
    import torch.distributed as dist
    from gtav_amd.train import backward_overlapped
    m, sd, x, t, a, vt = _setup()
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    whole = m.grad_arena.clone()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29571")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev())
    try:
        def fake_two_rank_sum(tensor):
            dist.all_reduce(tensor, op=dist.ReduceOp.SUM)      # the real collective on this rank's slice (identity at world size 1) ...
            tensor.mul_(2.0)                                   # ... plus the contribution of an identical second rank
        m.zero_grad()
        backward_overlapped(m, v, vt, world_size=2, all_reduce=fake_two_rank_sum)
        torch.cuda.synchronize()
        assert m.grad_divisor == 2.0                                  # the arena holds the SUM over the ranks; the optimizer divides
        assert rel_l2(m.grad_arena / m.grad_divisor, whole) < 1e-6
        m.grad_divisor = 1.0
    finally:
        if created:
            dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------------------------
# round 3: checkpoint / resume (train_dit.py:765-849), overflow by fp16 saturation, the general frame loop
# ------------------------------------------------------------------------------------------------------------------------
def test_save_state_load_state_resumes_bit_exactly(tmp_path):
    """accelerator.save_state / load_state (train_dit.py:765-849): three optimisation steps straight == two steps, save_state, a FRESH
    model (new handle: masters, AdamW moments, step counters, loss scale restored through the C-ABI), load_state, one more step — the
    weights must be EQUAL bit for bit, and step.json carries step / epoch / skip_iter like the reference's load_checkpoint."""
    from gtav_amd.model.dit import DiT
    from gtav_amd.train import load_state, save_state, training_step
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    kw = dict(lr=3e-4, weight_decay=0.01, max_grad_norm=1.0)
    m1 = TC.model(KW, 2, 5)
    for _ in range(3):
        training_step(m1, lat, a, tgt, ctx, cn, nz, **kw)
    m1.pull_weights()
    straight = {k: v.clone() for k, v in m1._sd.items()}
    m2 = TC.model(KW, 2, 5)
    for _ in range(2):
        training_step(m2, lat, a, tgt, ctx, cn, nz, **kw)
    ck = str(tmp_path / "train_checkpoints" / "dit_last")
    save_state(m2, ck, global_step=2, epoch=0)
    opt = m2.opt_state_dict()
    assert int(opt["step"][0]) == 2 and int(opt["step"][1]) == 0 and float(opt["v.blocks.0.s_mlp.fc1.weight"].abs().max()) > 0
    del m2
    m3 = DiT(**KW, max_batch=2, max_frames=5, init_weights=True, trainable=True)         # other weights until load_state
    st = load_state(m3, ck, steps_per_epoch=7, gradient_accumulation_steps=4)
    assert st["step"] == 2 and st["epoch"] == 0 and st["skip_iter"] == 8
    training_step(m3, lat, a, tgt, ctx, cn, nz, **kw)
    m3.pull_weights()
    for k in straight:
        assert torch.equal(m3._sd[k], straight[k]), k
    applied, skipped, _ = m3.train_stats()
    assert applied and skipped == 0 and int(m3.opt_state_dict()["step"][0]) == 3


def test_fp16_saturation_skips_the_step_and_loss_scaler_backs_off():
    """every fp16 gradient store saturates to +-65504, so an overflow at a too-large loss scale never makes the gradient norm
    non-finite — the saturation bit of the handle's error word is what skips the step.  A loss scale of 2^40 saturates the activation
    gradients: the step is skipped on the device (weights, moments, Adam step count untouched), the bit is consumed (check() is clean),
    and LossScaler halves the scale until steps apply again."""
    from gtav_amd.train import LossScaler, training_step
    m, sd, x, t, a, vt = _setup(B=2, T=5)
    lat, a5, tgt, ctx, cn, nz = TC.clip(KW)
    m.loss_scale = 2.0 ** 40
    training_step(m, lat, a5, tgt, ctx, cn, nz, lr=1e-3)
    applied, skipped, gnorm = m.train_stats()
    # (round 4: the backward pass turns the saturation bit into +inf in one gradient element — the form every data-parallel rank sees after the
    # all-reduce — so the reported norm of an overflowed step is inf)
    assert not applied and skipped == 1 and math.isinf(gnorm)
    assert int(m.opt_state_dict()["step"][0]) == 0                      # the Adam step count did not advance
    m.pull_weights()
    assert torch.equal(m._sd["blocks.0.s_mlp.fc1.weight"], sd["blocks.0.s_mlp.fc1.weight"])
    m.check()                                                           # the overflow bit was consumed by the step
    sc = LossScaler(m, check_every=1, growth_interval=1 << 30)
    for _ in range(40):
        training_step(m, lat, a5, tgt, ctx, cn, nz, lr=1e-3)
        sc.update()
        if m.train_stats()[0]:
            break
    assert m.train_stats()[0] and m.loss_scale < 2.0 ** 40
    assert int(m.opt_state_dict()["step"][0]) >= 1


def test_overflow_on_one_rank_skips_the_step_on_every_rank():
    """the skip decision of the optimizer step must be global.  Two data-parallel replicas emulated in one process (two handles,
    identical weights, the all-reduce SUM done by hand on the two gradient arenas): only replica A's inputs saturate its fp16 gradient stores.
    Its backward pass publishes the overflow as +inf in its arena, so after the "all-reduce" BOTH replicas see a non-finite norm and skip: weights
    bit-equal afterwards, Adam step counts equal, both skip counters 1.  (Round 3 tested the saturation bit per rank: A skipped, B stepped.)"""
    from gtav_amd.train import forward_loss
    lat, a5, tgt, ctx, cn, nz = TC.clip(KW)
    reps = [TC.model(KW, 2, 5) for _ in range(2)]
    lats = [lat * 3e4, lat]            # replica A: latents far outside the fp16 range of the activation gradients at the default loss scale
    for m, l in zip(reps, lats):
        m.zero_grad()
        forward_loss(m, l, a5, tgt, ctx, cn, nz, keep_activations=True, on_frame=lambda k, vp, vt, m=m: m.backward_(vp, vt))
    total = reps[0].grad_arena + reps[1].grad_arena          # what ncclAllReduce(SUM) leaves on every rank
    assert not torch.isfinite(total).all() and torch.isfinite(reps[1].grad_arena).all()
    for m in reps:
        m.grad_arena.copy_(total)
        m.grad_divisor = 2.0
        m.adamw_step(1e-3, weight_decay=0.01, max_grad_norm=1.0)
    stats = [m.train_stats() for m in reps]
    assert [bool(s[0]) for s in stats] == [False, False] and [s[1] for s in stats] == [1, 1]
    for m in reps:
        m.pull_weights()
    for k in reps[0]._sd:
        assert torch.equal(reps[0]._sd[k], reps[1]._sd[k]), k
    assert int(reps[0].opt_state_dict()["step"][0]) == int(reps[1].opt_state_dict()["step"][0]) == 0
    # and a clean step afterwards applies on both, identically
    for m in reps:
        m.zero_grad()
        forward_loss(m, lat, a5, tgt, ctx, cn, nz, keep_activations=True, on_frame=lambda k, vp, vt, m=m: m.backward_(vp, vt))
    total = reps[0].grad_arena + reps[1].grad_arena
    for m in reps:
        m.grad_arena.copy_(total)
        m.adamw_step(1e-3, weight_decay=0.01, max_grad_norm=1.0)
        m.pull_weights()
    assert all(m.train_stats()[0] for m in reps)
    for k in reps[0]._sd:
        assert torch.equal(reps[0]._sd[k], reps[1]._sd[k]), k


def test_frame_loop_three_target_frames_vs_reference_fixture_g10():
    """train.forward_loss on 7-frame clips (three target frames, 5-frame windows sliding; train_dit.py:590-682) against fixture G10 (the
    reference's statements on the reference DiT module): every target frame's v_pred / v_target, the per-frame losses through on_frame,
    the returned mean loss; and training_step differentiates every frame's loss (gradients add up over the frame loop)."""
    import os
    from safetensors.torch import load_file
    from gtav_amd.train import forward_loss, training_step
    g = load_file(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_frame_loop.safetensors"))
    m = TC.model(KW, 2, 5, sd=TC.state_dict(KW, 17))
    seen = {}

    def on_frame(k, v_pred, v_target):
        seen[k] = (v_pred.clone(), v_target.clone())
    cns, nzs = [g[f"ctx_noise{k}"] for k in range(3)], [g[f"noise{k}"] for k in range(3)]
    loss, vp, vt = forward_loss(m, g["latents"], g["actions"], g["target_idx"], g["ctx_idx"], cns, nzs, on_frame=on_frame)
    assert sorted(seen) == [0, 1, 2]
    for k in range(3):
        assert rel_l2(seen[k][1], g[f"v_target{k}"]) < 1e-6
        assert rel_l2(seen[k][0], g[f"v_pred{k}"]) < FWD_TOL
    assert abs(float(loss) - float(g["mean_loss"])) / float(g["mean_loss"]) < 2e-3
    # gradients of the three frames add up: one training_step == three backward passes accumulated
    m.zero_grad()
    for k in range(3):
        _, v, t_ = forward_loss(m, g["latents"][:, : 5 + k], g["actions"][:, : 5 + k], g["target_idx"][k], g["ctx_idx"][k], cns[k], nzs[k],
                                n_prompt_frames=4 + k, keep_activations=True)
        m.backward_(v, t_)
    acc = m.grad_arena.clone()
    training_step(m, g["latents"], g["actions"], g["target_idx"], g["ctx_idx"], cns, nzs, lr=0.0, max_grad_norm=0.0)
    assert rel_l2(m.grad_arena, acc) < 1e-5


def test_trainable_model_refuses_to_grow_before_destroying_its_state():
    """a trainable DiT that would have to grow its workspace (predict on the training model with more conditioning rows than
    reserved) must raise BEFORE the handle — the only home of the fp32 masters and the AdamW state — is destroyed, and stay usable."""
    from gtav_amd.train import training_step
    m, sd, x, t, a, vt = _setup(B=2, T=5)
    lat, a5, tgt, ctx, cn, nz = TC.clip(KW)
    training_step(m, lat, a5, tgt, ctx, cn, nz, lr=1e-4)
    with pytest.raises(RuntimeError, match="cannot grow"):
        m.reserve(4, 5, noise_steps=50)
    with pytest.raises(RuntimeError, match="cannot grow"):
        m(torch.randn(3, 5, 16, 8, 16), torch.zeros(3, 5, dtype=torch.long), None)
    training_step(m, lat, a5, tgt, ctx, cn, nz, lr=1e-4)                # same handle, state intact
    assert int(m.opt_state_dict()["step"][0]) == 2


def test_comm_from_torch_distributed_and_bucket_order_single_rank():
    """Multi-GPU readiness on the one-GPU box: the buckets of backward_overlapped are issued in the order their
    gradients become final (final layer, blocks depth-1 .. 0, embedders), every one exactly once, through gtav_amd.comm.Comm's all-reduce
    on a one-rank RCCL communicator; the arena afterwards equals the plain backward's."""
    from gtav_amd.comm import Comm
    from gtav_amd.train import backward_overlapped, gradient_buckets
    m, sd, x, t, a, vt = _setup()
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    whole = m.grad_arena.clone()
    comm = Comm(1, 0, Comm.unique_id())
    calls = []

    def ar(tensor):
        calls.append((tensor.data_ptr() - m.grad_arena.data_ptr()) // 4)
        comm.all_reduce_(tensor)
    m.zero_grad()
    backward_overlapped(m, v, vt, world_size=2, all_reduce=ar)           # world_size 2 arithmetic on one rank: the arena holds the "sum"
    torch.cuda.synchronize()
    want = [off for _, off, _ in gradient_buckets(m)]
    assert calls == want and len(set(calls)) == len(calls)
    assert m.grad_divisor == 2.0 and rel_l2(m.grad_arena, whole) < 1e-6
    m.grad_divisor = 1.0
    comm.close()
