"""Low-rank adapter (LoRA) fine-tuning of the DiT on a frozen backbone, on the GPU, in both operand types: DiT(trainable=True, train_lora_rank=r) trains the
adapter pairs lora_A / lora_B of every half-block's four GEMM Linears and nothing else (include/gtav_amd.h gtav_dit_train_set_lora; DESIGN.md 7 "Low-rank
adapters").  The toy model of tests/train_cases.py throughout.  The oracle for the adapter gradients is torch autograd on oracle.ref_cpu.dit_forward with every
adapted weight built as W0 + s B @ A from leaf tensors A and B, and the loss of dit_loss_and_grads; computed once per case, shared by both operand types."""
import ctypes as C
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import train_cases as TC  # noqa: E402
from train_cases import FWD_TOL, GRAD_TOL, grad_errors  # noqa: E402
from helpers import rel_l2  # noqa: E402

KW = TC.TOY_KW
LINEARS = ("attn.to_qkv", "attn.to_out", "mlp.fc1", "mlp.fc2")
_ADAPTERS, _ORACLE = {}, {}


def adapters(rank, live=True):
    """The adapters of one rank, built once, never modified: A as init_lora(0) draws it; B ~ N(0, 0.02) seeded (live: the merged weight differs materially from
    the base) or zero (the default initialisation)."""
    key = (rank, live)
    if key not in _ADAPTERS:
        from gtav_amd.model.dit import DiT
        sd = DiT(**KW, init_weights=False, trainable=True, train_lora_rank=rank).lora_state_dict()        # (no handle: nothing touches the device)
        g = torch.Generator().manual_seed(100 + rank)
        _ADAPTERS[key] = {k: (torch.randn(v.shape, generator=g) * 0.02 if live and ".lora_B." in k else v) for k, v in sd.items()}
    return _ADAPTERS[key]


def lora_model(B, T, dtype, rank, alpha=None, live=True, **dit_kwargs):
    m = TC.model(KW, B, T, dtype, train_lora_rank=rank, train_lora_alpha=alpha, **dit_kwargs)
    m.load_lora_state_dict(adapters(rank, live))
    return m


def lora_oracle(B, T, actions, rank, alpha=None, live=True):
    """(inputs, v_ref, {adapter name: gradient}) of autograd through the CPU oracle with W = W0 + (alpha / rank) B @ A"""
    key = (B, T, actions, rank, alpha, live)
    if key not in _ORACLE:
        from oracle import ref_cpu as O
        sd, inp = TC.state_dict(KW), TC.inputs(KW, B, T, actions)
        s = (rank if alpha is None else alpha) / rank
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in adapters(rank, live).items()}
        merged = dict(sd)
        for k in leaves:
            if k.endswith(".lora_A.weight"):
                stem = k[: -len(".lora_A.weight")]
                merged[stem + ".weight"] = sd[stem + ".weight"] + s * leaves[stem + ".lora_B.weight"] @ leaves[k]
        threads = torch.get_num_threads()
        torch.set_num_threads(min(threads, 16))
        try:
            with torch.enable_grad():
                x, t, a, vt = inp
                v_pred = O.dit_forward(merged, O.DiTConfig(**KW), x, t, a)
                torch.nn.functional.mse_loss(v_pred[:, -1:], vt).backward()          # the loss of dit_loss_and_grads
        finally:
            torch.set_num_threads(threads)
        grads = {k: v.grad for k, v in leaves.items()}
        assert all(g is not None and torch.isfinite(g).all() for g in grads.values())
        _ORACLE[key] = (inp, v_pred.detach(), grads)
    return _ORACLE[key]


def _param_count(rank):
    D, H = KW["hidden_size"], 4 * KW["hidden_size"]
    return 2 * KW["depth"] * rank * sum(n + k for n, k in ((3 * D, D), (D, D), (H, D), (D, H)))


# ---- 1. identity at initialisation -------------------------------------------------------------------------------------------------------------------------
@TC.DTYPES
def test_identity_at_initialisation(dtype):
    inp, _, grads = lora_oracle(2, 3, True, 16, live=False)
    x, t, a, vt = inp
    base = TC.model(KW, 2, 3, dtype)
    m = lora_model(2, 3, dtype, 16, live=False)
    v0, v = base.forward_train(x, t, a), m.forward_train(x, t, a)
    assert torch.equal(v0, v), "B = 0: the merged images are the base's, the forward the same bits"
    m.zero_grad()
    m.backward_(v, vt)
    m.check()
    for k in grads:
        if ".lora_A." in k:
            assert m.grad(k).abs().max() == 0, k              # dA = s (dY B)^T X with B = 0
    errs = grad_errors(m, grads, [k for k in grads if ".lora_B." in k], log=True)
    assert len(errs) == 16 and max(errs.values()) < GRAD_TOL[dtype], max(errs.items(), key=lambda kv: kv[1])


# ---- 2. gradient parity with live adapters -----------------------------------------------------------------------------------------------------------------
# (batch, frames) -> M token rows of 32 per frame: 96 = one partial 128-row tile, 192 = a whole tile and a partial one, 256 = two whole tiles
CASES = pytest.mark.parametrize("B,T,rank,alpha", [(1, 3, 16, None), (2, 3, 64, 32.0), (4, 2, 32, 64.0)], ids=["M96-r16", "M192-r64", "M256-r32"])


@TC.DTYPES
@pytest.mark.parametrize("actions", [True, False], ids=["actions", "noactions"])
@CASES
def test_adapter_gradients_match_autograd(B, T, rank, alpha, actions, dtype):
    inp, v_ref, grads = lora_oracle(B, T, actions, rank, alpha)
    m = lora_model(B, T, dtype, rank, alpha)
    v = TC.forward_backward(m, inp)
    assert rel_l2(v, v_ref) < FWD_TOL[dtype]
    errs = grad_errors(m, grads, log=True)
    assert len(errs) == len(grads) == 32
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"[lora margin M={B * T * 32} rank {rank} {'bf16' if dtype is TC.BF16 else 'fp16'}] worst adapter gradient {worst[0]} {worst[1]:.3e} = "
          f"{worst[1] / GRAD_TOL[dtype]:.3f} of GRAD_TOL")
    assert worst[1] < GRAD_TOL[dtype], worst


# ---- 3. the merged export is the model ---------------------------------------------------------------------------------------------------------------------
@TC.DTYPES
def test_merged_export_is_the_model(dtype):
    from gtav_amd.train import training_step
    m = lora_model(2, 5, dtype, 16)
    lat, a, tgt, ctx, cn, nz = TC.clip(KW)
    before = m.lora_state_dict()
    for _ in range(3):
        training_step(m, lat, a, tgt, ctx, cn, nz, lr=1e-3)
    applied, skipped, _ = m.train_stats()
    assert applied and skipped == 0
    after = m.lora_state_dict()
    assert all(not torch.equal(after[k], before[k]) for k in before), "A and B moved"
    merged = m.merged_state_dict()
    sd = TC.state_dict(KW)
    assert set(merged) == set(m.state_dict()) and not any("lora" in k for k in merged)        # the reference's key layout
    adapted = {f"blocks.{i}.{h}_{l}.weight" for i in range(KW["depth"]) for h in "st" for l in LINEARS}
    for k, v in sd.items():
        assert torch.equal(merged[k], v) != (k in adapted), k                                   # the adapted weights changed, nothing else did
    plain = TC.model(KW, 2, 5, dtype, sd=merged)
    x, t, act, _ = TC.inputs(KW, 2, 5, True)
    assert torch.equal(m.forward_train(x, t, act), plain.forward_train(x, t, act))
    # the base is frozen: the fp32 masters on the GPU still hold the bits that were loaded
    m.pull_weights()
    got = m.state_dict()
    assert all(torch.equal(got[k], v) for k, v in sd.items())


# ---- 4. optimizer ------------------------------------------------------------------------------------------------------------------------------------------
@TC.DTYPES
def test_adamw_over_the_adapters_matches_torch(dtype):
    """test_adamw_step_matches_torch (tests/test_gpu_train.py) restricted to the adapters: the oracle's gradients into the arena, three steps, that test's bounds."""
    from oracle import ref_cpu as O
    rank = 16
    (x, t, a, vt), _, grads = lora_oracle(2, 3, True, rank)
    names = sorted(grads)
    params = {k: adapters(rank)[k] for k in names}
    ref, norm_ref = O.adamw_reference(params, {k: grads[k] for k in names}, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0, steps=3)
    m = lora_model(2, 3, dtype, rank)
    m.forward_train(x, t, a)                      # builds the handle
    flat = torch.cat([grads[k].reshape(-1) for k in names]) * m.loss_scale
    assert flat.numel() == m.grad_arena.numel() == _param_count(rank) == 262144
    for _ in range(3):
        m.grad_arena.copy_(flat.to(m.grad_arena.device))
        m.adamw_step(1e-3, weight_decay=0.01, max_grad_norm=1.0)
    applied, skipped, norm = m.train_stats()
    assert applied and skipped == 0
    assert abs(norm - float(norm_ref)) / float(norm_ref) < 1e-5
    got = m.lora_state_dict()
    for k in names:
        upd, upd_ref = got[k] - params[k], ref[k] - params[k]
        assert rel_l2(upd, upd_ref) < 1e-4, (k, rel_l2(upd, upd_ref))


# ---- 5. recomputation --------------------------------------------------------------------------------------------------------------------------------------
@TC.DTYPES
def test_recompute_gives_the_same_bits(dtype):
    inp, _, grads = lora_oracle(2, 3, True, 32)
    m, mr = lora_model(2, 3, dtype, 32), lora_model(2, 3, dtype, 32, train_recompute=True)
    v, vr = TC.forward_backward(m, inp), TC.forward_backward(mr, inp)
    assert torch.equal(v, vr)
    assert torch.equal(m.grad_arena, mr.grad_arena) and m.grad_arena.abs().max() > 0
    assert mr.train_saved_bytes() < m.train_saved_bytes()


# ---- 6. checkpoint round trip ------------------------------------------------------------------------------------------------------------------------------
@TC.DTYPES
def test_checkpoint_round_trip(dtype, tmp_path):
    from safetensors import safe_open
    from gtav_amd.lib import GtavError
    from gtav_amd.train import load_state, save_state, training_step
    clip = TC.clip(KW)
    m = lora_model(2, 5, dtype, 16, alpha=8.0)
    for _ in range(2):
        training_step(m, *clip, lr=1e-3)
    d = str(tmp_path / "lora_ckpt")
    save_state(m, d, global_step=2, epoch=0)
    assert sorted(os.listdir(d)) == ["lora.safetensors", "optimizer.safetensors", "step.json"]          # no model.safetensors: the base is the caller's
    state = json.load(open(os.path.join(d, "step.json")))
    assert state["lora"] == {"rank": 16, "alpha": 8.0} and state["step"] == 2
    with safe_open(os.path.join(d, "lora.safetensors"), "pt") as f:
        assert f.metadata() == {"rank": "16", "alpha": "8.0"} and len(list(f.keys())) == 32
    with safe_open(os.path.join(d, "optimizer.safetensors"), "pt") as f:
        assert len(list(f.keys())) == 2 * 32 + 1                                                         # the adapters' moments and the counters
    m2 = TC.model(KW, 2, 5, dtype, train_lora_rank=16, train_lora_alpha=8.0)                             # fresh, the same base loaded
    assert load_state(m2, d)["step"] == 2
    for mm in (m, m2):
        training_step(mm, *clip, lr=1e-3)
    s1, s2 = m.lora_state_dict(), m2.lora_state_dict()
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    assert m.train_stats() == m2.train_stats()
    # the three refusals, by name
    full = TC.model(KW, 2, 5, dtype)
    with pytest.raises(GtavError, match="LoRA checkpoint"):
        load_state(full, d)
    with pytest.raises(GtavError, match="rank 16, this DiT's rank 32"):
        load_state(TC.model(KW, 2, 5, dtype, train_lora_rank=32), d)
    full.zero_grad()                                                                                     # builds the handle whose state is saved
    d_full = str(tmp_path / "full_ckpt")
    save_state(full, d_full, global_step=0, epoch=0)
    with pytest.raises(GtavError, match="full checkpoint"):
        load_state(m2, d_full)


# ---- 7. buckets, phases ------------------------------------------------------------------------------------------------------------------------------------
def test_gradient_buckets_tile_the_adapter_arena():
    from gtav_amd.train import backward_overlapped, gradient_buckets
    inp, _, _ = lora_oracle(2, 3, True, 16)
    m = lora_model(2, 3, TC.F16, 16)
    v = TC.forward_backward(m, inp)
    mono = m.grad_arena.clone()
    L = KW["depth"]
    buckets = gradient_buckets(m)
    assert [b[0] for b in buckets] == [L - l for l in reversed(range(L))], "one bucket per block, the last block's first; the frozen prefixes have none"
    spans = sorted((off, off + cnt) for _, off, cnt in buckets)
    assert spans[0][0] == 0 and spans[-1][1] == m.grad_arena.numel() == _param_count(16) and all(x[1] == y[0] for x, y in zip(spans, spans[1:]))
    assert m.param_range("blocks.0.") == (0, _param_count(16) // L) and m.param_range("final_layer.") == (0, 0)
    # the phased backward of the overlapped all-reduce gives the monolithic one's bits
    m.zero_grad()
    backward_overlapped(m, v, inp[3], world_size=1)
    assert torch.equal(m.grad_arena, mono)


# ---- 8. refusals, upload order -----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from gtav_amd import lib as L
    from gtav_amd.model.dit import DiT
    with pytest.raises(ValueError, match="train_lora_rank"):
        DiT(**KW, init_weights=False, trainable=True, train_lora_rank=24)
    with pytest.raises(ValueError, match="trainable=True"):
        DiT(**KW, init_weights=False, train_lora_rank=16)
    with pytest.raises(ValueError, match="train_range_policy"):
        DiT(**KW, init_weights=False, trainable=True, train_lora_rank=16, train_range_policy="auto")
    inp, _, _ = lora_oracle(2, 3, True, 16)
    m = lora_model(2, 3, TC.F16, 16)
    TC.forward_backward(m, inp)
    with pytest.raises(L.GtavError, match="blocks.0.s_attn.to_qkv.weight"):
        m.grad("blocks.0.s_attn.to_qkv.weight")
    bad = dict(adapters(16))
    bad["blocks.1.s_mlp.fc2.lora_B.weight"] = torch.zeros(256, 32)
    with pytest.raises(RuntimeError, match=r"blocks\.1\.s_mlp\.fc2\.lora_B\.weight has shape \(256, 32\)"):
        m.load_lora_state_dict(bad)
    # the library itself refuses a frozen parameter by name, and the opt-ins that come too late or do not combine
    lib, h = L.load(), m._handle
    buf = torch.zeros(768 * 256, device=m.device)
    for rc in (lib.gtav_dit_get_grad(h, b"blocks.0.s_attn.to_qkv.weight", buf.data_ptr(), buf.numel(), None),
               lib.gtav_dit_get_opt_state(h, b"blocks.0.s_attn.to_qkv.weight", buf.data_ptr(), buf.data_ptr(), buf.numel(), None),
               lib.gtav_dit_set_opt_state(h, b"final_layer.linear.bias", buf.data_ptr(), buf.data_ptr(), 64, None)):
        assert rc != 0 and b"is not a trainable parameter" in lib.gtav_last_error()
    assert lib.gtav_dit_train_set_lora(h, 16, 16.0) != 0 and b"already enabled" in lib.gtav_last_error()
    assert lib.gtav_dit_lora_get_merged(h, b"final_layer.linear.weight", buf.data_ptr(), 64 * 256, None) != 0 and b"not an adapted weight" in lib.gtav_last_error()
    cfg = L.DitConfig(max_frames=3, max_batch=1, max_cond_rows=3, mlp_ratio=4.0, **KW)
    h2 = C.c_void_p(None)
    L.check(lib.gtav_dit_create(C.byref(cfg), C.byref(h2)))
    try:
        assert lib.gtav_dit_train_set_lora(h2, 48, 48.0) != 0 and b"rank 48" in lib.gtav_last_error()
        assert lib.gtav_dit_train_set_lora(h2, 16, 0.0) != 0 and b"alpha" in lib.gtav_last_error()
        L.check(lib.gtav_dit_train_allow_mixed(h2, 1))
        assert lib.gtav_dit_train_set_lora(h2, 16, 16.0) != 0 and b"mixed operand groups" in lib.gtav_last_error()
        L.check(lib.gtav_dit_train_allow_mixed(h2, 0))
        L.check(lib.gtav_dit_train_set_lora(h2, 16, 16.0))
        assert lib.gtav_dit_train_allow_mixed(h2, 1) != 0 and b"low-rank adapters" in lib.gtav_last_error()
        n = C.c_int64(0)
        L.check(lib.gtav_dit_train_param_count(h2, C.byref(n)))
        assert n.value == _param_count(16)
    finally:
        lib.gtav_dit_destroy(h2)


def test_upload_order_does_not_matter():
    """A base weight sent again AFTER its adapters (set_weight writes the plain image) leaves the images merged: the forward keeps its bits."""
    from gtav_amd import lib as L
    inp, _, _ = lora_oracle(2, 3, True, 16)
    x, t, a, _ = inp
    m = lora_model(2, 3, TC.F16, 16)
    v = m.forward_train(x, t, a)
    lib, sd = L.load(), TC.state_dict(KW)
    for k in ("blocks.0.s_mlp.fc1.weight", "blocks.1.t_attn.to_qkv.weight"):
        w = sd[k].to(m.device).contiguous()
        L.check(lib.gtav_dit_set_weight(m._handle, k.encode(), w.data_ptr(), w.numel(), L.current_stream()))
    L.check(lib.gtav_dit_finalize(m._handle, L.current_stream()))
    assert torch.equal(m.forward_train(x, t, a), v)
