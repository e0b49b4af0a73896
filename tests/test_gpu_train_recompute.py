"""Opt-in activation recomputation of the DiT training step (DiT(trainable=True, train_recompute=True) -> gtav_dit_train_set_recompute): the forward keeps the
block-input residual states only, the backward re-runs each block's forward into ONE block-sized set of buffers before differentiating it.

The yardstick of every test is the PLAIN handle (train_recompute=False: the code path that existed before), never the recompute mode itself, and the bound is
equality bit for bit (torch.equal): the kernels are deterministic and the re-run repeats the forward's launches on the forward's inputs.  Geometry: the toy model of
tests/test_gpu_train.py with depth 3 — a first block (re-run from r_0: no pending update in front of it), a middle block (re-run with the saved statistics' shift)
and a last block (not re-run after a forward)."""
import ctypes as C
import math

import pytest
import torch

import train_cases as TC
from gtav_amd import lib as L
from gtav_amd.model.dit import DiT
from train_cases import BF16, DTYPES, F16

pytestmark = pytest.mark.gpu

DEPTH = 3
KW = dict(TC.TOY_KW, depth=DEPTH)

_PLAIN = {}


def _inputs(B, T, actions=True, kw=KW, seed=0):
    return TC.inputs(kw, B, T, actions, seed)


def _model(B, T, dtype=F16, recompute=False, kw=KW, window=None):
    return TC.model(kw, B, T, dtype, train_max_frames=window, train_recompute=recompute)


def _loss(m, v, vt):
    """mean((v[:, -1] - vt)^2) by the library's own kernel (train._frame_step), as a (1,) device tensor."""
    B, n = v.shape[0], v[0, 0].numel()
    out = torch.empty(1 + B, device=m.device, dtype=torch.float32)
    vtd = vt.to(m.device, torch.float32).contiguous()
    last = v[:, -1]
    with torch.cuda.device(m.device):
        L.check(L.load().gtav_mse(last.data_ptr(), v.stride(0), vtd.data_ptr(), n, B, n, out.data_ptr(), L.current_stream()))
    return out[:1].clone()


def _one_pass(m, x, t, a, vt):
    """forward, loss, zero_grad, monolithic backward: (v_pred, loss, gradient arena), cloned."""
    v = m.forward_train(x, t, a)
    loss = _loss(m, v, vt)
    m.zero_grad()
    m.backward_(v, vt)
    torch.cuda.synchronize()
    return v.clone(), loss, m.grad_arena.clone()


def _plain(B, T, actions, dtype, kw=KW, window=None):
    """The plain handle's result of one case: computed once, shared by the tests that need it, never modified."""
    key = (B, T, actions, dtype, tuple(sorted(kw.items())), window)
    if key not in _PLAIN:
        m = _model(B, T, dtype, False, kw, window)
        _PLAIN[key] = _one_pass(m, *_inputs(B, T, actions, kw))
        assert torch.isfinite(_PLAIN[key][2]).all() and float(_PLAIN[key][2].abs().max()) > 0
    return _PLAIN[key]


def _assert_same(got, want):
    for name, g, w in zip(("v_pred", "loss", "gradient arena"), got, want):
        assert g.shape == w.shape and torch.equal(g, w), f"{name}: {int((g != w).sum())} of {g.numel()} elements differ, max |diff| {float((g - w).abs().max()):.3e}"


# ---- 1 / 2: one step, bit for bit ---------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("actions", [True, False], ids=["actions", "noactions"])
@pytest.mark.parametrize("B,T", [(2, 3), (1, 5)])
def test_step_is_bit_equal_to_the_plain_handle(B, T, actions, dtype):
    m = _model(B, T, dtype, True)
    assert m.train_recompute
    got = _one_pass(m, *_inputs(B, T, actions))
    _assert_same(got, _plain(B, T, actions, dtype))
    m.check()          # the error words too: nothing was raised that the plain step does not raise


@DTYPES
def test_bit_equal_on_a_9_frame_window(dtype):
    """train_max_frames=9, (B, T) = (1, 9): the streaming temporal attention forward and backward."""
    m = _model(1, 9, dtype, True, window=9)
    _assert_same(_one_pass(m, *_inputs(1, 9, True)), _plain(1, 9, True, dtype, window=9))


@DTYPES
def test_bit_equal_on_200_token_frames(dtype):
    """20 x 40 latents = 200 tokens per frame, the smallest long-frame geometry of tests/test_gpu_train_long_frames.py, at (1, 2): the streaming spatial
    attention backward."""
    kw = dict(KW, input_h=20, input_w=40)
    m = _model(1, 2, dtype, True, kw=kw)
    _assert_same(_one_pass(m, *_inputs(1, 2, True, kw)), _plain(1, 2, True, dtype, kw=kw))


# ---- 3: phases --------------------------------------------------------------------------------------------------------------------------
def test_phased_backward_equals_the_plain_monolithic_backward():
    """Phases one at a time, then (over the same forward) in two uneven groups: the second pass finds block 0's activations in place and has to re-run the last
    block as well.  Then the monolithic backward twice over one forward (gradients accumulate) against the plain handle doing the same."""
    B, T = 2, 3
    x, t, a, vt = _inputs(B, T, True)
    v_ref, _, g_ref = _plain(B, T, True, F16)
    m = _model(B, T, F16, True)
    v = m.forward_train(x, t, a)
    assert torch.equal(v, v_ref)
    m.zero_grad()
    for p in range(DEPTH + 2):
        m.backward_phases_(v, vt, p, p + 1)
    assert torch.equal(m.grad_arena, g_ref)
    m.zero_grad()
    m.backward_phases_(v, vt, 0, 2)
    m.backward_phases_(v, vt, 2, DEPTH + 2)
    assert torch.equal(m.grad_arena, g_ref)
    m.backward_(v, vt)                                   # accumulates on top
    twice = m.grad_arena.clone()
    p = _model(B, T, F16, False)
    vp = p.forward_train(x, t, a)
    p.zero_grad()
    p.backward_(vp, vt)
    p.backward_(vp, vt)
    assert torch.equal(twice, p.grad_arena)


# ---- 4: optimisation steps, checkpoints across the modes ----------------------------------------------------------------------------------
def _multi_target_clip(n_target, B=2, F=5, seed=5):
    """TC.clip's latents and actions with n_target target frames: the index draws come before the noise draws."""
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B, F, 16, 8, 16, generator=g) * 0.5
    a = torch.zeros(B, F, 25)
    a[:, :, 3] = 1
    tgt = [torch.randint(1, 51, (B,), generator=g) for _ in range(n_target)]
    ctx = [torch.randint(1, 41, (B,), generator=g) for _ in range(n_target)]
    first = F - n_target
    cn = [torch.randn(B, first + k, 16, 8, 16, generator=g) for k in range(n_target)]
    nz = [torch.randn(B, 1, 16, 8, 16, generator=g) for _ in range(n_target)]
    return lat, a, tgt, ctx, cn, nz


def _state(m):
    m.pull_weights()
    st = {"w." + k: v.clone() for k, v in m._sd.items()}
    st.update(m.opt_state_dict())
    return st


def _assert_state_equal(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_three_optimisation_steps_and_checkpoints_across_the_modes(tmp_path):
    from gtav_amd.train import load_state, save_state, training_step
    ins = TC.clip(KW)
    kw = dict(lr=3e-4, weight_decay=0.01, max_grad_norm=1.0)
    plain, rc = _model(2, 5, F16, False), _model(2, 5, F16, True)
    for step in range(3):
        lp, lr_ = training_step(plain, *ins, **kw), training_step(rc, *ins, **kw)
        assert torch.equal(lp, lr_), step
        assert plain.train_stats() == rc.train_stats() and plain.train_stats()[0], step
        _assert_state_equal(_state(rc), _state(plain))
    # a checkpoint of either mode resumes in the other: the format does not know the mode
    save_state(plain, str(tmp_path / "plain"), global_step=3, epoch=0)
    save_state(rc, str(tmp_path / "rc"), global_step=3, epoch=0)
    training_step(plain, *ins, **kw)
    want = _state(plain)
    into_rc = DiT(**KW, max_batch=2, max_frames=5, init_weights=True, trainable=True, train_recompute=True)
    assert load_state(into_rc, str(tmp_path / "plain"))["step"] == 3
    training_step(into_rc, *ins, **kw)
    _assert_state_equal(_state(into_rc), want)
    into_plain = DiT(**KW, max_batch=2, max_frames=5, init_weights=True, trainable=True)
    assert load_state(into_plain, str(tmp_path / "rc"))["step"] == 3
    training_step(into_plain, *ins, **kw)
    _assert_state_equal(_state(into_plain), want)


# ---- 5: the frame loop ------------------------------------------------------------------------------------------------------------------
def test_frame_loop_with_three_target_frames():
    """A 5-frame clip with n_prompt_frames=2: target frames 2, 3, 4 see windows of 3, 4 and 5 frames, each differentiated inside the loop (training_step)."""
    from gtav_amd.train import training_step
    ins = _multi_target_clip(3)
    out = []
    for recompute in (False, True):
        m = _model(2, 5, F16, recompute)
        loss = training_step(m, *ins, lr=3e-4, weight_decay=0.01, max_grad_norm=1.0, n_prompt_frames=2)
        assert m.train_stats()[0]
        out.append((loss.clone(), m.grad_arena.clone(), _state(m)))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert float(out[0][1].abs().max()) > 0
    _assert_state_equal(out[1][2], out[0][2])


# ---- 6: accumulation --------------------------------------------------------------------------------------------------------------------
def test_two_micro_batches_accumulate():
    out = []
    for recompute in (False, True):
        m = _model(2, 3, F16, recompute)
        m.zero_grad()
        for seed in (0, 11):
            x, t, a, vt = _inputs(2, 3, True, seed=seed)
            v = m.forward_train(x, t, a)
            m.backward_(v, vt)
        g = m.grad_arena.clone()
        m.adamw_step(3e-4, weight_decay=0.01, max_grad_norm=1.0)
        assert m.train_stats()[0]
        out.append((g, _state(m)))
    assert torch.equal(out[0][0], out[1][0])
    assert not torch.equal(out[0][0], _plain(2, 3, True, F16)[2])        # (two micro-batches, not one)
    _assert_state_equal(out[1][1], out[0][1])


# ---- 7: overflow ------------------------------------------------------------------------------------------------------------------------
def test_fp16_saturation_skips_the_step_in_both_modes():
    """A loss scale of 2^40 saturates the fp16 activation gradients (tests/test_gpu_train.py test_fp16_saturation_skips_the_step_and_loss_scaler_backs_off): the
    step is skipped on the device with the same statistics, the weights stay, and the error word was consumed."""
    from gtav_amd.train import training_step
    ins = TC.clip(KW)
    stats = []
    for recompute in (False, True):
        m = _model(2, 5, F16, recompute)
        m.loss_scale = 2.0 ** 40
        training_step(m, *ins, lr=1e-3)
        applied, skipped, gnorm = m.train_stats()
        assert not applied and skipped == 1 and math.isinf(gnorm)
        assert int(m.opt_state_dict()["step"][0]) == 0
        m.pull_weights()
        assert torch.equal(m._sd["blocks.1.s_mlp.fc1.weight"], TC.state_dict(KW)["blocks.1.s_mlp.fc1.weight"])
        m.check()
        stats.append((applied, skipped, gnorm))
    assert stats[0] == stats[1]


# ---- 8: memory --------------------------------------------------------------------------------------------------------------------------
def test_saved_bytes():
    """gtav_dit_train_saved_bytes.  Plain: exactly what train_enable allocates for the saved activations — 4 L + 1 fp32 states, 2 L half-blocks of eight D-wide and
    two 4 D-wide 2-byte images, the final LayerNorm's output and the patch matrix, rows padded to 128.  Recompute: L + 4 states and 2 half-blocks of images, so per
    token (64 + 4 (L + 4)) D bytes against (64 L + 4 (4 L + 1)) D: 92 / 244 = 0.377 at L = 3.  eps = 0.01 covers what both modes keep outside the blocks (2 D + 2 Kpe
    bytes per token: 640 of 62 464 + 640 plain bytes at these sizes, which moves the ratio by 0.0064) and the saved shifts (4 (L - 1) bytes per token: 0.0001)."""
    B, T, D, Lb = 2, 3, KW["hidden_size"], DEPTH
    P = (KW["input_h"] // 2) * (KW["input_w"] // 2)
    Kpe = KW["in_channels"] * 4
    Mx = (B * T * P + 127) // 128 * 128
    plain, rc = _model(B, T, F16, False), _model(B, T, F16, True)
    pb, rb = plain.train_saved_bytes(), rc.train_saved_bytes()
    per_token_plain = (4 * Lb + 1) * 4 * D + 2 * Lb * (8 * D + 2 * 4 * D) * 2 + 2 * D + 2 * Kpe
    assert pb == Mx * per_token_plain
    per_token_rc = (Lb + 4) * 4 * D + 2 * (8 * D + 2 * 4 * D) * 2 + 2 * D + 2 * Kpe + 4 * (Lb - 1)
    assert rb == Mx * per_token_rc
    bound = (64 + 4 * (Lb + 4)) / (64 * Lb + 4 * (4 * Lb + 1))
    assert abs(bound - 92 / 244) < 1e-12
    print(f"[saved bytes] plain {pb}  recompute {rb}  ratio {rb / pb:.4f}  bound {bound:.4f} + 0.01")
    assert rb / pb <= bound + 0.01
    # the figure is the handle's, fixed at enable time: a step changes nothing
    _one_pass(rc, *_inputs(B, T, True))
    assert rc.train_saved_bytes() == rb
    # and bf16 operands have the same sizes
    assert _model(B, T, BF16, True).train_saved_bytes() == rb


# ---- 9: residual taps -------------------------------------------------------------------------------------------------------------------
def test_residual_taps():
    B, T = 2, 3
    x, t, a, vt = _inputs(B, T, True)
    plain, rc = _model(B, T, F16, False), _model(B, T, F16, True)
    vp, vr = plain.forward_train(x, t, a), rc.forward_train(x, t, a)
    for k in (0, 4, 8, 12):
        assert torch.equal(rc.residual_after(k, B, T), plain.residual_after(k, B, T)), k
    assert float(plain.residual_after(1, B, T).abs().max()) > 0          # the plain handle serves every state
    with pytest.raises(L.GtavError, match="train_get_residual: k=1 is a state inside a block"):
        rc.residual_after(1, B, T)
    # refused before anything happened: the handle still trains, and the taps survive the backward pass (which overwrites the ring states)
    rc.zero_grad()
    rc.backward_(vr, vt)
    assert torch.equal(rc.grad_arena, _plain(B, T, True, F16)[2])
    for k in (0, 4, 8, 12):
        assert torch.equal(rc.residual_after(k, B, T), plain.residual_after(k, B, T)), k


# ---- 10: the switch's order -------------------------------------------------------------------------------------------------------------
def test_set_recompute_after_train_enable_is_refused_and_changes_nothing():
    B, T = 2, 3
    lib = L.load()
    m = _model(B, T, F16, False)
    before = m.train_saved_bytes()                       # builds the handle: training is enabled
    assert lib.gtav_dit_train_set_recompute(m._handle, 1) != 0
    err = lib.gtav_last_error().decode()
    assert "train_set_recompute: training is already enabled" in err and "gtav_dit_train_enable" in err
    assert m.train_saved_bytes() == before
    _assert_same(_one_pass(m, *_inputs(B, T, True)), _plain(B, T, True, F16))
    assert float(m.residual_after(1, B, T).abs().max()) > 0              # still the plain mode: every state is kept
    # the same on a handle in recompute mode: switching it off after the fact is refused too
    r = _model(B, T, F16, True)
    rb = r.train_saved_bytes()
    assert lib.gtav_dit_train_set_recompute(r._handle, 0) != 0 and "train_set_recompute" in lib.gtav_last_error().decode()
    assert r.train_saved_bytes() == rb and rb < before
    _assert_same(_one_pass(r, *_inputs(B, T, True)), _plain(B, T, True, F16))
    # before train_enable, on a bare handle: accepted, and saved_bytes has nothing to report yet
    cfg = L.DitConfig(max_frames=T, max_batch=B, max_cond_rows=B * T, mlp_ratio=4.0, **{k: v for k, v in KW.items()})
    h = C.c_void_p()
    L.check(lib.gtav_dit_create(C.byref(cfg), C.byref(h)))
    try:
        n = C.c_int64(0)
        assert lib.gtav_dit_train_saved_bytes(h, C.byref(n)) != 0 and "train_saved_bytes: training is not enabled" in lib.gtav_last_error().decode()
        L.check(lib.gtav_dit_train_set_recompute(h, 1))
        L.check(lib.gtav_dit_train_set_recompute(h, 0))
    finally:
        lib.gtav_dit_destroy(h)
