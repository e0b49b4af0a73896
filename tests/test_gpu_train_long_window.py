"""DiT training on temporal windows of 9 .. 32 frames (DiT(trainable=True, train_max_frames=n), include/gtav_amd.h gtav_dit_train_allow_window): the whole step —
streaming temporal attention backward (csrc/train.hip attn_temporal_bwd_stream_kernel), the adaLN-gradient reduction above 80 conditioning rows, the
frame loop of train.py — against torch autograd on the CPU oracle, and the properties the 5-frame step is held to (tests/test_gpu_train.py,
test_gpu_train_bf16.py): phases, resume, loss going down, limits.

Bounds are the project's own for the same comparisons (tests/train_cases.py): forward within FWD_TOL, every gradient tensor within GRAD_TOL relative L2,
a trainable-vs-inference forward 1.5e-3.  Where a gradient tensor of a long window exceeds GRAD_TOL it is held to 1.5 x the worst tensor of the T = 8 step of the
same batch, measured in the same run (_gradient_case).  `pytest -s` prints every measured margin."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import train_cases as TC  # noqa: E402
from helpers import rel_l2_logged as rel_l2  # noqa: E402
from gtav_amd import lib as L  # noqa: E402
from gtav_amd.model.dit import DiT  # noqa: E402
from train_cases import DTYPES, F16, FWD_TOL, GRAD_TOL  # noqa: E402
from train_cases import TOY_KW as KW  # noqa: E402

KW_WIDE = dict(KW, hidden_size=1024, num_heads=16, depth=1)


def _inputs(B, T, actions=True):
    return TC.inputs(KW, B, T, actions)


def _model(B, T, dtype=F16, kw=KW):
    return TC.model(kw, B, T, dtype, train_max_frames=max(T, 8))


def _all_grads(m):
    return {k: m.grad(k).clone() for k in m._shapes()}


def _grad_errors(B, T, actions, dtype, kw=KW):
    """Forward error and the relative L2 error of every gradient tensor of one (B, T) step against torch autograd; tensors that are zero upstream must be zero."""
    _, inp, _, v_ref, grads = TC.oracle(kw, B, T, actions)
    m = _model(B, T, dtype, kw)
    v = TC.forward_backward(m, inp)
    return rel_l2(v, v_ref), TC.grad_errors(m, grads)


_T8 = {}


def _t8_worst(B, actions, dtype):
    """Worst gradient tensor of the T = 8 step of the same batch, actions and operand type: the longest window of the register-resident temporal backward, i.e. a
    step that runs none of the long-window code.  Computed once per case; `pytest -s` prints every tensor (profiles/long_window_train/grad_errors.txt)."""
    key = (B, actions, dtype)
    if key not in _T8:
        _, errs = _grad_errors(B, 8, actions, dtype)
        for k, e in sorted(errs.items()):
            print(f"[grad T8 B={B} actions={actions} {dtype}] {e:.3e} {k}")
        _T8[key] = max(errs.values())
    return _T8[key]


def _gradient_case(B, T, actions, dtype, kw=KW):
    """Acceptance of tests/test_gpu_train.py::test_gradients_match_autograd: forward within FWD_TOL, every gradient tensor within GRAD_TOL.  A tensor above GRAD_TOL
    is held to 1.5 x the worst tensor of the T = 8 step of the same batch instead (measured in the same run, on the kernels windows of <= 8 frames have always
    run): the margin is for the longer 2-byte reductions over frames, not for a wrong kernel — a tensor beyond it is a bug."""
    fwd, errs = _grad_errors(B, T, actions, dtype, kw)
    assert fwd < FWD_TOL[dtype]
    top = max(errs, key=errs.get)
    print(f"[grad B={B} T={T} actions={actions} {dtype} D={kw['hidden_size']}] worst {errs[top]:.3e} ({top}), GRAD_TOL {GRAD_TOL[dtype]:.1e}")
    over = {k: e for k, e in errs.items() if e > GRAD_TOL[dtype]}
    if not over:
        return
    bound = 1.5 * _t8_worst(B, actions, dtype)
    for k, e in sorted(over.items()):
        print(f"[grad B={B} T={T} actions={actions} {dtype}] above GRAD_TOL: {e:.3e} {k}; 1.5 x the T = 8 worst = {bound:.3e}")
    bad = {k: e for k, e in over.items() if e > bound}
    assert not bad, f"gradient mismatch beyond GRAD_TOL {GRAD_TOL[dtype]:.1e} and beyond 1.5 x the T = 8 worst {bound:.3e}: {bad}"


@DTYPES
@pytest.mark.parametrize("actions", [True, False], ids=["actions", "no_actions"])
@pytest.mark.parametrize("B,T", [(2, 9), (2, 17), (1, 32)])
def test_long_window_gradients_match_autograd(B, T, actions, dtype):
    _gradient_case(B, T, actions, dtype)


def test_96_conditioning_rows_take_the_general_adaln_reduction():
    """B = 3, T = 32: 96 conditioning rows, more than the 80 the matrix-core adaLN-gradient kernel holds (csrc/train.hip launch_ada_bwd_dx)."""
    _gradient_case(3, 32, True, F16)


def test_production_width_at_a_9_frame_window():
    """hidden 1024, 16 heads: the D = 1024 kernels (fused LayerNorm backward, grouped weight gradients, matrix-core adaLN reduction) behind a 9-frame window."""
    _gradient_case(1, 9, True, F16, KW_WIDE)


def test_short_windows_keep_their_bits_on_an_opted_in_handle():
    """A (2, 5) step on DiT(max_frames=16, train_max_frames=16) runs the kernels of the default DiT(max_frames=5): every gradient is equal bit for bit."""
    x, t, a, vt = _inputs(2, 5)
    got = []
    for m in (TC.model(KW, 2, 16, train_max_frames=16), TC.model(KW, 2, 5)):
        v = TC.forward_backward(m, (x, t, a, vt))
        got.append((v.clone(), _all_grads(m)))
    assert torch.equal(got[0][0], got[1][0])
    for k in got[0][1]:
        assert torch.equal(got[0][1][k], got[1][1][k]), k


# ------------------------------------------------------------------------------------------------------------------------
# training behaviour at a 12-frame window (the 5-frame tests of tests/test_gpu_train.py / test_gpu_train_bf16.py)
# ------------------------------------------------------------------------------------------------------------------------
def _multi_target_clip(n_target, B=2, F=12, seed=5):
    """A clip of F + n_target - 1 latent frames whose every target frame sees a window of F frames (one target frame: TC.clip(KW, B, F))."""
    g = torch.Generator().manual_seed(seed)
    total = F + n_target - 1
    lat = torch.randn(B, total, 16, 8, 16, generator=g) * 0.5
    a = torch.zeros(B, total, 25)
    a[:, :, 3] = 1
    tgt = torch.tensor([[30, 10], [12, 44], [3, 25]][:n_target])[:, :B]
    ctx = torch.tensor([[5, 20], [7, 2], [9, 30]][:n_target])[:, :B]
    cn = [torch.randn(B, F - 1, 16, 8, 16, generator=g) for _ in range(n_target)]
    nz = [torch.randn(B, 1, 16, 8, 16, generator=g) for _ in range(n_target)]
    return lat, a, tgt, ctx, cn, nz


@DTYPES
def test_training_steps_reduce_the_loss_at_12_frames(dtype):
    from gtav_amd.train import training_step
    m = _model(2, 12, dtype)
    lat, a, tgt, ctx, cn, nz = TC.clip(KW, F=12)
    losses = [float(training_step(m, lat, a, tgt, ctx, cn, nz, lr=2e-4, weight_decay=0.0, max_grad_norm=1.0, n_prompt_frames=11)) for _ in range(8)]
    print("losses:", " ".join(f"{l:.4f}" for l in losses))
    assert all(math.isfinite(l) for l in losses)
    applied, skipped, _ = m.train_stats()
    assert applied and skipped == 0
    assert losses[-1] < losses[0] * 0.9, losses                      # tests/test_gpu_train.py test_training_step_reduces_the_loss


@DTYPES
def test_phased_backward_equals_monolithic_at_12_frames(dtype):
    m = _model(2, 12, dtype)
    x, t, a, vt = _inputs(2, 12)
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    whole = m.grad_arena.clone()
    assert float(whole.abs().max()) > 0
    m.zero_grad()
    for phase in range(m.depth + 2):
        m.backward_phases_(v, vt, phase, phase + 1)
    assert torch.equal(m.grad_arena, whole)


@DTYPES
def test_save_state_load_state_resumes_bit_exactly_at_12_frames(dtype, tmp_path):
    """Three steps straight == two steps, save_state, a fresh model, load_state, one more step: equal weights bit for bit (no atomics anywhere in the step)."""
    from gtav_amd.train import load_state, save_state, training_step
    lat, a, tgt, ctx, cn, nz = TC.clip(KW, F=12)
    kw = dict(lr=3e-4, weight_decay=0.01, max_grad_norm=1.0, n_prompt_frames=11)
    m1 = _model(2, 12, dtype)
    for _ in range(3):
        training_step(m1, lat, a, tgt, ctx, cn, nz, **kw)
    m1.pull_weights()
    straight = {k: v.clone() for k, v in m1._sd.items()}
    del m1
    m2 = _model(2, 12, dtype)
    for _ in range(2):
        training_step(m2, lat, a, tgt, ctx, cn, nz, **kw)
    ck = str(tmp_path / "train_checkpoints" / "dit_last")
    save_state(m2, ck, global_step=2, epoch=0)
    del m2
    m3 = DiT(**KW, max_batch=2, max_frames=12, init_weights=True, trainable=True, train_dtype=dtype, train_max_frames=12)    # other weights until load_state
    assert load_state(m3, ck)["step"] == 2
    training_step(m3, lat, a, tgt, ctx, cn, nz, **kw)
    m3.pull_weights()
    for k in straight:
        assert torch.equal(m3._sd[k], straight[k]), k
    applied, skipped, _ = m3.train_stats()
    assert applied and skipped == 0 and int(m3.opt_state_dict()["step"][0]) == 3


def test_training_step_over_a_14_frame_clip_with_12_frame_windows():
    """n_prompt_frames = 11, max_frames = 12: target frames 11, 12, 13 each see a 12-frame window (the last two after the window slid).  The step is applied
    and its loss equals forward_loss of an inference model with the same weights (the project's trainable-vs-inference forward figure, 1.5e-3)."""
    from gtav_amd.train import forward_loss, training_step
    lat, a, tgt, ctx, cn, nz = _multi_target_clip(3)
    assert lat.shape[1] == 14
    m = _model(2, 12)
    seen = []
    orig = m.forward_train
    m.forward_train = lambda x, t, e=None: (seen.append(x.shape[1]), orig(x, t, e))[1]
    loss = float(training_step(m, lat, a, tgt, ctx, cn, nz, lr=2e-4, max_grad_norm=1.0, n_prompt_frames=11))
    assert seen == [12, 12, 12]
    applied, skipped, gnorm = m.train_stats()
    assert math.isfinite(loss) and applied and skipped == 0 and math.isfinite(gnorm) and gnorm > 0
    mi = DiT(**KW, max_batch=2, max_frames=12, init_weights=False)
    mi.load_state_dict(TC.state_dict(KW))
    ref = float(forward_loss(mi, lat, a, tgt, ctx, cn, nz, n_prompt_frames=11)[0])
    print(f"[14-frame clip] training_step loss {loss:.6f}, inference forward_loss {ref:.6f}, rel {abs(loss - ref) / ref:.3e}")
    assert abs(loss - ref) / ref < 1.5e-3


# ------------------------------------------------------------------------------------------------------------------------
# limits
# ------------------------------------------------------------------------------------------------------------------------
def test_opted_in_model_refuses_a_longer_window_by_name_and_still_trains():
    m = _model(2, 12)
    x, t, a, vt = _inputs(2, 12)
    x13, t13, a13, _ = _inputs(2, 13)
    with pytest.raises((ValueError, L.GtavError), match="train_max_frames=12"):
        m.forward_train(x13, t13, a13)
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    m.adamw_step(1e-3, weight_decay=0.01, max_grad_norm=1.0)
    m.check()
    assert m.train_stats()[0]
    with pytest.raises((ValueError, L.GtavError), match="train_max_frames=12"):    # still refused after training was enabled, and still usable afterwards
        m.forward_train(x13, t13, a13)
    assert torch.isfinite(m.forward_train(x, t, a)).all()


def test_train_allow_window_range_and_order():
    lib = L.load()
    h = C.c_void_p()
    c = L.DitConfig(max_frames=12, max_batch=1, max_cond_rows=12, mlp_ratio=4.0, **KW)
    L.check(lib.gtav_dit_create(C.byref(c), C.byref(h)))
    try:
        for n in (33, 7):
            assert lib.gtav_dit_train_allow_window(h, n) != 0
            assert b"[8, 32]" in lib.gtav_last_error() and f"max_frames={n}".encode() in lib.gtav_last_error()
        assert lib.gtav_dit_train_enable(h, None, 0) != 0 and b"at most 8 frames" in lib.gtav_last_error()    # the refused calls changed nothing
        L.check(lib.gtav_dit_train_allow_window(h, 10))
        assert lib.gtav_dit_train_enable(h, None, 0) != 0                                                     # 12 frames on a handle allowed 10
        assert b"at most 10 frames" in lib.gtav_last_error() and b"max_frames=12" in lib.gtav_last_error()
        L.check(lib.gtav_dit_train_allow_window(h, 12))
        L.check(lib.gtav_dit_train_enable(h, None, 0))
        assert lib.gtav_dit_train_allow_window(h, 16) != 0
        assert b"already enabled" in lib.gtav_last_error()
    finally:
        lib.gtav_dit_destroy(h)
