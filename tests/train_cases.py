"""Cases, tolerances and the oracle cache the DiT training tests share (imported like helpers.py: no fixtures).  tests/train_case_digests.json pins the bytes
inputs(), clip() and state_dict() return (tests/test_host_train_cases.py), so the margins `pytest -s` prints stay comparable from file to file."""
import pytest
import torch

from helpers import rel_l2, rel_l2_logged

F16, BF16 = torch.float16, torch.bfloat16
# relative L2 per gradient tensor against torch autograd on the fp32 CPU oracle; fp16 measured worst 3.5e-3 (toy model, B = 5) / 3.3e-3 (full size), `pytest -s`
# prints every margin.  bf16 keeps 3 fewer mantissa bits than fp16: 8 x the fp16 bound, 3.6e-2
GRAD_TOL = {F16: 4.5e-3, BF16: 8 * 4.5e-3}
FWD_TOL = {F16: 2e-3, BF16: 1.5e-2}            # v_pred against the oracle's; bf16: TOL_BF16 of tests/test_gpu_range.py (all-bf16 forwards measure 5-7e-3)
DTYPES = pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])

# the toy model: 32 tokens per frame
TOY_KW = dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=256, depth=2, num_heads=4, external_cond_dim=25)

_SD, _ORACLE = {}, {}


def _key(kw):
    return tuple(sorted(kw.items()))


def state_dict(kw, seed=1):
    """The synthetic checkpoint of one geometry: built once, shared, never modified."""
    key = (_key(kw), seed)
    if key not in _SD:
        import gtav_amd.weights as W
        _SD[key] = W.synth_state_dict(W.dit_param_shapes(**kw), seed=seed)
    return _SD[key]


def inputs(kw, B=2, T=3, actions=True, seed=0):
    """(x, t, a, vt) of one forward + backward: noisy latents, timesteps, action one-hots (None without actions), the last frame's v target."""
    C, h, w = kw["in_channels"], kw["input_h"], kw["input_w"]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, h, w, generator=g)
    t = torch.randint(0, 1000, (B, T), generator=g)
    a = None
    if actions:
        a = torch.zeros(B, T, kw["external_cond_dim"])
        a[:, :, 3] = 1
        a[0, T - 1, 7] = 1
    vt = torch.randn(B, 1, C, h, w, generator=g)
    return x, t, a, vt


def clip(kw, B=2, F=5, seed=5):
    """(lat, a, tgt, ctx, cn, nz) of one training_step on an F-frame clip with one target frame (n_prompt_frames = F - 1)."""
    C, h, w = kw["in_channels"], kw["input_h"], kw["input_w"]
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B, F, C, h, w, generator=g) * 0.5
    a = torch.zeros(B, F, kw["external_cond_dim"])
    a[:, :, 3] = 1
    tgt, ctx = torch.tensor([30, 10][:B]), torch.tensor([5, 20][:B])
    cn = torch.randn(B, F - 1, C, h, w, generator=g)
    nz = torch.randn(B, 1, C, h, w, generator=g)
    return lat, a, tgt, ctx, cn, nz


def model(kw, B, T, dtype=F16, sd=None, **dit_kwargs):
    """A trainable DiT of max_batch B and max_frames T on `dtype` operands, loaded with `sd` (default: state_dict(kw))."""
    from gtav_amd.model.dit import DiT
    m = DiT(**kw, max_batch=B, max_frames=T, init_weights=False, trainable=True, train_dtype=dtype, **dit_kwargs)
    m.load_state_dict(state_dict(kw) if sd is None else sd)
    return m


def oracle(kw, B, T, actions, sd_seed=1, seed=0):
    """(sd, inputs, loss_ref, v_ref, grads) of torch autograd on the CPU oracle for state_dict(kw, sd_seed) and inputs(kw, B, T, actions, seed): computed once per
    case and shared by every test (and operand type) that needs it — callers must not modify any of it.  For the toy-sized cases only: a full-size DiT-S/2 test
    computes its oracle itself, so that a session never holds several depth-16 gradient sets."""
    key = (_key(kw), B, T, actions, sd_seed, seed)
    if key not in _ORACLE:
        from oracle import ref_cpu as O
        sd, inp = state_dict(kw, sd_seed), inputs(kw, B, T, actions, seed)
        threads = torch.get_num_threads()
        torch.set_num_threads(min(threads, 16))
        try:
            loss_ref, v_ref, grads = O.dit_loss_and_grads(sd, O.DiTConfig(**kw), *inp)
        finally:
            torch.set_num_threads(threads)
        assert all(torch.isfinite(g).all() for g in grads.values())
        _ORACLE[key] = (sd, inp, loss_ref, v_ref, grads)
    return _ORACLE[key]


def forward_backward(m, inputs):
    """forward_train, zero_grad, the monolithic backward; nothing may be left in the error words.  Returns v_pred."""
    x, t, a, vt = inputs
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    m.check()
    return v


def grad_errors(m, grads, keys=None, log=False):
    """{name: relative L2 error} of the model's gradients `keys` (default: all) against the oracle's `grads`.  Every gradient must be finite, and exactly zero where
    the oracle's is (external_cond.* without actions: unused, gradient None upstream).  log=True prints each margin under the running test's name."""
    err = rel_l2_logged if log else rel_l2
    errs = {}
    for k in (keys or grads):
        g, gref = m.grad(k).cpu(), grads[k]
        assert torch.isfinite(g).all(), k
        if gref.norm() == 0:
            assert g.abs().max() == 0, k
            continue
        errs[k] = err(g, gref)
    return errs
