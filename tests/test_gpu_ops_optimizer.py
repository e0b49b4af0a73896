"""Per-element fp64 parity of the optimizer step's kernels (csrc/train.hip sumsq_kernel, clip_coef_kernel, adamw_multi_kernel in its three modes,
overflow_publish_kernel) on the GPU, in both operand types, through the test hooks gtav_op_train_sumsq / _clip_coef / _adamw_multi / _overflow_publish
(include/gtav_amd_testing.h): the launchers gtav_dit_adamw_step runs, over work items cut by the handle's own planner.

Inputs, fp64 references and the derived bounds come from the last section of tests/parity_bounds.py; tests/test_host_parity_bounds.py holds a float32 emulation of
the kernels as designed inside every bound and the listed wrong kernels outside.  None is taken from what a kernel returned.  Every buffer a launch is given
(masters, gradients, moments, shadows, both 2-byte images, the descriptor tables, ctl, the partial sums, the error word) sits between 64 guard words of a NaN
bit pattern that must be intact afterwards, and the 24-float gaps of the strided fp32 view hold the same pattern.  A step runs as the handle runs it: sumsq,
clip_coef (which writes ctl[1] and ctl[4 .. 7] on the device), then the AdamW launch; the reference takes the coefficient ctl[1] the device wrote (an fp32
number, like every hyperparameter) and the TRUE bias corrections 1 - beta^t.  `pytest -s` prints, per case and output, the worst ratio error / bound
(profiles/op_parity_optimizer/margins.txt is such a printout)."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import parity_bounds as PB  # noqa: E402
from helpers import dev, stream, tiled_index  # noqa: E402
from gtav_amd import lib as L  # noqa: E402

F16, BF16 = PB.F16, PB.BF16
DTYPES = pytest.mark.parametrize("dtype", PB.DTYPES, ids=[PB.NAME[d] for d in PB.DTYPES])
GUARD = 64                      # words in front of and behind every buffer (256 bytes of fp32, 128 of a 2-byte type: the payload stays 16-byte aligned)
NAN32, NAN16 = 0x7FC0A5A5, 0x7FA5
SENTINEL16 = 0x1234
B1, B2 = PB.ADAM_BETAS
ADAM_CASES = [(s, c, st) for s in PB.ADAM_SETTINGS for c in PB.ADAM_COEFS for st in PB.ADAM_STARTS]
ADAM_IDS = [f"{s}-{c}-{st}" for s, c, st in ADAM_CASES]
EMA_DECAY = 0.999


@pytest.fixture(autouse=True)
def _restore_hooks():
    yield
    L.load().gtav_op_set_operand_dtype(0)


def _use(dtype):
    L.load().gtav_op_set_operand_dtype(1 if dtype is BF16 else 0)
    return L.load()


class _Buf:
    """a caller-owned device buffer between guard words; the payload is carried as bit patterns (int32 / int16) in both directions"""

    def __init__(self, data):
        flat = data.contiguous().reshape(-1)
        self.n, self.dtype = flat.numel(), flat.dtype
        self.it, self.nan = (torch.int32, NAN32) if flat.element_size() == 4 else (torch.int16, NAN16)
        host = torch.full((self.n + 2 * GUARD,), self.nan, dtype=self.it)
        host[GUARD:GUARD + self.n] = flat.view(self.it)
        self.buf = host.to(dev())
        self.ptr = self.buf.data_ptr() + GUARD * flat.element_size()

    def bits(self, name=""):
        host = self.buf.cpu()
        assert (host[:GUARD] == self.nan).all() and (host[GUARD + self.n:] == self.nan).all(), f"{name}: a guard word was overwritten"
        return host[GUARD:GUARD + self.n].clone()

    def get(self, name=""):
        return self.bits(name).view(self.dtype)

    def put(self, i, value):
        self.buf[GUARD + i] = torch.tensor([value], dtype=self.dtype).view(self.it)[0].item()


def _void_array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*[p or None for p in ptrs])


def _int_array(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


class _Step:
    """The buffers of one AdamCase on the GPU and the launches of a step.  The gradients lie in ONE arena, parameter after parameter, every start padded with zeros
    to 4 floats (16-byte rows for the interior tiles; zeros add nothing to the norm)."""

    def __init__(self, c, dtype, image_fill=0):
        self.c, self.dtype = c, dtype
        self.p, self.m, self.v, self.e, self.w16, self.wT = [], [], [], [], [], []
        offs, chunks, off = [], [], 0
        for i, ps in enumerate(c.params):
            w0 = c.w0[i]
            if ps.ldp != ps.C:                                                        # the strided view: NaN in the gaps
                view = torch.full((ps.R, ps.ldp), NAN32, dtype=torch.int32).view(torch.float32)
                view[:, :ps.C] = w0
                w0 = view
            self.p.append(_Buf(w0))
            self.m.append(_Buf(c.m0[i]))
            self.v.append(_Buf(c.v0[i]))
            self.e.append(_Buf(c.e0[i]))
            self.w16.append(_Buf(torch.full((ps.w16_elems,), image_fill, dtype=torch.int16).view(dtype)) if ps.gemm else None)
            self.wT.append(_Buf(torch.full((ps.wT_elems,), image_fill, dtype=torch.int16).view(dtype)) if ps.has_wT else None)
            n = ps.R * ps.C
            offs.append(off)
            chunks += [c.g[i].reshape(-1), torch.zeros(PB.round_up(n, 4) - n)]
            off += PB.round_up(n, 4)
        self.offs, self.arena_n = offs, off
        self.arena = _Buf(torch.cat(chunks))
        self.part = _Buf(torch.zeros(PB.sumsq_parts(off)))
        self.n_items = sum(math.ceil(ps.R / 64) * math.ceil(ps.C / 64) if ps.gemm else math.ceil(ps.R * ps.C / 4096) for ps in c.params)
        self.desc_bytes = 88 * len(c.params) + 8 * self.n_items
        self.desc = _Buf(torch.zeros(self.desc_bytes // 4, dtype=torch.int32))
        self.ctl = _Buf(torch.zeros(8))
        self.err = _Buf(torch.zeros(1, dtype=torch.int32))

    def norm_and_coef(self, ema_decay=0.0):
        """sumsq + clip_coef as gtav_dit_adamw_step launches them -> ctl (8 floats, CPU)"""
        lib = _use(self.dtype)
        L.check(lib.gtav_op_train_sumsq(self.arena.ptr, self.arena_n, self.part.ptr, self.part.n, stream()))
        L.check(lib.gtav_op_train_clip_coef(self.ctl.ptr, self.part.ptr, self.part.n, PB.ADAM_INV_SCALE, self.c.max_norm, B1, B2, ema_decay, 0, self.err.ptr, stream()))
        torch.cuda.synchronize()
        self.part.bits("sumsq partial sums")
        assert self.err.get("error word").item() == 0
        return self.ctl.get("ctl")

    def adamw(self, mode, desc_bytes=None):
        lib, c = _use(self.dtype), self.c
        ps = c.params
        rc = lib.gtav_op_train_adamw_multi(
            mode, len(ps), _void_array([b.ptr for b in self.p]), _int_array([q.ldp for q in ps]), _int_array([q.R for q in ps]), _int_array([q.C for q in ps]),
            _void_array([self.arena.ptr + 4 * o for o in self.offs]), _void_array([b.ptr for b in self.m]), _void_array([b.ptr for b in self.v]),
            _void_array([b.ptr if mode else 0 for b in self.e]), _void_array([b.ptr if b else 0 for b in self.w16]), _int_array([q.Cp16 for q in ps]),
            _void_array([b.ptr if b else 0 for b in self.wT]), _int_array([q.RpT for q in ps]), self.desc.ptr, self.desc_bytes if desc_bytes is None else desc_bytes,
            self.ctl.ptr, c.lr, B1, B2, PB.ADAM_EPS, c.wd, stream())
        L.check(rc)
        torch.cuda.synchronize()
        self.desc.bits("descriptor tables")

    def masters(self, name="masters"):
        """the logical [R][C] masters (CPU), after checking that the gaps of the strided view still hold their NaN"""
        out = []
        for ps, b in zip(self.c.params, self.p):
            w = b.get(name)
            if ps.ldp != ps.C:
                w = w.reshape(ps.R, ps.ldp)
                assert (w[:, ps.C:].contiguous().view(torch.int32) == NAN32).all(), f"{name}: a launch wrote into the gap of the strided view"
                w = w[:, :ps.C].contiguous()
            out.append(w.reshape(ps.R, ps.C))
        return out

    def state(self, name=""):
        """bit patterns of everything a launch may touch, in a fixed order"""
        bufs = self.p + self.m + self.v + self.e + [b for b in self.w16 + self.wT if b] + [self.arena, self.ctl]
        return [b.bits(name) for b in bufs]

    def moments(self, which):
        return [b.get(which).reshape(ps.R, ps.C) for ps, b in zip(self.c.params, getattr(self, which))]

    def check_images(self, name):
        """both images of every GEMM weight, pads included, against the two converters' output for the master the launch wrote; on fp16 the masters beyond
        65504 are there as +-65504"""
        lib = _use(self.dtype)
        for i, ps in enumerate(self.c.params):
            if not ps.gemm:
                continue
            src = self.p[i]
            want = _Buf(torch.full((ps.w16_elems,), SENTINEL16, dtype=torch.int16).view(self.dtype))
            L.check(lib.gtav_op_convert_f16(src.ptr, ps.C, ps.R, ps.C, want.ptr, PB.round_up(ps.R, 128), ps.Cp16, 1, stream()))
            torch.cuda.synchronize()
            got = self.w16[i].bits(f"{name} W image")
            assert torch.equal(got, want.bits("convert_f16")), f"{name}: the W image of parameter {i} ({ps.R} x {ps.C}) differs from convert_f16 of its master"
            if self.dtype is F16:
                k = len(PB.ADAM_BEYOND_F16)
                w = self.masters()[i].reshape(-1)[3:3 + k]
                img = got.view(F16)[tiled_index(ps.R, ps.Cp16)[0, 3:3 + k]].float()
                assert torch.isfinite(img).all() and torch.equal(img, w.clamp(-PB.F16_MAX, PB.F16_MAX).to(F16).float()), (name, i, img, w)
            if ps.has_wT:
                want = _Buf(torch.full((ps.wT_elems,), SENTINEL16, dtype=torch.int16).view(self.dtype))
                L.check(lib.gtav_op_train_convert_t(src.ptr, ps.C, ps.R, ps.C, want.ptr, stream()))
                torch.cuda.synchronize()
                assert torch.equal(self.wT[i].bits(f"{name} W^T image"), want.bits("convert_t")), \
                    f"{name}: the W^T image of parameter {i} ({ps.R} x {ps.C}) differs from convert_t of its master"


def _bits_equal(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def _worst(got, ref, tol):
    r = (got.double() - ref).abs() / tol
    return torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf"))).max().item()


_RUNS = {}


def _run(case, dtype, mode):
    """Every step of one AdamCase in one mode: bounds, exact zeros, images and guards are checked on the way; -> [(w, m, v) of every step] for the tests that compare
    runs.  Computed once per (case, type, mode)."""
    key = (case, dtype, mode)
    if key in _RUNS:
        return _RUNS[key]
    c = PB.adam_case(*case)
    name = f"adamw mode {mode} {'-'.join(map(str, case))} {PB.NAME[dtype]}"
    s = _Step(c, dtype)
    if c.start != "fresh":
        s.ctl.put(4, float(c.start - 1))
    out = []
    for t in c.steps:
        w0, m0, v0, e0 = s.masters(), s.moments("m"), s.moments("v"), s.moments("e")
        ctl = s.norm_and_coef(EMA_DECAY if mode == 1 else 0.0).double()
        coef = ctl[1].item()
        # the coefficient, the step count and the fp32 bias corrections (a documented property of the design: parity_bounds.bc_allowed)
        if c.coef_kind == "unclipped":
            assert coef == PB.ADAM_INV_SCALE
        else:
            want = PB.ADAM_INV_SCALE * c.max_norm / (c.norm64 + PB.f32(1e-6))
            assert abs(coef - want) <= (PB.sumsq_depth(s.arena_n) / 2 + 5) * PB.EPS32 * PB.SECOND_ORDER * want, (name, coef, want)
        assert ctl[4].item() == t and ctl[2].item() == 0
        assert abs(ctl[3].item() - c.norm64) <= (PB.sumsq_depth(s.arena_n) / 2 + 2) * PB.EPS32 * PB.SECOND_ORDER * c.norm64
        for i, beta in ((5, B1), (6, B2)):
            d = abs(ctl[i].item() - PB.bc_ref(beta, t))
            print(f"[margin {name} t={t}] ctl[{i}]: |1 - powf(beta, t) - (1 - beta^t)| / allowed {d / PB.bc_allowed(beta, t):.3f}")
            assert d <= PB.bc_allowed(beta, t), (name, t, i, ctl[i].item())
        if mode == 1:
            assert ctl[7].item() == PB.f32(EMA_DECAY)
        s.adamw(mode)
        w, m, v, e = s.masters(name), s.moments("m"), s.moments("v"), s.moments("e")
        worst = {"w": 0.0, "m": 0.0, "v": 0.0, "e": 0.0}
        for i, ps in enumerate(c.params):
            r = PB.adam_reference(w0[i], c.g[i], m0[i], v0[i], coef, t, c.lr, c.wd)
            for k, x in zip("wmv", (w[i], m[i], v[i])):
                assert torch.isfinite(x).all(), (name, k, i)
                worst[k] = max(worst[k], _worst(x, r[k], r["tol_" + k]))
            if mode == 1:
                d = PB.f32(EMA_DECAY)
                worst["e"] = max(worst["e"], _worst(e[i], d * e0[i].double() + (1.0 - d) * w[i].double(), PB.ema_step_bound(e0[i], w[i])))
            else:
                assert _bits_equal([e[i]], [e0[i]]), (name, "mode 0 touched the shadow buffer", i)
            zero = (c.g[i] == 0) & (m0[i] == 0) & (v0[i] == 0)
            if zero.any():                                                            # the decay alone, and moments that stay exactly 0
                decay = torch.tensor(1.0) - torch.tensor(c.lr) * torch.tensor(c.wd)
                assert (m[i][zero] == 0).all() and (v[i][zero] == 0).all() and torch.equal(w[i][zero], (w0[i] * decay)[zero]), (name, "exact zeros", i)
        print(f"[margin {name} t={t}] per element: worst error / bound w {worst['w']:.3f} m {worst['m']:.3f} v {worst['v']:.3f}" + (f" e {worst['e']:.3f}" if mode == 1 else ""))
        assert max(worst.values()) <= 1.0, (name, t, worst)
        s.check_images(f"{name} t={t}")
        assert torch.equal(s.arena.get(), torch.cat([x for i, ps in enumerate(c.params) for x in
                                                     (c.g[i].reshape(-1), torch.zeros(PB.round_up(ps.R * ps.C, 4) - ps.R * ps.C))])), (name, "the gradients changed")
        out.append((w, m, v))
    _RUNS[key] = out
    return out


# ---- the AdamW launch -----------------------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("mode", (0, 1), ids=("step", "step+ema"))
@pytest.mark.parametrize("case", ADAM_CASES, ids=ADAM_IDS)
def test_adamw_within_bounds_and_bit_exact_images(case, mode, dtype):
    """every element of w, m, v (and e) inside its bound at every step; exact zeros; both images, pads included, bit for bit what the converters make of the
    master the launch wrote; guards and gaps intact"""
    _run(case, dtype, mode)


@DTYPES
@pytest.mark.parametrize("case", ADAM_CASES, ids=ADAM_IDS)
def test_adamw_one_arithmetic(case, dtype):
    """the same (w, g, m, v) in an interior tile, an element-wise tile and an fp32 run of one launch come out with equal bits; mode 1 gives mode 0's w, m, v; the
    same launches from the same state again give equal bits"""
    c = PB.adam_case(*case)
    plain, ema = _run(case, dtype, 0), _run(case, dtype, 1)
    for step, (w, m, v) in enumerate(plain):
        for what, tensors in (("w", w), ("m", m), ("v", v)):
            a = c.probe(tensors, "interior")
            for where in ("edge", "run"):
                b = c.probe(tensors, where)
                diff = (a.view(torch.int32) != b.view(torch.int32))
                assert not diff.any(), (f"step {step + 1}: {what} of the interior tile and of the {where} path differ in {int(diff.sum())} of {a.numel()} elements",
                                        a[diff][:4], b[diff][:4])
        for x, y in zip((w, m, v), ema[step]):
            assert _bits_equal(x, y), f"step {step + 1}: the step with the averaged weights is not the step alone"
    _RUNS.pop((case, dtype, 0))
    again = _run(case, dtype, 0)
    assert all(_bits_equal(x, y) for a, b in zip(plain, again) for x, y in zip(a, b))


@DTYPES
@pytest.mark.parametrize("mode", (0, 1), ids=("step", "step+ema"))
def test_adamw_skipped_step_writes_nothing(mode, dtype):
    """an inf in the arena: clip_coef leaves ctl[1] = 0 and ctl[4 .. 7] alone, counts the skip and still reports the norm; the AdamW launch then keeps every bit of
    w, m, v, e and of both images (prefilled with a sentinel)"""
    c = PB.adam_case("base", "clipped", 1000)
    s = _Step(c, dtype, image_fill=SENTINEL16)
    for i, x in enumerate((-1.0, -2.0, 7.0, -3.0, 999.0, 0.25, 0.125, 0.0625)):
        s.ctl.put(i, x)
    s.arena.put(s.offs[4] + 9, float("inf"))
    lib = _use(dtype)
    L.check(lib.gtav_op_train_sumsq(s.arena.ptr, s.arena_n, s.part.ptr, s.part.n, stream()))
    L.check(lib.gtav_op_train_clip_coef(s.ctl.ptr, s.part.ptr, s.part.n, PB.ADAM_INV_SCALE, c.max_norm, B1, B2, EMA_DECAY if mode else 0.0, 0, s.err.ptr, stream()))
    torch.cuda.synchronize()
    ctl = s.ctl.get("ctl").tolist()
    assert ctl[0] == float("inf") and ctl[1] == 0.0 and ctl[2] == 8.0 and ctl[3] == float("inf") and ctl[4:] == [999.0, 0.25, 0.125, 0.0625], ctl
    before = s.state()
    s.adamw(mode)
    after = s.state("skipped step")
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    s.masters("skipped step")


@DTYPES
def test_adamw_swap(dtype):
    """mode 2: w and e exchange exactly, g, m, v and ctl keep their bits, both images are the converters' output for the new w"""
    c = PB.adam_case("base", "clipped", 1000)
    s = _Step(c, dtype)
    w0, e0 = s.masters(), s.moments("e")
    fixed = lambda: [b.bits() for b in s.m + s.v + [s.arena, s.ctl]]
    before = fixed()
    s.adamw(2)
    assert _bits_equal(s.masters("swap"), e0) and _bits_equal(s.moments("e"), w0)
    assert all(torch.equal(a, b) for a, b in zip(before, fixed()))
    s.check_images("swap")
    s.adamw(2)                                                                        # and back: every bit of the start
    assert _bits_equal(s.masters("swap back"), w0) and _bits_equal(s.moments("e"), e0)
    s.check_images("swap back")


def test_adamw_hook_refuses_a_small_descriptor_buffer():
    s = _Step(PB.adam_case("base", "unclipped", "fresh"), F16)
    with pytest.raises(L.GtavError, match="descriptor"):
        s.adamw(0, desc_bytes=s.desc_bytes - 8)
    assert (s.desc.bits() == 0).all()


# ---- the norm and the coefficient -----------------------------------------------------------------------------------------------------------------------------
def _sumsq(c):
    """sumsq + clip_coef (inv_scale 1, no clipping) on one SumsqCase -> ctl (CPU)"""
    lib = L.load()
    g, part, ctl = _Buf(c.g), _Buf(torch.zeros(c.parts)), _Buf(torch.zeros(8))
    assert lib.gtav_op_train_sumsq_parts(c.n) == c.parts
    L.check(lib.gtav_op_train_sumsq(g.ptr, c.n, part.ptr, c.parts, stream()))
    L.check(lib.gtav_op_train_clip_coef(ctl.ptr, part.ptr, c.parts, 1.0, 0.0, B1, B2, 0.0, 0, 0, stream()))
    torch.cuda.synchronize()
    assert torch.equal(g.get("sumsq input").view(torch.int32), c.g.view(torch.int32))
    part.bits("partial sums")
    return ctl.get("ctl").double()


@pytest.mark.parametrize("n", PB.SUMSQ_N)
def test_sumsq_within_bound(n):
    c = PB.sumsq_case(n)
    ctl = _sumsq(c)
    w = abs(ctl[0].item() - c.ref) / c.tol
    print(f"[margin sumsq n={n}] |sum - ref| / bound {w:.3f} (chain of {PB.sumsq_depth(n)} roundings)")
    assert w <= 1.0, (n, ctl[0].item(), c.ref)
    assert ctl[1].item() == 1.0 and ctl[4].item() == 1.0 and ctl[2].item() == 0.0
    assert abs(ctl[3].item() - math.sqrt(c.ref)) <= (PB.sumsq_depth(n) / 2 + 2) * PB.EPS32 * PB.SECOND_ORDER * math.sqrt(c.ref)


@pytest.mark.parametrize("special", PB.SUMSQ_SPECIALS, ids=lambda s: "-".join(s))
@pytest.mark.parametrize("n", PB.SUMSQ_SPECIAL_N)
def test_sumsq_inf_and_nan_skip_the_step(n, special):
    ctl = _sumsq(PB.sumsq_case(n, special))
    assert not math.isfinite(ctl[0].item()) and not math.isfinite(ctl[3].item())
    assert ctl[1].item() == 0.0 and ctl[2].item() == 1.0 and ctl[4].item() == 0.0 and ctl[5].item() == 0.0 and ctl[6].item() == 0.0


def test_sumsq_hook_refuses_a_short_partial_sum_buffer():
    c = PB.sumsq_case(2049)
    g, part = _Buf(c.g), _Buf(torch.zeros(c.parts))
    assert L.load().gtav_op_train_sumsq(g.ptr, c.n, part.ptr, c.parts - 1, stream()) != 0
    assert "op_train_sumsq" in L.load().gtav_last_error().decode()
    torch.cuda.synchronize()
    assert (part.bits() == 0).all()


@pytest.mark.parametrize("name", list(PB.CLIP_CASES))
def test_clip_coef_fields(name):
    from gtav_amd.train import ema_decay_at
    c = PB.CLIP_CASES[name]
    part, ctl = _Buf(c.part), _Buf(torch.tensor(c.CTL_IN))
    err = _Buf(torch.tensor([c.err_in or 0], dtype=torch.int32))
    L.check(L.load().gtav_op_train_clip_coef(ctl.ptr, part.ptr, c.part.numel(), c.inv_scale, c.max_norm, B1, B2, c.ema_decay, int(c.warmup),
                                             0 if c.err_in is None else err.ptr, stream()))
    torch.cuda.synchronize()
    got, before = ctl.get("ctl"), torch.tensor(c.CTL_IN)
    assert torch.equal(part.get("partial sums").view(torch.int32), c.part.view(torch.int32))
    keep = lambda lo, hi: torch.equal(got[lo:hi].view(torch.int32), before[lo:hi].view(torch.int32))
    if c.finite:
        assert abs(got[0].item() - c.ssq) <= c.ssq_tol and abs(got[3].item() - c.norm) <= c.norm_tol, (name, got)
    else:
        assert not math.isfinite(got[0].item()) and not math.isfinite(got[3].item()) and math.isnan(got[0].item()) == math.isnan(c.ssq)
    if c.skip:
        assert got[1].item() == 0.0 and got[2].item() == c.CTL_IN[2] + 1 and keep(4, 8), (name, got)
        assert err.get().item() == ((c.err_in or 0) & ~(PB.ERR_F16_SAT | PB.ERR_NONFINITE)), name
        return
    assert err.get().item() == (c.err_in or 0) and keep(2, 3)
    if c.clipped:
        w = abs(got[1].item() - c.coef) / c.coef_tol
        print(f"[margin clip_coef {name}] |coefficient - ref| / bound {w:.3f}")
        assert w <= 1.0, (name, got[1].item(), c.coef)
    else:
        assert got[1].item() == c.inv_scale
    assert got[4].item() == c.t
    for i, beta in ((5, B1), (6, B2)):
        assert abs(got[i].item() - PB.bc_ref(beta, c.t)) <= PB.bc_allowed(beta, c.t), (name, i, got[i].item())
    if c.ema_decay > 0.0:
        assert got[7].item() == ema_decay_at(int(c.t), c.ema_decay, c.warmup), (name, got[7].item())
    else:
        assert keep(7, 8)


@pytest.mark.parametrize("bits,published", [(PB.ERR_F16_SAT, True), (PB.ERR_NONFINITE, True), (PB.ERR_F16_SAT | PB.ERR_NONFINITE | 1, True), (1, False), (0, False)])
def test_overflow_publish(bits, published):
    """with one of the two bits set the named element becomes +inf and nothing else changes; with both clear nothing changes at all"""
    g0 = PB.rand(9, seed=3)
    g, err = _Buf(g0), _Buf(torch.tensor([bits], dtype=torch.int32))
    L.check(L.load().gtav_op_train_overflow_publish(err.ptr, g.ptr + 4 * 5, stream()))
    torch.cuda.synchronize()
    want = g0.clone()
    if published:
        want[5] = float("inf")
    assert torch.equal(g.get("gradients").view(torch.int32), want.view(torch.int32)) and err.get("error word").item() == bits
