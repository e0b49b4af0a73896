"""Kernel-level parity of EVERY form of the deferred-residual LayerNorm (GPU), in both operand types: csrc/elementwise.hip ln_row_block_kernel applies
x += gate[frame] (bias + sum_k slab_k) and normalises the updated row, 65 times per DiT forward, in every VAE block and in every training forward; and
launch_branch_rows, which must write the bits of LnPending::y_save.  Reached through the test hooks gtav_op_ln_pending / gtav_op_branch_rows
(include/gtav_amd_testing.h): one launcher call, every LnPending field an argument, nothing validated in between.

Inputs, fp64 references and the three bounds (1 residual per element, 2 branch image bit for bit, 3 operand relative L2) come from tests/parity_bounds.py;
tests/test_host_parity_bounds.py holds an fp32 emulation inside them and five wrong kernels outside.  None is taken from what the kernels return.  `pytest -s`
prints, per case, the measured error as a fraction of its bound (profiles/op_parity_ln/margins.txt is such a printout)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import parity_bounds as PB  # noqa: E402
from helpers import assert_declared_plan, dev, stream, untile_typed  # noqa: E402
from gtav_amd import lib as L  # noqa: E402

F16, BF16 = PB.F16, PB.BF16
DTYPES = pytest.mark.parametrize("dtype", PB.DTYPES, ids=[PB.NAME[d] for d in PB.DTYPES])
ERR_TIMESTEP, ERR_F16_SAT = 1, PB.ERR_F16_SAT


@pytest.fixture(autouse=True)
def _restore_hooks():
    yield
    L.load().gtav_op_set_operand_dtype(0)


def _use(dtype):
    L.load().gtav_op_set_operand_dtype(1 if dtype is BF16 else 0)
    return L.load()


def _up(n, m):
    return (n + m - 1) // m * m


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), device=dev(), dtype=dtype)


def _bits(t):
    """the bit patterns of a tensor on the CPU, so that NaN sentinels compare equal to themselves"""
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Launch:
    """The device buffers of one gtav_op_ln_pending call on a PB.LnPendCase, fresh for every instance: the residual, the NaN-filled operand image with a spare
    row tile, the slabs with a NaN GUARD slab directly behind slab nsplit - 1 (a chunk slot at or above nsplit that was added would make the row NaN), the
    tables, and whichever of x_out / y_save / k_save the form asks for, NaN-filled as well.  err starts at err0."""

    def __init__(self, c, dtype, x_out=False, y_save=False, k_save=False, k_load=None, x=None, tperm=True, slabs=True, err0=0):
        self.c, self.dtype = c, dtype
        M, D, ld, ns = c.M, c.D, c.ld, c.nsplit
        self.x = (c.x if x is None else x).clone().to(dev())
        self.out = _nan((_up(M, 128) + 128, D), dtype)
        self.parts = None
        if ns and slabs:
            self.parts = _nan((ns + 1, M, ld), torch.float32)
            self.parts[:ns] = c.slabs.to(dev())
        self.bias = c.bias.to(dev()) if c.bias is not None and slabs else None
        self.mod = c.mod.to(dev())
        self.gamma, self.beta = c.gamma.to(dev()), c.beta.to(dev())
        self.rows = c.rows.to(dev()) if c.rows is not None else None
        self.gate_rows = c.gate_rows.to(dev()) if c.gate_rows is not None else None
        self.x_out = _nan((M, D), torch.float32) if x_out else None
        self.y_save = _nan((M, ld), dtype) if y_save else None
        self.k_save = _nan((M,), torch.float32) if k_save else None
        self.k_load = k_load
        self.tperm = c.tperm if (tperm and c.tperm) else (0, 0)
        self.err = torch.full((1,), err0, device=dev(), dtype=torch.int32)

    def args(self, **over):
        """the hook's argument list; `over` replaces descriptor fields by name (the refusals)"""
        c, D = self.c, self.c.D
        gated = c.gated and self.parts is not None
        a = dict(mode=c.mode, x=self.x.data_ptr(), ldx=D, out=self.out.data_ptr(), M=c.M, D=D,
                 p0=(self.mod[:, D:] if c.mode == 0 else self.gamma).data_ptr(), p1=(self.mod[:, 2 * D:] if c.mode == 0 else self.beta).data_ptr(),
                 mod_stride=3 * D if c.mode == 0 else 0, rows=L.ptr(self.rows), rows_per_mod=c.P,
                 parts=L.ptr(self.parts), nsplit=c.nsplit if self.parts is not None else 0, slab_stride=c.M * c.ld, ld=c.ld, bias=L.ptr(self.bias),
                 gate=self.mod.data_ptr() if gated else 0, gate_stride=3 * D if gated else 0, gate_rows=L.ptr(self.gate_rows) if gated else 0,
                 rows_per_gate=c.P if gated else 0, x_out=L.ptr(self.x_out), y_save=L.ptr(self.y_save), tperm_T=self.tperm[0], tperm_P=self.tperm[1],
                 k_save=L.ptr(self.k_save), k_load=L.ptr(self.k_load), err=self.err.data_ptr(), stream=stream())
        assert set(over) <= set(a), over
        a.update(over)
        return list(a.values())

    def run(self, lib):
        c = self.c
        assert_declared_plan("layernorm", c.mode, c.M, c.D, int(self.parts is not None), int(self.tperm[0] != 0), int(self.k_save is not None), int(self.k_load is not None))
        L.check(lib.gtav_op_ln_pending(*self.args()))
        torch.cuda.synchronize()
        return self

    def operand(self, tperm=True):
        """the M x D operand in TOKEN row order: the image untiled, then the inverse of the documented permutation"""
        got = untile_typed(self.out, self.c.M, self.c.D)
        return got[self.c.out_rows()] if (tperm and self.tperm[0]) else got

    def snapshot(self):
        return {k: _bits(v) for k, v in vars(self).items() if isinstance(v, torch.Tensor)}

    def changed(self, snap):
        """names of the buffers whose bits differ from the snapshot"""
        return [k for k, v in snap.items() if not torch.equal(_bits(getattr(self, k)), v)]


def _margin(name, dtype, what, value):
    print(f"[margin ln_pending {name} {PB.NAME[dtype]}] {what}: {value:.3f} of the bound")


def _check_residual(c, dtype, got, what="residual"):
    """assertion 1"""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), (c.name, "a chunk slot at or above nsplit was added, or the residual is not finite")
    frac, worst = PB.outside((got - c.ref_new).abs(), c.tol_new)
    _margin(c.name, dtype, f"{what} per element", worst)
    assert worst <= 1.0, (c.name, PB.NAME[dtype], what, worst, frac)


def _check_operand(c, dtype, run):
    """assertion 3"""
    got = run.operand().double()
    assert torch.isfinite(got).all(), c.name
    tol = PB.LN_TOL * PB.FACTOR[dtype]
    e, er = PB.rel_l2(got, c.ref_operand), PB.row_rel_l2(got, c.ref_operand)
    _margin(c.name, dtype, "operand rel-L2", e / tol)
    _margin(c.name, dtype, "operand worst row", er / tol)
    assert e < tol and er < tol, (c.name, PB.NAME[dtype], e, er, tol)
    assert torch.isnan(run.out[_up(c.M, 128):]).all(), "the row tile behind the last one was written"


def _check_inputs(c, run, x_kept):
    """the slabs bit-unchanged with the guard slab still NaN; x bit-unchanged where the update goes to x_out; the error word clean"""
    if run.parts is not None:
        assert _same_bits(run.parts[:c.nsplit], c.slabs) and torch.isnan(run.parts[c.nsplit]).all(), "the slab buffer was written"
    if x_kept:
        assert _same_bits(run.x, c.x), "x was written although the update goes to x_out"
    assert run.err.item() == 0


def _check_y_save(lib, c, dtype, run):
    """assertion 2: y_save and launch_branch_rows against the emulated ordered sum, bit for bit; the ld - D columns behind a row stay NaN"""
    want = c.y_save(dtype)
    assert _same_bits(run.y_save[:, :c.D], want), (c.name, "y_save differs from the store of the ordered fp32 sum")
    assert torch.isnan(run.y_save[:, c.D:]).all()
    y = _nan((c.M, c.ld), dtype)
    err = torch.zeros(1, device=dev(), dtype=torch.int32)
    L.check(lib.gtav_op_branch_rows(run.parts.data_ptr(), c.nsplit, c.M * c.ld, c.ld, L.ptr(run.bias), y.data_ptr(), c.M, c.D, err.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert _same_bits(y, run.y_save), (c.name, "launch_branch_rows differs from y_save")
    assert err.item() == 0


# ---- in place: the sampler's and the VAE's launches ---------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ["d64", "d192", "d256_rows", "d1280", "d1792"])
def test_in_place_forms(name, dtype):
    """gate + bias at one wave per block; the VAE's affine form without gate and bias at 48 of 64 threads and ld > D; the sampler step's row indirection with
    the fused temporal launch's output order at nsplit 3; blocks of 5 and 7 waves at nsplit 5 and 8"""
    lib, c = _use(dtype), PB.ln_pend_case(name)
    run = _Launch(c, dtype).run(lib)
    _check_residual(c, dtype, run.x)
    _check_operand(c, dtype, run)
    _check_inputs(c, run, x_kept=False)
    # every form also leaves the branch image to launch_branch_rows, in both types
    run2 = _Launch(c, dtype, x_out=True, y_save=True).run(lib)
    _check_y_save(lib, c, dtype, run2)
    _check_residual(c, dtype, run2.x_out, "x_out")
    _check_inputs(c, run2, x_kept=True)
    assert _same_bits(run2.out, run.out) and _same_bits(run2.x_out, run.x), "x_out / y_save change the bits of the launch"


# ---- the output order of the fused temporal launch ------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("name", ["d256_rows", "d1280_tperm"])
def test_tperm_with_slabs_is_a_row_permutation(name, dtype):
    """assertion 4 on the row-block kernel: after the inverse of the documented permutation, the bits of the same launch with tperm_T = 0.  With 16 positions
    per frame (the sampler-step case of the issue's table) the documented order IS the identity and the two images are equal as they are; with 32 they are not."""
    lib, c = _use(dtype), PB.ln_pend_case(name)
    a, b = _Launch(c, dtype).run(lib), _Launch(c, dtype, tperm=False).run(lib)
    assert _same_bits(a.out, b.out) == (c.tperm[1] == 16)
    assert _same_bits(a.operand(), b.operand())
    assert _same_bits(a.x, b.x)
    if name == "d1280_tperm":
        _check_operand(c, dtype, a)


@DTYPES
def test_tperm_without_slabs(dtype):
    """A descriptor that carries the permutation only (the LayerNorm behind a residual GEMM that wrote in place): bound 3 through the documented order, x
    untouched, and against the identity launch — which takes the wave-row kernel here, so to rounding (LN_TOL), not to the bit"""
    lib, c = _use(dtype), PB.ln_pend_case("d256_tperm")
    a = _Launch(c, dtype).run(lib)
    _check_operand(c, dtype, a)
    _check_inputs(c, a, x_kept=True)
    b = _Launch(c, dtype, tperm=False).run(lib)
    tol = PB.LN_TOL * PB.FACTOR[dtype]
    e = PB.row_rel_l2(a.operand().double(), b.operand().double())
    _margin(c.name, dtype, "permuted against identity launch, worst row", e / tol)
    assert e < tol


# ---- training forward and the recompute re-run -----------------------------------------------------------------------------------------------------------------
@DTYPES
def test_training_forward_and_recompute_rerun(dtype):
    """x_out + y_save + k_save (template KS = 1), then the k_load re-run on x_out (KS = 2, no update): assertions 1, 2, 3 and 5.  Rows 0 .. 63 are 300 +- 0.02."""
    lib, c = _use(dtype), PB.ln_pend_case("d1024_train")
    first = _Launch(c, dtype, x_out=True, y_save=True, k_save=True).run(lib)
    _check_residual(c, dtype, first.x_out, "x_out")
    _check_operand(c, dtype, first)
    _check_inputs(c, first, x_kept=True)
    _check_y_save(lib, c, dtype, first)
    assert _same_bits(first.k_save, c.x[:, 0]), "k_save is not the row's first element before the update"
    # the same launch without k_save runs the KS = 0 template: the same bits
    plain = _Launch(c, dtype, x_out=True, y_save=True).run(lib)
    assert _same_bits(plain.out, first.out) and _same_bits(plain.x_out, first.x_out) and _same_bits(plain.y_save, first.y_save)
    # the re-run from the stored state: no slabs, K read back
    again = _Launch(c, dtype, x=first.x_out.cpu(), slabs=False, k_load=first.k_save).run(lib)
    assert _same_bits(again.out, first.out), "the k_load re-run does not reproduce the forward's operand"
    assert _same_bits(again.x, first.x_out) and again.err.item() == 0


@DTYPES
def test_affine_forward_and_recompute_rerun(dtype):
    """The affine row-block forms that keep and read back the statistics' shift, ln_row_block_kernel<1, true, 1> and <1, false, 2>: no product caller launches them
    (a training handle's LayerNorms modulate), the hook does.  As above: assertions 1, 2, 3 and 5 on x_out + y_save + k_save, the bits of the launch without
    k_save, and the k_load re-run from x_out."""
    lib, c = _use(dtype), PB.ln_pend_case("d192_train")
    first = _Launch(c, dtype, x_out=True, y_save=True, k_save=True).run(lib)
    _check_residual(c, dtype, first.x_out, "x_out")
    _check_operand(c, dtype, first)
    _check_inputs(c, first, x_kept=True)
    _check_y_save(lib, c, dtype, first)
    assert _same_bits(first.k_save, c.x[:, 0]), "k_save is not the row's first element before the update"
    plain = _Launch(c, dtype, x_out=True, y_save=True).run(lib)
    assert _same_bits(plain.out, first.out) and _same_bits(plain.x_out, first.x_out) and _same_bits(plain.y_save, first.y_save)
    again = _Launch(c, dtype, x=first.x_out.cpu(), slabs=False, k_load=first.k_save).run(lib)
    assert _same_bits(again.out, first.out), "the k_load re-run does not reproduce the forward's operand"
    assert _same_bits(again.x, first.x_out) and again.err.item() == 0


@DTYPES
def test_hidden_2048_training_form(dtype):
    lib, c = _use(dtype), PB.ln_pend_case("d2048")
    run = _Launch(c, dtype, x_out=True, y_save=True).run(lib)
    _check_residual(c, dtype, run.x_out, "x_out")
    _check_operand(c, dtype, run)
    _check_inputs(c, run, x_kept=True)
    _check_y_save(lib, c, dtype, run)


# ---- the batch-1 step's launch, repeated ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_in_place_launch_is_reproducible(dtype):
    """720 rows of 1024 in place, five launches from fresh copies: the same bits every time.  In place the updated row overwrites xr[0], which every wave of the
    block reads as the shift of its statistics; a store in front of the block barrier shows as a launch that differs."""
    lib, c = _use(dtype), PB.ln_pend_case("d1024_step")
    first = None
    for rep in range(5):
        run = _Launch(c, dtype).run(lib)
        if first is None:
            first = run
            _check_residual(c, dtype, run.x)
            _check_operand(c, dtype, run)
            _check_inputs(c, run, x_kept=False)
        else:
            assert _same_bits(run.out, first.out) and _same_bits(run.x, first.x), f"launch {rep} differs from launch 0"


# ---- saturation of the branch image -----------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_branch_image_beyond_fp16(dtype):
    """Two sums beyond 65504: fp16 clamps to +-65504 in y_save AND in launch_branch_rows and raises exactly ERR_F16_SAT, in a word that already holds another
    bit; bf16 rounds the value and raises nothing.  (The LayerNorm launch used to clamp y_save in silence: the word stayed at 1.)"""
    lib, c = _use(dtype), PB.ln_pend_sat_case()
    run = _Launch(c, dtype, x_out=True, y_save=True, err0=ERR_TIMESTEP).run(lib)
    want = c.y_save(dtype)
    assert _same_bits(run.y_save, want)
    assert run.y_save[3, 5].item() == (PB.F16_MAX if dtype is F16 else 79872.0) and run.y_save[6, 60].item() == (-PB.F16_MAX if dtype is F16 else -70144.0)
    expect = ERR_TIMESTEP | (ERR_F16_SAT if dtype is F16 else 0)
    assert run.err.item() == expect, f"LayerNorm launch: error word {run.err.item()}, expected {expect}"
    assert torch.isfinite(untile_typed(run.out, c.M, c.D).float()).all() and torch.isfinite(run.x_out).all()
    y = _nan((c.M, c.ld), dtype)
    err = torch.full((1,), ERR_TIMESTEP, device=dev(), dtype=torch.int32)
    L.check(lib.gtav_op_branch_rows(run.parts.data_ptr(), c.nsplit, c.M * c.ld, c.ld, L.ptr(run.bias), y.data_ptr(), c.M, c.D, err.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert _same_bits(y, want) and err.item() == expect, f"launch_branch_rows: error word {err.item()}, expected {expect}"


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
def _refusals(run, k):
    """(name, fields replaced in the descriptor, the launcher's message)"""
    c = run.c
    upd = f"ln_{'modulate' if c.mode == 0 else 'affine'}: bad pending update"
    return [("nsplit 0", dict(nsplit=0), upd), ("nsplit 9", dict(nsplit=9), upd), ("ld % 4", dict(ld=c.ld + 2), upd),
            ("gate with rows_per_gate 0", dict(rows_per_gate=0), upd),
            ("k_save without slabs", dict(parts=0, k_save=k.data_ptr()), "ln: k_save needs a pending update and excludes k_load"),
            ("k_save with k_load", dict(k_save=k.data_ptr(), k_load=k.data_ptr()), "ln: k_save needs a pending update and excludes k_load"),
            ("k_load with slabs", dict(k_load=k.data_ptr()), "ln: k_load excludes a pending update"),
            ("tperm_P % 16", dict(tperm_T=5, tperm_P=8), "ln: bad output row permutation"),
            ("M % (T P)", dict(tperm_T=3, tperm_P=16), "ln: bad output row permutation")]


@DTYPES
def test_bad_descriptors_are_refused_by_name(dtype):
    """The hook validates nothing: these are the launchers' own refusals, each by its message and before any launch — every buffer keeps its bits."""
    lib, c = _use(dtype), PB.ln_pend_case("d256_rows")                    # gated, M = 160 = 2 x 5 x 16
    run = _Launch(c, dtype, x_out=True, y_save=True)
    k = _nan((c.M,), torch.float32)
    snap, ksnap = run.snapshot(), _bits(k)
    for name, over, msg in _refusals(run, k):
        rc = lib.gtav_op_ln_pending(*run.args(**over))
        assert rc != 0, f"{name}: accepted"
        assert lib.gtav_last_error().decode() == msg, (name, lib.gtav_last_error().decode())
    torch.cuda.synchronize()
    assert run.changed(snap) == [] and torch.equal(_bits(k), ksnap)
    aff = _Launch(PB.ln_pend_case("d192"), dtype)                         # the affine launcher has its own check of the descriptor
    asnap = aff.snapshot()
    for name, over in (("nsplit 0", dict(nsplit=0)), ("nsplit 9", dict(nsplit=9)), ("ld % 4", dict(ld=202))):
        assert lib.gtav_op_ln_pending(*aff.args(**over)) != 0, f"affine {name}: accepted"
        assert lib.gtav_last_error().decode() == "ln_affine: bad pending update"
    torch.cuda.synchronize()
    assert aff.changed(asnap) == []
    # launch_branch_rows: the same slab descriptor
    y = _nan((c.M, c.ld), dtype)
    for ns, ld in ((0, c.ld), (9, c.ld), (3, c.ld + 2)):
        assert lib.gtav_op_branch_rows(run.parts.data_ptr(), ns, c.M * c.ld, ld, 0, y.data_ptr(), c.M, c.D, 0, stream()) != 0
        assert lib.gtav_last_error().decode().startswith("branch_rows: bad slabs")
    torch.cuda.synchronize()
    assert torch.isnan(y).all()
    # and the accepted descriptor still runs
    run.run(lib)
    _check_residual(c, dtype, run.x_out, "x_out after the refusals")
