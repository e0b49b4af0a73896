"""Kernel-level parity of the backward-only training kernels (csrc/train.hip) on the GPU, through the test hooks gtav_op_train_* (include/gtav_amd_testing.h):
the LayerNorm + modulate backward with its per-frame reductions, the gate and GELU backward with their bias sums (fused AND unfused forms), the column-sum
family, the loss gradient, the layout converters and the fp32 conditioning path — typed kernels in BOTH operand types (gtav_op_set_operand_dtype).

References are fp64 math on the same rounded operands; inputs, references and bounds come from tests/parity_bounds.py, where every bound is derived, and
tests/test_host_parity_bounds.py shows on the CPU that a correct fp32 emulation stays inside each and the wrong variants do not.  None is taken from what a
kernel returned.  Operands are laid out on the host (helpers.tiled_index).  Every buffer a launch writes starts as NaNs of a fixed bit pattern (accumulating
outputs: random values) with spare rows / a spare row tile / neighbouring columns behind it: whatever the launch has no business writing must come back bit
for bit.  `pytest -s` prints, per case, the worst ratio error / bound (profiles/op_parity_train/margins.txt is such a printout).

The last section runs whole-model gradients at hidden sizes whose training step takes the kernels no other model test reaches."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import parity_bounds as PB  # noqa: E402
from helpers import assert_declared_plan, dev, stream, tiled_index  # noqa: E402
from gtav_amd import lib as L  # noqa: E402
from train_cases import GRAD_TOL  # noqa: E402

F16, BF16 = PB.F16, PB.BF16
DTYPES = pytest.mark.parametrize("dtype", PB.DTYPES, ids=[PB.NAME[d] for d in PB.DTYPES])
FUSED = pytest.mark.parametrize("fused", [1, 0], ids=["fused", "unfused"])
NAN16, NAN32 = 0x7FA5, 0x7FC00123        # a NaN in fp16, in bf16 and in fp32: what every buffer holds before a launch


@pytest.fixture(autouse=True)
def _restore_hooks():
    yield
    L.load().gtav_op_set_operand_dtype(0)


def _use(dtype=None):
    L.load().gtav_op_set_operand_dtype(1 if dtype is BF16 else 0)
    return L.load()


def _up(n, m):
    return (n + m - 1) // m * m


def _within(name, got, ref, tol, dtype=None):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), name
    frac, worst = PB.outside((got - ref).abs(), tol.expand_as(ref) if isinstance(tol, torch.Tensor) and tol.dim() else tol)
    print(f"[margin {name}{' ' + PB.NAME[dtype] if dtype else ''}] per element: worst error / bound {worst:.3f}")
    assert worst <= 1.0, (name, worst, frac)


def _row_within(name, got, ref, tol):
    e = PB.row_rel_l2(got.double().cpu(), ref)
    print(f"[margin {name}] worst row rel-L2 {e:.3e} = {e / tol:.3f} of the bound")
    assert e < tol, (name, e, tol)


# ---- buffers: NaN-filled, with the part a launch may write named, and the rest compared bit for bit afterwards -----------------------------------------------
def _nan32(*shape):
    return torch.full(shape, NAN32, dtype=torch.int32, device=dev()).view(torch.float32)


def _nan16(n, dtype):
    return torch.full((n,), NAN16, dtype=torch.int16, device=dev()).view(dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _untouched(name, buf, before, written):
    """`written`: bool mask (CPU, the buffer's shape) of the elements the launch may write; every other element still holds the bits of `before`"""
    now, was = _bits(buf).reshape(-1), _bits(before).reshape(-1)
    keep = ~written.reshape(-1)
    assert torch.equal(now[keep], was[keep]), f"{name}: a launch wrote outside its output ({int((now[keep] != was[keep]).sum())} elements)"


def _tiled_host(x, dtype, rows=None):
    """(R, K) values -> tile-major 2-byte image of round_up(rows or R, 128) x K on the GPU, laid out on the host; every pad row holds NaN"""
    R, K = x.shape
    Rp = _up(rows or R, 128)
    flat = torch.full((Rp * K,), NAN16, dtype=torch.int16)
    flat[tiled_index(R, K).reshape(-1)] = x.to(dtype).contiguous().view(torch.int16).reshape(-1)
    return flat.view(dtype).to(dev())


class _TiledOut:
    """a tile-major 2-byte output of logical (R, K), `written_rows` of which the launch writes, inside a NaN-filled buffer with one spare row tile"""

    def __init__(self, R, K, dtype, written_rows=None):
        self.R, self.K, self.dtype = R, K, dtype
        self.n = (_up(R, 128) + 128) * K
        self.buf = _nan16(self.n, dtype)
        self.before = self.buf.clone()
        self.written = torch.zeros(self.n, dtype=torch.bool)
        self.written[tiled_index(written_rows or R, K).reshape(-1)] = True

    def values(self, name, rows=None):
        """the logical rows as a CPU tensor, after checking that nothing else was written"""
        _untouched(name, self.buf, self.before, self.written)
        flat = self.buf.view(torch.int16).cpu()
        return flat[tiled_index(rows or self.R, self.K).reshape(-1)].reshape(rows or self.R, self.K).view(self.dtype)


class _Table:
    """an fp32 table [rows][stride] of random values in which the named column blocks (offset -> values, None = NaN) are set; everything else is a sentinel"""

    def __init__(self, rows, stride, blocks, width, seed=11):
        t = PB.rand(rows + 1, stride, seed=seed)
        self.written = torch.zeros(rows + 1, stride, dtype=torch.bool)
        for off, vals in blocks.items():
            t[:rows, off:off + width] = torch.full((rows, width), float("nan")) if vals is None else vals
            self.written[:rows, off:off + width] = True
        self.buf = t.to(dev())
        self.before = self.buf.clone()
        self.rows, self.width = rows, width

    def at(self, off):
        return self.buf[:, off:]         # a view whose data_ptr is the block's first element

    def block(self, name, off):
        _untouched(name, self.buf, self.before, self.written)
        return self.buf[:self.rows, off:off + self.width]


class _Ws:
    """a workspace of `need` floats with 64 sentinel floats behind it"""

    def __init__(self, need):
        self.need = int(need)
        self.buf = _nan32(self.need + 64)
        self.before = self.buf.clone()

    def check(self, name):
        w = torch.zeros(self.need + 64, dtype=torch.bool)
        w[:self.need] = True
        _untouched(name + " workspace", self.buf, self.before, w)


class _Err:
    """the caller's device error word between three sentinel words"""

    def __init__(self):
        self.buf = torch.tensor([0x1234, 0, 0x5678, 0x9ABC], dtype=torch.int32, device=dev())

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4

    def expect(self, name, bits):
        assert self.buf.cpu().tolist() == [0x1234, bits, 0x5678, 0x9ABC], (name, self.buf.cpu().tolist())


def _refused(rc, text):
    assert rc != 0, f"accepted: {text}"
    msg = L.load().gtav_last_error().decode()
    assert text in msg, msg


# ---- 1. LayerNorm + modulate backward and its per-frame reductions (fp32) --------------------------------------------------------------------------------------
def _ln_ws_need(fused, c):
    return c.frames * ((c.P + 15) // 16) * 2 * c.D if fused else 2 * c.M


def _run_ln_bwd(c, fused, accumulate):
    lib = _use()
    D, M = c.D, c.M
    if fused:
        assert_declared_plan("ln_mod_bwd_fused", c.frames, c.P, D)
    dxn, x, mod = c.dxn.to(dev()), c.x.to(dev()), c.mod.to(dev())
    dres = torch.cat((c.old if accumulate else torch.full((M, D), float("nan")), PB.rand(1, D, seed=12))).to(dev())      # one spare row
    dres_before = dres.clone()
    out = _Table(c.frames, c.stride, {c.SH: None, c.DS: None}, D)
    ws = _Ws(_ln_ws_need(fused, c))
    L.check(lib.gtav_op_train_ln_mod_bwd(fused, dxn.data_ptr(), x.data_ptr(), mod[:, c.SC:].data_ptr(), c.stride, c.frames, c.P, D, dres.data_ptr(), accumulate,
                                         out.at(c.SH).data_ptr(), out.at(c.DS).data_ptr(), ws.buf.data_ptr(), ws.need, stream()))
    torch.cuda.synchronize()
    name = f"ln_mod_bwd D={D} frames={c.frames} P={c.P} {'fused' if fused else 'unfused'} accumulate={accumulate}"
    w = torch.zeros(M + 1, D, dtype=torch.bool)
    w[:M] = True
    _untouched(name + " dres", dres, dres_before, w)
    ws.check(name)
    return name, dres[:M], out.block(name, c.SH), out.block(name, c.DS)


LN_BWD_RUNS = [(D, f, P, 1) for (D, f, P) in PB.LN_BWD_SHAPES if D in PB.LN_BWD_FUSED_D] + [(D, f, P, 0) for (D, f, P) in PB.LN_BWD_SHAPES]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("D,frames,P,fused", LN_BWD_RUNS)
def test_ln_mod_bwd(D, frames, P, fused, accumulate):
    c = PB.ln_bwd_case(D, frames, P)
    name, dres, dshift, dscale = _run_ln_bwd(c, fused, accumulate)
    _within(name + " dres", dres, c.ref_dres(accumulate), c.tol_dres(accumulate))
    _within(name + " dshift", dshift, c.ref_dshift, c.tol_dshift)
    _within(name + " dscale", dscale, c.ref_dscale, c.tol_dscale)


@FUSED
@pytest.mark.parametrize("D,frames,P", PB.LN_BWD_LARGE_MEAN, ids=[str(d) for d, _, _ in PB.LN_BWD_LARGE_MEAN])
def test_ln_mod_bwd_large_mean_rows(D, frames, P, fused):
    """rows of 300 +- 0.02 (PB.LnBwdCase): dres and dscale per row under LN_TOL, and everything per element.  The kernels formed x - fl(mean x) when this test was
    written: dscale was at 1.3 of its per-row bound, as the fp32 emulation of that form is (tests/test_host_parity_bounds.py); they now centre the row on its first
    element, like the forward LayerNorm."""
    c = PB.ln_bwd_case(D, frames, P, True)
    name, dres, dshift, dscale = _run_ln_bwd(c, fused, 0)
    _row_within(name + " large mean dres", dres, c.ref_dres(0), PB.LN_TOL)
    _row_within(name + " large mean dscale", dscale, c.ref_dscale, PB.LN_TOL)
    _within(name + " large mean dres", dres, c.ref_dres(0), c.tol_dres(0))
    _within(name + " large mean dshift", dshift, c.ref_dshift, c.tol_dshift)
    _within(name + " large mean dscale", dscale, c.ref_dscale, c.tol_dscale)


def test_ln_mod_bwd_refusals():
    lib = _use()
    c = PB.ln_bwd_case(384, 2, 24)
    buf = _nan32(c.M * c.D)
    tab = _nan32(c.frames * c.stride)
    args = lambda fused, D, ws_floats: (fused, buf.data_ptr(), buf.data_ptr(), tab.data_ptr(), 3 * D + 64, 2, 24, D, buf.data_ptr(), 0, tab.data_ptr(), tab.data_ptr(),
                                        buf.data_ptr(), ws_floats, stream())
    _refused(lib.gtav_op_train_ln_mod_bwd(*args(1, 384, 1 << 20)), "the fused launch exists at D = 256, 512, 1024 and 2048 only, not at D=384")
    _refused(lib.gtav_op_train_ln_mod_bwd(*args(1, 256, 2 * 2 * 2 * 256 - 1)), "op_train_ln_mod_bwd (fused): workspace of 2047 floats, 2048 needed")
    _refused(lib.gtav_op_train_ln_mod_bwd(*args(0, 384, 2 * 48 - 1)), "op_train_ln_mod_bwd (row statistics): workspace of 95 floats, 96 needed")
    torch.cuda.synchronize()
    assert (_bits(buf) == NAN32).all() and (_bits(tab) == NAN32).all()            # a refused call launches nothing


# ---- 2. gate backward ---------------------------------------------------------------------------------------------------------------------------------------
def _colsum_ws(M, N):
    return ((M + 255) // 256) * _up(N, 256)            # csrc/train.hip colsum_workspace


def _run_gate_bwd(c, fused, with_db=True):
    lib = _use(c.dtype)
    D, M, frames, P = c.D, c.M, c.frames, c.P
    dres, y, mod = c.dres.to(dev()), c.y.to(dev()), c.mod.to(dev())
    dy = _TiledOut(M, D, c.dtype)
    dgate = _Table(frames, c.stride, {c.G: None}, D)
    db = torch.cat((c.db0, PB.rand(32, seed=13))).to(dev())
    db_before = db.clone()
    ws = _Ws(frames * D if fused else _colsum_ws(M, D))
    err = _Err()
    L.check(lib.gtav_op_train_gate_bwd(fused, dres.data_ptr(), y.data_ptr(), mod[:, c.G:].data_ptr() if c.gate is not None else 0, c.stride, frames, P, D,
                                       dy.buf.data_ptr(), dgate.at(c.G).data_ptr(), db.data_ptr() if with_db else 0, ws.buf.data_ptr(), ws.need, err.ptr, stream()))
    torch.cuda.synchronize()
    name = f"gate_bwd D={D} frames={frames} P={P} {'fused' if fused else 'unfused'} gate={'yes' if c.gate is not None else 'null'}"
    w = torch.zeros(D + 32, dtype=torch.bool)
    w[:D] = with_db
    _untouched(name + " db", db, db_before, w)
    ws.check(name)
    return name, dy.values(name + " dy"), dgate.block(name + " dgate", c.G), db[:D], ws, err


@DTYPES
@pytest.mark.parametrize("gated", [True, False], ids=["gate", "nogate"])
@FUSED
@pytest.mark.parametrize("D,frames,P", PB.GATE_BWD_SHAPES)
def test_gate_bwd(D, frames, P, fused, gated, dtype):
    """rows M .. round_up(M, 128) of dy and the spare tile stay untouched (_TiledOut), like the neighbouring columns of the dgate table and the words behind db"""
    c = PB.gate_bwd_case(D, frames, P, dtype, gated)
    name, dy, dgate, db, _, err = _run_gate_bwd(c, fused)
    err.expect(name, 0)
    _within(name + " dy", dy, c.ref_dy, c.tol_dy, dtype)
    _within(name + " dgate", dgate, c.ref_dgate, c.tol_dgate, dtype)
    _within(name + " db", db, c.ref_db, c.tol_db(bool(fused)), dtype)


@DTYPES
def test_gate_bwd_deferred_bias_and_colsum_reduce_multi(dtype):
    """db null: the fused launch leaves its per-frame partial sums in ws; one colsum_reduce_multi launch then adds them, beside a second job of another width"""
    lib = _use(dtype)
    c = PB.gate_bwd_case(256, 3, 24, dtype)
    name, dy, dgate, _, ws, err = _run_gate_bwd(c, 1, with_db=False)
    _within(name + " deferred dy", dy, c.ref_dy, c.tol_dy, dtype)
    other = PB.colsum_case(7, 100)                          # 7 splits of 100 columns
    ws2 = other.a.to(dev())
    db = [torch.cat((c.db0, PB.rand(32, seed=13))).to(dev()), torch.cat((other.db0, PB.rand(32, seed=14))).to(dev())]
    before = [d.clone() for d in db]
    L.check(lib.gtav_op_train_colsum_reduce_multi((C.c_void_p * 2)(ws.buf.data_ptr(), ws2.data_ptr()), (C.c_void_p * 2)(db[0].data_ptr(), db[1].data_ptr()),
                                                  (C.c_int32 * 2)(c.frames, 7), (C.c_int32 * 2)(c.D, 100), 2, stream()))
    torch.cuda.synchronize()
    for d, b, n in zip(db, before, (c.D, 100)):
        w = torch.zeros(n + 32, dtype=torch.bool)
        w[:n] = True
        _untouched(name + " deferred db", d, b, w)
    _within(name + " deferred db", db[0][:c.D], c.ref_db, c.tol_db(True), dtype)
    _within(name + " second job", db[1][:100], other.ref, other.tol)


@DTYPES
@FUSED
@pytest.mark.parametrize("gated", [True, False], ids=["gate", "nogate"])
def test_gate_bwd_saturation(fused, gated, dtype):
    """one product of 70000: fp16 stores +-65504 there and raises ERR_F16_SAT in the caller's word and nothing else; bf16 stores the rounded value, no bit"""
    c = PB.gate_bwd_case(128, 2, 5, dtype, gated, True)
    name, dy, dgate, db, _, err = _run_gate_bwd(c, fused)
    m0, d0 = c.sat_at
    ref, tol = c.ref_dy.clone(), c.tol_dy
    if dtype is F16:
        err.expect(name, PB.ERR_F16_SAT)
        assert abs(dy[m0, d0].item()) == PB.F16_MAX and dy[m0, d0].item() * ref[m0, d0].item() > 0
        ref[m0, d0] = dy[m0, d0].double()
    else:
        err.expect(name, 0)
    _within(name + " saturation dy", dy, ref, tol, dtype)
    _within(name + " saturation dgate", dgate, c.ref_dgate, c.tol_dgate, dtype)


def test_gate_bwd_refusals():
    lib = _use()
    b = _nan32(4096)
    args = lambda fused, db, ws_floats: (fused, b.data_ptr(), b.data_ptr(), 0, 128, 2, 5, 128, b.data_ptr(), b.data_ptr(), db, b.data_ptr(), ws_floats, 0, stream())
    _refused(lib.gtav_op_train_gate_bwd(*args(1, b.data_ptr(), 255)), "op_train_gate_bwd (fused): workspace of 255 floats, 256 needed")
    _refused(lib.gtav_op_train_gate_bwd(*args(0, b.data_ptr(), 255)), "op_train_gate_bwd (column sums): workspace of 255 floats, 256 needed")
    _refused(lib.gtav_op_train_gate_bwd(*args(0, 0, 256)), "the unfused form adds its column sums to db, which is null")
    torch.cuda.synchronize()
    assert (_bits(b) == NAN32).all()


# ---- 3. GELU backward with the fc1 bias sums ----------------------------------------------------------------------------------------------------------------
def _run_gelu_bwd(c, fused, with_db=True):
    lib = _use(c.dtype)
    M, N = c.M, c.N
    Mp = _up(M, 128)
    dh, u = _tiled_host(c.dh, c.dtype), _tiled_host(c.u, c.dtype)              # pad rows: NaN
    du = _TiledOut(M, N, c.dtype, written_rows=Mp)                             # the whole padded image is transformed
    db = torch.cat((c.db0, PB.rand(32, seed=13))).to(dev())
    db_before = db.clone()
    ws = _Ws(((Mp + 511) // 512) * N if fused else _colsum_ws(M, N))
    err = _Err()
    L.check(lib.gtav_op_train_gelu_bwd(fused, dh.data_ptr(), u.data_ptr(), du.buf.data_ptr(), M, N, db.data_ptr() if with_db else 0, ws.buf.data_ptr(), ws.need, err.ptr,
                                       stream()))
    torch.cuda.synchronize()
    name = f"gelu_bwd {M}x{N} {'fused' if fused else 'unfused'}"
    w = torch.zeros(N + 32, dtype=torch.bool)
    w[:N] = with_db
    _untouched(name + " db", db, db_before, w)
    ws.check(name)
    return name, du.values(name + " du", M), (db[:N] if with_db else (db, db_before, ws)), err


@DTYPES
@pytest.mark.parametrize("sweep", [True, False], ids=["sweep", "random"])
@FUSED
@pytest.mark.parametrize("M,N", PB.GELU_BWD_SHAPES)
def test_gelu_bwd(M, N, fused, sweep, dtype):
    """the pad rows of dh and u hold NaN: db stays finite and inside its bound, du of the real rows inside its own"""
    c = PB.gelu_bwd_case(M, N, dtype, sweep)
    name, du, db, err = _run_gelu_bwd(c, fused)
    name += " sweep" if sweep else " random"
    err.expect(name, 0)
    _within(name + " du", du, c.ref_du, c.tol_du, dtype)
    _within(name + " db", db, c.ref_db, c.tol_db(bool(fused)), dtype)


@DTYPES
def test_gelu_bwd_deferred_bias(dtype):
    """db null, as a training handle launches it: the per-split partial sums stay in ws (3 row splits here) and colsum_reduce_multi adds them in split order"""
    c = PB.gelu_bwd_case(1100, 128, dtype, False)
    name, du, (db, before, ws), err = _run_gelu_bwd(c, 1, with_db=False)
    _within(name + " deferred du", du, c.ref_du, c.tol_du, dtype)
    L.check(_use(dtype).gtav_op_train_colsum_reduce_multi((C.c_void_p * 1)(ws.buf.data_ptr()), (C.c_void_p * 1)(db.data_ptr()), (C.c_int32 * 1)(3), (C.c_int32 * 1)(c.N), 1, stream()))
    torch.cuda.synchronize()
    w = torch.zeros(c.N + 32, dtype=torch.bool)
    w[:c.N] = True
    _untouched(name + " deferred db", db, before, w)
    _within(name + " deferred db", db[:c.N], c.ref_db, c.tol_db(True), dtype)


@DTYPES
@FUSED
def test_gelu_bwd_saturation(fused, dtype):
    c = PB.gelu_bwd_case(100, 128, dtype, False, True)
    name, du, db, err = _run_gelu_bwd(c, fused)
    at = c.sat_at
    ref = c.ref_du.clone()
    assert ref[at].item() > PB.F16_MAX
    if dtype is F16:
        err.expect(name, PB.ERR_F16_SAT)
        assert du[at].item() == PB.F16_MAX
        ref[at] = PB.F16_MAX
    else:
        err.expect(name, 0)
    _within(name + " saturation du", du, ref, c.tol_du, dtype)


def test_gelu_bwd_refusals():
    lib = _use()
    b = _nan32(128 * 128)
    args = lambda fused, M, ws_floats: (fused, b.data_ptr(), b.data_ptr(), b.data_ptr(), M, 128, b.data_ptr(), b.data_ptr(), ws_floats, 0, stream())
    _refused(lib.gtav_op_train_gelu_bwd(*args(1, 513, 255)), "op_train_gelu_bwd (fused): workspace of 255 floats, 256 needed")
    _refused(lib.gtav_op_train_gelu_bwd(*args(0, 513, 767)), "op_train_gelu_bwd (column sums): workspace of 767 floats, 768 needed")
    torch.cuda.synchronize()
    assert (_bits(b) == NAN32).all()


# ---- 4. column sums -------------------------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("N", PB.COLSUM_TILED_N)
@pytest.mark.parametrize("M", PB.COLSUM_TILED_M)
def test_colsum_tiled(M, N, dtype):
    """two launches into one db: the second accumulates.  Pad rows of the image hold NaN."""
    lib = _use(dtype)
    c = PB.colsum_case(M, N, dtype, 2)
    a = _tiled_host(c.a, dtype)
    db = torch.cat((c.db0, PB.rand(32, seed=13))).to(dev())
    before = db.clone()
    ws = _Ws(_colsum_ws(M, N))
    for _ in range(2):
        L.check(lib.gtav_op_train_colsum_tiled(a.data_ptr(), M, N, db.data_ptr(), ws.buf.data_ptr(), ws.need, stream()))
    torch.cuda.synchronize()
    w = torch.zeros(N + 32, dtype=torch.bool)
    w[:N] = True
    _untouched("colsum_tiled db", db, before, w)
    ws.check("colsum_tiled")
    _within(f"colsum_tiled {M}x{N} two launches", db[:N], c.ref, c.tol, dtype)


@pytest.mark.parametrize("N", PB.COLSUM_F32_N)
@pytest.mark.parametrize("M", PB.COLSUM_F32_M)
def test_colsum_f32(M, N):
    lib = _use()
    c = PB.colsum_case(M, N)
    lda = N + 3
    a = torch.full((M + 1, lda), float("nan"))
    a[:M, :N] = c.a
    a = a.to(dev())
    db = torch.cat((c.db0, PB.rand(32, seed=13))).to(dev())
    before = db.clone()
    ws = _Ws(_colsum_ws(M, N))
    L.check(lib.gtav_op_train_colsum_f32(a.data_ptr(), lda, M, N, db.data_ptr(), ws.buf.data_ptr(), ws.need, stream()))
    torch.cuda.synchronize()
    w = torch.zeros(N + 32, dtype=torch.bool)
    w[:N] = True
    _untouched("colsum_f32 db", db, before, w)
    ws.check("colsum_f32")
    _within(f"colsum_f32 {M}x{N} lda={lda}", db[:N], c.ref, c.tol)


@pytest.mark.parametrize("njobs", [1, 2, 3, 4])
def test_colsum_reduce_multi(njobs):
    """jobs of different widths (none a multiple of 32) and split counts on both sides of the kernel's eight split lanes"""
    lib = _use()
    widths = (50, 100, 33, 70)
    splits = {1: (17,), 2: (1, 9), 3: (7, 8, 9), 4: (1, 7, 8, 17)}[njobs]
    cases = [PB.colsum_case(s, n) for s, n in zip(splits, widths)]
    ws = [c.a.to(dev()) for c in cases]
    db = [torch.cat((c.db0, PB.rand(32, seed=13))).to(dev()) for c in cases]
    before = [d.clone() for d in db]
    P = C.c_void_p * njobs
    I = C.c_int32 * njobs
    L.check(lib.gtav_op_train_colsum_reduce_multi(P(*[w.data_ptr() for w in ws]), P(*[d.data_ptr() for d in db]), I(*splits), I(*widths[:njobs]), njobs, stream()))
    torch.cuda.synchronize()
    for c, d, b in zip(cases, db, before):
        w = torch.zeros(c.N + 32, dtype=torch.bool)
        w[:c.N] = True
        _untouched("colsum_reduce_multi db", d, b, w)
        _within(f"colsum_reduce_multi {njobs} jobs: {c.M} splits x {c.N}", d[:c.N], c.ref, c.tol)
    _refused(lib.gtav_op_train_colsum_reduce_multi(P(*[w.data_ptr() for w in ws]), P(*[d.data_ptr() for d in db]), I(*splits), I(*widths[:njobs]), 5, stream()),
             "colsum_reduce_multi: 5 jobs")


# ---- 5. the loss gradient ---------------------------------------------------------------------------------------------------------------------------------------
def _run_mse_bwd(c):
    from oracle import ref_cpu as O
    lib = _use(c.dtype)
    B, T, Cc, H, W, p = c.shape
    gh, gw, F, ldf = H // p, W // p, Cc * p * p, c.ldf
    M = B * T * gh * gw
    dfo = _TiledOut(M, ldf, c.dtype)
    err = _Err()
    vp, vt = c.vpred.to(dev()), c.vtarget.to(dev())
    L.check(lib.gtav_op_train_mse_bwd_patch(vp.data_ptr(), vt.data_ptr(), B, T, Cc, H, W, p, c.scale, dfo.buf.data_ptr(), ldf, err.ptr, stream()))
    torch.cuda.synchronize()
    name = f"mse_bwd_patch {c.shape} ldf={ldf}"
    tok = dfo.values(name)                                                        # [M][ldf], rows M .. round_up(M, 128) untouched
    assert (tok[:, F:].view(torch.int16) == 0).all(), "columns F .. ldf must be exactly zero"
    img = O.dit_unpatchify(tok[:, :F].float().reshape(B * T, gh, gw, F), O.DiTConfig(input_h=H, input_w=W, patch_size=p, in_channels=Cc)).reshape(B, T, Cc, H, W)
    assert (img[:, :T - 1] == 0).all(), "frames other than the last must be exactly zero"
    return name, img, err


@DTYPES
@pytest.mark.parametrize("shape", PB.MSE_BWD_SHAPES, ids=["F64", "F12"])
def test_mse_bwd_patch(shape, dtype):
    """the token order is the inverse of DiT.unpatchify: the oracle's unpatchify of the launch's tokens is the gradient image"""
    c = PB.mse_bwd_case(*shape, dtype)
    name, img, err = _run_mse_bwd(c)
    err.expect(name, 0)
    _within(name, img, c.ref, c.tol, dtype)


@DTYPES
def test_mse_bwd_patch_saturation(dtype):
    c = PB.mse_bwd_case(*PB.MSE_BWD_SHAPES[0], dtype, True)
    name, img, err = _run_mse_bwd(c)
    b, ch, yy, xx = c.sat_at
    ref = c.ref.clone()
    assert ref[b, -1, ch, yy, xx].item() > PB.F16_MAX
    if dtype is F16:
        err.expect(name, PB.ERR_F16_SAT)
        assert img[b, -1, ch, yy, xx].item() == PB.F16_MAX
        ref[b, -1, ch, yy, xx] = PB.F16_MAX
    else:
        err.expect(name, 0)
    _within(name + " saturation", img, ref, c.tol, dtype)


# ---- 6. layout converters: bit for bit -----------------------------------------------------------------------------------------------------------------------------
LAYOUT_R, LAYOUT_C = (1, 63, 64, 65, 200), (64, 192)


def _same_bits(name, got, want):
    assert torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)), f"{name}: {int((got.view(torch.int16) != want.view(torch.int16)).sum())} elements differ"


@DTYPES
@pytest.mark.parametrize("Cc", LAYOUT_C)
@pytest.mark.parametrize("R", LAYOUT_R)
def test_to_tiled(R, Cc, dtype):
    lib = _use(dtype)
    a = PB.rand(R, Cc, seed=1, scale=30.0)
    a[0, 0], a[R - 1, Cc - 1] = 2.0 ** -26, -(1.0 + 2.0 ** -9)              # below half a subnormal step of fp16; a tie of bf16
    out, err = _TiledOut(R, Cc, dtype), _Err()
    ad = a.to(dev())
    L.check(lib.gtav_op_train_to_tiled(ad.data_ptr(), R, Cc, out.buf.data_ptr(), err.ptr, stream()))
    torch.cuda.synchronize()
    err.expect("to_tiled", 0)
    _same_bits(f"to_tiled {R}x{Cc}", out.values("to_tiled"), a.to(dtype))


@DTYPES
@pytest.mark.parametrize("Cc", LAYOUT_C)
@pytest.mark.parametrize("R", LAYOUT_R)
def test_transpose_tiled(R, Cc, dtype):
    """dst logical [C][round_up(R, 64)]: the host permutation bit for bit, zeros in the K padding; the pad rows of src hold NaN and are never read"""
    lib = _use(dtype)
    Rp = _up(R, 64)
    a = PB.rand(R, Cc, seed=1).to(dtype)
    src = _tiled_host(a, dtype)
    out = _TiledOut(Cc, Rp, dtype)
    L.check(lib.gtav_op_train_transpose_tiled(src.data_ptr(), R, Cc, out.buf.data_ptr(), stream()))
    torch.cuda.synchronize()
    got = out.values("transpose_tiled")
    _same_bits(f"transpose_tiled {R}x{Cc}", got[:, :R], a.t())
    assert (got[:, R:].view(torch.int16) == 0).all(), "K padding must be zero"


@DTYPES
@pytest.mark.parametrize("Cc", LAYOUT_C + (100,))
@pytest.mark.parametrize("R", LAYOUT_R)
def test_convert_t(R, Cc, dtype):
    """fp32 [R][C] (leading dimension > C) -> the 2-byte transpose [round_up(C, 128)][round_up(R, 64)], zero padding in both directions"""
    lib = _use(dtype)
    Rp, Cp, lds = _up(R, 64), _up(Cc, 128), Cc + 5
    a = PB.rand(R, Cc, seed=1, scale=30.0)
    a[0, 0], a[R - 1, Cc - 1] = 2.0 ** -26, -(1.0 + 2.0 ** -9)
    src = torch.full((R + 1, lds), float("nan"))
    src[:R, :Cc] = a
    src = src.to(dev())
    out = _TiledOut(Cp, Rp, dtype)
    L.check(lib.gtav_op_train_convert_t(src.data_ptr(), lds, R, Cc, out.buf.data_ptr(), stream()))
    torch.cuda.synchronize()
    got = out.values("convert_T")
    _same_bits(f"convert_T {R}x{Cc}", got[:Cc, :R], a.t().to(dtype))
    assert (got[Cc:].view(torch.int16) == 0).all() and (got[:, R:].view(torch.int16) == 0).all(), "padding must be zero"


@DTYPES
def test_layout_converters_saturation(dtype):
    """to_tiled reports a clamped value in the caller's word; convert_T (weights) clamps without a word.  bf16 rounds, nothing is clamped."""
    lib = _use(dtype)
    R, Cc = 65, 64
    a = PB.rand(R, Cc, seed=1)
    a[64, 3], a[2, 60] = 70000.0, -1.0e9
    want = a.to(dtype) if dtype is BF16 else a.clamp(-PB.F16_MAX, PB.F16_MAX).to(dtype)
    ad = a.to(dev())
    out, err = _TiledOut(R, Cc, dtype), _Err()
    L.check(lib.gtav_op_train_to_tiled(ad.data_ptr(), R, Cc, out.buf.data_ptr(), err.ptr, stream()))
    outT = _TiledOut(128, 128, dtype)
    L.check(lib.gtav_op_train_convert_t(ad.data_ptr(), Cc, R, Cc, outT.buf.data_ptr(), stream()))
    torch.cuda.synchronize()
    err.expect("to_tiled saturation", PB.ERR_F16_SAT if dtype is F16 else 0)
    _same_bits("to_tiled saturation", out.values("to_tiled"), want)
    _same_bits("convert_T saturation", outT.values("convert_T")[:Cc, :R], want.t())


# ---- 7. the fp32 conditioning path ---------------------------------------------------------------------------------------------------------------------------------
def _padded(x, ld, seed):
    """(R, C) -> a device buffer [R + 1][ld] of sentinel values with x in its first columns, its CPU copy, and the mask of x"""
    R, Cc = x.shape
    buf = PB.rand(R + 1, ld, seed=seed)
    buf[:R, :Cc] = x
    w = torch.zeros(R + 1, ld, dtype=torch.bool)
    w[:R, :Cc] = True
    d = buf.to(dev())
    return d, d.clone(), w


def test_silu_and_silu_bwd():
    lib = _use()
    c = PB.silu_case()
    R, Cc = c.R, c.C
    x, _, _ = _padded(c.x, Cc + 3, 21)
    dy, _, _ = _padded(c.dy, Cc + 9, 22)
    nan = torch.full((R, Cc), float("nan"))
    y, y0, wy = _padded(nan, Cc + 5, 23)
    dx, dx0, wdx = _padded(nan, Cc + 1, 24)
    L.check(lib.gtav_op_train_silu(x.data_ptr(), Cc + 3, y.data_ptr(), Cc + 5, R, Cc, stream()))
    L.check(lib.gtav_op_train_silu_bwd(dy.data_ptr(), Cc + 9, x.data_ptr(), Cc + 3, dx.data_ptr(), Cc + 1, R, Cc, stream()))
    torch.cuda.synchronize()
    _untouched("silu y", y, y0, wy)
    _untouched("silu_bwd dx", dx, dx0, wdx)
    _within("silu", y[:R, :Cc], c.ref_y, c.tol_y)
    _within("silu_bwd", dx[:R, :Cc], c.ref_dx, c.tol_dx)


def _run_gemm_tn_f32(name, c, R, N, K, lddy, dy_offset=0):
    lib = _use()
    assert_declared_plan("gemm_tn_f32", R, N, K)
    lddw = K + 4
    flat = torch.full((dy_offset + (R + 1) * lddy,), float("nan"))
    flat[dy_offset:].reshape(R + 1, lddy)[:R, :N] = c.a
    dY = flat.to(dev())
    X, _, _ = _padded(c.b, K + 3, 31)
    dW, dW0, w = _padded(c.old, lddw, 32)
    L.check(lib.gtav_op_train_gemm_tn_f32(dY.data_ptr() + 4 * dy_offset, lddy, X.data_ptr(), K + 3, R, N, K, dW.data_ptr(), lddw, stream()))
    torch.cuda.synchronize()
    _untouched(name, dW, dW0, w)
    _within(name, dW[:N, :K], c.ref, c.tol)


@pytest.mark.parametrize("R,N,K", PB.GEMM_TN_F32_MFMA)
def test_gemm_tn_f32_matrix_cores(R, N, K):
    """dW += dY^T X into a pre-filled dW with lddw > K"""
    _run_gemm_tn_f32(f"gemm_tn_f32 mfma {R}x{N}x{K}", PB.gemm_f32_case(R, N, K, True, True), R, N, K, N + 4)


@pytest.mark.parametrize("R,N,K,form", PB.GEMM_TN_F32_VALU)
def test_gemm_tn_f32_valu(R, N, K, form):
    """the action embedder's shape on the vector loads, and the two ways to the scalar loads: rows of dY that are not 16-byte multiples, a dY that is not aligned"""
    lddy = {"full": N + 4, "odd lddy": N + 1, "dY offset": N + 4}[form]
    _run_gemm_tn_f32(f"gemm_tn_f32 valu {R}x{N}x{K} {form}", PB.gemm_f32_case(R, N, K, True, False), R, N, K, lddy, 1 if form == "dY offset" else 0)


@pytest.mark.parametrize("R,N,K", PB.GEMM_NN_F32)
def test_gemm_nn_f32(R, N, K):
    """dX = dY W: N = 256 / 2048 / 4096 keep 16 / 8 / 4 rows of dY in LDS"""
    lib = _use()
    assert_declared_plan("gemm_nn_f32", R, N, K)
    c = PB.gemm_f32_case(N, R, K, False, False)
    dY, _, _ = _padded(c.a.t().contiguous(), N + 4, 41)
    W, _, _ = _padded(c.b, K + 3, 42)
    dX, dX0, w = _padded(torch.full((R, K), float("nan")), K + 5, 43)
    L.check(lib.gtav_op_train_gemm_nn_f32(dY.data_ptr(), N + 4, W.data_ptr(), K + 3, R, N, K, dX.data_ptr(), K + 5, stream()))
    torch.cuda.synchronize()
    name = f"gemm_nn_f32 {R}x{N}x{K}"
    _untouched(name, dX, dX0, w)
    _within(name, dX[:R, :K], c.ref, c.tol)


def test_gemm_nn_f32_refuses_rows_beyond_lds():
    lib = _use()
    b = _nan32(8192 + 64)
    _refused(lib.gtav_op_train_gemm_nn_f32(b.data_ptr(), 8192, b.data_ptr(), 1, 1, 8192, 1, b.data_ptr(), 1, stream()), "gemm_nn_f32: N=8192")


def _run_ada_bwd_dx(name, MODW, D, R, mfma):
    lib = _use()
    assert_declared_plan("ada_bwd_dx", MODW, D, R)
    c = PB.gemm_f32_case(MODW, R, D, False, mfma, scale=MODW ** -0.5)
    dmod, W = c.a.t().contiguous().to(dev()), c.b.to(dev())
    dSc, dSc0, w = _padded(torch.full((R, D), float("nan")), D, 51)
    part = _Ws(((MODW + 1023) // 1024) * R * D)                                  # csrc/train.hip ada_bwd_dx_workspace
    L.check(lib.gtav_op_train_ada_bwd_dx(dmod.data_ptr(), MODW, W.data_ptr(), D, R, dSc.data_ptr(), part.buf.data_ptr(), part.need, stream()))
    torch.cuda.synchronize()
    _untouched(name, dSc, dSc0, w)
    part.check(name)
    _within(name, dSc[:R], c.ref, c.tol)


@pytest.mark.parametrize("MODW,D,R", PB.ADA_BWD_MFMA)
def test_ada_bwd_dx_matrix_cores(MODW, D, R):
    _run_ada_bwd_dx(f"ada_bwd_dx mfma MODW={MODW} D={D} R={R}", MODW, D, R, True)


@pytest.mark.parametrize("MODW,D,R", PB.ADA_BWD_VALU)
def test_ada_bwd_dx_valu(MODW, D, R):
    """the launcher takes the VALU kernel where the matrix-core one does not fit: more than 80 conditioning rows, or a hidden size that is no multiple of 64"""
    _run_ada_bwd_dx(f"ada_bwd_dx valu MODW={MODW} D={D} R={R}", MODW, D, R, False)


def test_ada_bwd_dx_needs_its_workspace():
    lib = _use()
    b = _nan32(4096)
    _refused(lib.gtav_op_train_ada_bwd_dx(b.data_ptr(), 64, b.data_ptr(), 64, 1, b.data_ptr(), 0, 0, stream()), "op_train_ada_bwd_dx: workspace of 0 floats, 64 needed")
    _refused(lib.gtav_op_train_ada_bwd_dx(b.data_ptr(), 64, b.data_ptr(), 64, 1, b.data_ptr(), b.data_ptr(), 63, stream()), "op_train_ada_bwd_dx: workspace of 63 floats, 64 needed")


# ---- 8. whole-model gradients at the hidden sizes whose training step runs the other kernels -------------------------------------------------------------------------
# hidden 512: ln_mod_bwd_fused_kernel<2>; hidden 768 (a multiple of 256 without a fused kernel): the two-kernel LayerNorm backward; 1280 and 2048: the widths
# above 1024 (LayerNorm blocks of 5 and 8 waves, ln_mod_bwd_fused_kernel<8>).  Bounds: GRAD_TOL of
# tests/train_cases.py (fp16, and 8 x that in bf16).


def _toy(hidden, heads):
    return dict(input_h=8, input_w=16, patch_size=2, in_channels=16, hidden_size=hidden, depth=2, num_heads=heads, external_cond_dim=25)


@functools.lru_cache(maxsize=None)
def _toy_reference(hidden, heads):
    """(state dict, inputs, the oracle's fp32 autograd gradients), computed once for both operand types"""
    import gtav_amd.weights as W
    from oracle import ref_cpu as O
    kw = _toy(hidden, heads)
    sd = W.synth_state_dict(W.dit_param_shapes(**kw), seed=1)
    g = torch.Generator().manual_seed(0)
    B, T = 2, 3
    x = torch.randn(B, T, 16, 8, 16, generator=g)
    t = torch.randint(0, 1000, (B, T), generator=g)
    a = torch.zeros(B, T, 25)
    a[:, :, 3] = 1
    a[0, T - 1, 7] = 1
    vt = torch.randn(B, 1, 16, 8, 16, generator=g)
    _, v_ref, grads = O.dit_loss_and_grads(sd, O.DiTConfig(**kw), x, t, a, vt)
    return sd, (x, t, a, vt), v_ref, grads


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("hidden,heads", [(512, 8), (768, 12), (1280, 20), (2048, 32)])
def test_model_gradients_at_other_hidden_sizes(hidden, heads, dtype):
    from gtav_amd.model.dit import DiT
    sd, (x, t, a, vt), v_ref, grads = _toy_reference(hidden, heads)
    m = DiT(**_toy(hidden, heads), max_batch=2, max_frames=3, init_weights=False, trainable=True, train_dtype=dtype)
    m.load_state_dict(sd)
    v = m.forward_train(x, t, a)
    m.zero_grad()
    m.backward_(v, vt)
    m.check()
    worst = {}
    for k, gref in grads.items():
        g = m.grad(k).cpu()
        assert torch.isfinite(g).all(), k
        if gref.norm() == 0:
            assert g.abs().max() == 0, k
            continue
        worst[k] = PB.rel_l2(g, gref)
    k = max(worst, key=worst.get)
    print(f"[margin model gradients hidden={hidden} {PB.NAME[dtype]}] worst rel-L2 {worst[k]:.3e} ({k}) = {worst[k] / GRAD_TOL[dtype]:.3f} of the bound")
    bad = {k: e for k, e in worst.items() if e > GRAD_TOL[dtype]}
    assert not bad, f"gradient mismatch: {bad}"


def test_hidden_384_is_refused_by_name():
    """hidden sizes that are no multiple of 256 never reach a training step: the handle refuses them when it is created"""
    from gtav_amd.model.dit import DiT
    import gtav_amd.weights as W
    m = DiT(**_toy(384, 6), max_batch=2, max_frames=3, init_weights=False, trainable=True)
    m.load_state_dict(W.synth_state_dict(W.dit_param_shapes(**_toy(384, 6)), seed=1))
    g = torch.Generator().manual_seed(0)
    with pytest.raises(L.GtavError, match="hidden_size=384 must be a multiple of 256, <= 2048"):
        m.forward_train(torch.randn(2, 3, 16, 8, 16, generator=g), torch.randint(0, 1000, (2, 3), generator=g), None)
