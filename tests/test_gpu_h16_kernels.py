"""Kernel parity of the 16-bit MFMA kernels, the x16 head and pooling kernels and the 16-bit weight packers in BOTH product libraries
(libhyperpri_hip.so: h16_t = bf16; libhyperpri_hip_f16.so: IEEE half, the *_f16 MFMA and ds_read_tr16 builtins), through the C ABI
against fp64 references.  _h16_cases.py has the cases, the references and the bounds; test_h16_cases_cpu.py proves on the CPU what is
relied on here (exact operands, integer budgets below 2^24, lossless edge outputs, a bound that a lost k-step, a shifted input and two
swapped channels each exceed).

Per entry point three kinds of test, every one parametrized over the library:

``int``    small-integer operands: fp32 outputs equal the fp64 reference bit for bit, 16-bit outputs the reference rounded once; the
           statistics records of the row GEMM and of the convolution hold exact counts, means within 64 u of the exact mean (two
           roundings of the per-wave mean of an exact sum, then at most three Chan merges of about five roundings each on differences
           of at most 2 max|v|) and M2 / count within the 1e-4 scale^2 the suite applies to these records elsewhere.
``real``   Gaussian operands rounded to the library's type: |got - ref| <= (n + 2) u (sum |a||b| + |bias| + |prior|) ELEMENTWISE, u = 2^-24,
           n the element's number of terms -- factor 1 in front of u, resting on one assumption: the MFMA's fp32 accumulation rounds to
           nearest per add.  The ratio is recorded as h16/<kernel>/<lib>/<shape>.  A 16-bit view written by the same launch must equal
           the fp32 view rounded once by torch; a 16-bit output without an fp32 twin must lie between torch's roundings of ref - bound
           and ref + bound (rounding is monotone).  Statistics: means within (256 + 64) u (any order of at most 256 adds, then the merges).
``range``  the edge tables: roundings to nearest even, half's subnormals (as operands of the MFMA and as stored values), overflow to inf
           at 65520 -- expected bits are torch's.

Every output buffer is compared in FULL with its expected contents: the channels beside a channel-slice view, the pad columns, the
canvas ring of the transposed forms (a sentinel everywhere a launch must not write, exact zeros where the contract zero-fills).  A
failure names the first wrong (row, channel).

Loss scale (hpri_set_loss_scale): what it multiplies (the gradient the fused heads form from logits and target), exactly (a power of
two), what it leaves alone (a plain dy), that it refuses 0 and negative values and that it belongs to the calling thread.

Not covered: the real-valued kind of the head's backward WITH the loss inside (the sigmoid is not a bilinear form; the integer kind
reaches that path with logits 0 and +-200, whose sigmoid is exact, and the loss-scale tests with real logits).

Measured on an MI355X: the 506 tests of the file take 3.5 s together, the slowest (the first launch of the session) 0.95 s; the worst
bound ratio is 0.057 for the MFMA kernels and 0.40 for the head's three-class data gradient (profiles/h16_parity_margins.json).
Needs a real MI355X: ``-m gpu``."""
import ctypes
import functools
import os
import threading

import pytest
import torch

import _direct_cases as D
import _h16_cases as HC
import _persistent_cases as PC
from _h16_cases import SENTINEL, U, X_PAD_VALUE, rup, sid
from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
KINDS = ("int", "real")
GUARD = 64


def P(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib16(request):
    """(library, 16-bit torch dtype, name) of each product library: the "bf16" entry points use the library's own 16-bit type."""
    from hyperpri_amd import _lib
    if request.param == "bf16":
        return _lib.load(), torch.bfloat16, "bf16"
    if not os.path.exists(_lib.LIB_F16_PATH):
        pytest.skip("the half-precision library is not built")
    return _lib.load_f16(), torch.float16, "f16"      # (a library that is there and does not load is an error, not a skip)


def _ok(L, rc):
    assert rc == 0, L.hpri_last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# Buffers and comparisons
# ---------------------------------------------------------------------------------------------------------------------------
def _frame(rows, cs, fill=SENTINEL):
    return torch.full((rows, cs), fill, dtype=torch.float64)


def _put(buf, off, vals, cw=None, pad=0.0):
    """vals into channels [off, off + C) of buf; ``pad`` (None: leave) into [off + C, off + cw)."""
    C = vals.shape[1]
    buf[:, off:off + C] = vals.to(buf.dtype)
    if cw is not None and cw > C and pad is not None:
        buf[:, off + C:off + cw] = pad
    return buf


def _where(bad):
    idx = torch.nonzero(bad)
    return int(bad.sum()), tuple(int(v) for v in idx[0])


def _check32(name, got, want, bnd=None, key=None):
    """The whole fp32 buffer: |got - want| <= bnd elementwise (bnd None or 0: equal), want / bnd fp64 arrays of the buffer's shape."""
    g = got.detach().cpu().double().reshape(want.shape)
    err = (g - want).abs()
    bad = ~(err == 0) if bnd is None else ~(err <= bnd)
    if key is not None and bnd is not None:
        live = bnd > 0
        record_margin(key, float((err[live] / bnd[live]).nan_to_num(1e30).max()) if bool(live.any()) else 0.0, 1.0)
    if bool(bad.any()):
        n, at = _where(bad)
        pytest.fail("%s: %d wrong elements of %d, first at (row, channel) %s: got %r, want %r%s" % (
            name, n, bad.numel(), at, float(g[at]), float(want[at]), "" if bnd is None else " +- %g (error %g)" % (float(bnd[at]), float(err[at]))))


def _check16(name, got, want):
    """The whole 16-bit buffer, bit for bit."""
    g = got.detach().cpu().reshape(want.shape)
    bad = g.view(torch.int16) != want.view(torch.int16)
    if bool(bad.any()):
        n, at = _where(bad)
        pytest.fail("%s: %d wrong 16-bit elements of %d, first at (row, channel) %s: got %r (0x%04x), want %r (0x%04x)" % (
            name, n, bad.numel(), at, float(g[at]), int(g.view(torch.int16)[at]) & 0xFFFF, float(want[at]), int(want.view(torch.int16)[at]) & 0xFFFF))


def _check16_between(name, got, want, bnd, dt):
    """A 16-bit buffer without an fp32 twin: the kernel rounds an fp32 value within bnd of want once, and rounding is monotone."""
    g = got.detach().cpu().reshape(want.shape).double()
    lo, hi = (want - bnd).float().to(dt).double(), (want + bnd).float().to(dt).double()
    bad = ~((lo <= g) & (g <= hi))
    if bool(bad.any()):
        n, at = _where(bad)
        pytest.fail("%s: %d wrong 16-bit elements of %d, first at (row, channel) %s: got %r, want within [%r, %r]" % (
            name, n, bad.numel(), at, float(g[at]), float(lo[at]), float(hi[at])))


def _out32(kind, name, got, want, bnd, key):
    """int: equal; real: within the bound (which is 0 wherever the launch must not write or writes an exact value)."""
    _check32(name, got, want, None if kind == "int" else bnd, None if kind == "int" else key)


def _planes(vals, dt, cs, coff, zero_to):
    """16-bit rows of cs elements: vals in [coff, coff + C), zeros up to coff + zero_to, X_PAD_VALUE everywhere else."""
    p = torch.full((vals.shape[0], cs), X_PAD_VALUE, dtype=dt)
    p[:, coff:coff + zero_to] = 0
    p[:, coff:coff + vals.shape[1]] = vals.to(dt)
    return p.to(DEV)


def _pack(L, dt, w, mode, K, ncols, T, d1, cup):
    kp, ncp = rup(K, 32), rup(ncols, 64)
    wp = torch.empty((kp // 32) * T * ncp * 32, dtype=dt, device=DEV)
    wd = w.contiguous().to(DEV)                                               # (named: a temporary would be freed before the launch)
    _ok(L, L.hpri_pack_weight_bf16(P(wd), P(wp), mode, K, ncols, ncp, T, d1, cup, 0, _st()))
    torch.cuda.synchronize()
    return wp, ncp


def _check_stats(name, kind, stats, tiles, cp, C, vals):
    """One (mean, M2, count, 0) record per tile and column: count exact, mean and M2 / count against fp64 over the tile's rows."""
    s = stats.view(len(tiles), cp, 4).double().cpu()
    sc = max(1.0, float(vals.abs().max()))
    tol = (64 if kind == "int" else 320) * U * sc
    for t, rows in enumerate(tiles):
        v = vals[rows]
        cnt = s[t, :C, 2]
        badc = ~((cnt == float(rows.numel())) & (s[t, :C, 3] == 0))
        assert not bool(badc.any()), "%s: record of tile %d, column %d: count %r, want %d (NaN: never written)" % (
            name, t, int(torch.nonzero(badc)[0]), float(cnt[int(torch.nonzero(badc)[0])]), rows.numel())
        e_mean = (s[t, :C, 0] - v.mean(0)).abs()
        e_var = (s[t, :C, 1] / rows.numel() - v.var(0, unbiased=False)).abs()
        record_margin(name + "/record_mean", float(e_mean.max() / tol), 1.0)
        record_margin(name + "/record_var", float(e_var.max() / (1e-4 * sc * sc)), 1.0)
        assert bool((e_mean <= tol).all()), "%s: mean of tile %d, column %d off by %g (tolerance %g)" % (name, t, int(e_mean.argmax()), float(e_mean.max()), tol)
        assert bool((e_var <= 1e-4 * sc * sc).all()), "%s: M2 / count of tile %d, column %d off by %g" % (name, t, int(e_var.argmax()), float(e_var.max()))


def _cw(C):
    """Written width of the row kernels: four pad columns behind C where the packed columns (a multiple of 64) have room."""
    return min(rup(C, 4) + 4, rup(C, 64))


def _gemm_tiles(N, HW):
    return [torch.arange(n * HW + p0, n * HW + min(HW, p0 + 256)) for n in range(N) for p0 in range(0, HW, 256)]


def _guarded(n, fill=SENTINEL, dtype=torch.float32):
    """A flat buffer of n elements with GUARD sentinels on either side (device), and the view of the n elements."""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guard_frame(n, inner):
    """Expected contents (fp64) of a _guarded buffer whose n elements hold ``inner``."""
    out = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64)
    out[GUARD:GUARD + n] = inner.reshape(-1).double()
    return out


def _guard_bound(n, inner):
    out = torch.zeros(n + 2 * GUARD, dtype=torch.float64)
    out[GUARD:GUARD + n] = inner.reshape(-1)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# hpri_gemm_bf16v3
# ---------------------------------------------------------------------------------------------------------------------------
def _gemm_forward(L, dt, x, w, bias, N, HW, with_stats=True):
    """One launch: the fp32 view inside a wider buffer, the 16-bit view inside another, per-tile statistics."""
    K, C = x.shape[1], w.shape[0]
    rows, kp, cw = N * HW, rup(K, 32), _cw(C)
    xcs, xoff = kp + 16, 8
    xp = _planes(x, dt, xcs, xoff, kp)
    wp, ncp = _pack(L, dt, w, 0, K, C, 1, K, 0)
    ycs, yoff, y16cs, y16off = cw + 12, 4, cw + 8, 4
    y = _frame(rows, ycs).float().to(DEV)
    y16 = _frame(rows, y16cs).to(dt).to(DEV)
    tl = ctypes.c_int()
    _ok(L, L.hpri_gemm_bf16v3_plan(N, HW, ctypes.byref(tl)))
    assert tl.value == len(_gemm_tiles(N, HW))
    stats = torch.full((tl.value * ncp * 4,), NAN, device=DEV) if with_stats else None
    bd = None if bias is None else bias.to(DEV)
    _ok(L, L.hpri_gemm_bf16v3(P(xp), xcs, xoff, P(wp), P(bd), P(y), ycs, yoff, P(y16), y16cs, y16off, P(stats),
                              ncp if with_stats else 0, N, HW, kp, C, ncp, cw, 0, _st()))
    torch.cuda.synchronize()
    return dict(y=y, y16=y16, stats=stats, ycs=ycs, yoff=yoff, y16cs=y16cs, y16off=y16off, cw=cw, ncp=ncp, rows=rows, C=C)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", HC.GEMM_FWD, ids=sid)
def test_gemm_forward(lib16, shape, kind):
    """y = x w^T + b: fp32 view, 16-bit view and statistics of one launch.  (1,5,8,4): below one tile; (2,300,40,24): ragged rows that
    must not straddle images; (2,129,238,150): several k-steps; (3,257,64,330): one row over a 256-row tile, a ragged third column block."""
    L, dt, lib = lib16
    N, HW, K, C = shape
    c = HC.case("rows", kind, lib, shape)
    name = "h16/gemm_fwd/%s/%s" % (lib, sid(shape))
    r = _gemm_forward(L, dt, c["a"], c["b"], c["bias"], N, HW)
    want = c["ref"] + c["bias"].double()
    bnd = HC.bound(c, c["bias"].double().abs())
    _out32(kind, name, r["y"], _put(_frame(r["rows"], r["ycs"]), r["yoff"], want.float(), r["cw"]), _put(_frame(r["rows"], r["ycs"], 0.0), r["yoff"], bnd), name)
    twin = want if kind == "int" else r["y"].cpu()[:, r["yoff"]:r["yoff"] + C]
    _check16(name + " y16", r["y16"], _put(_frame(r["rows"], r["y16cs"]).to(dt), r["y16off"], twin.float().to(dt), r["cw"]))
    _check_stats(name, kind, r["stats"], _gemm_tiles(N, HW), r["ncp"], C, want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("into", ["fp32", "16-bit"])
@pytest.mark.parametrize("shape", HC.GEMM_DGRAD, ids=sid)
def test_gemm_data_gradient_accumulates(lib16, shape, into, kind):
    """dx += dy W (pack mode 1: K = out features, columns = in features) into fp32 rows, and into 16-bit rows (read, add in fp32, round
    once); the pad columns of an accumulating launch receive exact zeros, i.e. keep what they hold."""
    L, dt, lib = lib16
    N, HW, K, C = shape
    c = HC.case("rows", kind, lib, shape)
    name = "h16/gemm_dgrad_%s/%s/%s" % (into, lib, sid(shape))
    rows, kp, cw = N * HW, rup(K, 32), _cw(C)
    xcs, xoff = kp + 16, 8
    xp = _planes(c["a"], dt, xcs, xoff, kp)
    wp, ncp = _pack(L, dt, c["b"].t(), 1, K, C, 1, C, 0)                       # the layer's weight [out = K][in = C]
    ycs, yoff = cw + 12, 4
    odt = torch.float32 if into == "fp32" else dt
    prior = c["prior"].to(odt)
    before = _put(_frame(rows, ycs), yoff, prior, cw, 5.0)
    want = _put(before.clone(), yoff, (c["ref"] + prior.double()).float(), cw, None)
    bnd = _put(_frame(rows, ycs, 0.0), yoff, HC.bound(c, prior.double().abs()))
    y = before.to(odt).to(DEV)
    y32, y16 = (y, None) if into == "fp32" else (None, y)
    _ok(L, L.hpri_gemm_bf16v3(P(xp), xcs, xoff, P(wp), P(None), P(y32), ycs if y32 is not None else 0, yoff if y32 is not None else 0, P(y16),
                              ycs if y16 is not None else 0, yoff if y16 is not None else 0, P(None), 0, N, HW, kp, C, ncp, cw, 1, _st()))
    torch.cuda.synchronize()
    if into == "fp32":
        _out32(kind, name, y, want, bnd, name)
    elif kind == "int":
        _check16(name, y, want.float().to(dt))
    else:
        _check16_between(name, y, want, bnd, dt)


def test_gemm_refuses_a_written_width_beyond_the_pack(lib16):
    """Columns beyond Ncols_pad multiply a clamped packed row, not zeros: a written width that reaches them (64 packed columns of a
    128-column block, y_cw = 68) is an error return of the row GEMM and of the transposed convolution's data gradient, and nothing
    is written."""
    L, dt, lib = lib16
    c = HC.case("rows", "int", lib, (1, 5, 32, 64))
    xp = _planes(c["a"], dt, 48, 8, 32)
    wp, ncp = _pack(L, dt, c["b"], 0, 32, 64, 1, 32, 0)
    assert ncp == 64
    y = _frame(5, 80).float().to(DEV)
    assert L.hpri_gemm_bf16v3(P(xp), 48, 8, P(wp), P(None), P(y), 80, 4, P(None), 0, 0, P(None), 0, 1, 5, 32, 64, 64, 68, 0, _st()) != 0
    _ok(L, L.hpri_gemm_bf16v3(P(xp), 48, 8, P(wp), P(None), P(y), 80, 4, P(None), 0, 0, P(None), 0, 1, 5, 32, 64, 64, 64, 0, _st()))
    torch.cuda.synchronize()
    _check32("h16/gemm_width/%s" % lib, y, _put(_frame(5, 80), 4, c["ref"]))
    c = HC.case("convt_dgrad", "int", lib, (1, 2, 3, 64, 32, 0, 0))
    dyp = c["a"].reshape(-1, 32).to(dt).to(DEV)
    wp, cinp = _pack(L, dt, c["b"], 3, 128, 64, 1, 32, 32)
    assert cinp == 64
    dx = _frame(6, 80).float().to(DEV)
    assert L.hpri_convt_dgrad_bf16v3(P(dyp), 32, 0, P(wp), P(dx), 80, 4, 1, 2, 3, 32, 64, 64, 68, 4, 6, 0, 0, 0, _st()) != 0
    torch.cuda.synchronize()
    _check32("h16/convt_dgrad_width/%s" % lib, dx, _frame(6, 80))


def _canvas(H, W, dY, dX):
    """The [H2, W2] canvas of a 2H x 2W patch grid at offset (dY, dX): a ring of dY rows / dX columns on both sides."""
    return 2 * H + 2 * dY, 2 * W + 2 * dX, dY, dX


def _put_patches(canvas, vals, N, H2, W2, py0, px0, coff):
    """vals [N, 2H, 2W, C] into channels [coff, coff + C) of the patch grid of a [N*H2*W2, cs] canvas"""
    canvas.view(N, H2, W2, -1)[:, py0:py0 + vals.shape[1], px0:px0 + vals.shape[2], coff:coff + vals.shape[3]] = vals.to(canvas.dtype)
    return canvas


def _convt_forward(L, dt, x, wt, bias, shape):
    N, H, W, Cin, Cup, dY, dX = shape
    H2, W2, py0, px0 = _canvas(H, W, dY, dX)
    kp = rup(Cin, 32)
    xcs, xoff = kp + 16, 8
    xp = _planes(x.reshape(-1, Cin), dt, xcs, xoff, kp)
    wp, ncp = _pack(L, dt, wt, 2, Cin, 4 * Cup, 1, Cup, Cup)
    ycs, yoff = Cup + 12, 8
    y = _frame(N * H2 * W2, ycs).float().to(DEV)
    y16 = _frame(N * H2 * W2, ycs).to(dt).to(DEV)
    bd = bias.to(DEV)
    _ok(L, L.hpri_convt_fwd_bf16v3(P(xp), xcs, xoff, P(wp), P(bd), P(y), ycs, yoff, P(y16), ycs, yoff, N, H, W, kp, Cup, ncp, H2, W2,
                                   py0, px0, _st()))
    torch.cuda.synchronize()
    place = lambda frame, vals: _put_patches(frame, vals, N, H2, W2, py0, px0, yoff)
    take = lambda buf: buf.view(N, H2, W2, ycs)[:, py0:py0 + 2 * H, px0:px0 + 2 * W, yoff:yoff + Cup]
    return y, y16, ycs, N * H2 * W2, place, take


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", HC.CONVT, ids=sid)
def test_transposed_convolution_forward(lib16, shape, kind):
    """hpri_convt_fwd_bf16v3: the depth-to-space scatter into a channel slice of a canvas (odd offsets, a ring that must stay), fp32
    and 16-bit at once; Cup = 48 is no multiple of 32."""
    L, dt, lib = lib16
    c = HC.case("convt_fwd", kind, lib, shape)
    name = "h16/convt_fwd/%s/%s" % (lib, sid(shape))
    y, y16, ycs, rows, place, take = _convt_forward(L, dt, c["a"], c["b"], c["bias"], shape)
    want = c["ref"] + c["bias"].double()
    _out32(kind, name, y, place(_frame(rows, ycs), want.float()), place(_frame(rows, ycs, 0.0), HC.bound(c, c["bias"].double().abs())), name)
    twin = want.float() if kind == "int" else take(y.cpu())
    _check16(name + " y16", y16, place(_frame(rows, ycs).to(dt), twin.to(dt)))


def _convt_dgrad(L, dt, dy, wt, prior, shape, form):
    """form: "acc0" / "acc1" (fp32 rows) or "y16".  Returns (dx buffer, its fp64 contents before the launch, xcs, xoff, cw)."""
    N, H, W, Cin, Cup, dY, dX = shape
    H2, W2, py0, px0 = _canvas(H, W, dY, dX)
    dcs, doff = Cup + 48, 32
    dyp = _put_patches(torch.full((N * H2 * W2, dcs), X_PAD_VALUE, dtype=dt), dy, N, H2, W2, py0, px0, doff).to(DEV)
    wp, cinp = _pack(L, dt, wt, 3, 4 * Cup, Cin, 1, Cup, Cup)
    cw, xoff = _cw(Cin), 4
    xcs = cw + 8
    before = _frame(N * H * W, xcs)
    if form == "acc1":
        _put(before, xoff, prior, cw, 5.0)
    odt = dt if form == "y16" else torch.float32
    dx = before.to(odt).to(DEV)
    if form == "y16":
        rc = L.hpri_convt_dgrad_bf16v3_y16(P(dyp), dcs, doff, P(wp), P(dx), xcs, xoff, N, H, W, Cup, Cin, cinp, cw, H2, W2, py0, px0, _st())
    else:
        rc = L.hpri_convt_dgrad_bf16v3(P(dyp), dcs, doff, P(wp), P(dx), xcs, xoff, N, H, W, Cup, Cin, cinp, cw, H2, W2, py0, px0,
                                       int(form == "acc1"), _st())
    _ok(L, rc)
    torch.cuda.synchronize()
    return dx, before, xcs, xoff, cw


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["acc0", "acc1", "y16"])
@pytest.mark.parametrize("shape", [s for s in HC.CONVT if s[4] % 32 == 0], ids=sid)
def test_transposed_convolution_data_gradient(lib16, shape, form, kind):
    """hpri_convt_dgrad_bf16v3 (plain and accumulating) and _y16: K = 4 Cup gathered from the four parities of a canvas whose ring and
    whose channels beside the gradient's hold values that must not be read."""
    L, dt, lib = lib16
    N, H, W, Cin = shape[:4]
    c = HC.case("convt_dgrad", kind, lib, shape)
    name = "h16/convt_dgrad_%s/%s/%s" % (form, lib, sid(shape))
    dx, before, xcs, xoff, cw = _convt_dgrad(L, dt, c["a"], c["b"], c["prior"], shape, form)
    old = c["prior"].double() if form == "acc1" else 0.0
    want = _put(before.clone(), xoff, (c["ref"] + old).float(), cw, None if form == "acc1" else 0.0)
    bnd = _put(_frame(N * H * W, xcs, 0.0), xoff, HC.bound(c, c["prior"].double().abs() if form == "acc1" else 0.0))
    if form != "y16":
        _out32(kind, name, dx, want, bnd, name)
    elif kind == "int":
        _check16(name, dx, want.float().to(dt))
    else:
        _check16_between(name, dx, want, bnd, dt)
        fp32 = _convt_dgrad(L, dt, c["a"], c["b"], c["prior"], shape, "acc0")[0]           # the same accumulation, rounded once
        _check16(name + " == the fp32 form rounded once", dx, fp32.cpu().to(dt))


# ---------------------------------------------------------------------------------------------------------------------------
# hpri_conv_bf16v3, hpri_conv_bf16v3_y2
# ---------------------------------------------------------------------------------------------------------------------------
def _conv_plan(L, N, H, W, cs16, cout_pad):
    k, tl, wsf = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    _ok(L, L.hpri_conv_bf16v3_plan(N, H, W, cs16, cout_pad, ctypes.byref(k), ctypes.byref(tl), ctypes.byref(wsf)))
    return k.value, tl.value, torch.empty(max(wsf.value, 4), device=DEV)


def _conv_tiles(N, H, W, ksplit, ntiles):
    """Rows of every statistics record: the 256-pixel tiles of the plan, or (split-K) 64 consecutive pixels of an image."""
    if ksplit > 1:
        tiles = [torch.arange(n * H * W + p0, n * H * W + min(H * W, p0 + 64)) for n in range(N) for p0 in range(0, H * W, 64)]
    else:
        segs, per = PC.v3_segments(H, W)
        tin = torch.tensor([[PC.tile_in_image(segs, y, x) for x in range(W)] for y in range(H)]).reshape(-1)
        tiles = [n * H * W + torch.nonzero(tin == t).reshape(-1) for n in range(N) for t in range(per)]
    assert len(tiles) == ntiles, (len(tiles), ntiles)
    return tiles


def _conv(L, dt, x, w, bias, shape, form):
    """form: "fwd_stats" (bias, statistics), "dgrad_acc_view" (mode-1 pack, accumulate into a channel-slice view), "relu_bias",
    "y16" (the 16-bit output bit).  x [N,H,W,Cin], w = the effective forward weight [Cout,Cin,3,3]."""
    N, H, W, Cin, Cout = shape
    cs16, cout_pad = rup(Cin, 32), rup(Cout, 64)
    ksplit, ntiles, ws = _conv_plan(L, N, H, W, cs16, cout_pad)
    xcs, xoff = cs16 + 16, 8
    xp = _planes(x.reshape(-1, Cin), dt, xcs, xoff, cs16)
    if form == "dgrad_acc_view":
        # the data-gradient pack takes the LAYER's weight [its Cout = K][its Cin = columns] and rotates the taps itself
        wp, _ = _pack(L, dt, w.permute(1, 0, 2, 3).flip(2, 3), 1, Cin, Cout, 9, Cout, 0)
    else:
        wp, _ = _pack(L, dt, w, 0, Cin, Cout, 9, Cin, 0)
    cw = min(Cout + 8, cout_pad)
    ycs, yoff = cw + 16, 8
    return dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, cs16=cs16, cout_pad=cout_pad, ksplit=ksplit, ntiles=ntiles, ws=ws, xp=xp, xcs=xcs, xoff=xoff,
                wp=wp, cw=cw, ycs=ycs, yoff=yoff, npx=N * H * W, bias=None if bias is None else bias.to(DEV))


def _conv_launch(L, p, y, stats, flags, bias=True):
    return L.hpri_conv_bf16v3(P(p["xp"]), 0, p["xcs"], p["xoff"], P(p["wp"]), P(p["bias"] if bias else None), P(y), p["ycs"], p["yoff"], P(stats),
                              p["N"], p["H"], p["W"], p["cs16"], p["Cout"], p["cout_pad"], p["cw"], flags, 0, P(p["ws"]), p["ws"].numel(), _st())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["fwd_stats", "dgrad_acc_view", "relu_bias", "y16"])
@pytest.mark.parametrize("shape", HC.CONV, ids=sid)
def test_plane_convolution(lib16, shape, form, kind):
    """hpri_conv_bf16v3.  (1,4,32,64,64): one tile row; (1,17,23,40,64), (1,33,31,238,64): ragged widths, 238 -> padded K (a split-K
    problem where the plan says so: then the 16-bit output is refused and the records cover 64 pixels); (2,36,50,64,64): two images."""
    L, dt, lib = lib16
    c = HC.case("conv", kind, lib, shape)
    name = "h16/conv_%s/%s/%s" % (form, lib, sid(shape))
    p = _conv(L, dt, c["a"], c["b"], c["bias"], shape, form)
    npx, ycs, yoff, cw, Cout = p["npx"], p["ycs"], p["yoff"], p["cw"], p["Cout"]
    bias, prior = c["bias"].double(), c["prior"]
    if form == "dgrad_acc_view":
        before = _put(_frame(npx, ycs), yoff, prior, cw, 5.0)
        want = _put(before.clone(), yoff, (c["ref"] + prior.double()).float(), cw, None)
        bnd = _put(_frame(npx, ycs, 0.0), yoff, HC.bound(c, prior.double().abs()))
        y = before.float().to(DEV)
        _ok(L, _conv_launch(L, p, y, None, 1, bias=False))
        torch.cuda.synchronize()
        return _out32(kind, name, y, want, bnd, name)
    vals = c["ref"] + bias
    bnd = _put(_frame(npx, ycs, 0.0), yoff, HC.bound(c, bias.abs()))
    if form == "relu_bias":
        vals = torch.relu(vals)                                              # (|relu(a) - relu(b)| <= |a - b|: the bound holds)
    want = _put(_frame(npx, ycs), yoff, vals.float(), cw)
    if form == "y16":
        y = _frame(npx, ycs).to(dt).to(DEV)
        rc = _conv_launch(L, p, y, None, 4)
        if p["ksplit"] > 1:
            assert rc != 0, "a 16-bit output of a split-K problem must be refused"
            torch.cuda.synchronize()
            return _check16(name + " (refused: untouched)", y, _frame(npx, ycs).to(dt))
        _ok(L, rc)
        torch.cuda.synchronize()
        if kind == "int":
            return _check16(name, y, want.float().to(dt))
        _check16_between(name, y, want, bnd, dt)
        y32 = _frame(npx, ycs).float().to(DEV)
        _ok(L, _conv_launch(L, p, y32, None, 0))
        torch.cuda.synchronize()
        return _check16(name + " == the fp32 form rounded once", y, y32.cpu().to(dt))
    y = _frame(npx, ycs).float().to(DEV)
    stats = torch.full((p["ntiles"] * p["cout_pad"] * 4,), NAN, device=DEV) if form == "fwd_stats" else None
    _ok(L, _conv_launch(L, p, y, stats, 2 if form == "relu_bias" else 0))
    torch.cuda.synchronize()
    _out32(kind, name, y, want, bnd, name)
    if stats is not None:
        _check_stats(name, kind, stats, _conv_tiles(p["N"], p["H"], p["W"], p["ksplit"], p["ntiles"]), p["cout_pad"], Cout, vals)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("only", [0, 1, 3])
def test_plane_convolution_second_output(lib16, only, kind):
    """hpri_conv_bf16v3_y2 over (2,19,30,32,192): channels [128, 192) also (1: only) as 16-bit rows; 3: the main output as compact 16-bit
    rows of the channels below as well.  The statistics are those of the plain launch."""
    L, dt, lib = lib16
    shape = HC.CONV_Y2
    c = HC.case("conv", kind, lib, shape)
    name = "h16/conv_y2_only%d/%s/%s" % (only, lib, sid(shape))
    p = _conv(L, dt, c["a"], c["b"], None, shape, "fwd")
    assert p["ksplit"] == 1
    npx, Cout, cout_pad = p["npx"], p["Cout"], p["cout_pad"]
    c0, cw2 = 128, 64
    ref, bnd = c["ref"], HC.bound(c)
    y2cs, y2off = cw2 + 8, 4
    y2 = _frame(npx, y2cs).to(dt).to(DEV)
    want2, bnd2 = _put(_frame(npx, y2cs), y2off, ref[:, c0:c0 + cw2].float()), _put(_frame(npx, y2cs, 0.0), y2off, bnd[:, c0:c0 + cw2])
    if only == 3:
        ycs, yoff, ycw, odt = c0 + 8, 4, c0, dt
    else:
        ycs, yoff, ycw, odt = Cout + 8, 4, Cout, torch.float32
    want = _put(_frame(npx, ycs), yoff, ref[:, :c0].float())
    bndy = _put(_frame(npx, ycs, 0.0), yoff, bnd[:, :c0])
    if only == 0:
        _put(want, yoff, ref.float())
        _put(bndy, yoff, bnd)
    y = _frame(npx, ycs).to(odt).to(DEV)
    stats = torch.full((p["ntiles"] * cout_pad * 4,), NAN, device=DEV)
    _ok(L, L.hpri_conv_bf16v3_y2(P(p["xp"]), p["xcs"], p["xoff"], P(p["wp"]), P(None), P(y), ycs, yoff, P(stats), p["N"], p["H"], p["W"], p["cs16"], Cout,
                                 cout_pad, ycw, P(y2), y2cs, y2off, c0, cw2, only, _st()))
    torch.cuda.synchronize()
    if only == 3:
        if kind == "int":
            _check16(name + " y", y, want.float().to(dt))
        else:
            _check16_between(name + " y", y, want, bndy, dt)
    else:
        _out32(kind, name + " y", y, want, bndy, name)
    if kind == "int":
        _check16(name + " y2", y2, want2.float().to(dt))
    elif only == 0:
        _check16(name + " y2 == the fp32 view rounded once", y2, _put(_frame(npx, y2cs).to(dt), y2off, y.cpu()[:, yoff + c0:yoff + c0 + cw2].to(dt)))
    else:
        _check16_between(name + " y2", y2, want2, bnd2, dt)
    _check_stats(name, kind, stats, _conv_tiles(p["N"], p["H"], p["W"], 1, p["ntiles"]), cout_pad, Cout, ref)


# ---------------------------------------------------------------------------------------------------------------------------
# Weight gradients: hpri_conv_wgrad_bf16v2, hpri_wgrad1x1_bf16v3, hpri_wgrad_convt_bf16v3 (+ hpri_wgrad_reduce_ex)
# ---------------------------------------------------------------------------------------------------------------------------
def _reduce(L, ws, sp, cr, nr, Cin, Cout, ks, dst_mode, cup, acc, prior):
    n = prior.numel()
    buf, dw = _guarded(n)
    dw.copy_(prior.reshape(-1).float())
    _ok(L, L.hpri_wgrad_reduce_ex(P(ws), P(dw), sp, cr, nr, Cin, Cout, ks, dst_mode, cup, acc, _st()))
    torch.cuda.synchronize()
    return buf


def _wgrad_verdict(kind, name, c, buf, acc):
    old = c["prior"].double() if acc else 0.0
    n = c["ref"].numel()
    _out32(kind, name, buf, _guard_frame(n, (c["ref"] + old).float()), _guard_bound(n, HC.bound(c, c["prior"].double().abs() if acc else 0.0)), name)


def _wgrad_planes(vals, dt):
    """16-bit rows for the weight-gradient kernels: valid width rup(C, 8) (zeros behind C), X_PAD_VALUE outside it."""
    C = vals.shape[1]
    cs, coff, valid = rup(C, 32) + 16, 8, rup(C, 8)
    return _planes(vals, dt, cs, coff, valid), cs, coff, valid


def _wgrad_conv(L, dt, x, dy, prior, shape, acc):
    N, H, W, Cin, Cout = shape
    cs16, cout_pad = rup(Cin, 32), rup(Cout, 64)
    xp, xcs, xoff, xv = _wgrad_planes(x.reshape(-1, Cin), dt)
    dp, dcs, doff, dv = _wgrad_planes(dy.reshape(-1, Cout), dt)
    sp, cr, nr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _ok(L, L.hpri_wgrad_bf16v2_plan(N, H, W, cs16, cout_pad, ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr)))
    ws = torch.full((sp.value * 9 * cr.value * nr.value,), NAN, device=DEV)
    _ok(L, L.hpri_conv_wgrad_bf16v2(P(xp), xcs, xoff, xv, P(dp), dcs, doff, dv, P(ws), ws.numel(), N, H, W, cs16, cout_pad, _st()))
    return _reduce(L, ws, sp.value, cr.value, nr.value, Cin, Cout, 3, 0, 0, acc, prior), sp.value


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("shape", HC.WGRAD_CONV, ids=sid)
def test_convolution_weight_gradient(lib16, shape, acc, kind):
    """hpri_conv_wgrad_bf16v2 + hpri_wgrad_reduce_ex.  (1,17,23,5,7): x_cvalid = 8 below the pad of 32 with junk behind it;
    (2,36,50,64,64): more than one split."""
    L, dt, lib = lib16
    c = HC.case("wgrad_conv", kind, lib, shape)
    name = "h16/wgrad_conv_acc%d/%s/%s" % (acc, lib, sid(shape))
    buf, splits = _wgrad_conv(L, dt, c["a"], c["b"], c["prior"], shape, acc)
    _wgrad_verdict(kind, name, c, buf, acc)


def _wgrad1x1(L, dt, x, dy, prior, acc):
    Pn, Cin, Cout = x.shape[0], x.shape[1], dy.shape[1]
    xp, xcs, xoff, xv = _wgrad_planes(x, dt)
    dp, dcs, doff, dv = _wgrad_planes(dy, dt)
    sp, cr, nr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _ok(L, L.hpri_wgrad1x1_bf16v3_plan(Pn, rup(Cin, 32), rup(Cout, 64), ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr)))
    ws = torch.full((sp.value * cr.value * nr.value,), NAN, device=DEV)
    _ok(L, L.hpri_wgrad1x1_bf16v3(P(xp), xcs, xoff, xv, P(dp), dcs, doff, dv, P(ws), ws.numel(), Pn, rup(Cin, 32), rup(Cout, 64), _st()))
    return _reduce(L, ws, sp.value, cr.value, nr.value, Cin, Cout, 1, 0, 0, acc, prior)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("shape", HC.WGRAD_1X1, ids=sid)
def test_linear_weight_gradient(lib16, shape, acc, kind):
    """hpri_wgrad1x1_bf16v3: dW[n][c] = sum_p dY[p][n] X[p][c] over ragged pixel counts and valid widths below the tile widths."""
    L, dt, lib = lib16
    c = HC.case("wgrad1x1", kind, lib, shape)
    name = "h16/wgrad1x1_acc%d/%s/%s" % (acc, lib, sid(shape))
    _wgrad_verdict(kind, name, c, _wgrad1x1(L, dt, c["a"], c["b"], c["prior"], acc), acc)


def _wgrad_convt(L, dt, x, dy, prior, shape):
    N, H, W, Cin, Cup, dY, dX = shape
    H2, W2, py0, px0 = _canvas(H, W, dY, dX)
    xp, xcs, xoff, xv = _wgrad_planes(x.reshape(-1, Cin), dt)
    dcs, doff = Cup + 72, 64
    dyp = _put_patches(torch.full((N * H2 * W2, dcs), X_PAD_VALUE, dtype=dt), dy, N, H2, W2, py0, px0, doff).to(DEV)
    cin_pad = rup(Cin, 32)
    sp, cr, nr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _ok(L, L.hpri_wgrad1x1_bf16v3_plan(N * H * W, cin_pad, 4 * Cup, ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr)))
    ws = torch.full((sp.value * cr.value * nr.value,), NAN, device=DEV)
    _ok(L, L.hpri_wgrad_convt_bf16v3(P(xp), xcs, xoff, xv, P(dyp), dcs, doff, P(ws), ws.numel(), N, H, W, cin_pad, Cup, H2, W2, py0, px0, _st()))
    return _reduce(L, ws, sp.value, cr.value, nr.value, Cin, 4 * Cup, 1, 1, Cup, 0, prior)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", HC.WGRAD_CONVT, ids=sid)
def test_transposed_convolution_weight_gradient(lib16, shape, kind):
    """hpri_wgrad_convt_bf16v3: x planes at low resolution, dy planes at high resolution in a canvas (a ring in the second shape),
    gathered by parity."""
    L, dt, lib = lib16
    c = HC.case("wgrad_convt", kind, lib, shape)
    name = "h16/wgrad_convt/%s/%s" % (lib, sid(shape))
    _wgrad_verdict(kind, name, c, _wgrad_convt(L, dt, c["a"], c["b"], c["prior"], shape), 0)


# ---------------------------------------------------------------------------------------------------------------------------
# The head over 16-bit rows: hpri_outconv_fwd_x16 / hpri_outconv_bwd_x16
# ---------------------------------------------------------------------------------------------------------------------------
def _head_source(x, dt, coff):
    """x [N HW, C] as 16-bit rows at channel offset coff of a wider buffer: X_PAD_VALUE in front of the slice, zeros behind it."""
    C = x.shape[1]
    cs = rup(C, 32) + coff + (32 if coff else 0)
    buf = torch.zeros(x.shape[0], cs, dtype=dt)
    buf[:, :coff] = X_PAD_VALUE
    buf[:, coff:coff + C] = x.to(dt)
    return buf.to(DEV), cs


# logit, target -> sigmoid(logit) - target, exactly: expf(-0) = 1 and expf(-200) = 0 in fp32
EXACT_BCE = {1: (0.0, 0.0), -1: (0.0, 1.0), 2: (200.0, 0.0), -2: (-200.0, 1.0), 0: (200.0, 1.0)}        # 2 x (sigmoid - target)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("loss", [False, True], ids=["plain", "loss"])
@pytest.mark.parametrize("shape", HC.HEAD, ids=sid)
def test_head_forward(lib16, shape, loss, kind):
    """hpri_outconv_fwd_x16: logits [N, K, HW] (whole buffer, guarded), with the loss partials of BCE-with-logits where asked."""
    L, dt, lib = lib16
    N, HW, C, K, coff = shape
    c = HC.head_case(kind, lib, shape)["fwd"]
    name = "h16/head_fwd_%s/%s/%s" % ("loss" if loss else "plain", lib, sid(shape))
    x, cs = _head_source(c["a"], dt, coff)
    w, b = c["b"].to(DEV), c["bias"].to(DEV)
    buf, y = _guarded(N * K * HW)
    tgt = (torch.rand(N, K, HW, generator=torch.Generator().manual_seed(5)) > 0.7).float().to(DEV)
    nblk = L.hpri_outconv_fwd_bce_blocks(N, HW)
    part = torch.zeros(nblk, dtype=torch.float64, device=DEV)
    _ok(L, L.hpri_outconv_fwd_x16(P(x), cs, coff, P(w), P(b), P(y), P(tgt) if loss else P(None), P(part) if loss else P(None), nblk if loss else 0,
                                  N, HW, C, K, _st()))
    torch.cuda.synchronize()
    to_nkp = lambda t: t.view(N, HW, K).permute(0, 2, 1)
    want = to_nkp(c["ref"] + c["bias"].double())
    _out32(kind, name, buf, _guard_frame(N * K * HW, want.float()), _guard_bound(N * K * HW, to_nkp(HC.bound(c, c["bias"].double().abs()))), name)
    if loss:
        out = torch.empty((), device=DEV)
        _ok(L, L.hpri_bce_finish(P(part), nblk, N * K * HW, P(out), _st()))
        ref = torch.nn.functional.binary_cross_entropy_with_logits(y.double().cpu().view(N, K, HW), tgt.double().cpu())
        assert abs(out.item() - ref.item()) <= 1e-6 * max(1.0, abs(ref.item()))


def _head_backward(L, dt, h, shape, src, tgt, gs, acc, dx16):
    """One hpri_outconv_bwd_x16 launch.  Returns (dx buffer, its contents before, dcs, doff, dcw, guarded dw, guarded db)."""
    N, HW, C, K, coff = shape
    x, cs = _head_source(h["fwd"]["a"], dt, coff)
    w = h["fwd"]["b"].to(DEV)
    dcw, doff = rup(C, 4) + 4, 4
    dcs = dcw + 12
    before = _frame(N * HW, dcs)
    if acc:
        _put(before, doff, h["dx"]["prior"].to(dt if dx16 else torch.float32), dcw, 5.0)
    dx = before.to(dt if dx16 else torch.float32).to(DEV)
    bw, dw = _guarded(K * C)
    bb, db = _guarded(K)
    if acc:
        dw.copy_(h["dw"]["prior"].reshape(-1))
        db.copy_(h["db_prior"])
    nblk, cpart = ctypes.c_int(), ctypes.c_int()
    _ok(L, L.hpri_outconv_bwd_plan(N, HW, C, K, ctypes.byref(nblk), ctypes.byref(cpart)))
    ws = torch.full((nblk.value * K * 2 * cpart.value,), NAN, device=DEV)
    _ok(L, L.hpri_outconv_bwd_x16(P(src), P(tgt), P(gs), P(x), cs, coff, P(w), P(dx), int(dx16), dcs, doff, dcw, acc, P(dw), P(db), acc, P(ws),
                                  ws.numel(), N, HW, C, K, _st()))
    torch.cuda.synchronize()
    return dx, before, dcs, doff, dcw, bw, bb


HEAD_BWD = [(s, dx16) for s in HC.HEAD for dx16 in (False, True) if s[3] == 1 or not dx16]      # 16-bit dx rows are built for one class


@pytest.mark.parametrize("kind,loss", [("int", False), ("int", True), ("real", False)], ids=["int-plain", "int-loss", "real-plain"])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("shape,dx16", HEAD_BWD, ids=["%s-dx%d" % (sid(s), 16 if d else 32) for s, d in HEAD_BWD])
def test_head_backward(lib16, shape, dx16, acc, kind, loss):
    """hpri_outconv_bwd_x16: dx into a channel-slice view (fp32, or 16-bit rows for one class), dw, db; plain dy, or -- integer kind
    -- the loss inside with logits 0 / +-200 and gscale = 2 N K P, for which 2 (sigmoid - target) is an exact small integer."""
    L, dt, lib = lib16
    N, HW, C, K, coff = shape
    h = HC.head_case(kind, lib, shape)
    name = "h16/head_bwd_%s_%s_acc%d/%s/%s" % ("loss" if loss else "plain", "dx16" if dx16 else "dx32", acc, lib, sid(shape))
    g = h["dx"]["a"]                                                           # dy [N HW, K]
    to_nkp = lambda t: t.view(N, HW, K).permute(0, 2, 1).contiguous()
    if loss:
        g = g.clamp(-2, 2)
        lut = torch.tensor([EXACT_BCE[v] for v in range(-2, 3)])
        pair = lut[(g + 2).long()]
        src, tgt = to_nkp(pair[..., 0]).to(DEV), to_nkp(pair[..., 1]).to(DEV)
        gs = torch.tensor([2.0 * N * K * HW], device=DEV)
    else:
        src, tgt, gs = to_nkp(g).to(DEV), None, None
    cdx, cdw = dict(h["dx"]), dict(h["dw"])
    if loss:                                                                   # the clamped gradient: magnitudes only shrink
        cdx.update(a=g, ref=HC.product("rows", g, cdx["b"]), mag=HC.product("rows", g.abs(), cdx["b"].abs()))
        cdw.update(b=g, ref=HC.product("wgrad1x1", cdw["a"], g), mag=HC.product("wgrad1x1", cdw["a"].abs(), g.abs()))
    dx, before, dcs, doff, dcw, bw, bb = _head_backward(L, dt, h, shape, src, tgt, gs, acc, dx16)
    odt = dt if dx16 else torch.float32
    old = cdx["prior"].to(odt).double() if acc else 0.0
    want = _put(before.clone(), doff, (cdx["ref"] + old).float(), dcw, None if acc else 0.0)
    bnd = _put(_frame(N * HW, dcs, 0.0), doff, HC.bound(cdx, old.abs() if acc else 0.0))
    if not dx16:
        _out32(kind, name + " dx", dx, want, bnd, name + "/dx")
    elif kind == "int":
        _check16(name + " dx", dx, want.float().to(dt))
    else:
        _check16_between(name + " dx", dx, want, bnd, dt)
    oldw = cdw["prior"].double() if acc else 0.0
    _out32(kind, name + " dw", bw, _guard_frame(K * C, (cdw["ref"] + oldw).float()), _guard_bound(K * C, HC.bound(cdw, cdw["prior"].double().abs() if acc else 0.0)),
           name + "/dw")
    oldb = h["db_prior"].double() if acc else 0.0
    db_ref = g.double().sum(0)
    db_bnd = (N * HW + 2) * U * (g.double().abs().sum(0) + (h["db_prior"].double().abs() if acc else 0.0))
    _out32(kind, name + " db", bb, _guard_frame(K, (db_ref + oldb).float()), _guard_bound(K, db_bnd), name + "/db")


# ---------------------------------------------------------------------------------------------------------------------------
# Max-pooling over / into 16-bit rows: selections and one fp32 add, so both kinds are compared exactly
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("outputs", ["y+planes", "planes", "y"])
@pytest.mark.parametrize("shape", HC.POOL, ids=sid)
def test_maxpool_forward(lib16, shape, outputs, kind):
    """hpri_maxpool2_fwd_x16 over a channel slice of 16-bit rows (odd H and W in the first shape, ties inside the windows): the fp32
    output and / or the 16-bit plane, whose pad channels [C, pl_cw) are zero-filled."""
    L, dt, lib = lib16
    N, H, W, C = shape
    p = HC.pool_case(kind, lib, shape)
    name = "h16/maxpool_fwd_%s/%s/%s" % (outputs, lib, sid(shape))
    OH, OW = H // 2, W // 2
    xs, xoff = C + 16, 8
    x = _planes(p["x"].reshape(-1, C), dt, xs, xoff, C)
    ycs, yoff = C + 8, 4
    pl_cs, pl_coff, pl_cw = C + 16, 4, C + 4
    y = _frame(N * OH * OW, ycs).float().to(DEV) if "y" in outputs else None
    pl = _frame(N * OH * OW, pl_cs).to(dt).to(DEV) if "planes" in outputs else None
    _ok(L, L.hpri_maxpool2_fwd_x16(P(x), xs, xoff, P(y), ycs if y is not None else 0, yoff if y is not None else 0, N, H, W, C, P(pl),
                                   N * OH * OW * pl_cs if pl is not None else 0, pl_cs if pl is not None else 0, pl_coff if pl is not None else 0,
                                   pl_cw if pl is not None else 0, 1 if pl is not None else 0, _st()))
    torch.cuda.synchronize()
    vals = p["fwd"].reshape(-1, C)
    if y is not None:
        _check32(name + " y", y, _put(_frame(N * OH * OW, ycs), yoff, vals))
    if pl is not None:
        _check16(name + " planes", pl, _put(_frame(N * OH * OW, pl_cs), pl_coff, vals, pl_cw).float().to(dt))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("dx16", [0, 1], ids=["dx32", "dx16"])
@pytest.mark.parametrize("x16", [0, 1], ids=["x32", "x16"])
@pytest.mark.parametrize("shape", HC.POOL, ids=sid)
def test_maxpool_backward(lib16, shape, x16, dx16, acc, kind):
    """hpri_maxpool2_bwd_x16, every storage combination: the gradient goes to the FIRST maximum of a window in scan order, an odd last
    row / column receives zero; written or added (one fp32 add), as fp32 or rounded once to 16-bit rows."""
    L, dt, lib = lib16
    N, H, W, C = shape
    p = HC.pool_case(kind, lib, shape)
    name = "h16/maxpool_bwd_x%d_dx%d_acc%d/%s/%s" % (16 if x16 else 32, 16 if dx16 else 32, acc, lib, sid(shape))
    OH, OW = H // 2, W // 2
    xs, xoff = C + 16, 8
    xv = p["x"].reshape(-1, C)
    x = _planes(xv, dt, xs, xoff, C) if x16 else _put(_frame(N * H * W, xs, X_PAD_VALUE), xoff, xv).float().to(DEV)
    dcs, doff = C + 8, 4
    dy = _put(_frame(N * OH * OW, dcs, X_PAD_VALUE), doff, p["dy"].reshape(-1, C)).float().to(DEV)
    odt = dt if dx16 else torch.float32
    gcs, goff = C + 12, 8
    before = _frame(N * H * W, gcs)
    old = p["prior"].reshape(-1, C).to(odt)
    if acc:
        _put(before, goff, old)
    dx = before.to(odt).to(DEV)
    _ok(L, L.hpri_maxpool2_bwd_x16(P(x), x16, xs, xoff, P(dy), dcs, doff, P(dx), dx16, gcs, goff, N, H, W, C, acc, _st()))
    torch.cuda.synchronize()
    routed = p["routed"].reshape(-1, C).float()
    vals = routed + old.float() if acc else routed                             # one fp32 add: torch's is the kernel's
    if dx16:
        _check16(name, dx, _put(before.clone().float().to(dt), goff, vals.to(dt)))
    else:
        _check32(name, dx, _put(before.clone(), goff, vals))


# ---------------------------------------------------------------------------------------------------------------------------
# The 16-bit weight packers
# ---------------------------------------------------------------------------------------------------------------------------
PACK_KS = (5, 32, 40)
PACK_NCOLS = ((7, 64), (70, 128))


def _range_values(dt):
    """fp32 weights that walk the roundings of the 16-bit type (ties to even, and in half the subnormals and the overflow threshold)."""
    eps = torch.finfo(dt).eps
    v = [1 + eps / 2, 1 + 3 * eps / 2, -(1 + eps / 2), 1 + eps / 2 + eps / 1024]
    if dt == torch.float16:
        v += [65519.0, 65520.0, -65520.0, 131008.0, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24, 1023 * 2.0 ** -24, -(2.0 ** -25), 2.0 ** -25 * 1.0001]
    return torch.tensor(v)


@functools.lru_cache(maxsize=None)
def _pack_case(dt, mode, K, ncols, ncols_pad, T, scaled=False):
    """Source weight in its nn.Parameter layout (the first elements replaced by the range values), the packer's (src_d1, Cup) and the
    expected panel values [chunks][T][32][ncols_pad] in fp32 (tests/_direct_cases.py: pack_expected)."""
    g = torch.Generator().manual_seed(1000 * mode + 10 * K + ncols + T)
    cup = 0
    if mode == 0:
        w, d1 = torch.randn(ncols, K, T, generator=g), K
    elif mode == 1:
        w, d1 = torch.randn(K, ncols, T, generator=g), ncols
    elif mode == 2:
        cup = D.cdiv(ncols, 4)
        w, d1 = torch.randn(K, cup, 4, generator=g), cup
    else:
        cup = D.cdiv(K, 4)
        w, d1 = torch.randn(ncols, cup, 4, generator=g), cup
    rv = _range_values(dt)
    if not scaled:
        w.view(-1)[:rv.numel()] = rv
    scale = (torch.rand(ncols, generator=g) + 0.5) if scaled else None
    want = D.pack_expected(w, mode, K, ncols, ncols_pad, T, d1, cup, None if scale is None else scale.numpy())
    return w, d1, cup, scale, torch.from_numpy(want)


def _pack_cases():
    return [(m, K, n, npad, T) for m in (0, 1, 2, 3) for K in PACK_KS for (n, npad) in PACK_NCOLS for T in ((9, 1) if m < 2 and K == 5 else (9,) if m < 2 else (1,))]


def _split_planes(want, split, dt):
    """[chunks][T][32][ncols_pad] fp32 -> [chunks][T][plane][ncols_pad][32]: plane p = round16(rest), rest -= plane."""
    rest = want.permute(0, 1, 3, 2).contiguous()
    out = []
    for _ in range(split + 1):
        h = rest.to(dt)
        out.append(h)
        rest = rest - h.float()
    return torch.stack(out, 2)


@pytest.mark.parametrize("mode,K,ncols,ncols_pad,T", _pack_cases())
def test_pack_weight_16(lib16, mode, K, ncols, ncols_pad, T):
    """hpri_pack_weight_bf16: the packed words equal torch's .to(dtype) of the weight bit for bit (the destination starts as NaN: pad
    rows and columns are written, as zeros); the split planes exist in the bf16 library only."""
    L, dt, lib = lib16
    w, d1, cup, _, want = _pack_case(dt, mode, K, ncols, ncols_pad, T)
    wd = w.to(DEV)
    for split in ((0, 1, 2) if lib == "bf16" else (0,)):
        wantp = _split_planes(want, split, dt)
        wp = torch.full((wantp.numel(),), NAN, dtype=dt, device=DEV)
        _ok(L, L.hpri_pack_weight_bf16(P(wd), P(wp), mode, K, ncols, ncols_pad, T, d1, cup, split, _st()))
        torch.cuda.synchronize()
        _check16("h16/pack/%s/mode%d/%dx%dx%d/split%d" % (lib, mode, K, ncols, T, split), wp, wantp.reshape(-1, 32))
    if dt == torch.float16 and mode == 0:
        assert int(torch.isinf(wantp.float()).sum()) >= 3 and int(((wantp.float() != 0) & (wantp.float().abs() < 2.0 ** -14)).sum()) >= 3


@pytest.mark.parametrize("K", PACK_KS)
@pytest.mark.parametrize("ncols,ncols_pad", PACK_NCOLS)
def test_pack_weight_16_scaled(lib16, K, ncols, ncols_pad):
    """hpri_pack_weight_bf16_scaled: one fp32 multiply by the per-output-channel scale, then the rounding."""
    L, dt, lib = lib16
    w, d1, _, scale, want = _pack_case(dt, 0, K, ncols, ncols_pad, 9, scaled=True)
    wantp = _split_planes(want, 0, dt)
    wp = torch.full((wantp.numel(),), NAN, dtype=dt, device=DEV)
    wd, sd = w.to(DEV), scale.to(DEV)
    _ok(L, L.hpri_pack_weight_bf16_scaled(P(wd), P(wp), P(sd), K, ncols, ncols_pad, 9, d1, 0, _st()))
    torch.cuda.synchronize()
    _check16("h16/pack_scaled/%s/%dx%d" % (lib, K, ncols), wp, wantp.reshape(-1, 32))


@pytest.mark.parametrize("mode,K,ncols,ncols_pad,gap_at,gap_len", [(0, 40, 7, 64, 5, 27), (0, 40, 70, 128, 5, 27), (0, 32, 70, 128, 0, 3),
                                                                   (1, 40, 70, 128, 7, 25), (1, 5, 7, 64, 2, 3), (1, 32, 70, 128, 45, 25)])
def test_pack_weight_16_gap(lib16, mode, K, ncols, ncols_pad, gap_at, gap_len):
    """hpri_pack_weight_bf16_gap: gap_len structural zeros from gap_at on along the input-channel axis."""
    L, dt, lib = lib16
    T = 9
    width = (K if mode == 0 else ncols) - gap_len
    g = torch.Generator().manual_seed(77 + gap_at)
    w = torch.randn(ncols, width, T, generator=g) if mode == 0 else torch.randn(K, width, T, generator=g)
    rv = _range_values(dt)
    w.view(-1)[:rv.numel()] = rv
    want = torch.from_numpy(D.pack_expected(w, mode, K, ncols, ncols_pad, T, width, 0, None, gap_at, gap_len))
    wantp = _split_planes(want, 0, dt)
    wp = torch.full((wantp.numel(),), NAN, dtype=dt, device=DEV)
    wd = w.to(DEV)
    _ok(L, L.hpri_pack_weight_bf16_gap(P(wd), P(wp), mode, K, ncols, ncols_pad, T, width, gap_at, gap_len, _st()))
    torch.cuda.synchronize()
    _check16("h16/pack_gap/%s/mode%d/%dx%d" % (lib, mode, K, ncols), wp, wantp.reshape(-1, 32))


# ---------------------------------------------------------------------------------------------------------------------------
# Range tables
# ---------------------------------------------------------------------------------------------------------------------------
def _edge(lib, form):
    return HC.edge_problem(lib, *HC.EDGE[form])


def test_range_gemm(lib16):
    """Rows GEMM, K = C = 32 on 8 rows: the fp32 view holds every edge output exactly (a subnormal half operand is consumed at its value),
    the 16-bit view torch's rounding of it -- ties to even, gradual underflow, inf from 65520 on."""
    L, dt, lib = lib16
    e = _edge(lib, "rows")
    r = _gemm_forward(L, dt, e["A"], e["B"], None, 1, e["A"].shape[0], with_stats=False)
    name = "h16/range_gemm/%s" % lib
    _check32(name + " y", r["y"], _put(_frame(r["rows"], r["ycs"]), r["yoff"], e["y64"], r["cw"]))
    _check16(name + " y16", r["y16"], _put(_frame(r["rows"], r["y16cs"]).to(dt), r["y16off"], e["y64"].float().to(dt), r["cw"]))
    assert torch.equal(HC.round16(e["y64"].float(), dt), e["bits"])


def test_range_transposed_convolution(lib16):
    """ConvTranspose on a 1 x 2 x 3 grid, 32 -> 32 channels, one selector per tap: forward (fp32 and 16-bit views), data gradient (fp32
    rows and _y16)."""
    L, dt, lib = lib16
    shape = (1, 2, 3, 32, 32, 1, 1)
    N, H, W, Cin, Cup = shape[:5]
    e = _edge(lib, "convt_fwd")                                               # [6 pixels, 32] x [4 * 32 columns, 32]
    wt = e["B"].view(2, 2, Cup, Cin).permute(3, 2, 0, 1).contiguous()         # column tap * Cup + co -> wt[ci][co][a][b]
    y, y16, ycs, rows, place, _ = _convt_forward(L, dt, e["A"].view(N, H, W, Cin), wt, torch.zeros(Cup), shape)
    vals = e["y64"].view(N, H, W, 2, 2, Cup).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, Cup)
    assert torch.equal(vals, HC.product("convt_fwd", e["A"].view(N, H, W, Cin), wt))
    name = "h16/range_convt_fwd/%s" % lib
    _check32(name + " y", y, place(_frame(rows, ycs), vals))
    _check16(name + " y16", y16, place(_frame(rows, ycs).to(dt), vals.float().to(dt)))
    e = _edge(lib, "convt_dgrad")                                             # [6 pixels, K = 4 * 32] x [32 columns, K]
    dy = e["A"].view(N, H, W, 2, 2, Cup).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, Cup)
    wt = e["B"].view(Cin, 2, 2, Cup).permute(0, 3, 1, 2).contiguous()         # k = tap * Cup + co -> wt[ci][co][a][b]
    assert torch.equal(e["y64"], HC.product("convt_dgrad", dy, wt))
    name = "h16/range_convt_dgrad/%s" % lib
    for form in ("acc0", "y16"):
        dx, before, xcs, xoff, cw = _convt_dgrad(L, dt, dy, wt, None, shape, form)
        if form == "acc0":
            _check32(name + " dx", dx, _put(before.clone(), xoff, e["y64"], cw))
        else:
            _check16(name + " dx16", dx, _put(before.clone(), xoff, e["y64"], cw).float().to(dt))


def test_range_plane_convolution(lib16):
    """3x3 convolution over 1 x 4 x 32 with 32 -> 64 channels, only the centre tap non-zero: fp32 output, the 16-bit output bit; and
    32 -> 128 channels through hpri_conv_bf16v3_y2 with both outputs as 16-bit rows."""
    L, dt, lib = lib16
    for form, Cout in (("conv", 64), ("conv_y2", 128)):
        e = _edge(lib, form)
        shape = (1, 4, 32, 32, Cout)
        w = torch.zeros(Cout, 32, 3, 3)
        w[:, :, 1, 1] = e["B"]
        x = e["A"].view(1, 4, 32, 32)
        assert torch.equal(e["y64"], HC.product("conv", x, w))
        p = _conv(L, dt, x, w, None, shape, "fwd")
        assert p["ksplit"] == 1
        npx, name = p["npx"], "h16/range_%s/%s" % (form, lib)
        if form == "conv":
            want = _put(_frame(npx, p["ycs"]), p["yoff"], e["y64"], p["cw"])
            y = _frame(npx, p["ycs"]).float().to(DEV)
            _ok(L, _conv_launch(L, p, y, None, 0))
            y16 = _frame(npx, p["ycs"]).to(dt).to(DEV)
            _ok(L, _conv_launch(L, p, y16, None, 4))
            torch.cuda.synchronize()
            _check32(name + " y", y, want)
            _check16(name + " y16", y16, want.float().to(dt))
        else:
            c0, cw2 = 64, 64
            y = _frame(npx, c0 + 8).to(dt).to(DEV)
            y2 = _frame(npx, cw2 + 8).to(dt).to(DEV)
            stats = torch.full((p["ntiles"] * p["cout_pad"] * 4,), NAN, device=DEV)
            _ok(L, L.hpri_conv_bf16v3_y2(P(p["xp"]), p["xcs"], p["xoff"], P(p["wp"]), P(None), P(y), c0 + 8, 4, P(stats), 1, 4, 32, p["cs16"], Cout,
                                         p["cout_pad"], c0, P(y2), cw2 + 8, 4, c0, cw2, 3, _st()))
            torch.cuda.synchronize()
            _check16(name + " y", y, _put(_frame(npx, c0 + 8), 4, e["y64"][:, :c0]).float().to(dt))
            _check16(name + " y2", y2, _put(_frame(npx, cw2 + 8), 4, e["y64"][:, c0:]).float().to(dt))


def test_range_weight_gradients(lib16):
    """The weight-gradient kernels consume 16-bit operands through the transposed LDS reads and the MFMA: every fp32 output of the edge
    tables exactly (subnormal half operands at their value).  1x1: two-term selectors over 64 pixels; 3x3 over 1 x 4 x 32 and the
    transposed convolution over 1 x 4 x 16: one non-zero pixel per input channel, so every tap is a single product (or zero)."""
    L, dt, lib = lib16
    e = _edge(lib, "wgrad1x1")                                                 # rows = Cout, K = pixels, columns = Cin
    x, dy = e["B"].t().contiguous(), e["A"].t().contiguous()
    assert torch.equal(e["y64"], HC.product("wgrad1x1", x, dy))
    buf = _wgrad1x1(L, dt, x, dy, torch.zeros(dy.shape[1], x.shape[1]), 0)
    _check32("h16/range_wgrad1x1/%s" % lib, buf, _guard_frame(e["y64"].numel(), e["y64"]))
    e = _edge(lib, "wgrad_conv")
    x, dy = e["B"].t().reshape(1, 4, 32, 32), e["A"].t().reshape(1, 4, 32, 64)
    ref = HC.product("wgrad_conv", x, dy)
    assert torch.equal(ref, ref.float().double()) and torch.equal(ref[:, :, 1, 1], e["y64"])
    buf, _ = _wgrad_conv(L, dt, x, dy, torch.zeros(64, 32, 3, 3), (1, 4, 32, 32, 64), 0)
    _check32("h16/range_wgrad_conv/%s" % lib, buf, _guard_frame(ref.numel(), ref))
    e = _edge(lib, "wgrad_convt")                                              # rows = tap * Cup + co (Cup = 64), K = 64 pixels, columns = Cin
    x = e["B"].t().reshape(1, 4, 16, 32)
    dy = e["A"].t().reshape(1, 4, 16, 2, 2, 64).permute(0, 1, 3, 2, 4, 5).reshape(1, 8, 32, 64)
    ref = HC.product("wgrad_convt", x, dy)
    assert torch.equal(ref, ref.float().double()) and torch.equal(ref.permute(2, 3, 1, 0).reshape(256, 32), e["y64"])
    buf = _wgrad_convt(L, dt, x, dy, torch.zeros(32, 64, 2, 2), (1, 4, 16, 32, 64, 1, 1))
    _check32("h16/range_wgrad_convt/%s" % lib, buf, _guard_frame(ref.numel(), ref))


def test_range_head_and_pooling_stores(lib16):
    """The 16-bit stores of the elementwise kernels: the head's dx_bf16 (dx = dy w with w = 1) and hpri_maxpool2_bwd_x16 round an fp32
    gradient holding every edge output as torch does."""
    L, dt, lib = lib16
    vals = torch.unique(_edge(lib, "rows")["y64"].reshape(-1)).float()
    n = vals.numel()
    # head: N = 1, HW = n pixels, C = 8 channels, one class
    x = torch.zeros(n, 32, dtype=dt, device=DEV)
    w = torch.ones(1, 8, device=DEV)
    dx = _frame(n, 16).to(dt).to(DEV)
    dw, db = torch.zeros(1, 8, device=DEV), torch.zeros(1, device=DEV)
    nblk, cpart = ctypes.c_int(), ctypes.c_int()
    _ok(L, L.hpri_outconv_bwd_plan(1, n, 8, 1, ctypes.byref(nblk), ctypes.byref(cpart)))
    ws = torch.empty(nblk.value * 2 * cpart.value, device=DEV)
    gd = vals.to(DEV)
    _ok(L, L.hpri_outconv_bwd_x16(P(gd), P(None), P(None), P(x), 32, 0, P(w), P(dx), 1, 16, 4, 8, 0, P(dw), P(db), 0, P(ws), ws.numel(), 1, n, 8,
                                  1, _st()))
    torch.cuda.synchronize()
    _check16("h16/range_head_dx16/%s" % lib, dx, _put(_frame(n, 16), 4, vals[:, None].expand(n, 8).double()).float().to(dt))
    # pooling: one window per value (N = 1, H = 2, W = 2 n, C = 4), the maximum in the second column of each window
    C = 4
    xin = torch.zeros(1, 2, 2 * n, C)
    xin[:, 0, 1::2] = 1.0
    dy = vals[None, None, :, None].expand(1, 1, n, C).contiguous()
    g = _frame(2 * 2 * n, C + 8).to(dt).to(DEV)
    xd, dyd = xin.to(dt).to(DEV), dy.to(DEV)
    _ok(L, L.hpri_maxpool2_bwd_x16(P(xd), 1, C, 0, P(dyd), C, 0, P(g), 1, C + 8, 4, 1, 2, 2 * n, C, 0, _st()))
    torch.cuda.synchronize()
    routed = torch.zeros(1, 2, 2 * n, C, dtype=torch.float64)
    routed[:, 0, 1::2] = dy.double()
    _check16("h16/range_maxpool_dx16/%s" % lib, g, _put(_frame(4 * n, C + 8), 4, routed.reshape(-1, C)).float().to(dt))


# ---------------------------------------------------------------------------------------------------------------------------
# hpri_set_loss_scale
# ---------------------------------------------------------------------------------------------------------------------------
LS_SHAPE = (1, 333, 64, 1, 0)                                                 # 333 logits: s = 512, then 16 x 512


def _ls_inputs(lib):
    N, HW, C, K, _ = LS_SHAPE
    g = torch.Generator().manual_seed(91)
    dt = HC.DTYPES[lib]
    x = (torch.randn(N * HW, C, generator=g) * 1.5 + 0.3).to(dt).float()
    return dict(x=x, w=torch.randn(K, C, generator=g) / 8, logits=torch.randn(N, K, HW, generator=g) * 2, tgt=(torch.rand(N, K, HW, generator=g) > 0.7).float(),
                dy=torch.randn(N, K, HW, generator=g) * 1e-3, gamma=torch.randn(C, generator=g) + 0.2, beta=torch.randn(C, generator=g) * 0.5)


def _ls_x16(L, dt, i, with_target, dx16):
    N, HW, C, K, _ = LS_SHAPE
    xb, cs = _head_source(i["x"], dt, 0)
    dx = torch.zeros(N * HW, C, dtype=dt if dx16 else torch.float32, device=DEV)
    dw, db = torch.zeros(K, C, device=DEV), torch.zeros(K, device=DEV)
    nblk, cpart = ctypes.c_int(), ctypes.c_int()
    _ok(L, L.hpri_outconv_bwd_plan(N, HW, C, K, ctypes.byref(nblk), ctypes.byref(cpart)))
    ws = torch.empty(nblk.value * K * 2 * cpart.value, device=DEV)
    src = (i["logits"] if with_target else i["dy"]).to(DEV)
    tgt, gs = (i["tgt"].to(DEV), torch.tensor([0.5], device=DEV)) if with_target else (None, None)
    w = i["w"].to(DEV)
    _ok(L, L.hpri_outconv_bwd_x16(P(src), P(tgt), P(gs), P(xb), cs, 0, P(w), P(dx), int(dx16), C, 0, C, 0, P(dw), P(db), 0, P(ws), ws.numel(),
                                  N, HW, C, K, _st()))
    torch.cuda.synchronize()
    return dict(dx=dx.cpu(), dw=dw.cpu(), db=db.cpu())


def _ls_bce(L, dt, i, with_target, dx16=False):
    N, HW, C, K, _ = LS_SHAPE
    x = i["x"].to(DEV)
    dx = torch.zeros(N * HW, C, device=DEV)
    dw, db = torch.zeros(K, C, device=DEV), torch.zeros(K, device=DEV)
    nblk, cpart = ctypes.c_int(), ctypes.c_int()
    _ok(L, L.hpri_outconv_bwd_plan(N, HW, C, K, ctypes.byref(nblk), ctypes.byref(cpart)))
    ws = torch.empty(nblk.value * K * 2 * cpart.value, device=DEV)
    w, logits, tgt, gs, dy = i["w"].to(DEV), i["logits"].to(DEV), i["tgt"].to(DEV), torch.tensor([0.5], device=DEV), i["dy"].to(DEV)
    common = (P(x), C, 0, P(w), P(dx), C, 0, C, 0, P(dw), P(db), 0, P(ws), ws.numel(), N, HW, C, K, _st())
    if with_target:
        _ok(L, L.hpri_outconv_bwd_bce(P(logits), P(tgt), P(gs), *common))
    else:
        _ok(L, L.hpri_outconv_bwd(P(dy), *common))
    torch.cuda.synchronize()
    return dict(dx=dx.cpu(), dw=dw.cpu(), db=db.cpu())


def _ls_bn_head(L, dt, i, with_target, dx16=False):
    N, HW, C, K, _ = LS_SHAPE
    x = i["x"].to(DEV)
    xd = x.double()
    mean = xd.mean(0).float().contiguous()
    invstd = (1.0 / torch.sqrt(xd.var(0, unbiased=False) + 1e-5)).float().contiguous()
    scale = (i["gamma"].to(DEV) * invstd).contiguous()
    shift = (i["beta"].to(DEV) - mean * scale).contiguous()
    dx = torch.zeros(N * HW, C, device=DEV)
    out = {k: torch.zeros(n, device=DEV) for k, n in (("dgamma", C), ("dbeta", C), ("dbias", C), ("dw", C), ("db", 1))}
    ws = torch.empty(L.hpri_bn_relu_outconv_bwd_ws(N, HW, C), device=DEV)
    src = (i["logits"] if with_target else i["dy"]).to(DEV)
    tgt, gs = (i["tgt"].to(DEV), torch.tensor([0.5], device=DEV)) if with_target else (None, None)
    w = i["w"].to(DEV)
    _ok(L, L.hpri_bn_relu_outconv_bwd(P(src), P(tgt), P(gs), P(x), C, 0, P(w), P(dx), C, 0, C, P(mean), P(invstd), P(scale), P(shift),
                                      P(out["dgamma"]), P(out["dbeta"]), 0, P(out["dbias"]), 0, P(out["dw"]), P(out["db"]), 0, P(ws), ws.numel(), N, HW, C, 1,
                                      1, _st()))
    torch.cuda.synchronize()
    return dict(dx=dx.cpu(), **{k: v.cpu() for k, v in out.items()})


LS_ENTRIES = {"outconv_bwd_x16": _ls_x16, "outconv_bwd_bce": _ls_bce, "bn_relu_outconv_bwd": _ls_bn_head}


def _set_scale(L, s):
    _ok(L, L.hpri_set_loss_scale(s))


@pytest.mark.parametrize("entry", sorted(LS_ENTRIES))
def test_loss_scale_multiplies_the_fused_loss_gradient_exactly(lib16, entry):
    """With a target the fused heads form s x the loss gradient: every output equals the scale-1 output times s bit for bit (s a power of
    two, every value a normal fp32), for s = the next power of two above the number of logits and 16 times that; a 16-bit dx equals
    torch's rounding of s x the fp32 dx.  Without a target (a plain dy) nothing changes with s."""
    L, dt, lib = lib16
    run, i = LS_ENTRIES[entry], _ls_inputs(lib)
    n_logits = LS_SHAPE[0] * LS_SHAPE[1] * LS_SHAPE[3]
    s0 = 1 << n_logits.bit_length()
    assert s0 == 512
    try:
        _set_scale(L, 1.0)
        base, plain = run(L, dt, i, True, False), run(L, dt, i, False, False)
        for k, v in base.items():
            tiny = (v != 0) & (v.abs() < 2.0 ** -126)
            assert float(v.abs().max()) > 0 or k == "dbias", k
            assert not bool(tiny.any()) and bool(torch.isfinite(v).all()), "%s: the case must keep every value a normal fp32" % k
        if entry == "outconv_bwd_x16":
            _check16("%s/%s dx16 at scale 1" % (entry, lib), run(L, dt, i, True, True)["dx"], base["dx"].to(dt))
        for s in (float(s0), 16.0 * s0):
            _set_scale(L, s)
            got = run(L, dt, i, True, False)
            for k in base:
                _check32("%s/%s %s at scale %g" % (entry, lib, k, s), got[k], (base[k] * s).double())
            if entry == "outconv_bwd_x16":
                _check16("%s/%s dx16 at scale %g" % (entry, lib, s), run(L, dt, i, True, True)["dx"], (base["dx"] * s).to(dt))
            same = run(L, dt, i, False, False)
            for k in plain:
                _check32("%s/%s %s of a plain dy at scale %g" % (entry, lib, k, s), same[k], plain[k].double())
    finally:
        _set_scale(L, 1.0)


def test_loss_scale_refuses_zero_and_negative_values(lib16):
    L, dt, lib = lib16
    try:
        _set_scale(L, 4.0)
        assert L.hpri_set_loss_scale(0.0) != 0 and L.hpri_set_loss_scale(-2.0) != 0 and L.hpri_set_loss_scale(float("nan")) != 0
        i = _ls_inputs(lib)
        got = _ls_x16(L, dt, i, True, False)                                   # a refused value leaves the scale as it was
        _set_scale(L, 1.0)
        base = _ls_x16(L, dt, i, True, False)
        for k in base:
            _check32("refused scale/%s %s" % (lib, k), got[k], (base[k] * 4.0).double())
    finally:
        _set_scale(L, 1.0)


def test_loss_scale_belongs_to_the_calling_thread(lib16):
    """Set on the main thread, a launch from a fresh thread runs at scale 1 (the header: the heads of the CALLING THREAD)."""
    L, dt, lib = lib16
    i = _ls_inputs(lib)
    try:
        _set_scale(L, 1.0)
        base = _ls_x16(L, dt, i, True, False)
        _set_scale(L, 512.0)
        box = {}

        def work():
            try:
                box["got"] = _ls_x16(L, dt, i, True, False)
            except BaseException as exc:                                       # noqa: BLE001 -- handed to the main thread
                box["exc"] = exc
        t = threading.Thread(target=work)
        t.start()
        t.join()
        assert "exc" not in box, box.get("exc")
        for k in base:
            _check32("fresh thread/%s %s" % (lib, k), box["got"][k], base[k].double())
        here = _ls_x16(L, dt, i, True, False)
        for k in base:
            _check32("main thread/%s %s" % (lib, k), here[k], (base[k] * 512.0).double())
    finally:
        _set_scale(L, 1.0)
