"""The bandwidth-bound kernels of elementwise.hip that sit between the convolutions, called directly through the C ABI
(include/hyperpri_hip.h) against a plain reference of the same operation computed on the CPU: the layout passes
(hpri_nchw_to_nhwc(_pl), hpri_nhwc_to_nchw, hpri_to_planes), MaxPool2d(2) forward, the slice copy / shifted copy / pad fill /
product of Up.forward, the bilinear x2 upsample with its adjoint, and the counter-based generator behind bench.py.

Three rules hold in every test.  (1) Untouched memory: each destination starts as random "prior" data, and every element outside
the region the kernel owns -- the other channels of the row stride, the pixels outside a padded window, the floats in front of
and behind a dense tensor -- must come back bit for bit.  (2) NaN bait: those outside regions of every SOURCE hold NaN / inf,
which a kernel that read them would carry into a result.  (3) Grid-stride reach: each kernel launched through ew_blocks (capped
at 8192 blocks of 256 threads) runs one case of more than 8192 * 256 work items, so that its stride loop is taken; every other
case is tiny.  Cases that write 16-bit planes run against both product libraries (bf16: libhyperpri_hip.so; IEEE half:
libhyperpri_hip_f16.so).  Needs a real MI355X: ``-m gpu``.

Copies, maxima and single fp32 operations are gated bit for bit (recorded as the number of differing elements against a bound of
0).  Tolerances are multiples of U = 2^-24, the unit roundoff of fp32, derived next to each gate and recorded as error / bound."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24                   # unit roundoff of fp32
NAN, INF = float("nan"), float("inf")
ERR_ARG, ERR_UNSUPPORTED = -1, -2
GUARD = 64                       # floats of prior data / bait around a dense tensor (256 bytes: keeps the 16-byte alignment)
CAP = 8192 * 256                 # work items one launch of ew_blocks covers without striding


def rup(x, m):
    return (x + m - 1) // m * m


def P(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    from hyperpri_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib16(request):
    """(library, 16-bit torch dtype) of each product library: the "bf16" entry points use the library's own 16-bit type."""
    from hyperpri_amd import _lib
    if request.param == "bf16":
        return _lib.load(), torch.bfloat16
    if not os.path.exists(_lib.LIB_F16_PATH):
        pytest.skip("the half-precision library is not built")
    return _lib.load_f16(), torch.float16            # (a library that is there and does not load is an error, not a skip)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed):
    return torch.randn(shape, generator=_gen(seed))


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _exact(key, got, want):
    """Bit for bit (signed zeros included); the number of differing elements goes to the margins file against a bound of 0."""
    assert got.shape == want.shape and got.dtype == want.dtype, (key, got.shape, want.shape)
    bad = int((_bits(got) != _bits(want)).sum())
    record_margin(key, bad, 0)
    assert bad == 0, (key, bad, "elements differ")


def _gate(key, err, tol):
    """max err / tol over the elements (0 / 0 counts as 0: an exactly right value where the bound is 0)."""
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    m = float(r.max()) if r.numel() else 0.0
    record_margin(key, m, 1.0)
    assert m <= 1.0, (key, m)


def _view(npx, cs, coff, vals):
    """[npx][cs] SOURCE buffer: channels [coff, coff + C) = vals, every other channel NaN / +inf / -inf."""
    buf = torch.tensor([NAN, INF, -INF])[torch.arange(npx * cs) % 3].view(npx, cs).clone()
    buf[:, coff:coff + vals.shape[1]] = vals
    return buf


def _dense(vals, shift=0):
    """A dense SOURCE tensor between GUARD floats of NaN; shift: its first element moved by that many floats (misalignment).
    Returns the device buffer (keep it alive) and the device view."""
    n = vals.numel()
    buf = torch.full((GUARD + shift + n + GUARD,), NAN)
    buf[GUARD + shift:GUARD + shift + n] = vals.reshape(-1)
    d = buf.to(DEV)
    return d, d[GUARD + shift:GUARD + shift + n]


def _split(y, npl, dt):
    """The planes a kernel must write for fp32 values y: plane k = round-to-nearest-even 16-bit value of the residual after planes
    0 .. k-1 (the subtractions are exact in fp32)."""
    out, r = [], y.clone()
    for _ in range(npl):
        h = r.to(dt)
        out.append(h)
        r = r - h.float()
    return out


def _check_planes(key, planes, prior, pl_coff, pl_cw, y, C):
    """planes [npl][npx][pl_cs] == the split of y [npx][C] bit for bit; pad channels [C, pl_cw) exactly zero; the rest prior."""
    want = prior.clone()
    for k, h in enumerate(_split(y, planes.shape[0], planes.dtype)):
        want[k][:, pl_coff:pl_coff + C] = h
        want[k][:, pl_coff + C:pl_coff + pl_cw] = 0
    _exact(key, planes, want)


def _plane_prior(npl, npx, pl_cs, dt, seed):
    return _randn((npl, npx, pl_cs), seed).to(dt)


# ------------------------------------------------------------------------------------------------------------------------------
# hpri_nchw_to_nhwc(_pl), hpri_to_planes, hpri_nhwc_to_nchw
# ------------------------------------------------------------------------------------------------------------------------------
LAYOUT_C = [1, 3, 31, 33, 63, 64, 65, 100]


def _layout_case(lib, key, N, C, Pn, cs, coff, Cw, shift=0):
    vals = _randn((N, C, Pn), 100 * C + Pn + N)
    keep, src = _dense(vals, shift)
    prior = _randn((N * Pn, cs), 7)
    d = prior.to(DEV)
    rc = lib.hpri_nchw_to_nhwc(P(src), P(d), N, C, Pn, cs, coff, Cw, _st())
    assert rc == 0, (key, lib.hpri_last_error())
    torch.cuda.synchronize()
    want = prior.clone()
    want[:, coff:coff + C] = vals.permute(0, 2, 1).reshape(N * Pn, C)
    want[:, coff + C:coff + Cw] = 0
    _exact(key, d.cpu(), want)


@pytest.mark.parametrize("Pn", [124, 128, 132, 260])
def test_nchw_to_nhwc_float4_form(lib, Pn):
    """The 64 channel x 128 pixel float4 kernel (P % 4 == 0, aligned bases, cs / coff / Cw multiples of 4) at pixel counts on
    either side of its tile and channel counts on either side of 32 / 64: == permute bit for bit, channels [C, Cw) zero (Cw up
    to 7 channels past C, and past the 64-channel tile for C = 64), coff > 0 and cs > coff + Cw with the prior data kept."""
    for C in LAYOUT_C:
        for N in (1, 3):
            Cw = rup(C, 4) + (4 if C in (3, 64) else 0)
            _layout_case(lib, f"nchw_to_nhwc/v4/P{Pn}", N, C, Pn, 8 + Cw + 4, 8, Cw)


@pytest.mark.parametrize("Pn,shift,odd", [(1, 0, 1), (63, 0, 1), (65, 0, 1), (128, 1, 0), (128, 0, 1), (260, 0, 1)])
def test_nchw_to_nhwc_scalar_form(lib, Pn, shift, odd):
    """The 32 x 64 scalar kernel, taken when P is no multiple of 4, when the source starts one float off a 16-byte boundary
    (shift) or when coff / Cw / cs are no multiples of 4 (odd)."""
    for C in LAYOUT_C:
        for N in (1, 3):
            coff, Cw = (3, C + 2) if odd else (8, rup(C, 4) + 4)
            _layout_case(lib, f"nchw_to_nhwc/scalar/P{Pn}s{shift}o{odd}", N, C, Pn, coff + Cw + (3 if odd else 4), coff, Cw, shift)


def _to_planes_ref_call(lib, y, C, npl, dt):
    """hpri_to_planes on the fp32 rows y [npx][C] (dense plane rows of rup(C, 8) channels): the planes' channels [0, C)."""
    npx, cs, cs16 = y.shape[0], rup(C, 4), rup(C, 8)
    x = torch.zeros(npx, cs)
    x[:, :C] = y
    pl = torch.zeros(npl, npx, cs16, dtype=dt, device=DEV)
    xd = x.to(DEV)
    rc = lib.hpri_to_planes(P(xd), cs, 0, P(pl), npx * cs16, cs16, 0, npx, C, cs16, npl, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    return pl.cpu()[:, :, :C]


@pytest.mark.parametrize("npl", [1, 2, 3])
@pytest.mark.parametrize("with_dst", [1, 0])
def test_nchw_to_nhwc_plane_output(lib16, npl, with_dst):
    """hpri_nchw_to_nhwc_pl: plane k = round16(x - the earlier planes), pl_cw > Cw with the pad channels [C, pl_cw) zero,
    pl_coff > 0, the fp32 destination as before or absent (dst == NULL: planes only); hpri_to_planes gives the same planes."""
    lib, dt = lib16
    for N, C, Pn in [(1, 3, 132), (3, 64, 260), (1, 65, 128), (2, 100, 124)]:
        key = f"nchw_to_nhwc_pl/{dt}/npl{npl}/dst{with_dst}/{N}x{C}x{Pn}"
        npx, Cw, coff = N * Pn, rup(C, 4), 4
        cs = coff + Cw + 4
        pl_coff, pl_cw = 4, rup(C, 4) + 8
        pl_cs = pl_coff + pl_cw + 4
        vals = _randn((N, C, Pn), C + npl) * 1.5
        keep, src = _dense(vals)
        prior = _randn((npx, cs), 8)
        d = prior.to(DEV) if with_dst else None
        pprior = _plane_prior(npl, npx, pl_cs, dt, 9)
        planes = pprior.to(DEV)
        rc = lib.hpri_nchw_to_nhwc_pl(P(src), P(d), N, C, Pn, cs, coff, Cw, P(planes), npx * pl_cs, pl_cs, pl_coff, pl_cw, npl, _st())
        assert rc == 0, (key, lib.hpri_last_error())
        torch.cuda.synchronize()
        y = vals.permute(0, 2, 1).reshape(npx, C).contiguous()
        if with_dst:
            want = prior.clone()
            want[:, coff:coff + C] = y
            want[:, coff + C:coff + Cw] = 0
            _exact(key + "/dst", d.cpu(), want)
        got = planes.cpu()
        _check_planes(key + "/planes", got, pprior, pl_coff, pl_cw, y, C)
        _exact(key + "/to_planes", _to_planes_ref_call(lib, y, C, npl, dt), got[:, :, pl_coff:pl_coff + C].contiguous())


def test_nchw_to_nhwc_plane_output_needs_the_aligned_form(lib16):
    """Planes (or a planes-only call) for a problem the float4 kernel cannot take: HPRI_ERR_UNSUPPORTED, nothing written."""
    lib, dt = lib16
    N, C = 1, 8
    for Pn, shift, coff in [(63, 0, 0), (64, 1, 0), (64, 0, 2)]:
        keep, src = _dense(_randn((N, C, Pn), 1), shift)
        d = torch.zeros(N * Pn, 16, device=DEV)
        planes = torch.zeros(N * Pn, 8, dtype=dt, device=DEV)
        for dst in (d, None):
            rc = lib.hpri_nchw_to_nhwc_pl(P(src), P(dst), N, C, Pn, 16, coff, 8, P(planes), N * Pn * 8, 8, 0, 8, 1, _st())
            assert rc == ERR_UNSUPPORTED, (Pn, shift, coff, rc)
        torch.cuda.synchronize()
        assert torch.all(d == 0) and torch.all(planes == 0)
    # neither output, a view wider than the row, Cw < C: argument errors
    keep, src = _dense(_randn((1, 8, 64), 1))
    d = torch.zeros(64, 16, device=DEV)
    assert lib.hpri_nchw_to_nhwc_pl(P(src), P(None), 1, 8, 64, 16, 0, 8, P(None), 0, 0, 0, 0, 0, _st()) == ERR_ARG
    assert lib.hpri_nchw_to_nhwc(P(src), P(d), 1, 8, 64, 16, 12, 8, _st()) == ERR_ARG
    assert lib.hpri_nchw_to_nhwc(P(src), P(d), 1, 8, 64, 16, 0, 4, _st()) == ERR_ARG


@pytest.mark.parametrize("C", [1, 5, 8, 13, 1650])
@pytest.mark.parametrize("npl", [1, 2, 3])
def test_to_planes_vs_torch(lib16, C, npl):
    """hpri_to_planes in its own right: plane k = round16(x - the earlier planes) of a channel-slice view whose other channels --
    the ones right behind C that a whole-quad read would take included -- are NaN / inf; C on both sides of the quad test
    ``c + h * 4 + 3 < C`` (whole quads, scalar tails, both halves of the 8-channel piece); cw16 > C zero-filled; coff16 > 0."""
    lib, dt = lib16
    npx = 37
    cs, coff = rup(C, 4) + 8, 4
    cw16, coff16 = rup(C, 8) + 8, 8
    cs16 = coff16 + cw16 + 8
    y = _randn((npx, C), C) * 1.5
    x = _view(npx, cs, coff, y).to(DEV)
    pprior = _plane_prior(npl, npx, cs16, dt, 3)
    planes = pprior.to(DEV)
    rc = lib.hpri_to_planes(P(x), cs, coff, P(planes), npx * cs16, cs16, coff16, npx, C, cw16, npl, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    _check_planes(f"to_planes/{dt}/C{C}/npl{npl}", planes.cpu(), pprior, coff16, cw16, y, C)


def test_to_planes_grid_stride_and_errors(lib16):
    """More 8-channel pieces than 8192 blocks of 256 threads cover at once; then the argument errors."""
    lib, dt = lib16
    C, cw16 = 5, 16
    npx = CAP // 2 + 1001                                     # 2 pieces per pixel
    y = _randn((npx, C), 4)
    x = _view(npx, 8, 0, y).to(DEV)
    pprior = _plane_prior(1, npx, cw16 + 8, dt, 5)
    planes = pprior.to(DEV)
    assert npx * (cw16 // 8) > CAP
    rc = lib.hpri_to_planes(P(x), 8, 0, P(planes), npx * (cw16 + 8), cw16 + 8, 8, npx, C, cw16, 1, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    _check_planes(f"to_planes/{dt}/grid_stride", planes.cpu(), pprior, 8, cw16, y, C)
    for bad in [dict(cw16=12), dict(coff16=4), dict(cs16=20), dict(cs=6), dict(coff=2), dict(npl=0), dict(npl=4), dict(cw16=0), dict(P=0)]:
        a = dict(cs=8, coff=0, cs16=24, coff16=8, P=16, cw16=16, npl=1)
        a.update(bad)
        rc = lib.hpri_to_planes(P(x), a["cs"], a["coff"], P(planes), 16 * 24, a["cs16"], a["coff16"], a["P"], C, a["cw16"], a["npl"], _st())
        assert rc == ERR_ARG, bad
    assert lib.hpri_to_planes(P(None), 8, 0, P(planes), 16 * 24, 24, 8, 16, C, 16, 1, _st()) == ERR_ARG
    assert lib.hpri_to_planes(P(x), 8, 0, P(None), 16 * 24, 24, 8, 16, C, 16, 1, _st()) == ERR_ARG


@pytest.mark.parametrize("acc", [0, 1])
def test_nhwc_to_nchw(lib, acc):
    """src [N][P][cs] + coff -> dst [N][C][P] bit for bit, around the 64 pixel x 32 channel tile; accumulate is ONE fp32 add, so
    torch's fp32 dst + src.  The source's other channels are NaN / inf; the floats around the dense destination are kept."""
    for N in (1, 2):
        for C in (1, 2, 31, 32, 33, 70):
            for Pn in (1, 63, 64, 65, 200):
                key = f"nhwc_to_nchw/acc{acc}"
                coff = 3
                cs = coff + C + 2
                vals = _randn((N * Pn, C), C + Pn)
                src = _view(N * Pn, cs, coff, vals).to(DEV)
                prior = _randn((GUARD + N * C * Pn + GUARD,), 11)
                d = prior.to(DEV)
                rc = lib.hpri_nhwc_to_nchw(P(src), P(d[GUARD:]), N, C, Pn, cs, coff, acc, _st())
                assert rc == 0, (key, lib.hpri_last_error())
                torch.cuda.synchronize()
                t = vals.view(N, Pn, C).permute(0, 2, 1).reshape(-1)
                want = prior.clone()
                want[GUARD:GUARD + t.numel()] = (prior[GUARD:GUARD + t.numel()] + t) if acc else t
                _exact(key, d.cpu(), want)
    assert lib.hpri_nhwc_to_nchw(P(src), P(d), 1, 8, 4, 8, 4, 0, _st()) == ERR_ARG          # C + coff > cs


# ------------------------------------------------------------------------------------------------------------------------------
# hpri_maxpool2_fwd / hpri_maxpool2_fwd_pl
# ------------------------------------------------------------------------------------------------------------------------------
def _pool_case(N, H, W, C, x_cs, x_coff, seed, ints=False):
    """x [N*H*W][x_cs] with ties inside the windows; NaN / inf in the other channels AND in the last row / column that the floor
    of an odd size drops.  No NaN inside the pooled region: fmaxf returns the other operand where ATen propagates the NaN -- a
    difference by design that this test keeps out of the way.  Returns (buffer, pooled reference [N*OH*OW][C])."""
    OH, OW = H // 2, W // 2
    if ints:
        v = torch.randint(-8, 9, (N, H, W, C), generator=_gen(seed)).float()        # many ties, cheap to draw
    else:
        v = _randn((N, H, W, C), seed)
        v[:, ::2, ::2] = v[:, ::2, ::2].round()
        v[:, :2 * OH:2, 1:2 * OW:2] = v[:, :2 * OH:2, 0:2 * OW:2]                    # the first two values of each window tie
    ref = F.max_pool2d(v[:, :2 * OH, :2 * OW].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(N * OH * OW, C).contiguous()
    v[:, 2 * OH:] = NAN
    v[:, :, 2 * OW:] = INF
    v = v.reshape(N * H * W, C)
    return (v if (x_cs == C and x_coff == 0) else _view(N * H * W, x_cs, x_coff, v)), ref


POOL_SHAPES = [(1, 2, 2, 4), (2, 9, 11, 8), (3, 7, 8, 12), (1, 3, 2, 4), (2, 4, 5, 16)]


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_forward_vs_torch(lib, shape):
    """hpri_maxpool2_fwd == F.max_pool2d bit for bit; x and y are different channel-slice views."""
    N, H, W, C = shape
    x_cs, x_coff, y_cs, y_coff = C + 8, 4, C + 12, 8
    xb, ref = _pool_case(N, H, W, C, x_cs, x_coff, 21)
    x = xb.to(DEV)
    prior = _randn((ref.shape[0], y_cs), 22)
    y = prior.to(DEV)
    rc = lib.hpri_maxpool2_fwd(P(x), x_cs, x_coff, P(y), y_cs, y_coff, N, H, W, C, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    want = prior.clone()
    want[:, y_coff:y_coff + C] = ref
    _exact(f"maxpool2_fwd/{N}x{H}x{W}x{C}", y.cpu(), want)


@pytest.mark.parametrize("shape", POOL_SHAPES)
@pytest.mark.parametrize("npl", [1, 2, 3])
def test_maxpool_forward_plane_output(lib16, shape, npl):
    """hpri_maxpool2_fwd_pl: the same y, and planes == the 16-bit split of the pooled values with zero pad channels [C, pl_cw)."""
    lib, dt = lib16
    N, H, W, C = shape
    x_cs, x_coff, y_cs, y_coff = C + 4, 0, C + 8, 4
    pl_coff, pl_cw = 4, C + 8
    pl_cs = pl_coff + pl_cw + 4
    xb, ref = _pool_case(N, H, W, C, x_cs, x_coff, 23)
    x = xb.to(DEV)
    npo = ref.shape[0]
    prior = _randn((npo, y_cs), 24)
    y = prior.to(DEV)
    pprior = _plane_prior(npl, npo, pl_cs, dt, 25)
    planes = pprior.to(DEV)
    rc = lib.hpri_maxpool2_fwd_pl(P(x), x_cs, x_coff, P(y), y_cs, y_coff, N, H, W, C, P(planes), npo * pl_cs, pl_cs, pl_coff, pl_cw, npl, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    key = f"maxpool2_fwd_pl/{dt}/npl{npl}/{N}x{H}x{W}x{C}"
    want = prior.clone()
    want[:, y_coff:y_coff + C] = ref
    _exact(key + "/y", y.cpu(), want)
    _check_planes(key + "/planes", planes.cpu(), pprior, pl_coff, pl_cw, ref, C)


def test_maxpool_forward_grid_stride_and_errors(lib):
    """More output quads than one launch covers at once (odd height: the dropped row holds NaN); then the argument errors."""
    N, H, W, C = 1, 2051, 2050, 8
    xb, ref = _pool_case(N, H, W, C, C, 0, 26, ints=True)
    assert ref.shape[0] * (C // 4) > CAP
    x = xb.to(DEV)
    y_cs, y_coff = C + 4, 4
    prior = _randn((ref.shape[0], y_cs), 27)
    y = prior.to(DEV)
    rc = lib.hpri_maxpool2_fwd(P(x), C, 0, P(y), y_cs, y_coff, N, H, W, C, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    want = prior.clone()
    want[:, y_coff:y_coff + C] = ref
    _exact("maxpool2_fwd/grid_stride", y.cpu(), want)
    for a in [dict(H=1), dict(W=1), dict(C=6), dict(x_cs=10), dict(y_coff=2), dict(N=0)]:
        k = dict(N=1, H=4, W=4, C=8, x_cs=8, y_coff=4)
        k.update(a)
        assert lib.hpri_maxpool2_fwd(P(x), k["x_cs"], 0, P(y), y_cs, k["y_coff"], k["N"], k["H"], k["W"], k["C"], _st()) == ERR_ARG, a
    assert lib.hpri_maxpool2_fwd(P(x), 8, 0, P(None), y_cs, 4, 1, 4, 4, 8, _st()) == ERR_ARG


# ------------------------------------------------------------------------------------------------------------------------------
# hpri_copy_slice, hpri_shift_copy, hpri_fill_pad, hpri_mul
# ------------------------------------------------------------------------------------------------------------------------------
def _copy_slice_case(lib, key, Pn, C, s_cs, s_coff, d_cs, d_coff, acc):
    vals = _randn((Pn, C), C + acc)
    s = _view(Pn, s_cs, s_coff, vals).to(DEV)
    prior = _randn((Pn, d_cs), 31)
    d = prior.to(DEV)
    rc = lib.hpri_copy_slice(P(s), s_cs, s_coff, P(d), d_cs, d_coff, Pn, C, acc, _st())
    assert rc == 0, (key, lib.hpri_last_error())
    torch.cuda.synchronize()
    want = prior.clone()
    want[:, d_coff:d_coff + C] = (prior[:, d_coff:d_coff + C] + vals) if acc else vals          # accumulate: one fp32 add
    _exact(key, d.cpu(), want)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("C", [4, 64, 132])
def test_copy_slice(lib, C, acc):
    """The skip-concat copy between two different channel-slice views, written or added (one fp32 add) bit for bit."""
    _copy_slice_case(lib, f"copy_slice/C{C}/acc{acc}", 77, C, C + 12, 8, C + 20, 4, acc)


@pytest.mark.parametrize("acc", [0, 1])
def test_copy_slice_grid_stride_and_errors(lib, acc):
    _copy_slice_case(lib, f"copy_slice/grid_stride/acc{acc}", CAP + 1003, 4, 8, 4, 8, 0, acc)
    t = torch.zeros(64, device=DEV)
    for a in [dict(C=6), dict(s_cs=6), dict(s_coff=2), dict(d_cs=10), dict(d_coff=1), dict(Pn=0), dict(C=0)]:
        k = dict(Pn=2, C=4, s_cs=8, s_coff=0, d_cs=8, d_coff=0)
        k.update(a)
        assert lib.hpri_copy_slice(P(t), k["s_cs"], k["s_coff"], P(t), k["d_cs"], k["d_coff"], k["Pn"], k["C"], 0, _st()) == ERR_ARG, a


def _shift_copy_case(lib, key, N, Hs, Ws, Hd, Wd, oy, ox, C, acc, slices=True):
    """d[n][y][x] = s[n][y - oy][x - ox] inside the source, 0 elsewhere == F.pad with signed widths (left ox, right Wd - Ws - ox,
    top oy, bottom Hd - Hs - oy: negative widths crop).  The source pixels the shift crops away hold NaN."""
    s_cs, s_coff, d_cs, d_coff = (C + 8, 4, C + 12, 8) if slices else (C, 0, C, 0)
    v = _randn((N, Hs, Ws, C), Hs + 3 * Ws + acc)
    ys, xs = torch.arange(Hs), torch.arange(Ws)
    used = ((ys + oy >= 0) & (ys + oy < Hd)).view(Hs, 1) & ((xs + ox >= 0) & (xs + ox < Wd)).view(1, Ws)
    if bool(used.any()):
        ref = F.pad(v.permute(0, 3, 1, 2), (ox, Wd - Ws - ox, oy, Hd - Hs - oy)).permute(0, 2, 3, 1)
    else:
        ref = torch.zeros(N, Hd, Wd, C)                        # shifted out of the destination altogether (F.pad cannot crop more than it has)
    assert ref.shape == (N, Hd, Wd, C)
    baited = torch.where(used.view(1, Hs, Ws, 1), v, torch.full_like(v, NAN)).reshape(N * Hs * Ws, C)
    s = (_view(N * Hs * Ws, s_cs, s_coff, baited) if slices else baited).to(DEV)
    prior = _randn((N * Hd * Wd, d_cs), 33)
    d = prior.to(DEV)
    rc = lib.hpri_shift_copy(P(s), s_cs, s_coff, Hs, Ws, P(d), d_cs, d_coff, N, Hd, Wd, oy, ox, C, acc, _st())
    assert rc == 0, (key, lib.hpri_last_error())
    torch.cuda.synchronize()
    r = ref.reshape(N * Hd * Wd, C)
    want = prior.clone()
    want[:, d_coff:d_coff + C] = (prior[:, d_coff:d_coff + C] + r) if acc else r
    _exact(key, d.cpu(), want)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("sizes", [(5, 7, 8, 6), (9, 4, 6, 8), (6, 6, 6, 6)])
def test_shift_copy_vs_pad(lib, sizes, acc):
    """Source smaller / larger than the destination in either direction, every sign of the offsets, two images, slice views."""
    Hs, Ws, Hd, Wd = sizes
    for oy, ox in [(0, 0), (1, 2), (-1, -2), (2, -1), (Hd + 1, 0), (0, -Ws)]:
        _shift_copy_case(lib, f"shift_copy/{Hs}x{Ws}->{Hd}x{Wd}/acc{acc}", 2, Hs, Ws, Hd, Wd, oy, ox, 8, acc)


def test_shift_copy_grid_stride_and_errors(lib):
    _shift_copy_case(lib, "shift_copy/grid_stride", 1, 1449, 1452, 1450, 1451, 1, -1, 4, 0, slices=False)
    assert 1450 * 1451 > CAP
    t = torch.zeros(256, device=DEV)
    for a in [dict(C=6), dict(s_cs=6), dict(d_coff=2), dict(Hs=0), dict(Wd=0), dict(N=0)]:
        k = dict(N=1, Hs=2, Ws=2, Hd=2, Wd=2, C=4, s_cs=4, d_coff=0)
        k.update(a)
        rc = lib.hpri_shift_copy(P(t), k["s_cs"], 0, k["Hs"], k["Ws"], P(t), 8, k["d_coff"], k["N"], k["Hd"], k["Wd"], 0, 0, k["C"], 0, _st())
        assert rc == ERR_ARG, a


def _fill_pad_want(prior, N, H, W, coff, C, rect):
    y0, y1, x0, x1 = rect
    want = prior.clone().view(N, H, W, -1)
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = True
    sl = want[:, :, :, coff:coff + C]
    sl[:] = torch.where(inside.view(1, H, W, 1), sl, torch.zeros_like(sl))
    return want.view(N * H * W, -1)


FILL_RECTS = [(2, 5, 1, 4), (0, 0, 0, 0), (0, 6, 0, 7), (1, 6, 0, 3)]


@pytest.mark.parametrize("rect", FILL_RECTS)
def test_fill_pad(lib, rect):
    """Channels [coff, coff + C) of every pixel outside [y0, y1) x [x0, x1) become +0, nothing else changes: an interior
    rectangle, the empty one (everything zeroed), the full image (nothing written), one that touches two borders."""
    N, H, W, C, cs, coff = 2, 6, 7, 8, 20, 4
    prior = _randn((N * H * W, cs), 41)
    d = prior.to(DEV)
    rc = lib.hpri_fill_pad(P(d), cs, coff, N, H, W, C, *rect, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    _exact(f"fill_pad/{rect}", d.cpu(), _fill_pad_want(prior, N, H, W, coff, C, rect))


@pytest.mark.parametrize("rect", FILL_RECTS)
def test_fill_pad_on_16bit_rows_with_halved_arguments(lib, rect):
    """The pad ring of the upsampled half inside a concat's bf16 planes (engine.py, _upsample_into): the 16-bit buffer passed as
    float* with cs / coff / C halved, pairs of 16-bit zeros written as floats.  The contract needs cs, coff and C of the 16-bit
    buffer to be multiples of 8 (the float4 stores cover 8 of its channels): here 32, 8 and 16."""
    N, H, W = 2, 6, 7
    cs16, coff16, C16 = 32, 8, 16
    prior = _randn((N * H * W, cs16), 42).to(torch.bfloat16)
    d = prior.to(DEV)
    rc = lib.hpri_fill_pad(P(d), cs16 // 2, coff16 // 2, N, H, W, C16 // 2, *rect, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    _exact(f"fill_pad/x16/{rect}", d.cpu(), _fill_pad_want(prior, N, H, W, coff16, C16, rect))
    # what the engine must never pass: a 16-bit offset or count that is a multiple of 4 but not of 8 is an error return
    assert lib.hpri_fill_pad(P(d), cs16 // 2, 12 // 2, N, H, W, C16 // 2, *rect, _st()) == ERR_ARG
    assert lib.hpri_fill_pad(P(d), cs16 // 2, coff16 // 2, N, H, W, 12 // 2, *rect, _st()) == ERR_ARG
    assert lib.hpri_fill_pad(P(d), 36 // 2, coff16 // 2, N, H, W, C16 // 2, *rect, _st()) == ERR_ARG


def test_fill_pad_grid_stride(lib):
    N, H, W, C, cs = 1, 1450, 1451, 4, 4
    assert H * W > CAP
    prior = _randn((N * H * W, cs), 43)
    d = prior.to(DEV)
    rect = (3, 1447, 2, 1450)
    rc = lib.hpri_fill_pad(P(d), cs, 0, N, H, W, C, *rect, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    _exact("fill_pad/grid_stride", d.cpu(), _fill_pad_want(prior, N, H, W, 0, C, rect))


def _mul_case(lib, key, Pn, C, views, acc):
    (a_cs, a_coff), (b_cs, b_coff), (o_cs, o_coff) = views
    av, bv = _randn((Pn, C), 51), _randn((Pn, C), 52)
    a, b = _view(Pn, a_cs, a_coff, av).to(DEV), _view(Pn, b_cs, b_coff, bv).to(DEV)
    prior = _randn((Pn, o_cs), 53)
    o = prior.to(DEV)
    rc = lib.hpri_mul(P(a), a_cs, a_coff, P(b), b_cs, b_coff, P(o), o_cs, o_coff, Pn, C, acc, _st())
    assert rc == 0, (key, lib.hpri_last_error())
    torch.cuda.synchronize()
    got = o.cpu()
    if not acc:
        want = prior.clone()
        want[:, o_coff:o_coff + C] = av * bv                    # one rounding: torch's fp32 product bit for bit
        _exact(key, got, want)
        return
    # a * b + z: the compiler may round the product and then the sum (errors <= U |ab| and U |ab + z| to first order) or fuse them
    # (one rounding, <= U |ab + z|); the gate U |ab| + U |ab + z| admits both and nothing more
    ab = av.double() * bv.double()
    ref = ab + prior[:, o_coff:o_coff + C].double()
    _gate(key, (got[:, o_coff:o_coff + C].double() - ref).abs(), U * ab.abs() + U * ref.abs())
    rest = got.clone()
    rest[:, o_coff:o_coff + C] = prior[:, o_coff:o_coff + C]
    _exact(key + "/outside", rest, prior)


@pytest.mark.parametrize("acc", [0, 1])
def test_mul(lib, acc):
    """The attention product a * b over three different channel-slice views, written (bit-exact) or accumulated."""
    for C in (4, 36):
        _mul_case(lib, f"mul/acc{acc}", 91, C, ((C + 8, 4), (C + 4, 0), (C + 16, 12)), acc)
    t = torch.zeros(64, device=DEV)
    for a in [dict(C=6), dict(a_cs=6), dict(b_coff=2), dict(o_cs=10), dict(Pn=0)]:
        k = dict(Pn=2, C=4, a_cs=8, b_coff=0, o_cs=8)
        k.update(a)
        assert lib.hpri_mul(P(t), k["a_cs"], 0, P(t), 8, k["b_coff"], P(t), k["o_cs"], 0, k["Pn"], k["C"], acc, _st()) == ERR_ARG, a


@pytest.mark.parametrize("acc", [0, 1])
def test_mul_grid_stride(lib, acc):
    _mul_case(lib, f"mul/grid_stride/acc{acc}", CAP + 517, 4, ((4, 0), (8, 4), (8, 0)), acc)


# ------------------------------------------------------------------------------------------------------------------------------
# hpri_upsample2x_fwd / hpri_upsample2x_bwd
# ------------------------------------------------------------------------------------------------------------------------------
class _Interp:
    """The (2n x n) matrix A of nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True) along one axis, by ATen's rule
    evaluated in float32 as the kernel evaluates it: scale = (in - 1) / (out - 1), src = scale * o, i0 = int(src),
    l1 = src - i0, l0 = 1 - l1, i1 = i0 + (i0 < in - 1).  Row o holds l0 at column i0 and l1 at column i1 (both at i0 when they
    coincide); the weights are fp32 values, everything done WITH them below is fp64.  The matrix is kept as its two taps per
    row, so A X and A^T G cost two gathers / scatters whatever the size; dense() is the same matrix written out."""

    def __init__(self, n):
        f = np.float32
        out = 2 * n
        o = np.arange(out, dtype=f)
        scale = f(n - 1) / f(out - 1)
        src = scale * o
        assert src.dtype == f
        i0 = src.astype(np.int32)
        l1 = src - i0.astype(f)
        l0 = f(1.0) - l1
        i1 = i0 + (i0 < n - 1)
        assert i0.min() >= 0 and i1.max() <= n - 1
        self.n, self.out = n, out
        self.i0, self.i1 = torch.from_numpy(i0.astype(np.int64)), torch.from_numpy(i1.astype(np.int64))
        self.l0, self.l1 = torch.from_numpy(l0.astype(np.float64)), torch.from_numpy(l1.astype(np.float64))
        # the taps of the same rule in exact arithmetic (what an fp64 evaluation sees): src = o (in - 1) / (out - 1)
        j0 = (np.arange(out, dtype=np.int64) * (n - 1)) // (out - 1)
        self.j0, self.j1 = torch.from_numpy(j0), torch.from_numpy(np.minimum(j0 + 1, n - 1))

    def _w(self, w, x, dim):
        shape = [1] * x.dim()
        shape[dim] = -1
        return w.view(shape)

    def apply(self, x, dim):
        """A x along ``dim`` (fp64)."""
        return self._w(self.l0, x, dim) * x.index_select(dim, self.i0) + self._w(self.l1, x, dim) * x.index_select(dim, self.i1)

    def adjoint(self, g, dim):
        """A^T g along ``dim`` (fp64)."""
        shape = list(g.shape)
        shape[dim] = self.n
        out = torch.zeros(shape, dtype=torch.float64)
        out.index_add_(dim, self.i0, self._w(self.l0, g, dim) * g)
        out.index_add_(dim, self.i1, self._w(self.l1, g, dim) * g)
        return out

    def dense(self):
        a = torch.zeros(self.out, self.n, dtype=torch.float64)
        r = torch.arange(self.out)
        a.index_put_((r, self.i0), self.l0, accumulate=True)
        a.index_put_((r, self.i1), self.l1, accumulate=True)
        return a

    def column_counts(self):
        """Non-zero entries per column: the outputs that take a term from each input."""
        cnt = torch.zeros(self.n, dtype=torch.int64)
        second = (self.l1 != 0) & ((self.i1 != self.i0) | (self.l0 == 0))
        cnt.index_add_(0, self.i0[self.l0 != 0], torch.ones(int((self.l0 != 0).sum()), dtype=torch.int64))
        cnt.index_add_(0, self.i1[second], torch.ones(int(second.sum()), dtype=torch.int64))
        return cnt

    def tap_max(self, x, dim):
        """max |x| over the taps of either evaluation of the rule (float32 and exact), along ``dim``."""
        m = None
        for idx in (self.i0, self.i1, self.j0, self.j1):
            v = x.index_select(dim, idx)
            m = v if m is None else torch.maximum(m, v)
        return m


def _up_refs(x, with_b=True):
    """x [N][H][W][C] fp32 -> (reference (a) = Ay X Ax^T in fp64, sum |w| |v| = Ay |X| Ax^T, reference (b) = torch's own bilinear
    interpolation in fp64, max |v| over the taps of both).  The weights are >= 0, so |A| = A."""
    N, H, W, C = x.shape
    ay, ax = _Interp(H), _Interp(W)
    xd = x.double()
    ref_a = ax.apply(ay.apply(xd, 1), 2)
    mag = ax.apply(ay.apply(xd.abs(), 1), 2)
    if not with_b:
        return ref_a, mag, None, None
    ref_b = F.interpolate(xd.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    vmax = ax.tap_max(ay.tap_max(xd.abs(), 1), 2)
    return ref_a, mag, ref_b, vmax


def _tol_b(H, W, vmax):
    """Gate (b), against an fp64 evaluation of the interpolation: the kernel's src = fl(fl(scale) * o) carries two roundings,
    |src32 - src| <= 2 U src <= 2 U in, and so does l1 wherever the index is the same; where the fp32 src lands on the other
    side of an integer the interpolant is continuous, so the same bound holds for the value.  The result moves by
    |row1 - row0| <= 2 max|v| per unit of ly1 and as much per unit of lx1: 2 max|v| (2 U H + 2 U W) = 4 (H + W) U max|v|; the
    arithmetic on top of that is gate (a)'s 8 U sum |w| |v| <= 8 U max|v|."""
    return (8 + 4 * (H + W)) * U * vmax


UP_SHAPES = [(1, 1), (1, 5), (4, 1), (2, 2), (3, 5), (7, 6), (38, 3), (3, 60), (76, 5), (5, 121), (152, 3), (3, 242), (304, 2), (2, 484)]
UP_PAD = (1, 2, 2, 1)            # py0, px0, rows below the window, columns right of it


def _up_geometry(H, W):
    py0, px0, eb, er = UP_PAD
    return py0, px0, 2 * H + py0 + eb, 2 * W + px0 + er


def _up_fwd(lib, xv, x_cs, x_coff, y_cs, y_coff, seed, pad=True):
    """One forward launch on x values xv [N][H][W][C]; returns (y region [N][2H][2W][C], the whole y buffer, its prior)."""
    N, H, W, C = xv.shape
    py0, px0, H2, W2 = _up_geometry(H, W) if pad else (0, 0, 2 * H, 2 * W)
    flat = xv.reshape(N * H * W, C)
    x = (flat if (x_cs == C and x_coff == 0) else _view(N * H * W, x_cs, x_coff, flat)).to(DEV)
    prior = _randn((N * H2 * W2, y_cs), seed)
    y = prior.to(DEV)
    rc = lib.hpri_upsample2x_fwd(P(x), x_cs, x_coff, P(y), y_cs, y_coff, N, H, W, H2, W2, py0, px0, C, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    got = y.cpu()
    win = got.view(N, H2, W2, y_cs)[:, py0:py0 + 2 * H, px0:px0 + 2 * W, y_coff:y_coff + C]
    rest = got.clone()
    rest.view(N, H2, W2, y_cs)[:, py0:py0 + 2 * H, px0:px0 + 2 * W, y_coff:y_coff + C] = \
        prior.view(N, H2, W2, y_cs)[:, py0:py0 + 2 * H, px0:px0 + 2 * W, y_coff:y_coff + C]
    return win.contiguous(), rest, prior


def _up_fwd_case(lib, key, N, H, W, C):
    xv = _randn((N, H, W, C), 61 + H + 7 * W)
    ref_a, mag, ref_b, vmax = _up_refs(xv)
    # the two references agree within gate (b) (no GPU involved: the fp32-rule matrices against torch's fp64 interpolation)
    _gate(key + "/ref_a_vs_ref_b", (ref_a - ref_b).abs(), _tol_b(H, W, vmax))
    got, rest, prior = _up_fwd(lib, xv, C + 8, 4, C + 12, 8, 62)
    _exact(key + "/outside", rest, prior)
    # gate (a): with the same fp32 weights the kernel rounds each term four times on its way into the result (inner product,
    # inner sum, outer product, outer sum; fewer where the compiler fuses): 4 U sum |w| |v| to first order, 8 U with the
    # second-order terms and the freedom of contraction covered
    _gate(key + "/a", (got.double() - ref_a).abs(), 8 * U * mag)
    _gate(key + "/b", (got.double() - ref_b).abs(), _tol_b(H, W, vmax))


@pytest.mark.parametrize("shape", UP_SHAPES)
def test_upsample_forward_vs_fp64(lib, shape):
    """hpri_upsample2x_fwd into a window at (py0, px0) of a larger destination image, slice views, two images: against the
    fp32-rule matrices in fp64 (tight) and against torch's fp64 interpolation (independent); H or W of 1, the smallest, odd
    sizes and the deep-level sizes of the workload as thin strips."""
    H, W = shape
    _up_fwd_case(lib, f"upsample2x_fwd/{H}x{W}", 2, H, W, 8)


def test_upsample_forward_every_height_to_48(lib):
    """Every H in 1..48 (W = 2, C = 4), so that every size whose fp32 src lands just under an integer is hit."""
    for H in range(1, 49):
        _up_fwd_case(lib, "upsample2x_fwd/sweepH", 1, H, 2, 4)


def test_upsample_forward_grid_stride_and_errors(lib):
    N, H, W, C = 1, 726, 727, 4
    assert N * 4 * H * W * (C // 4) > CAP
    xv = _randn((N, H, W, C), 63)
    ref_a, mag, _, _ = _up_refs(xv, with_b=False)
    got, rest, prior = _up_fwd(lib, xv, C, 0, C, 0, 64)
    _exact("upsample2x_fwd/grid_stride/outside", rest, prior)
    _gate("upsample2x_fwd/grid_stride/a", (got.double() - ref_a).abs(), 8 * U * mag)
    # a window that exceeds the destination image, a negative offset, misaligned channels: error returns
    t = torch.zeros(4096, device=DEV)
    for a in [dict(H2=7), dict(W2=7), dict(py0=1), dict(px0=1), dict(py0=-1, H2=9), dict(px0=-1), dict(C=6), dict(x_cs=6), dict(y_coff=2), dict(H=0)]:
        k = dict(H=4, W=4, H2=8, W2=8, py0=0, px0=0, C=4, x_cs=4, y_coff=0)
        k.update(a)
        rc = lib.hpri_upsample2x_fwd(P(t), k["x_cs"], 0, P(t), 4, k["y_coff"], 1, k["H"], k["W"], k["H2"], k["W2"], k["py0"], k["px0"], k["C"], _st())
        assert rc == ERR_ARG, a
        rc = lib.hpri_upsample2x_bwd(P(t), k["x_cs"], 0, P(t), 4, k["y_coff"], 1, k["H"], k["W"], k["H2"], k["W2"], k["py0"], k["px0"], k["C"], 0, _st())
        assert rc == ERR_ARG, a


def _up_bwd(lib, gv, H, W, dy_cs, dy_coff, dx_cs, dx_coff, acc, seed, pad=True):
    """One backward launch: gv [N][2H][2W][C] sits in the (py0, px0) window of a larger dy image whose other pixels -- and other
    channels -- are NaN / inf.  Returns (dx values [N][H][W][C], the dx buffer with them put back to the prior, the prior)."""
    N, C = gv.shape[0], gv.shape[3]
    py0, px0, H2, W2 = _up_geometry(H, W) if pad else (0, 0, 2 * H, 2 * W)
    if pad:
        img = torch.tensor([NAN, INF, -INF])[torch.arange(N * H2 * W2 * C) % 3].view(N, H2, W2, C).clone()
        img[:, py0:py0 + 2 * H, px0:px0 + 2 * W] = gv
    else:
        img = gv
    flat = img.reshape(N * H2 * W2, C)
    dy = (flat if (dy_cs == C and dy_coff == 0) else _view(N * H2 * W2, dy_cs, dy_coff, flat)).to(DEV)
    prior = _randn((N * H * W, dx_cs), seed)
    dx = prior.to(DEV)
    rc = lib.hpri_upsample2x_bwd(P(dy), dy_cs, dy_coff, P(dx), dx_cs, dx_coff, N, H, W, H2, W2, py0, px0, C, acc, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    got = dx.cpu()
    vals = got[:, dx_coff:dx_coff + C].reshape(N, H, W, C).contiguous()
    rest = got.clone()
    rest[:, dx_coff:dx_coff + C] = prior[:, dx_coff:dx_coff + C]
    return vals, rest, prior


def _up_bwd_gate(key, got, gv, H, W, old):
    """dx against the fp64 adjoint Ay^T G Ax of reference (a).  Per input pixel the kernel sums, in one fp32 chain, the products
    w * g of the T = ny * nx outputs whose footprint holds it (ny, nx = the non-zero entries of the pixel's columns of Ay and
    Ax: src moves by scale < 1/2 per output and the footprint is the open interval (i - 1, i + 1), so at most 5 per axis,
    T <= 25): T - 1 roundings of the chain, and per term the rounding of wy * wx, of w * g, and one more per axis where both
    taps of an output fall on the same input pixel (ly0 + ly1 at the last row) -- (T + 3) U sum |w| |g| to first order, gated
    at (T + 4) U with the second-order terms: 8 U for a 1 x 1 image, 20 U where four outputs per axis meet (the most any size
    here has), never more than 29 U.  accumulate adds one rounding of the final sum: U |old + dx|."""
    ay, ax = _Interp(H), _Interp(W)
    gd = gv.double()
    ref = ax.adjoint(ay.adjoint(gd, 1), 2)
    mag = ax.adjoint(ay.adjoint(gd.abs(), 1), 2)
    terms = (ay.column_counts().view(1, H, 1, 1) * ax.column_counts().view(1, 1, W, 1)).double()
    assert int(terms.max()) <= 25
    tol = (terms + 4) * U * mag
    if old is not None:
        ref = ref + old.double()
        tol = tol + U * ref.abs()
    _gate(key, (got.double() - ref).abs(), tol)
    return (terms + 4) * U * mag                             # the bound of the kernel's own sum, without the accumulate term


def _up_bwd_case(lib, key, N, H, W, C, acc):
    gv = _randn((N, 2 * H, 2 * W, C), 71 + H + 5 * W)
    dx_cs, dx_coff = C + 12, 8
    got, rest, prior = _up_bwd(lib, gv, H, W, C + 8, 4, dx_cs, dx_coff, acc, 72)
    _exact(key + "/outside", rest, prior)
    old = prior[:, dx_coff:dx_coff + C].reshape(N, H, W, C) if acc else None
    tol_b = _up_bwd_gate(key + "/adjoint", got, gv, H, W, old)
    if acc:
        return
    # <up(x), g> == <x, up^T(g)> with both sides from the kernels, summed in fp64, and each side against the fp64 inner product
    # <Ay X Ax^T, g> of reference (a) (which equals <x, Ay^T G Ax> to fp64 roundoff, nine orders below these bounds).  Each side
    # may be off by its kernel's elementwise bound summed against the other factor: the forward's 8 U sum |w| |v| against |g|,
    # the backward's (T + 4) U sum |w| |g| (at most 20 U here, under the 32 U of the elementwise gate's ceiling) against |x|;
    # the two sides differ by at most the sum of the two.  These are worst-case bounds of sums of some 10^2 .. 10^4 rounding
    # errors of either sign, which cancel: the ratios they record are small by nature, and the elementwise gates stay the sharp
    # ones.  What this adds is a check that needs no reference: a backward that is not the forward's transpose fails it.
    xv = _randn((N, H, W, C), 73)
    up, _, _ = _up_fwd(lib, xv, C, 0, C, 0, 74)
    ref_up, mag_f, _, _ = _up_refs(xv, with_b=False)
    gd, xd = gv.double(), xv.double()
    ip = float((ref_up * gd).sum())
    lhs, rhs = float((up.double() * gd).sum()), float((xd * got.double()).sum())
    bound_f = float((8 * U * mag_f * gd.abs()).sum())
    bound_b = float((tol_b * xd.abs()).sum())
    for name, err, bound in (("forward_side", abs(lhs - ip), bound_f), ("backward_side", abs(rhs - ip), bound_b),
                             ("identity", abs(lhs - rhs), bound_f + bound_b)):
        record_margin(f"{key}/{name}", err / bound, 1.0)
        assert err <= bound, (key, name, lhs, rhs, ip, bound)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("shape", UP_SHAPES)
def test_upsample_backward_vs_fp64_adjoint(lib, shape, acc):
    """hpri_upsample2x_bwd reading the (py0, px0) window of a larger gradient image (NaN / inf everywhere else), written or
    accumulated into a slice view: the adjoint of the forward's matrices, and the inner-product identity with the forward."""
    H, W = shape
    _up_bwd_case(lib, f"upsample2x_bwd/{H}x{W}/acc{acc}", 2, H, W, 8, acc)


@pytest.mark.parametrize("acc", [0, 1])
def test_upsample_backward_every_height_to_48(lib, acc):
    for H in range(1, 49):
        _up_bwd_case(lib, f"upsample2x_bwd/sweepH/acc{acc}", 1, H, 2, 4, acc)


def test_upsample_backward_grid_stride(lib):
    N, H, W, C = 1, 1450, 1451, 4
    assert N * H * W * (C // 4) > CAP
    gv = _randn((N, 2 * H, 2 * W, C), 75)
    got, rest, prior = _up_bwd(lib, gv, H, W, C, 0, C, 0, 0, 76, pad=False)
    _exact("upsample2x_bwd/grid_stride/outside", rest, prior)
    _up_bwd_gate("upsample2x_bwd/grid_stride/adjoint", got, gv, H, W, None)


def test_interpolation_matrix_helper():
    """The reference helper against itself: the tap form equals the dense matrix, rows sum to 1 within one rounding of l0, the
    adjoint is the transpose."""
    for n in (1, 2, 3, 7, 38):
        a = _Interp(n)
        d = a.dense()
        assert d.shape == (2 * n, n) and float((d.sum(1) - 1).abs().max()) <= U
        x = torch.randn(n, 3, generator=_gen(n)).double()
        g = torch.randn(2 * n, 3, generator=_gen(n + 1)).double()
        assert float((a.apply(x, 0) - d @ x).abs().max()) <= 1e-14
        assert float((a.adjoint(g, 0) - d.t() @ g).abs().max()) <= 1e-14
        assert torch.equal(a.column_counts(), (d != 0).sum(0))
    d = _Interp(2).dense()                                   # scale = fl(1 / 3); src = 0, fl(1/3), 2 fl(1/3), fl(3 fl(1/3)) = 1
    third = float(np.float32(1) / np.float32(3))
    assert d[0].tolist() == [1.0, 0.0] and d[3].tolist() == [0.0, 1.0] and float(d[1, 1]) == third and float(d[2, 1]) == 2 * third


# ------------------------------------------------------------------------------------------------------------------------------
# hpri_synth_fill
# ------------------------------------------------------------------------------------------------------------------------------
SEEDS = [0, 1234, 2 ** 63 + 5, 2 ** 64 - 1]


def _synth_case(lib, key, n, seed, mode, thr, scale):
    from hyperpri_amd import synth
    prior = _randn((GUARD + n + GUARD,), 81)
    d = prior.to(DEV)
    rc = lib.hpri_synth_fill(P(d[GUARD:]), n, seed, mode, float(np.float32(thr)), float(np.float32(scale)), _st())
    assert rc == 0, (key, lib.hpri_last_error())
    torch.cuda.synchronize()
    u = synth.uniform(seed, n)
    assert u.dtype == np.float32
    if mode == 0:
        v = u
    elif mode == 1:
        v = (u > np.float32(thr)).astype(np.float32)
    else:
        v = (np.float32(2.0) * u - np.float32(1.0)) * np.float32(scale)        # 2u - 1 is exact in fp32 (u = k / 2^24): one rounding
        assert v.dtype == np.float32
    want = prior.clone()
    want[GUARD:GUARD + n] = torch.from_numpy(v)
    _exact(key, d.cpu(), want)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_synth_fill_equals_the_numpy_twin(lib, mode):
    """hpri_synth_fill == hyperpri_amd.synth.uniform bit for bit (bench.py fills on the device what the golden generators fill
    with numpy): mode 0 = u, mode 1 = (u > thr), mode 2 = (2u - 1) * scale; seeds up to 2^64 - 1 (the product with the golden
    ratio wraps); sizes around the block and one past the grid cap; the floats around the tensor kept."""
    scale = 1.0 / np.sqrt(27.0)
    for seed in SEEDS:
        for n in (1, 255, 257, 4097):
            _synth_case(lib, f"synth_fill/mode{mode}", n, seed, mode, 0.9, scale)
    _synth_case(lib, f"synth_fill/mode{mode}/grid_stride", CAP + 257, SEEDS[2], mode, 0.9, scale)
    t = torch.zeros(8, device=DEV)
    assert lib.hpri_synth_fill(P(t), 0, 1, mode, 0.5, 1.0, _st()) == ERR_ARG
    assert lib.hpri_synth_fill(P(None), 8, 1, mode, 0.5, 1.0, _st()) == ERR_ARG
    assert lib.hpri_synth_fill(P(t), 8, 1, 3, 0.5, 1.0, _st()) == ERR_ARG
    assert lib.hpri_synth_fill(P(t), 8, 1, -1, 0.5, 1.0, _st()) == ERR_ARG
