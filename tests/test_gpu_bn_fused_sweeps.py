"""The sweeps fused with the last BatchNorm stage and with the BatchNorm backward (elementwise.hip: hpri_bn_relu_outconv_fwd,
hpri_bn_relu_outconv_bwd, hpri_bn_relu_bwd_pool, hpri_bn_apply_relu_pool) called through the C ABI, against the kernels they replace and against plain fp64 torch, and the engine routes (engine.FUSE_HEAD_BN,
engine.FUSE_POOL_BN, engine.FUSE_POOL_FWD) on the tiny nets that have a reference fixture.  Needs a real MI355X: ``-m gpu``.

Head forward: logits and the fp64 loss partials from the pre-BN tensor, BIT FOR BIT those of hpri_bn_apply_relu_pl +
hpri_outconv_fwd / hpri_outconv_fwd_bce.

Head backward (x -> BN -> ReLU -> y -> 1x1 head, one class): the fused entry shares the block plan, the per-thread summation order and
both finalize kernels with hpri_outconv_bwd(_bce) + hpri_bn_relu_bwd, so dx, dgamma, dbeta, dbias, dw and db are compared BIT FOR
BIT with that four-kernel route fed the y of hpri_bn_apply_relu (margin: none needed, none taken).

Pooling (y feeds MaxPool2d(2) and a skip): the gradient g = route(dpool) + dskip that hpri_maxpool2_bwd leaves in memory is an
exact elementwise function of the inputs, so the fused kernels form the same g; the per-channel sums run in another order (by
window, not by pixel), so the gates are those of test_gpu_bn_kernels.py, stated in U = 2^-24: each sum within (L + 8) U of the sum
of the absolute values of its terms, L = the longest fp32 chain of one channel (4 pixels per window x windows per thread + the
rows of the workgroup reduction), dx within four roundings of each term plus the propagated error of the two means.  On top, the
per-element gradient is recovered from dx by inverting dx = scale * (g - k1 - xhat * k2) with the kernel's own sums and must
equal hpri_maxpool2_bwd + add within the roundings of that inversion: a misrouted window is off by a whole gradient value.
Largest ratio error / bound seen on MI355X: dbeta 0.056, dgamma 0.053, dx 0.34, recovered gradient 0.32; sums against the replaced
route 0.044; engine routes: error with the routes on / (2 x error with them off + floor) at most 0.55 (the two errors are equal).

Pooling forward: y and the pooled map of the one-pass kernel BIT FOR BIT those of hpri_bn_apply_relu_pl + hpri_maxpool2_fwd
(hpri_maxpool2_fwd itself is pinned against F.max_pool2d in test_gpu_glue_kernels.py, hpri_bn_apply_relu_pl in
test_gpu_bn_kernels.py)."""
import ctypes
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
EPS = 1e-5
NAN, INF = float("nan"), float("inf")
G = os.path.join(os.path.dirname(__file__), "golden")


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


def _gate(key, err, tol):
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    m = float(r.max()) if r.numel() else 0.0
    record_margin(key, m, 1.0)
    assert m <= 1.0, (key, m)


def _view(npx, C, Cw, cs, coff, seed, offset=0.3, pad_nan=True):
    """[npx][cs] buffer whose channels [coff, coff + C) are random, pad channels [coff + C, coff + Cw) NaN / +-inf, the rest NaN."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.full((npx, cs), NAN, device=DEV)
    buf[:, coff:coff + C] = torch.randn(npx, C, device=DEV, generator=g) * 1.5 + offset
    if Cw > C:
        pat = torch.tensor([NAN, INF, -INF] if pad_nan else [0.0, 0.0, 0.0], device=DEV)
        buf[:, coff + C:coff + Cw] = pat[torch.arange(npx * (Cw - C), device=DEV) % 3].view(npx, Cw - C)
    return buf


def _stats(xv, C, seed, positive_gamma=False):
    """fp32 mean / invstd / scale / shift of xv [npx][C] (one group), as hpri_bn_finalize would leave them."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = xv.double()
    mean = x.mean(0).float()
    invstd = (1.0 / torch.sqrt(x.var(0, unbiased=False) + EPS)).float()
    gamma = torch.randn(C, device=DEV, generator=g) + 0.2
    if positive_gamma:
        gamma = gamma.abs() + 0.5
    beta = torch.randn(C, device=DEV, generator=g) * 0.5
    scale = gamma * invstd
    shift = beta - mean * scale
    return {"mean": mean.contiguous(), "invstd": invstd.contiguous(), "scale": scale.contiguous(), "shift": shift.contiguous()}


def _apply(lib, xb, xcs, xoff, st, npx, C, Cw, relu):
    """y [npx][Cw] of hpri_bn_apply_relu_pl: the activation the replaced kernels read."""
    y = torch.full((npx, Cw), 7.0, device=DEV)
    rc = lib.hpri_bn_apply_relu_pl(P(xb), xcs, xoff, P(y), Cw, 0, P(st["scale"]), P(st["shift"]), npx, npx, C, Cw, relu, P(None), 0, 0, 0,
                                   0, 0, _st())
    assert rc == 0, lib.hpri_last_error()
    return y


def _bn_bwd(lib, g, gcs, goff, xb, xcs, xoff, dx, dxcs, dxoff, st, dgam, dbet, acc, dbias, acc_db, npx, C, Cw, relu, ubs):
    nblk, cpart = ctypes.c_int(), ctypes.c_int()
    assert lib.hpri_col_reduce_plan(npx, 1, C, ctypes.byref(nblk), ctypes.byref(cpart)) == 0
    ws = torch.full((2 * (nblk.value * 2 * cpart.value + 2 * C),), NAN, device=DEV)
    rc = lib.hpri_bn_relu_bwd(P(g), gcs, goff, P(xb), xcs, xoff, P(dx), dxcs, dxoff, P(st["mean"]), P(st["invstd"]), P(st["scale"]),
                              P(st["shift"]), P(dgam), P(dbet), acc, P(dbias), acc_db, P(ws), ws.numel(), npx, npx, C, Cw, relu, ubs, _st())
    assert rc == 0, lib.hpri_last_error()


# ------------------------------------------------------------------------------------------------------------------------------
# 0. head forward
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("bce", [True, False], ids=["bce", "plain"])
@pytest.mark.parametrize("sliced", [False, True], ids=["plain", "sliced"])
@pytest.mark.parametrize("C", [3, 64, 68])
@pytest.mark.parametrize("H,W", [(5, 7), (37, 41)])
def test_head_forward_equals_apply_plus_outconv(lib, H, W, C, sliced, bce, relu):
    """N = 2; 5 x 7 = 70 pixels: fewer than one four-in-flight round of the grid (every group clamps and masks), 37 x 41: whole
    rounds plus a ragged one; C = 3 (today's route takes outconv_fwd_wide_kernel), 64 (one quad per lane), 68 (two quads on lane 0);
    pad channels of x hold NaN / inf.  Logits, every loss partial and the finished loss bit for bit."""
    N = 2
    npx, Cw = N * H * W, rup(C, 4)
    xcs, xoff = (Cw + 12, 8) if sliced else (Cw, 0)
    xb = _view(npx, C, Cw, xcs, xoff, seed=C + npx + 1)
    st = _stats(xb[:, xoff:xoff + C], C, seed=4)
    gen = torch.Generator(device=DEV).manual_seed(17 + C)
    w = torch.randn(C, device=DEV, generator=gen)
    b = torch.randn(1, device=DEV, generator=gen)
    tgt = (torch.rand(npx, device=DEV, generator=gen) > 0.7).float() if bce else None
    nb = lib.hpri_outconv_fwd_bce_blocks(N, H * W)
    y = _apply(lib, xb, xcs, xoff, st, npx, C, Cw, relu)
    lg0, lg1 = torch.full((npx,), 7.0, device=DEV), torch.full((npx,), 7.0, device=DEV)
    p0, p1 = (torch.full((nb,), NAN, dtype=torch.float64, device=DEV) for _ in range(2))
    if bce:
        rc = lib.hpri_outconv_fwd_bce(P(y), Cw, 0, P(w), P(b), P(lg0), P(tgt), P(p0), nb, N, H * W, C, 1, _st())
    else:
        rc = lib.hpri_outconv_fwd(P(y), Cw, 0, P(w), P(b), P(lg0), N, H * W, C, 1, _st())
    assert rc == 0, lib.hpri_last_error()
    rc = lib.hpri_bn_relu_outconv_fwd(P(xb), xcs, xoff, P(st["scale"]), P(st["shift"]), relu, P(w), P(b), P(lg1), P(tgt), P(p1 if bce else None),
                                      nb if bce else 0, N, H * W, C, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(lg1).all() and float(lg1.abs().max()) > 0
    assert torch.equal(lg0, lg1), float((lg0 - lg1).abs().max())
    if bce:
        assert torch.equal(p0, p1)
        l0, l1 = torch.empty((), device=DEV), torch.empty((), device=DEV)
        assert lib.hpri_bce_finish(P(p0), nb, npx, P(l0), _st()) == 0 and lib.hpri_bce_finish(P(p1), nb, npx, P(l1), _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(l0, l1) and torch.isfinite(l1)


def test_head_forward_rejects_bad_arguments(lib):
    t = torch.zeros(2048, device=DEV)
    null = ctypes.c_void_p(0)
    assert lib.hpri_bn_relu_outconv_fwd(P(t), 260, 0, P(t), P(t), 1, P(t), null, P(t), null, null, 0, 1, 4, 260, _st()) == -1   # C > 256
    assert lib.hpri_bn_relu_outconv_fwd(P(t), 8, 0, P(t), P(t), 1, P(t), null, P(t), P(t), P(t), 0, 1, 4, 8, _st()) == -3       # no room for the partials


# ------------------------------------------------------------------------------------------------------------------------------
# 1. head backward
# ------------------------------------------------------------------------------------------------------------------------------
def _head_case(lib, N, H, W, C, sliced, bce, acc, relu=1, ubs=1):
    npx = N * H * W
    Cw = rup(C, 4)
    xcs, xoff = (Cw + 12, 8) if sliced else (Cw, 0)
    dxcs, dxoff = (Cw + 8, 4) if sliced else (Cw, 0)
    xb = _view(npx, C, Cw, xcs, xoff, seed=C + npx)
    st = _stats(xb[:, xoff:xoff + C], C, seed=3)
    gen = torch.Generator(device=DEV).manual_seed(11 + C)
    w = torch.randn(C, device=DEV, generator=gen)
    dy = torch.randn(npx, device=DEV, generator=gen) * (2.0 if bce else 1e-3)      # the logits, or a logit gradient
    tgt = (torch.rand(npx, device=DEV, generator=gen) > 0.7).float() if bce else None
    gs = torch.tensor([0.75], device=DEV) if bce else None
    init = [torch.randn(n, device=DEV, generator=gen) for n in (C, C, C, C, 1)]    # dgamma, dbeta, dbias, dw, db before the call

    # today's route: y, then the head's two kernels (g = dlogit * w in memory), then the BatchNorm backward reading g and x
    y = _apply(lib, xb, xcs, xoff, st, npx, C, Cw, relu)
    dgam0, dbet0, dbias0, dw0, db0 = (t.clone() for t in init)
    g = torch.full((npx, Cw), 7.0, device=DEV)
    nblk, cpart = ctypes.c_int(), ctypes.c_int()
    assert lib.hpri_outconv_bwd_plan(N, H * W, C, 1, ctypes.byref(nblk), ctypes.byref(cpart)) == 0
    ws = torch.full((nblk.value * 2 * cpart.value,), NAN, device=DEV)
    if bce:
        rc = lib.hpri_outconv_bwd_bce(P(dy), P(tgt), P(gs), P(y), Cw, 0, P(w), P(g), Cw, 0, Cw, 0, P(dw0), P(db0), acc, P(ws), ws.numel(),
                                      N, H * W, C, 1, _st())
    else:
        rc = lib.hpri_outconv_bwd(P(dy), P(y), Cw, 0, P(w), P(g), Cw, 0, Cw, 0, P(dw0), P(db0), acc, P(ws), ws.numel(), N, H * W, C, 1, _st())
    assert rc == 0, lib.hpri_last_error()
    dx0 = torch.full((npx, dxcs), 7.0, device=DEV)
    _bn_bwd(lib, g, Cw, 0, xb, xcs, xoff, dx0, dxcs, dxoff, st, dgam0, dbet0, acc, dbias0, acc, npx, C, Cw, relu, ubs)

    # the fused entry: x and the logit-gradient source only
    dgam1, dbet1, dbias1, dw1, db1 = (t.clone() for t in init)
    dx1 = torch.full((npx, dxcs), 7.0, device=DEV)
    ws1 = torch.full((lib.hpri_bn_relu_outconv_bwd_ws(N, H * W, C),), NAN, device=DEV)
    rc = lib.hpri_bn_relu_outconv_bwd(P(dy), P(tgt), P(gs), P(xb), xcs, xoff, P(w), P(dx1), dxcs, dxoff, Cw, P(st["mean"]), P(st["invstd"]),
                                      P(st["scale"]), P(st["shift"]), P(dgam1), P(dbet1), acc, P(dbias1), acc, P(dw1), P(db1), acc, P(ws1),
                                      ws1.numel(), N, H * W, C, relu, ubs, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(dx1[:, dxoff:dxoff + Cw]).all() and torch.isfinite(dw1).all()
    for a, b, what in ((dx0, dx1, "dx"), (dgam0, dgam1, "dgamma"), (dbet0, dbet1, "dbeta"), (dbias0, dbias1, "dbias"), (dw0, dw1, "dw"),
                       (db0, db1, "db")):
        assert torch.equal(a, b), (what, float((a - b).abs().max()))
    assert torch.all(dx1[:, dxoff + C:dxoff + Cw] == 0), "pad channels of dx must be zeros"
    assert torch.all(dx1[:, :dxoff] == 7.0) and torch.all(dx1[:, dxoff + Cw:] == 7.0), "written outside the view"
    assert float(dx1[:, dxoff:dxoff + C].abs().max()) > 0 and float(dw1.abs().max()) > 0


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("bce", [True, False], ids=["bce", "dlogit"])
@pytest.mark.parametrize("sliced", [False, True], ids=["plain", "sliced"])
@pytest.mark.parametrize("C", [3, 64, 68])
@pytest.mark.parametrize("H,W", [(5, 7), (37, 41)])
def test_head_backward_equals_the_four_kernel_route(lib, H, W, C, sliced, bce, acc):
    """N = 2; 5 x 7: fewer pixels than a workgroup covers in two four-in-flight rounds, 37 x 41: several blocks, main loop and
    remainder; C = 3 (not a multiple of 4), 64 (16 quads), 68 (17 quads: a 32-quad row with pad quads)."""
    _head_case(lib, 2, H, W, C, sliced, bce, acc)


@pytest.mark.parametrize("relu,ubs", [(0, 1), (1, 0), (0, 0)])
def test_head_backward_without_relu_and_with_running_statistics(lib, relu, ubs):
    """relu = 0 (BatchNorm only) and use_batch_stats = 0 (eval-mode statistics: dx = scale * g, dbias = the column sum of dx)."""
    _head_case(lib, 2, 37, 41, 6, True, True, 1, relu=relu, ubs=ubs)


def test_head_backward_rejects_bad_arguments(lib):
    null = ctypes.c_void_p(0)
    t = torch.zeros(64, device=DEV)
    args = lambda C, ws: (P(t), null, null, P(t), 8, 0, P(t), P(t), 8, 0, 8, P(t), P(t), P(t), P(t), null, null, 0, null, 0, P(t), null, 0,
                          P(t), ws, 1, 4, C, 1, 1, _st())
    assert lib.hpri_bn_relu_outconv_bwd(*args(5, 0)) == -3            # workspace too small
    assert lib.hpri_bn_relu_outconv_bwd(*args(9, 1 << 20)) == -1      # C beyond the channel width
    assert lib.hpri_bn_relu_bwd_pool(null, 0, 0, null, 8, 0, P(t), 8, 0, P(t), 8, 0, P(t), P(t), P(t), P(t), null, null, 0, null, 0, P(t),
                                     64, 1, 2, 2, 4, 4, _st()) == -1  # no pooled gradient


# ------------------------------------------------------------------------------------------------------------------------------
# 2. pooling backward
# ------------------------------------------------------------------------------------------------------------------------------
def _pool_case(lib, N, H, W, C, skip, acc=0):
    npx, OH, OW = N * H * W, H // 2, W // 2
    Cw = rup(C, 4)
    xcs, xoff = Cw + 4, 4
    xb = _view(npx, C, Cw, xcs, xoff, seed=H * W + C)
    xv = xb[:, xoff:xoff + C]
    st = _stats(xv, C, seed=5, positive_gamma=True)
    # crafted windows: every fifth window holds four equal values that give one positive y (a four-way tie: the first pixel
    # takes the gradient), the next one four values far below the mean (y = 0 four times: routed to the first pixel, then masked)
    x4 = xb.view(N, H, W, xcs)
    wy, wx = torch.meshgrid(torch.arange(OH, device=DEV), torch.arange(OW, device=DEV), indexing="ij")
    kind = (wy * OW + wx) % 5
    for k, val in ((0, st["mean"] + 4.0 / st["invstd"]), (1, st["mean"] - 100.0 / st["invstd"])):
        sel = (kind == k).repeat_interleave(2, 0).repeat_interleave(2, 1)          # [2 OH][2 OW]
        x4[:, :2 * OH, :2 * OW, xoff:xoff + C] = torch.where(sel[None, :, :, None], val.view(1, 1, 1, C), x4[:, :2 * OH, :2 * OW, xoff:xoff + C])
    y = _apply(lib, xb, xcs, xoff, st, npx, C, Cw, 1)
    y4 = y.view(N, H, W, Cw)
    tie = y4[:, 0:2 * OH:2, 0:2 * OW:2, :C][:, kind == 0]
    assert torch.all(tie > 0) and torch.equal(tie, y4[:, 1:2 * OH:2, 1:2 * OW:2, :C][:, kind == 0])
    assert torch.all(y4[:, :2 * OH, :2 * OW, :C][:, (kind == 1).repeat_interleave(2, 0).repeat_interleave(2, 1)] == 0)
    dscs, dsoff = Cw + 16, 8                                            # the skip gradient: a channel slice of a concat's gradient
    ds = _view(npx, C, Cw, dscs, dsoff, seed=7 + C, offset=0.0) if skip else None
    dpcs, dpoff = Cw + 4, 0
    dp = _view(N * OH * OW, C, Cw, dpcs, dpoff, seed=9 + C, offset=0.0)

    # today's route: the summed gradient in memory, then the BatchNorm backward
    g = torch.full((npx, Cw), 7.0, device=DEV)
    if skip:
        g.copy_(ds[:, dsoff:dsoff + Cw])
    rc = lib.hpri_maxpool2_bwd(P(y), Cw, 0, P(dp), dpcs, dpoff, P(g), Cw, 0, N, H, W, Cw, int(skip), _st())
    assert rc == 0, lib.hpri_last_error()
    gen = torch.Generator(device=DEV).manual_seed(13)
    init = [torch.randn(C, device=DEV, generator=gen) for _ in range(3)]
    dgam0, dbet0, dbias0 = (t.clone() for t in init)
    dx0 = torch.full((npx, Cw), 7.0, device=DEV)
    _bn_bwd(lib, g, Cw, 0, xb, xcs, xoff, dx0, Cw, 0, st, dgam0, dbet0, acc, dbias0, acc, npx, C, Cw, 1, 1)

    # the fused entry
    nblk, cpart = ctypes.c_int(), ctypes.c_int()
    assert lib.hpri_bn_relu_bwd_pool_plan(N, H, W, C, ctypes.byref(nblk), ctypes.byref(cpart)) == 0
    ws = torch.full((nblk.value * 2 * cpart.value + 2 * C,), NAN, device=DEV)
    dgam1, dbet1, dbias1 = (t.clone() for t in init)
    dxcs, dxoff = Cw + 8, 4
    dx1 = torch.full((npx, dxcs), 7.0, device=DEV)
    rc = lib.hpri_bn_relu_bwd_pool(P(ds), dscs, dsoff, P(dp), dpcs, dpoff, P(xb), xcs, xoff, P(dx1), dxcs, dxoff, P(st["mean"]),
                                   P(st["invstd"]), P(st["scale"]), P(st["shift"]), P(dgam1), P(dbet1), acc, P(dbias1), acc, P(ws), ws.numel(),
                                   N, H, W, C, Cw, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    key = f"fused/pool/{H}x{W}xC{C}/skip{int(skip)}/acc{acc}"
    dxv = dx1[:, dxoff:dxoff + C]
    assert torch.isfinite(dx1[:, dxoff:dxoff + Cw]).all() and torch.isfinite(dgam1).all() and torch.isfinite(dbet1).all()
    assert torch.all(dx1[:, dxoff + C:dxoff + Cw] == 0), "pad channels of dx must be zeros (the inputs hold NaN / inf there)"
    assert torch.all(dx1[:, :dxoff] == 7.0) and torch.all(dx1[:, dxoff + Cw:] == 7.0), "written outside the view"
    assert torch.equal(dbias1, init[2] if acc else torch.zeros_like(dbias1)), "training mode: dbias is exact zeros, or unchanged when accumulating"
    if acc:      # the parameter gradients were added to what the slots held: one more rounding each, the sums themselves as below
        dgam1, dbet1, dgam0, dbet0 = (t.double() - i.double() for t, i in ((dgam1, init[0]), (dbet1, init[1]), (dgam0, init[0]), (dbet0, init[1])))

    # fp64 reference from the gradient the replaced kernel left (an exact elementwise function of the inputs) and the forward mask
    gm = g[:, :C].double() * (y[:, :C] > 0)
    mu, istd, sc = (st[k].double() for k in ("mean", "invstd", "scale"))
    xh = (xv.double() - mu) * istd
    s1, s2, a1, a2 = gm.sum(0), (gm * xh).sum(0), gm.abs().sum(0), (gm * xh).abs().sum(0)
    cq = 1
    while cq < (C + 3) // 4 and cq < 64:
        cq <<= 1
    rows = 256 // cq
    nwin = N * ((H + 1) // 2) * ((W + 1) // 2)
    L = 4 * -(-(-(-nwin // nblk.value)) // rows) + rows
    tol_rel = (L + 8) * U
    ra, rb = (2 * U * (init[0].double().abs() + s2.abs()), 2 * U * (init[1].double().abs() + s1.abs())) if acc else (0.0, 0.0)
    _gate(key + "/dbeta", (dbet1.double() - s1).abs(), tol_rel * a1 + 2 * U * s1.abs() + rb)
    _gate(key + "/dgamma", (dgam1.double() - s2).abs(), tol_rel * a2 + 2 * U * s2.abs() + ra)
    k1, k2 = s1 / npx, s2 / npx
    d1, d2 = tol_rel * a1 / npx + 3 * U * k1.abs(), tol_rel * a2 / npx + 3 * U * k2.abs()
    ref = sc * (gm - k1 - xh * k2)
    tol = sc.abs() * (4 * U * (gm.abs() + k1.abs() + 2 * (xh * k2).abs()) + d1 + xh.abs() * d2)
    _gate(key + "/dx", (dxv.double() - ref).abs(), tol)
    # ... and against the replaced route itself: each is within its bound of fp64 (that route's chain: pixels per thread + rows)
    nb0, cp0 = ctypes.c_int(), ctypes.c_int()
    assert lib.hpri_col_reduce_plan(npx, 1, C, ctypes.byref(nb0), ctypes.byref(cp0)) == 0
    L0 = -(-(-(-npx // nb0.value)) // rows) + rows
    _gate(key + "/dbeta_vs_route", (dbet1.double() - dbet0.double()).abs(), (L + L0 + 16) * U * a1 + 4 * U * s1.abs() + 2 * rb)
    _gate(key + "/dgamma_vs_route", (dgam1.double() - dgam0.double()).abs(), (L + L0 + 16) * U * a2 + 4 * U * s2.abs() + 2 * ra)
    # the per-element gradient, recovered from dx with the kernel's OWN sums: g = dx / scale + k1 + xhat * k2; three roundings in
    # dx, then the division and two sums in double -- a window routed to another pixel is off by that window's whole gradient
    kk1, kk2 = dbet1.double() / npx, dgam1.double() / npx
    rec = dxv.double() / sc + kk1 + xh * kk2
    tol_g = 8 * U * (gm.abs() + kk1.abs() + 2 * (xh * kk2).abs())
    _gate(key + "/gradient_from_dx", (rec - gm).abs(), tol_g)


@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("C", [4, 6, 64])
@pytest.mark.parametrize("H,W", [(4, 6), (5, 7), (9, 34)])
def test_pool_backward_vs_fp64_and_the_replaced_route(lib, H, W, C, skip):
    """N = 2; even, both odd (last row and column take the skip term only), one odd with a long row; C = 6 leaves two pad channels
    that hold NaN / inf in x, dskip and dpool."""
    _pool_case(lib, 2, H, W, C, skip)


@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
def test_pool_backward_accumulates_into_parameter_slots(lib, skip):
    """accumulate_param_grads = accumulate_dbias = 1 (gradient accumulation, a gradient sink's second micro-batch): dgamma / dbeta
    are added to what the slots hold (one rounding of the sum more, stated in the gate), dbias is left as it is."""
    _pool_case(lib, 2, 9, 34, 6, skip, acc=1)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("C", [4, 6, 64])
@pytest.mark.parametrize("H,W", [(4, 6), (5, 7), (9, 34)])
def test_pool_forward_equals_apply_plus_maxpool(lib, H, W, C, relu):
    """hpri_bn_apply_relu_pool: y (a channel slice of a wider buffer, as a skip tensor is) and the pooled map against
    hpri_bn_apply_relu_pl + hpri_maxpool2_fwd, bit for bit; odd H / W: the last row / column is written in y and has no pooled value;
    C = 6: the pad channels of x hold NaN / inf and come out as zeros in both outputs; nothing outside the views is written."""
    N = 2
    npx, OH, OW, Cw = N * H * W, H // 2, W // 2, rup(C, 4)
    xcs, xoff = Cw + 4, 4
    xb = _view(npx, C, Cw, xcs, xoff, seed=3 * H * W + C)
    st = _stats(xb[:, xoff:xoff + C], C, seed=6)
    y0 = _apply(lib, xb, xcs, xoff, st, npx, C, Cw, relu)
    p0 = torch.full((N * OH * OW, Cw), 7.0, device=DEV)
    assert lib.hpri_maxpool2_fwd(P(y0), Cw, 0, P(p0), Cw, 0, N, H, W, Cw, _st()) == 0, lib.hpri_last_error()
    ycs, yoff, pcs, poff = Cw + 16, 8, Cw + 8, 4
    y1 = torch.full((npx, ycs), 7.0, device=DEV)
    p1 = torch.full((N * OH * OW, pcs), 7.0, device=DEV)
    rc = lib.hpri_bn_apply_relu_pool(P(xb), xcs, xoff, P(y1), ycs, yoff, P(p1), pcs, poff, P(st["scale"]), P(st["shift"]), N, H, W, C, Cw,
                                     relu, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    assert torch.equal(y1[:, yoff:yoff + Cw], y0) and torch.equal(p1[:, poff:poff + Cw], p0)
    assert torch.isfinite(p0).all() and float(p0.abs().max()) > 0
    assert torch.all(y1[:, :yoff] == 7.0) and torch.all(y1[:, yoff + Cw:] == 7.0), "written outside y's view"
    assert torch.all(p1[:, :poff] == 7.0) and torch.all(p1[:, poff + Cw:] == 7.0), "written outside the pooled view"


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the engine routes on the tiny nets with a reference fixture
# ------------------------------------------------------------------------------------------------------------------------------
def _tiny_step(name, xseed, xshape, fused):
    """One forward_loss + backward of a tiny net with both routes on or off: logits, loss, gradients, kernels launched."""
    import hyperpri_amd as H
    from hyperpri_amd import engine as E
    from oracle import hyperpri_oracle as O
    net = H.UNet(3, 1, bilinear=False) if name == "net_unet3_tiny" else H.CubeNET(6, 1, first_depth=64, bilinear=False)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())
    net.load_state_dict(O.synth_state_dict(shapes))
    net = net.to(DEV).train()
    u = lambda seed, shape: torch.from_numpy(O._u(seed, int(np.prod(shape))).reshape(shape).copy())
    x = u(xseed, xshape).to(DEV)
    mask = (u(4321, (xshape[0], 1) + tuple(xshape[-2:])) > 0.9).float().to(DEV)
    old = E.FUSE_HEAD_BN, E.FUSE_POOL_BN, E.FUSE_POOL_FWD
    E.FUSE_HEAD_BN = E.FUSE_POOL_BN = E.FUSE_POOL_FWD = fused
    calls = []
    real = E._lib.call

    def spy(fn, *a):
        calls.append(fn)
        return real(fn, *a)
    E._lib.call = spy
    try:
        logits = net(x)
        loss = torch.nn.BCEWithLogitsLoss()(logits, mask)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        E._lib.call = real
        E.FUSE_HEAD_BN, E.FUSE_POOL_BN, E.FUSE_POOL_FWD = old
    grads = OrderedDict((k, p.grad.detach().clone()) for k, p in net.named_parameters())
    return logits.detach().clone(), loss.detach().clone(), grads, calls


@pytest.mark.parametrize("name,xseed,xshape", [("net_unet3_tiny", 1234, (2, 3, 36, 50)), ("net_cubenet64_tiny", 1235, (2, 1, 6, 36, 50))])
def test_engine_routes_on_and_off_against_the_fixture(name, xseed, xshape):
    """Logits and loss bit-equal with the routes on and off; with them on, the four encoder levels and the head take the fused
    entries and hpri_maxpool2_bwd / hpri_outconv_bwd are not launched; every parameter gradient's error against the fixture's
    reference gradient (its stored values: the first 16 of each tensor) is at most twice its error with the routes off, plus one
    ulp of the tensor's largest value -- the routes differ in summation order only, a misrouted gradient is wrong by order one."""
    z = np.load(os.path.join(G, name + ".npz"))
    lg1, loss1, g1, calls1 = _tiny_step(name, xseed, xshape, True)
    lg0, loss0, g0, calls0 = _tiny_step(name, xseed, xshape, False)
    assert torch.equal(lg1, lg0) and torch.equal(loss1, loss0)
    assert calls1.count("hpri_bn_relu_bwd_pool") == 4 and calls1.count("hpri_bn_relu_outconv_bwd") == 1
    assert calls1.count("hpri_bn_relu_outconv_fwd") == 1 and "hpri_outconv_fwd" not in calls1
    assert calls1.count("hpri_bn_apply_relu_pool") == 4 and "hpri_maxpool2_fwd_pl" not in calls1 and calls0.count("hpri_maxpool2_fwd_pl") == 4
    assert calls1.count("hpri_bn_apply_relu_pl") == calls0.count("hpri_bn_apply_relu_pl") - 5 and "hpri_bn_relu_outconv_fwd" not in calls0
    assert not any(c in ("hpri_maxpool2_bwd", "hpri_outconv_bwd", "hpri_outconv_bwd_bce") for c in calls1)
    assert calls0.count("hpri_maxpool2_bwd") == 4 and not any(c in ("hpri_bn_relu_bwd_pool", "hpri_bn_relu_outconv_bwd") for c in calls0)
    names = list(z["grad_names"])
    assert names == list(g1.keys())
    for i, k in enumerate(names):
        n = min(16, g1[k].numel())
        head = torch.from_numpy(z["grad_head"][i][:n].astype(np.float64))
        e1 = float((g1[k].double().flatten().cpu()[:n] - head).abs().max())
        e0 = float((g0[k].double().flatten().cpu()[:n] - head).abs().max())
        floor = float(g0[k].abs().max()) * 2.0 ** -23
        record_margin(f"fused/engine/{name}/{k}", e1, 2 * e0 + floor)
        assert e1 <= 2 * e0 + floor, (k, e1, e0, floor)
