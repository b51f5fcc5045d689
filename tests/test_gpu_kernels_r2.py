"""Round-2 kernels called directly through the C ABI (include/hyperpri_hip.h) against a plain torch reference of the
same op in fp64 on the CPU: the fp32 Winograd F(2x2,3x3) forward / data-gradient (conv_wino4.hip) and weight-gradient
(conv_wino.hip) kernels -- Conv2d(k=3, padding=1) of model_parts.py:23,26 and its autograd -- and the bf16-plane convolution
and weight gradient (conv_bf16v3.hip, conv_wgrad_bf16v2.hip; precision mode "bf16").  Odd and ragged geometries,
accumulate / ReLU epilogues, BatchNorm partial statistics, channel-slice views.  Needs a real MI355X: ``-m gpu``."""
import ctypes

import pytest
import torch

from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rup(x, m):
    return (x + m - 1) // m * m


def P(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from hyperpri_amd import _lib
    return _lib.load()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chan_stats(stats, tiles, cout_pad, cout):
    """Per-tile (mean, M2, count) records -> per-channel mean and biased variance (Chan merge in fp64)."""
    s = stats.view(tiles, cout_pad, 4).double().cpu()
    n = s[:, :, 2]
    mean = (s[:, :, 0] * n).sum(0) / n.sum(0)
    m2 = (s[:, :, 1] + n * (s[:, :, 0] - mean) ** 2).sum(0)
    return mean[:cout], (m2 / n.sum(0))[:cout], n.sum(0)[:cout]


GEOM = [(1, 17, 23, 5, 7), (2, 36, 50, 64, 64), (1, 76, 121, 128, 192), (2, 38, 60, 40, 64), (1, 16, 16, 8, 64),
        (1, 1, 1, 8, 8), (1, 2, 3, 3, 1), (1, 33, 31, 238, 64)]


# The single-valued ``kern`` parametrisations keep the test ids and the record_margin keys these kernels have always had.
@pytest.mark.parametrize("shape", GEOM)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kern", ["wino4"])
def test_winograd_forward_and_data_gradient_vs_fp64(lib, shape, mode, kern):
    """mode 0: y = conv2d(x, W) + b.  mode 1: the data-gradient form -- the same kernel on the transposed, 180-degree
    rotated weight (pack mode 1), as engine.py uses it for dX."""
    N, H, W, Cin, Cout = shape
    torch.manual_seed(11 + mode)
    cs, cout_pad, ycs = rup(Cin, 8), rup(Cout, 64), rup(Cout, 8)
    x = torch.zeros(N * H * W, cs, device=DEV)
    x[:, :Cin] = torch.randn(N * H * W, Cin, device=DEV)
    if mode == 0:
        w = torch.randn(Cout, Cin, 3, 3, device=DEV) * 0.1
        d1 = Cin
        wt = w.double().cpu()
    else:
        w = torch.randn(Cin, Cout, 3, 3, device=DEV) * 0.1
        d1 = Cout
        wt = w.double().cpu().permute(1, 0, 2, 3).flip(2, 3)
    b = torch.randn(Cout, device=DEV)
    up = torch.empty(lib.hpri_wino_packed_floats(Cin, cout_pad), device=DEV)
    assert lib.hpri_wino4_pack(P(w), P(up), P(None), mode, Cin, Cout, cout_pad, d1, _st()) == 0
    xt = x[:, :Cin].reshape(N, H, W, Cin).permute(0, 3, 1, 2).double().cpu()
    ref = torch.nn.functional.conv2d(xt, wt, b.double().cpu(), padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
    tl = ctypes.c_int()
    lib.hpri_conv_wino4_plan(N, H, W, ctypes.byref(tl))
    for acc, want in ((0, ref), (2, ref.clamp(min=0)), (1, ref + 0.25)):
        y = torch.full((N * H * W, ycs), 0.25, device=DEV)
        stats = torch.zeros(tl.value * cout_pad * 4, device=DEV) if acc != 1 else None
        rc = lib.hpri_conv_wino4(P(x), cs, 0, P(up), P(b), P(y), ycs, 0, P(stats), N, H, W, cs, Cout, cout_pad, ycs, acc, _st())
        assert rc == 0, lib.hpri_last_error()
        torch.cuda.synchronize()
        got = y[:, :Cout].double().cpu()
        scale = max(1.0, float(want.abs().max()))
        err = float((got - want).abs().max())
        record_margin(f"{kern}/fwd{mode}/acc{acc}/{N}x{H}x{W}x{Cin}x{Cout}", err, 5e-5 * scale)
        assert err < 5e-5 * scale, (shape, mode, acc, err)
        if Cout < ycs:
            assert float(y[:, Cout:].abs().max()) in (0.0, 0.25)       # pad channels: zero-filled or untouched, never garbage
        if stats is not None:
            mean, var, cnt = _chan_stats(stats, tl.value, cout_pad, Cout)
            assert torch.all(cnt == N * H * W)
            assert float((mean - want.mean(0)).abs().max()) < 1e-4 * scale
            assert float((var - want.var(0, unbiased=False)).abs().max()) < 1e-4 * scale * scale


@pytest.mark.parametrize("kern", ["wino4"])
def test_winograd_forward_channel_slice_views(lib, kern):
    """Input and output are channel slices of wider buffers (the skip-concat layout, model_parts.py:87): the kernel
    must read only [coff, coff+Cin) and write only [coff, coff+Cout)."""
    N, H, W, Cin, Cout = 1, 20, 28, 16, 64
    torch.manual_seed(5)
    xcs, xoff, ycs, yoff = 40, 8, 136, 64
    xb = torch.randn(N * H * W, xcs, device=DEV)
    w = torch.randn(Cout, Cin, 3, 3, device=DEV) * 0.1
    cout_pad = rup(Cout, 64)
    up = torch.empty(lib.hpri_wino_packed_floats(Cin, cout_pad), device=DEV)
    assert lib.hpri_wino4_pack(P(w), P(up), P(None), 0, Cin, Cout, cout_pad, Cin, _st()) == 0
    yb = torch.full((N * H * W, ycs), 7.0, device=DEV)
    rc = lib.hpri_conv_wino4(P(xb), xcs, xoff, P(up), P(None), P(yb), ycs, yoff, P(None), N, H, W, Cin, Cout, cout_pad, Cout, 0, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    xt = xb[:, xoff:xoff + Cin].reshape(N, H, W, Cin).permute(0, 3, 1, 2).double().cpu()
    ref = torch.nn.functional.conv2d(xt, w.double().cpu(), None, padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
    assert float((yb[:, yoff:yoff + Cout].double().cpu() - ref).abs().max()) < 5e-5 * float(ref.abs().max())
    assert torch.all(yb[:, :yoff] == 7.0) and torch.all(yb[:, yoff + Cout:] == 7.0)


@pytest.mark.parametrize("kern", ["wino4"])
def test_winograd_rejects_unaligned_output(lib, kern):
    """The output transform stores float4 channel vectors: a channel stride that is not a multiple of 4 is an error
    return (HPRI_REQUIRE), not a silent scatter over the neighbouring pixels."""
    N, H, W, Cin, Cout = 1, 8, 8, 8, 7
    x = torch.zeros(N * H * W, 8, device=DEV)
    up = torch.zeros(lib.hpri_wino_packed_floats(Cin, 64), device=DEV)
    y = torch.zeros(N * H * W * 8, device=DEV)
    rc = lib.hpri_conv_wino4(P(x), 8, 0, P(up), P(None), P(y), 7, 0, P(None), N, H, W, 8, Cout, 64, 7, 0, _st())
    assert rc != 0
    assert b"y_cs" in lib.hpri_last_error() or b"align" in lib.hpri_last_error().lower()


@pytest.mark.parametrize("shape", GEOM + [(2, 76, 121, 64, 128), (2, 152, 242, 16, 64)])
def test_winograd_weight_gradient_vs_fp64(lib, shape):
    """dW = sum over tiles of V (x) (A dY A^T) in the Winograd domain, then G^T dU G -- against conv2d_weight in
    fp64; a second call with accumulate=1 must add onto the first (the fused tape's gradient sink)."""
    N, H, W, Cin, Cout = shape
    torch.manual_seed(23)
    cs, cso, cout_pad = rup(Cin, 8), rup(Cout, 8), rup(Cout, 64)
    x = torch.zeros(N * H * W, cs, device=DEV)
    x[:, :Cin] = torch.randn(N * H * W, Cin, device=DEV)
    dy = torch.zeros(N * H * W, cso, device=DEV)
    dy[:, :Cout] = torch.randn(N * H * W, Cout, device=DEV)
    xt = x[:, :Cin].reshape(N, H, W, Cin).permute(0, 3, 1, 2).double().cpu()
    dt = dy[:, :Cout].reshape(N, H, W, Cout).permute(0, 3, 1, 2).double().cpu()
    ref = torch.nn.grad.conv2d_weight(xt, (Cout, Cin, 3, 3), dt, padding=1)
    sp, cr, nr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib.hpri_wino_wgrad_plan(N, H, W, cs, cout_pad, ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr))
    ws = torch.empty(sp.value * 16 * cr.value * nr.value, device=DEV)
    dw = torch.full((Cout, Cin, 3, 3), 0.5, device=DEV)
    for acc in (0, 1):
        rc = lib.hpri_conv_wino_wgrad(P(x), cs, 0, cs, P(dy), cso, 0, cso, P(ws), ws.numel(), N, H, W, cs, cout_pad, _st())
        assert rc == 0, lib.hpri_last_error()
        assert lib.hpri_wino_wgrad_reduce(P(ws), P(dw), N, H, W, Cin, cs, Cout, cout_pad, acc, _st()) == 0
    torch.cuda.synchronize()
    sc = max(1.0, float(ref.abs().max()))
    err = float((dw.double().cpu() - 2 * ref).abs().max())
    record_margin(f"wino/wgrad/{N}x{H}x{W}x{Cin}x{Cout}", err, 4e-5 * sc)
    assert err < 4e-5 * sc, (shape, err)
    # too small a workspace is an error return, not an overrun
    rc = lib.hpri_conv_wino_wgrad(P(x), cs, 0, cs, P(dy), cso, 0, cso, P(ws), max(ws.numel() // 2, 1) - 1, N, H, W, cs, cout_pad, _st())
    assert rc != 0


@pytest.mark.parametrize("shape", [(2, 36, 50, 64, 64), (1, 76, 121, 128, 192), (1, 17, 23, 40, 64), (1, 33, 31, 238, 64),
                                   (2, 38, 60, 256, 128), (1, 1, 1, 32, 64), (1, 9, 100, 6, 64), (3, 16, 16, 32, 320)])
@pytest.mark.parametrize("kern", ["bf16v3"])
def test_bf16_plane_conv_vs_fp64_of_rounded_operands(lib, shape, kern):
    """conv_bf16v3 (4-wave workgroups, two per CU, 16x16x32 MFMA): operands are bf16 planes in HBM
    (written by hpri_to_planes), products accumulate in fp32.  The reference is conv2d in fp64 of the SAME bf16-rounded
    operands, so the only difference is fp32 summation order."""
    N, H, W, Cin, Cout = shape
    torch.manual_seed(31)
    cs, cs16, cout_pad = rup(Cin, 8), rup(Cin, 32), rup(Cout, 64)
    x = torch.zeros(N * H * W, cs, device=DEV)
    x[:, :Cin] = torch.randn(N * H * W, Cin, device=DEV)
    w = torch.randn(Cout, Cin, 3, 3, device=DEV) * 0.05
    b = torch.randn(Cout, device=DEV)
    planes = torch.empty(N * H * W * cs16, dtype=torch.bfloat16, device=DEV)
    assert lib.hpri_to_planes(P(x), cs, 0, P(planes), 0, cs16, 0, N * H * W, Cin, cs16, 1, _st()) == 0
    wpb = torch.empty(((Cin + 31) // 32) * 9 * cout_pad * 32, dtype=torch.bfloat16, device=DEV)
    assert lib.hpri_pack_weight_bf16(P(w), P(wpb), 0, Cin, Cout, cout_pad, 9, Cin, 0, 0, _st()) == 0
    k, tl, wsf = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    lib.hpri_conv_bf16v3_plan(N, H, W, cs16, cout_pad, ctypes.byref(k), ctypes.byref(tl), ctypes.byref(wsf))
    ws = torch.empty(max(wsf.value, 4), device=DEV)
    stats = torch.zeros(tl.value * cout_pad * 4, device=DEV)
    y = torch.zeros(N * H * W, Cout, device=DEV)
    rc = lib.hpri_conv_bf16v3(P(planes), 0, cs16, 0, P(wpb), P(b), P(y), Cout, 0, P(stats), N, H, W, cs16, Cout, cout_pad, Cout, 0, 0,
                              P(ws), ws.numel(), _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    # the plane pass rounds to nearest-even bf16 and zero-fills the channel pad
    pl = planes.view(N * H * W, cs16)
    assert torch.equal(pl[:, :Cin], x[:, :Cin].to(torch.bfloat16))
    assert float(pl[:, Cin:].float().abs().max()) == 0.0 if cs16 > Cin else True
    xr = x[:, :Cin].to(torch.bfloat16).double().cpu().reshape(N, H, W, Cin).permute(0, 3, 1, 2)
    wr = w.to(torch.bfloat16).double().cpu()
    ref = torch.nn.functional.conv2d(xr, wr, b.double().cpu(), padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
    sc = max(1.0, float(ref.abs().max()))
    err = float((y.double().cpu() - ref).abs().max())
    record_margin(f"{kern}/{N}x{H}x{W}x{Cin}x{Cout}", err, 2e-5 * sc)
    assert err < 2e-5 * sc, (shape, err)
    mean, var, cnt = _chan_stats(stats, tl.value, cout_pad, Cout)
    assert torch.all(cnt == N * H * W)
    assert float((mean - ref.mean(0)).abs().max()) < 1e-4 * sc
    assert float((var - ref.var(0, unbiased=False)).abs().max()) < 1e-4 * sc * sc


@pytest.mark.parametrize("shape", [(2, 36, 50, 64, 6), (1, 19, 40, 128, 72), (2, 38, 60, 256, 128)])
def test_bf16_plane_conv_v3_data_gradient_views_and_epilogues(lib, shape):
    """conv_bf16v3 as the data gradient (mode-1 pack: K = Cout of the layer, columns = its Cin, rotated taps) writing a
    channel-slice VIEW of a wider gradient buffer, accumulating into what is there (a skip gradient), with the columns' zero
    pad kept zero; then the ReLU epilogue of the folded predict path; then the error returns of the boundary."""
    N, H, W, K, Cols = shape                   # dy has K channels, the result Cols channels
    torch.manual_seed(7)
    cs16, cols_pad, cw = rup(K, 32), rup(Cols, 64), rup(Cols, 8)
    dy = torch.randn(N * H * W, K, device=DEV)
    planes = torch.zeros(N * H * W, cs16, dtype=torch.bfloat16, device=DEV)
    planes[:, :K] = dy.to(torch.bfloat16)
    w = torch.randn(K, Cols, 3, 3, device=DEV) * 0.05                       # the layer's weight [Cout = K][Cin = Cols]
    wpd = torch.empty(((K + 31) // 32) * 9 * cols_pad * 32, dtype=torch.bfloat16, device=DEV)
    assert lib.hpri_pack_weight_bf16(P(w), P(wpd), 1, K, Cols, cols_pad, 9, Cols, 0, 0, _st()) == 0
    k, tl, wsf = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    lib.hpri_conv_bf16v3_plan(N, H, W, cs16, cols_pad, ctypes.byref(k), ctypes.byref(tl), ctypes.byref(wsf))
    ws = torch.empty(max(wsf.value, 4), device=DEV)
    ycs, yoff = cw + 16, 8                                                  # a view inside a wider buffer
    prior = torch.randn(N * H * W, ycs, device=DEV)
    ybuf = prior.clone()
    rc = lib.hpri_conv_bf16v3(P(planes), 0, cs16, 0, P(wpd), P(None), P(ybuf), ycs, yoff, P(None), N, H, W, cs16, Cols, cols_pad, cw, 1, 0,
                              P(ws), ws.numel(), _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    xr = planes[:, :K].double().cpu().reshape(N, H, W, K).permute(0, 3, 1, 2)
    wr = w.to(torch.bfloat16).double().cpu()
    ref = torch.nn.functional.conv_transpose2d(xr, wr, padding=1).permute(0, 2, 3, 1).reshape(-1, Cols)     # = dX of conv2d(pad 1)
    sc = max(1.0, float(ref.abs().max()))
    got = ybuf.double().cpu()
    err = float((got[:, yoff:yoff + Cols] - (prior.double().cpu()[:, yoff:yoff + Cols] + ref)).abs().max())
    record_margin(f"bf16v3/dgrad/{N}x{H}x{W}x{K}x{Cols}", err, 2e-5 * sc)
    assert err < 2e-5 * sc, (shape, err)
    # pad columns [Cols, cw) of the view: accumulate adds exact zeros; everything outside the view is untouched
    assert torch.equal(got[:, yoff + Cols:yoff + cw], prior.double().cpu()[:, yoff + Cols:yoff + cw])
    assert torch.equal(got[:, :yoff], prior.double().cpu()[:, :yoff]) and torch.equal(got[:, yoff + cw:], prior.double().cpu()[:, yoff + cw:])
    # ReLU epilogue (accumulate bit 1), bias, no statistics: the folded predict path
    b = torch.randn(Cols, device=DEV)
    y2 = torch.full((N * H * W, cw), 7.0, device=DEV)
    rc = lib.hpri_conv_bf16v3(P(planes), 0, cs16, 0, P(wpd), P(b), P(y2), cw, 0, P(None), N, H, W, cs16, Cols, cols_pad, cw, 2, 0,
                              P(ws), ws.numel(), _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    ref2 = torch.relu(ref + b.double().cpu())
    assert float((y2.double().cpu()[:, :Cols] - ref2).abs().max()) < 2e-5 * sc
    assert float(y2[:, Cols:].abs().max()) == 0.0 if cw > Cols else True
    # boundary errors: unaligned output view, channel stride too small, split planes, missing split-K workspace
    assert lib.hpri_conv_bf16v3(P(planes), 0, cs16, 0, P(wpd), P(b), P(y2), cw, 2, P(None), N, H, W, cs16, Cols, cols_pad, cw, 0, 0,
                                P(ws), ws.numel(), _st()) != 0
    assert lib.hpri_conv_bf16v3(P(planes), 0, cs16 - 8, 0, P(wpd), P(b), P(y2), cw, 0, P(None), N, H, W, cs16, Cols, cols_pad, cw, 0, 0,
                                P(ws), ws.numel(), _st()) != 0
    assert lib.hpri_conv_bf16v3(P(planes), 0, cs16, 0, P(wpd), P(b), P(y2), cw, 0, P(None), N, H, W, cs16, Cols, cols_pad, cw, 0, 1,
                                P(ws), ws.numel(), _st()) != 0
    if k.value > 1:
        assert lib.hpri_conv_bf16v3(P(planes), 0, cs16, 0, P(wpd), P(b), P(y2), cw, 0, P(None), N, H, W, cs16, Cols, cols_pad, cw, 0, 0,
                                    P(None), 0, _st()) != 0


@pytest.mark.parametrize("shape", [(1, 17, 23, 5, 7), (2, 36, 50, 64, 64), (1, 76, 121, 128, 192), (2, 38, 60, 40, 64), (1, 4, 32, 64, 64),
                                   (1, 3, 3, 8, 8), (1, 33, 31, 238, 64), (1, 1, 1, 3, 1)])
def test_bf16_plane_weight_gradient_vs_fp64_of_rounded_operands(lib, shape):
    """conv_wgrad_bf16v2: X and dY planes by LDS-DMA, transposed LDS reads, fp32 accumulate, deterministic split-K.
    Reference: conv2d_weight in fp64 of the same bf16-rounded operands; accumulate=1 adds onto the first result."""
    N, H, W, Cin, Cout = shape
    torch.manual_seed(41)
    cs, cso, cs16, cso16 = rup(Cin, 8), rup(Cout, 8), rup(Cin, 32), rup(Cout, 32)
    x = torch.zeros(N * H * W, cs, device=DEV)
    x[:, :Cin] = torch.randn(N * H * W, Cin, device=DEV)
    dy = torch.zeros(N * H * W, cso, device=DEV)
    dy[:, :Cout] = torch.randn(N * H * W, Cout, device=DEV)
    xp = torch.empty(N * H * W * cs16, dtype=torch.bfloat16, device=DEV)
    dp = torch.empty(N * H * W * cso16, dtype=torch.bfloat16, device=DEV)
    assert lib.hpri_to_planes(P(x), cs, 0, P(xp), 0, cs16, 0, N * H * W, Cin, cs16, 1, _st()) == 0
    assert lib.hpri_to_planes(P(dy), cso, 0, P(dp), 0, cso16, 0, N * H * W, Cout, cso16, 1, _st()) == 0
    sp, cr, nr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib.hpri_wgrad_bf16v2_plan(N, H, W, cs16, rup(Cout, 64), ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr))
    ws = torch.empty(sp.value * 9 * cr.value * nr.value, device=DEV)
    dw = torch.full((Cout, Cin, 3, 3), 0.5, device=DEV)
    for acc in (0, 1):
        rc = lib.hpri_conv_wgrad_bf16v2(P(xp), cs16, 0, cs16, P(dp), cso16, 0, cso16, P(ws), ws.numel(), N, H, W, cs16, rup(Cout, 64), _st())
        assert rc == 0, lib.hpri_last_error()
        rc = lib.hpri_wgrad_reduce_ex(P(ws), P(dw), sp.value, cr.value, nr.value, Cin, Cout, 3, 0, 0, acc, _st())
        assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    xr = x[:, :Cin].to(torch.bfloat16).double().cpu().reshape(N, H, W, Cin).permute(0, 3, 1, 2)
    dr = dy[:, :Cout].to(torch.bfloat16).double().cpu().reshape(N, H, W, Cout).permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(xr, (Cout, Cin, 3, 3), dr, padding=1)
    sc = max(1.0, float(ref.abs().max()))
    err = float((dw.double().cpu() - 2 * ref).abs().max())
    record_margin(f"wgrad_bf16v2/{N}x{H}x{W}x{Cin}x{Cout}", err, 4e-6 * sc)
    assert err < 4e-6 * sc, (shape, err)
    # a workspace that is too small is an error return
    assert lib.hpri_conv_wgrad_bf16v2(P(xp), cs16, 0, cs16, P(dp), cso16, 0, cso16, P(ws), ws.numel() - 1, N, H, W, cs16, rup(Cout, 64), _st()) != 0
    # misaligned channel stride is an error return
    assert lib.hpri_conv_wgrad_bf16v2(P(xp), cs16 + 4, 0, cs16, P(dp), cso16, 0, cso16, P(ws), ws.numel(), N, H, W, cs16, rup(Cout, 64), _st()) != 0


@pytest.mark.parametrize("shape", [(2, 9, 11, 8), (1, 36, 50, 64), (3, 7, 8, 12), (1, 2, 2, 4), (2, 25, 12, 40)])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_maxpool_backward_one_thread_per_window(lib, shape, accumulate):
    """hpri_maxpool2_bwd (round 3: one thread per 2x2 window) against torch's max_pool2d autograd: odd heights / widths (the floor
    drops the last row / column: zero gradient there), ties (the FIRST maximum in scan order takes the gradient, as ATen), a
    channel-slice view of a wider gradient buffer, accumulate."""
    N, H, W, C = shape
    torch.manual_seed(23)
    x = torch.randn(N, H, W, C, device=DEV)
    x[:, ::2, ::2] = x[:, ::2, ::2].round()                   # ties inside windows
    x[:, : H // 2 * 2 : 2, 1 : W // 2 * 2 : 2] = x[:, : H // 2 * 2 : 2, : W // 2 * 2 : 2]
    OH, OW = H // 2, W // 2
    dy = torch.randn(N, OH, OW, C, device=DEV)
    cs, off = C + 8, 4
    prior = torch.randn(N * H * W, cs, device=DEV)
    dx = prior.clone()
    rc = lib.hpri_maxpool2_bwd(P(x), C, 0, P(dy), C, 0, P(dx), cs, off, N, H, W, C, accumulate, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    xr = x.permute(0, 3, 1, 2).detach().cpu().double().requires_grad_(True)
    yr = torch.nn.functional.max_pool2d(xr, 2)
    yr.backward(dy.permute(0, 3, 1, 2).cpu().double())
    ref = xr.grad.permute(0, 2, 3, 1).reshape(-1, C)
    got = dx.double().cpu()
    want = ref + (prior.double().cpu()[:, off:off + C] if accumulate else 0)
    assert torch.equal(got[:, off:off + C].float(), want.float())
    assert torch.equal(got[:, :off], prior.double().cpu()[:, :off]) and torch.equal(got[:, off + C:], prior.double().cpu()[:, off + C:])


@pytest.mark.parametrize("case", [  # P, s_cs, s_coff, d_cs, d_coff, C, Cz
    (500, 1656, 0, 3304, 0, 1650, 0), (500, 1656, 0, 3304, 1650, 1650, 1654), (300, 3304, 1650, 1656, 0, 1650, 1656),
    (257, 1001, 3, 2051, 7, 997, 1000), (64, 300, 1, 301, 2, 256, 0), (1000, 56, 0, 112, 50, 50, 54), (1, 3300, 1650, 3314, 1664, 1650, 0)])
@pytest.mark.parametrize("acc", [0, 1])
def test_copy_slice_any_rows_and_elements(lib, case, acc):
    """hpri_copy_slice_any (SpectralUNET's 1650-channel concat halves, models.py:139-143): the row-walking form (wide rows; 8-byte
    pieces when every stride, offset and count is even, single floats otherwise) and the element loop (narrow rows) copy / add the
    slice, zero-fill [C, Cz) and leave every other element of the destination alone -- bit-exact."""
    Pn, scs, sco, dcs, dco, C, Cz = case
    torch.manual_seed(2)
    s = torch.randn(Pn, scs, device=DEV)
    d0 = torch.randn(Pn, dcs, device=DEV)
    d = d0.clone()
    assert lib.hpri_copy_slice_any(P(s), scs, sco, P(d), dcs, dco, Pn, C, Cz, acc, _st()) == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    want = d0.clone()
    want[:, dco:dco + C] = s[:, sco:sco + C] + (d0[:, dco:dco + C] if acc else 0)
    if Cz > C and not acc:
        want[:, dco + C:dco + Cz] = 0
    assert torch.equal(d, want)


@pytest.mark.parametrize("shape", [(2, 8, 10, 64), (1, 9, 7, 32), (2, 5, 121, 96)])
def test_maxpool_over_bf16_rows(lib, shape):
    """hpri_maxpool2_fwd_x16 / hpri_maxpool2_bwd_x16 (round 4; model_parts.py:40 on a planes-only skip): forward == the fp32 kernel on the
    same (bf16-exact) values, fp32 output optional; backward == the fp32 kernel on those values, the gradient written / accumulated as
    fp32 or as bf16 rows (rounded once per write).  The fp32 forward it is compared with, hpri_maxpool2_fwd_pl, is pinned against
    F.max_pool2d in test_gpu_glue_kernels.py; the fp32 backward in test_maxpool_backward_one_thread_per_window above."""
    N, H, W, C = shape
    torch.manual_seed(6)
    xs = C + 32                                               # the skip half of a wider plane buffer
    x16 = torch.zeros(N * H * W, xs, dtype=torch.bfloat16, device=DEV)
    x16[:, :C] = torch.randn(N * H * W, C, device=DEV).to(torch.bfloat16)
    xf = x16[:, :C].float().contiguous()
    OH, OW = H // 2, W // 2
    y_ref = torch.empty(N * OH * OW, C, device=DEV)
    pl_ref = torch.empty(N * OH * OW, C, dtype=torch.bfloat16, device=DEV)
    assert lib.hpri_maxpool2_fwd_pl(P(xf), C, 0, P(y_ref), C, 0, N, H, W, C, P(pl_ref), N * OH * OW * C, C, 0, C, 1, _st()) == 0
    y = torch.empty_like(y_ref)
    pl = torch.empty_like(pl_ref)
    assert lib.hpri_maxpool2_fwd_x16(P(x16), xs, 0, P(y), C, 0, N, H, W, C, P(pl), N * OH * OW * C, C, 0, C, 1, _st()) == 0, lib.hpri_last_error()
    pl2 = torch.empty_like(pl_ref)
    assert lib.hpri_maxpool2_fwd_x16(P(x16), xs, 0, P(None), 0, 0, N, H, W, C, P(pl2), N * OH * OW * C, C, 0, C, 1, _st()) == 0     # planes only
    assert lib.hpri_maxpool2_fwd_x16(P(x16), xs, 0, P(None), 0, 0, N, H, W, C, P(None), 0, 0, 0, 0, 0, _st()) != 0                 # nothing to write
    torch.cuda.synchronize()
    assert torch.equal(y, y_ref) and torch.equal(pl, pl_ref) and torch.equal(pl2, pl_ref)
    dy = torch.randn(N * OH * OW, C, device=DEV)
    for acc in (0, 1):
        d0 = torch.randn(N * H * W, C, device=DEV)
        want = d0.clone()
        assert lib.hpri_maxpool2_bwd(P(xf), C, 0, P(dy), C, 0, P(want), C, 0, N, H, W, C, acc, _st()) == 0
        got = d0.clone()
        assert lib.hpri_maxpool2_bwd_x16(P(x16), 1, xs, 0, P(dy), C, 0, P(got), 0, C, 0, N, H, W, C, acc, _st()) == 0, lib.hpri_last_error()
        d16 = d0.to(torch.bfloat16)
        want16 = d16.float()
        assert lib.hpri_maxpool2_bwd(P(xf), C, 0, P(dy), C, 0, P(want16), C, 0, N, H, W, C, acc, _st()) == 0
        got16 = d16.clone()
        assert lib.hpri_maxpool2_bwd_x16(P(x16), 1, xs, 0, P(dy), C, 0, P(got16), 1, C, 0, N, H, W, C, acc, _st()) == 0
        gotf = d16.clone()                                   # fp32 input of the pool, bf16 gradient rows
        assert lib.hpri_maxpool2_bwd_x16(P(xf), 0, C, 0, P(dy), C, 0, P(gotf), 1, C, 0, N, H, W, C, acc, _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        assert torch.equal(got16, want16.to(torch.bfloat16)) and torch.equal(gotf, got16)
