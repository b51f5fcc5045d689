"""The pixel-reduction weight gradient (csrc/conv_wgrad.hip: hpri_conv_wgrad, hpri_conv_wgrad_bf16 with split 0 / 1 / 2, and the
fixed-order reduce kernels behind hpri_wgrad_reduce) called through the C ABI at the geometries of tests/_direct_cases.py: one
strip, a second strip with one valid column, two images, several (C, N) blocks of 64 (3x3) and 128 (1x1), x_cvalid / dy_cvalid
with 1e3 beyond them, the ConvTranspose2d form (B_S2D gather of dY, (Cin, Cup, 2, 2) destination through both of its reduce
kernels), accumulate 0 / 1, the XCD-aware 1-D grid with empty slabs, and -- for split >= 1 at 3x3 -- the kernel row carried in the
grid (one and three N blocks).

Integer operands inside the 2^24 budget must give the fp64 gradient exactly, whatever the slab order; random operands are held to
the project's gates (tests/test_gpu_kernels_r2.py): fp32 4e-5 * max(1, max|ref|); plain bf16 2e-5 * scale against fp64 of the
bf16-rounded operands; bf16x3 2^-16 * sum|x||dy| per element (the dropped lo*lo term, conv_wgrad.hip) plus the fp32 gate; bf16x6
the fp32 gate.  conv_wgrad_bf16_kernel builds the planes of BOTH operands as pack_weight_bf16_kernel does (plane = bf16(rest);
rest -= plane, LOAD_UNIT), so every operand set of the case module is exact by the kernel's own construction, in either direction.

The workspace starts as NaN: every slab element must have been written before the reduce reads it, and the gradient buffer
is longer than the gradient and must keep its tail.  Needs a real MI355X: ``-m gpu``."""
import ctypes

import pytest
import torch

import _direct_cases as D
from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 16


def P(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    from hyperpri_amd import _lib
    return _lib.load()


def _plan(lib, N, H, W, cin_pad, cout_pad, ks):
    sp, cr, nr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.hpri_wgrad_plan(N, H, W, cin_pad, cout_pad, ks, ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr)) == 0
    return sp.value, cr.value, nr.value


def _operand(rows, coff, data, valid):
    """[rows, coff + valid + 8] buffer: `data` at channel coff, zeros up to the valid count, 1e3 everywhere else."""
    b = torch.full((rows, coff + valid + 8), D.X_PAD_VALUE)
    b[:, coff:coff + valid] = 0.0
    b[:, coff:coff + data.shape[1]] = data
    return b.to(DEV)


def _kernel(lib, kern, xb, x_coff, x_cvalid, db, dy_coff, dy_cvalid, ws, ws_floats, N, H, W, cin_pad, cout_pad, ks, bmode, H2, W2, py0, px0,
            cup):
    if kern == "f32":
        return lib.hpri_conv_wgrad(P(xb), xb.shape[1], x_coff, x_cvalid, P(db), db.shape[1], dy_coff, dy_cvalid, P(ws), ws_floats,
                                   N, H, W, cin_pad, cout_pad, ks, bmode, H2, W2, py0, px0, cup, _st())
    return lib.hpri_conv_wgrad_bf16(P(xb), xb.shape[1], x_coff, x_cvalid, P(db), db.shape[1], dy_coff, dy_cvalid, P(ws), ws_floats,
                                    N, H, W, cin_pad, cout_pad, ks, bmode, H2, W2, py0, px0, cup, D.split_of(kern), _st())


def run_wgrad(lib, kern, x, dy, ks, *, dw0=None, acc=0, x_coff=0, dy_coff=0, convt=None, min_zero_slabs=0):
    """dW of a convolution (convt None: dy [N,H,W,Cout] -> [Cout,Cin,ks,ks]) or of ConvTranspose2d(k2,s2) (convt = the case:
    dy [N,H2,W2,Cup] hi-res -> [Cin,Cup,2,2]); fp64 on the CPU, plus the number of slabs."""
    N, H, W, Cin = x.shape
    npix, cin_pad = N * H * W, D.rup(Cin, 8)
    xb = _operand(npix, x_coff, x.reshape(npix, Cin), cin_pad)
    if convt is None:
        Cout = dy.shape[3]
        dy_cvalid, bmode, H2, W2, py0, px0, cup, dst_mode = D.rup(Cout, 8), 0, 0, 0, 0, 0, 0, 0
        db = _operand(npix, dy_coff, dy.reshape(npix, Cout), dy_cvalid)
        shape = (Cout, Cin, ks, ks)
    else:
        cup = convt["shape"][4]
        H2, W2, py0, px0 = convt["H2"], convt["W2"], convt["py0"], convt["px0"]
        Cout, dy_cvalid, bmode, dst_mode = 4 * cup, 4 * cup, 1, 1
        hb = torch.full((N, H2, W2, dy_coff + cup + 8), D.X_PAD_VALUE)          # 1e3 outside the patch grid and outside the view
        hb[:, py0:py0 + 2 * H, px0:px0 + 2 * W, dy_coff:dy_coff + cup] = D.convt_patch(dy, H, W, py0, px0)
        db = hb.reshape(N * H2 * W2, -1).to(DEV)
        shape = (Cin, cup, 2, 2)
    cout_pad = D.rup(Cout, 64)
    splits, cr, nr = _plan(lib, N, H, W, cin_pad, cout_pad, ks)
    T = ks * ks
    ws = torch.full((splits * T * cr * nr,), D.WS_SENTINEL, device=DEV)
    numel = shape[0] * shape[1] * shape[2] * shape[3]
    dwb = torch.full((numel + TAIL,), D.SENTINEL)
    if acc:
        dwb[:numel] = dw0.reshape(-1)
    dwb = dwb.to(DEV)
    args = (N, H, W, cin_pad, cout_pad, ks, bmode, H2, W2, py0, px0, cup)
    # too small a workspace is an error return and writes nothing
    assert _kernel(lib, kern, xb, x_coff, cin_pad, db, dy_coff, dy_cvalid, ws, ws.numel() - 1, *args) != 0
    torch.cuda.synchronize()
    assert torch.isnan(ws).all()
    rc = _kernel(lib, kern, xb, x_coff, cin_pad, db, dy_coff, dy_cvalid, ws, ws.numel(), *args)
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(ws).all(), "a slab element the reduce reads was not written"
    if min_zero_slabs:
        zero = int((ws.view(splits, -1).abs().amax(1) == 0).sum())
        assert zero >= min_zero_slabs, (zero, min_zero_slabs)
    rc = lib.hpri_wgrad_reduce(P(ws), P(dwb), N, H, W, Cin, cin_pad, Cout, cout_pad, ks, dst_mode, cup, acc, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    out = dwb.cpu()
    assert torch.all(out[numel:] == D.SENTINEL), "the reduce wrote past the gradient"
    return out[:numel].double().reshape(shape), splits


def _opsets(small, wide, third, deep):
    out = [(n, "small", k) for n in small for k in D.KERNS]
    out += [(n, o, k) for n in wide for o in ("a_wide", "b_wide") for k in ("bf16x3", "bf16x6")]
    out += [(n, o, "bf16x6") for n in third for o in ("a_third", "b_third")]
    return out + [(n, o, "bf16x6") for n in deep for o in ("a_deep", "b_deep")]


@pytest.mark.parametrize("name,opset,kern", _opsets(D.WGRAD_CASES, D.WIDE_WGRAD_CASES, D.THIRD_WGRAD_CASES, D.DEEP_WGRAD_CASES))
def test_integer_weight_gradient_equals_fp64(lib, name, opset, kern):
    """accumulate 0, then 1 onto an integer prior; operands as channel slices of wider buffers whose other channels hold 1e3."""
    c = D.WGRAD_CASES[name]
    i = D.wgrad_inputs(name, opset)
    assert D.wgrad_budget(i["x"], i["dy"], c["ks"], i["dw0"]) < D.LIMIT
    ref = D.ref_wgrad(i["x"], i["dy"], c["ks"])
    N, H, W, Cin, Cout = c["shape"]
    dw, splits = run_wgrad(lib, kern, i["x"], i["dy"], c["ks"], x_coff=4, dy_coff=8)
    assert splits > 1 or N * D.cdiv(H, 2) * D.cdiv(W, 32) == 1                      # pixel-split slabs wherever there are two strips
    assert torch.equal(dw, ref), (name, opset, kern, float((dw - ref).abs().max()))
    dw, _ = run_wgrad(lib, kern, i["x"], i["dy"], c["ks"], dw0=i["dw0"], acc=1)
    assert torch.equal(dw, ref + i["dw0"].double()), (name, opset, kern)


def _convt_opsets():
    out = _opsets(D.CONVT_CASES, D.CONVT_CASES, D.THIRD_CONVT_CASES, ())
    return out


@pytest.mark.parametrize("name,opset,kern", _convt_opsets())
def test_integer_transposed_weight_gradient_equals_fp64(lib, name, opset, kern):
    """B_S2D with dst_mode 1: dW[ci][co][tap] of ConvTranspose2d(k2, s2) from the patch grid of the hi-res gradient.  Cup = 32 with
    at most 16 slabs is reduced by wgrad_reduce_convt_kernel, Cup = 8 by the generic kernel (hpri_wgrad_reduce's dispatch)."""
    c = D.CONVT_CASES[name]
    N, H, W, Cin, Cup = c["shape"]
    i = D.convt_inputs(name, opset)
    dyp = D.convt_patch(i["dy_w"], H, W, c["py0"], c["px0"])
    assert D.convt_grad_budgets(i["x"], i["wt"], dyp, dw0=i["dw0"])[1] < D.LIMIT
    _, ref = D.ref_convt_grads(i["x"], i["wt"], dyp)
    dw, splits = run_wgrad(lib, kern, i["x"], i["dy_w"], 1, convt=c, x_coff=4, dy_coff=4)
    assert splits > 1
    if Cup % 16 == 0:
        assert splits <= 16, "this case is meant for wgrad_reduce_convt_kernel"
    assert torch.equal(dw, ref), (name, opset, kern, float((dw - ref).abs().max()))
    dw, _ = run_wgrad(lib, kern, i["x"], i["dy_w"], 1, convt=c, dw0=i["dw0"], acc=1)
    assert torch.equal(dw, ref + i["dw0"].double()), (name, opset, kern)


def _compare_random(kern, tag, dw, ref_of, a, b):
    ref = ref_of(a, b)
    sc = max(1.0, float(ref.abs().max()))
    err = (dw - ref).abs()
    if kern == "f32":
        record_margin(f"direct/wgrad/{tag}", float(err.max()), 4e-5 * sc)
        assert float(err.max()) < 4e-5 * sc, (tag, float(err.max()))
    elif kern == "bf16":
        ref16 = ref_of(a.bfloat16(), b.bfloat16())
        sc16 = max(1.0, float(ref16.abs().max()))
        e16 = float((dw - ref16).abs().max())
        record_margin(f"direct_bf16/wgrad/{tag}", e16, 2e-5 * sc16)
        assert e16 < 2e-5 * sc16, (tag, e16)
    elif kern == "bf16x3":
        bound = ref_of(a.abs(), b.abs()) * 2.0 ** -16 + 4e-5 * sc
        record_margin(f"direct_bf16/x3/wgrad/{tag}", float(err.max()), float(bound.min()))
        assert torch.all(err < bound), (tag, float(err.max()), float((err / bound).max()))
    else:
        record_margin(f"direct_bf16/x6/wgrad/{tag}", float(err.max()), 4e-5 * sc)
        assert float(err.max()) < 4e-5 * sc, (tag, float(err.max()))


@pytest.mark.parametrize("kern", D.KERNS)
@pytest.mark.parametrize("name", D.RANDOM_WGRAD_CASES)
def test_random_weight_gradient_vs_fp64(lib, name, kern):
    c = D.WGRAD_CASES[name]
    i = D.wgrad_inputs(name, random=True)
    dw, _ = run_wgrad(lib, kern, i["x"], i["dy"], c["ks"], x_coff=4)
    _compare_random(kern, f"{kern}/{name}", dw, lambda a, b: D.ref_wgrad(a, b, c["ks"]), i["x"], i["dy"])


@pytest.mark.parametrize("kern", D.KERNS)
@pytest.mark.parametrize("name", ("convt_cup8_off01", "convt_cup32"))
def test_random_transposed_weight_gradient_vs_fp64(lib, name, kern):
    c = D.CONVT_CASES[name]
    N, H, W, Cin, Cup = c["shape"]
    i = D.convt_inputs(name, random=True)
    dw, _ = run_wgrad(lib, kern, i["x"], i["dy_w"], 1, convt=c)
    dyp = D.convt_patch(i["dy_w"], H, W, c["py0"], c["px0"])
    _compare_random(kern, f"{kern}/convt/{name}", dw, lambda a, b: D.ref_convt_grads(a, torch.zeros(Cin, Cup, 2, 2), b)[1], i["x"], dyp)


@pytest.mark.parametrize("kern", D.KERNS)
def test_xcd_grid_with_empty_slabs(lib, kern):
    """Options wgrad_xcd_min_tiles = wgrad_xcd_min_strips = 1: the 1-D grid with 8k pixel splits.  The case has 10 strips, so most
    slabs are empty and must be written as zeros; the integer gradient is still exact and the random one inside the gates."""
    name = D.XCD_WGRAD_CASE
    c = D.WGRAD_CASES[name]
    N, H, W, Cin, Cout = c["shape"]
    strips = N * D.cdiv(H, 2) * D.cdiv(W, 32)
    opts = (b"wgrad_xcd_min_tiles", b"wgrad_xcd_min_strips")
    saved = [lib.hpri_get_option(o) for o in opts]
    i, r = D.wgrad_inputs(name), D.wgrad_inputs(name, random=True)
    assert D.wgrad_budget(i["x"], i["dy"], c["ks"], i["dw0"]) < D.LIMIT
    try:
        for o in opts:
            assert lib.hpri_set_option(o, 1) == 0
        splits, _, _ = _plan(lib, N, H, W, D.rup(Cin, 8), D.rup(Cout, 64), c["ks"])
        assert splits % 8 == 0 and splits > strips
        dw, sp = run_wgrad(lib, kern, i["x"], i["dy"], c["ks"], dw0=i["dw0"], acc=1, min_zero_slabs=splits - strips)
        assert sp == splits
        dwr, _ = run_wgrad(lib, kern, r["x"], r["dy"], c["ks"])
    finally:
        for o, v in zip(opts, saved):
            lib.hpri_set_option(o, v)
    assert [lib.hpri_get_option(o) for o in opts] == saved
    assert torch.equal(dw, D.ref_wgrad(i["x"], i["dy"], c["ks"]) + i["dw0"].double()), kern
    _compare_random(kern, f"{kern}/xcd/{name}", dwr, lambda a, b: D.ref_wgrad(a, b, c["ks"]), r["x"], r["dy"])
