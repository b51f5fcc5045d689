"""The implicit-GEMM convolution kernels (csrc/conv_fwd.hip: hpri_conv_fwd, hpri_conv_fwd_bf16 with split 0 / 1 / 2,
hpri_splitk_finish, hpri_convt_fwd_bf16_pl) called through the C ABI at the smallest geometries that reach each launch path
(tests/_direct_cases.py): column bands of width 32 / 16 / 8 / 4, both workgroup shapes and the narrow bf16x6 one, split-K with
uneven chunk splits and a partial last chunk, the XCD-aware 1-D grid, channel-slice views, the accumulate / ReLU / statistics
epilogues, the data-gradient form (pack mode 1), the ConvTranspose2d scatter (E_D2S, pack mode 2) and gather (A_S2D, pack mode 3).

Two kinds of comparison:
  * integer operands inside the 2^24 budget (asserted again here): the result must EQUAL the fp64 reference, whatever the summation
    order -- any mis-indexed pixel, tap, channel or K chunk is off by a whole integer;
  * random operands against fp64 under the project's existing gates (tests/test_gpu_kernels_r2.py): fp32 5e-5 * max(1, max|ref|);
    plain bf16 2e-5 * scale against fp64 of the bf16-rounded operands; bf16x3 the bound its comment derives (2^-16 * sum|x||w| per
    element for the dropped lo*lo term) plus the fp32 gate; bf16x6 the fp32 gate.  The bf16x3 / bf16x6 errors against fp64 of the
    unrounded operands are recorded (record_margin: direct_bf16/...) as measurements.

Every buffer is wider than the view and pre-filled: outputs with a sentinel no integer result can equal (channels outside
[coff, coff + y_cw) must keep it, channels [Cout, y_cw) must be exactly 0 -- or unchanged where the call accumulates), inputs with
1e3 outside the view and in the pad channels [Cin, Cin_pad), which meet the packer's zero rows.

Epilogue order (conv_fwd_epilogue.inc, splitk_finish_kernel): v = acc + bias; ReLU (bit 1); THEN y = v + y_prior (bit 0).  So
accumulate = 3 is relu(conv + bias) + y_prior, not relu of the sum.  The statistics are those of v.  Needs a real MI355X."""
import ctypes

import pytest
import torch

import _direct_cases as D
from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def P(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    from hyperpri_amd import _lib
    return _lib.load()


def _plan(lib, kern, N, H, W, cin_pad, cout_pad, ks, amode=0, epi=0):
    k, t, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    if kern == "f32":
        rc = lib.hpri_conv_fwd_plan(N, H, W, cin_pad, cout_pad, ks, amode, epi, ctypes.byref(k), ctypes.byref(t), ctypes.byref(w))
    else:
        rc = lib.hpri_conv_fwd_bf16_plan(N, H, W, cin_pad, cout_pad, ks, amode, epi, D.split_of(kern), ctypes.byref(k), ctypes.byref(t),
                                         ctypes.byref(w))
    assert rc == 0
    return k.value, t.value, w.value


def _pack(lib, kern, w, mode, K, ncols, ncols_pad, T, src_d1, cup=0):
    """The packed panel of `w` for the kernel family; the buffer starts as NaN, so an element the packer skips poisons the result."""
    wd = w.to(DEV).contiguous()
    if kern == "f32":
        wp = torch.full((lib.hpri_packed_weight_floats(K, ncols_pad, T),), NAN, device=DEV)
        rc = lib.hpri_pack_weight(P(wd), P(wp), mode, K, ncols, ncols_pad, T, cup, K, src_d1, _st())
    else:
        split = D.split_of(kern)
        wp = torch.full((D.cdiv(K, 32) * T * (split + 1) * ncols_pad * 32,), NAN, dtype=torch.bfloat16, device=DEV)
        rc = lib.hpri_pack_weight_bf16(P(wd), P(wp), mode, K, ncols, ncols_pad, T, src_d1, cup, split, _st())
    assert rc == 0, lib.hpri_last_error()
    return wp


def _launch(lib, kern, xb, x_cs, x_coff, wp, bias, yb, y_cs, y_coff, stats, N, H, W, cin_pad, cout, cout_pad, y_cw, ks, amode, epi, acc,
            H2, W2, py0, px0, cup, ws, ws_floats):
    if kern == "f32":
        return lib.hpri_conv_fwd(P(xb), x_cs, x_coff, P(wp), P(bias), P(yb), y_cs, y_coff, P(stats), N, H, W, cin_pad, cout, cout_pad, y_cw,
                                 ks, amode, epi, acc, H2, W2, py0, px0, cup, P(ws), ws_floats, _st())
    return lib.hpri_conv_fwd_bf16(P(xb), x_cs, x_coff, P(wp), P(bias), P(yb), y_cs, y_coff, P(stats), N, H, W, cin_pad, cout, cout_pad, y_cw,
                                  ks, amode, epi, acc, H2, W2, py0, px0, cup, D.split_of(kern), P(ws), ws_floats, _st())


def _view(rows, width, coff, data, fill):
    """A [rows, width] buffer of `fill` with `data` ([rows, C]) at channel offset coff."""
    b = torch.full((rows, width), fill)
    b[:, coff:coff + data.shape[1]] = data
    return b.to(DEV)


def run_direct(lib, kern, x, w, bias, *, mode=0, acc=0, y0=None, stats=False, y_cw=None, x_coff=0, y_coff=0):
    """conv (k = 1 | 3, padding k // 2) of x [N,H,W,Cin] with the effective forward weight w [Cout,Cin,k,k]; mode 1 hands the
    packer the layer weight whose data gradient this is (w transposed and rotated by 180 degrees).  Checks the buffer layout and
    returns (y [N*H*W, Cout] fp64, (mean, var, count) or None, ksplit, stat_tiles)."""
    N, H, W, Cin = x.shape
    Cout, _, ks, _ = w.shape
    npix, cin_pad, cout_pad = N * H * W, D.rup(Cin, 8), D.rup(Cout, 64)
    y_cw = D.rup(Cout, 8) if y_cw is None else y_cw
    x_cs, y_cs = x_coff + cin_pad + 4, y_coff + y_cw + 4
    xb = _view(npix, x_cs, x_coff, x.reshape(npix, Cin), D.X_PAD_VALUE)
    if mode == 0:
        wp = _pack(lib, kern, w, 0, Cin, Cout, cout_pad, ks * ks, Cin)
    else:
        wp = _pack(lib, kern, w.permute(1, 0, 2, 3).flip(2, 3), 1, Cin, Cout, cout_pad, ks * ks, Cout)
    yb = torch.full((npix, y_cs), D.SENTINEL)
    if acc & 1:
        yb[:, y_coff:y_coff + y_cw] = 5.0
        yb[:, y_coff:y_coff + Cout] = y0
    yb = yb.to(DEV)
    k, tiles, wsf = _plan(lib, kern, N, H, W, cin_pad, cout_pad, ks)
    ws = torch.full((max(wsf, 4),), NAN, device=DEV)
    st = torch.full((tiles * cout_pad * 4,), D.SENTINEL, device=DEV) if stats else None
    bd = None if bias is None else bias.to(DEV)
    rc = _launch(lib, kern, xb, x_cs, x_coff, wp, bd, yb, y_cs, y_coff, st, N, H, W, cin_pad, Cout, cout_pad, y_cw, ks, 0, 0, acc,
                 0, 0, 0, 0, 0, ws, wsf)
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    full = yb.cpu()
    assert torch.all(full[:, :y_coff] == D.SENTINEL) and torch.all(full[:, y_coff + y_cw:] == D.SENTINEL), "wrote outside the view"
    assert torch.all(full[:, y_coff + Cout:y_coff + y_cw] == (5.0 if acc & 1 else 0.0)), "pad channels [Cout, y_cw)"
    merged = D.chan_merge(st.cpu(), tiles, cout_pad, Cout) if stats else None
    return full[:, y_coff:y_coff + Cout].double(), merged, k, tiles


def _want(ref, acc, y0):
    v = ref.clamp(min=0) if acc & 2 else ref
    return v, (v + y0.double() if acc & 1 else v)


def _check_stats(merged, v, npix, tag):
    mean, var, cnt = merged
    sc = max(1.0, float(v.abs().max()))
    assert torch.all(cnt == npix), tag
    em, ev = float((mean - v.mean(0)).abs().max()), float((var - v.var(0, unbiased=False)).abs().max())
    record_margin(f"{tag}/bn_mean", em, 1e-4 * sc)
    record_margin(f"{tag}/bn_var", ev, 1e-4 * sc * sc)
    assert em < 1e-4 * sc and ev < 1e-4 * sc * sc, (tag, em, ev)


def _assert_reached(name, kern, k, tiles):
    """The fp32 plan shows the path the case was chosen for (the bf16 families have their own workgroup shapes and plans)."""
    c = D.FWD_CASES[name]
    N, H, W, Cin, Cout = c["shape"]
    if kern != "f32":
        return
    if c["ksplit"] is not None:
        assert k == c["ksplit"], (name, k)
    if c["seg"] is not None:
        assert (tiles != D.plain_tiles(N, H, W, D.rup(Cout, 64))) == c["seg"], (name, tiles)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. integer operands, zero tolerance
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", D.KERNS)
@pytest.mark.parametrize("name", list(D.FWD_CASES))
def test_integer_forward_equals_fp64(lib, name, kern):
    """Operand set `small` at every geometry: y = conv + bias with statistics, then y += on an integer prior.  In the three bf16
    plane layouts the lo / mid planes are zero, so this is an indexing test of each."""
    i = D.fwd_inputs(name)
    assert D.fwd_budget(i["x"], i["w"], i["bias"], i["y0"]) < D.LIMIT
    ref = D.ref_conv(i["x"], i["w"], i["bias"])
    y, merged, k, tiles = run_direct(lib, kern, i["x"], i["w"], i["bias"], stats=True)
    _assert_reached(name, kern, k, tiles)
    assert torch.equal(y, ref), (name, kern, float((y - ref).abs().max()))
    _check_stats(merged, ref, ref.shape[0], f"direct/fwd/int/{kern}/{name}")
    y, _, _, _ = run_direct(lib, kern, i["x"], i["w"], i["bias"], acc=1, y0=i["y0"])
    assert torch.equal(y, ref + i["y0"].double()), (name, kern)


def _plane_cases():
    out = [(n, o, k) for n in D.WIDE_FWD_CASES for o in ("a_wide", "b_wide") for k in ("bf16x3", "bf16x6")]
    out += [(n, o, "bf16x6") for n in D.THIRD_FWD_CASES for o in ("a_third", "b_third")]
    return out + [(n, o, "bf16x6") for n in D.DEEP_FWD_CASES for o in ("a_deep", "b_deep")]


@pytest.mark.parametrize("name,opset,kern", _plane_cases())
def test_integer_forward_second_and_third_plane(lib, name, opset, kern):
    """One operand needs hi + lo (bf16x3, bf16x6) resp. hi + mid (+ lo) (bf16x6), the other one plane only, so every product the
    kernels drop is exactly zero and the result must still equal fp64.  The kernel builds the activation planes as the packer
    builds the weight planes (plane = bf16(rest); rest -= plane), hence both directions are exact by construction; the fp32 kernel
    runs the same operands as a control."""
    i = D.fwd_inputs(name, opset)
    assert D.fwd_budget(i["x"], i["w"], i["bias"], i["y0"]) < D.LIMIT
    ref = D.ref_conv(i["x"], i["w"], i["bias"])
    for kk in (kern, "f32"):
        y, _, _, _ = run_direct(lib, kk, i["x"], i["w"], i["bias"], acc=1, y0=i["y0"])
        assert torch.equal(y, ref + i["y0"].double()), (name, opset, kk, float((y - ref - i["y0"].double()).abs().max()))


@pytest.mark.parametrize("kern", D.KERNS)
@pytest.mark.parametrize("name", D.EPILOGUE_CASES)
def test_integer_epilogues_and_channel_slices(lib, name, kern):
    """accumulate 0..3 x bias present / null, input and output as channel slices at non-zero offsets of wider buffers,
    statistics where the call does not accumulate (with split-K they come from hpri_splitk_finish).  The last 12 output channels
    of the geometry are left out, so Cout is no multiple of 4, the plan (a function of Cout_pad) is the same and y_cw = Cout_pad
    exceeds Cout by 12 channels that must come out as zeros."""
    i = D.fwd_inputs(name)
    N, H, W, Cin, Cout = D.FWD_CASES[name]["shape"]
    cout = Cout - 12
    w, y0 = i["w"][:cout], i["y0"][:, :cout]
    for with_bias in (True, False):
        bias = i["bias"][:cout] if with_bias else None
        ref = D.ref_conv(i["x"], w, bias)
        for acc in (0, 1, 2, 3):
            stats = acc in (0, 2)
            y, merged, k, tiles = run_direct(lib, kern, i["x"], w, bias, acc=acc, y0=y0, stats=stats, y_cw=D.rup(Cout, 64), x_coff=8, y_coff=4)
            _assert_reached(name, kern, k, tiles)
            v, want = _want(ref, acc, y0)
            assert torch.equal(y, want), (name, kern, with_bias, acc, float((y - want).abs().max()))
            if stats:
                _check_stats(merged, v, N * H * W, f"direct/fwd/epi/{kern}/{name}/acc{acc}")


@pytest.mark.parametrize("kern", D.KERNS)
@pytest.mark.parametrize("name", D.DGRAD_CASES)
def test_integer_data_gradient_form(lib, name, kern):
    """Pack mode 1: the packer receives the layer weight [K = layer Cout][layer Cin][taps]; the kernel then computes the
    convolution with the transposed, 180-degree rotated weight -- the data gradient."""
    i = D.fwd_inputs(name)
    ref = D.ref_conv(i["x"], i["w"], None)
    y, _, _, _ = run_direct(lib, kern, i["x"], i["w"], None, mode=1)
    assert torch.equal(y, ref), (name, kern)
    # the same through the autograd of conv2d in fp64: dX of the layer whose weight the packer was given
    layer_w = i["w"].permute(1, 0, 2, 3).flip(2, 3).double()
    N, H, W, K = i["x"].shape
    inp = torch.zeros(N, layer_w.shape[1], H, W, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(inp, layer_w, padding=1).backward(i["x"].double().permute(0, 3, 1, 2))
    assert torch.equal(y, inp.grad.permute(0, 2, 3, 1).reshape(N * H * W, -1))


@pytest.mark.parametrize("name", list(D.XCD_FWD_CASES))
def test_xcd_grid_gives_the_same_bits(lib, name):
    """Option conv_nbx_min = 2 turns on the XCD-aware 1-D grid (the tile counts are no multiples of 8: blocks of the last round
    return early).  Block order must not change a bit; integer operands must still equal fp64."""
    c = D.XCD_FWD_CASES[name]
    N, H, W, Cin, Cout = c["shape"]
    opt = b"conv_nbx_min"
    saved = lib.hpri_get_option(opt)
    for kern in D.KERNS:
        k, tiles, _ = _plan(lib, kern, N, H, W, D.rup(Cin, 8), D.rup(Cout, 64), c["ks"])
        assert k == 1 and (tiles % 8 != 0 or kern != "f32"), (name, kern, tiles)      # the 4x1 bf16 kernel has its own tile count
        r, i = D.fwd_inputs(name, random=True), D.fwd_inputs(name)
        assert D.fwd_budget(i["x"], i["w"], i["bias"]) < D.LIMIT
        base = run_direct(lib, kern, r["x"], r["w"], r["bias"], stats=True, acc=2)
        try:
            assert lib.hpri_set_option(opt, 2) == 0
            xcd = run_direct(lib, kern, r["x"], r["w"], r["bias"], stats=True, acc=2)
            yi, _, _, _ = run_direct(lib, kern, i["x"], i["w"], i["bias"])
        finally:
            lib.hpri_set_option(opt, saved)
        assert torch.equal(base[0], xcd[0]) and all(torch.equal(a, b) for a, b in zip(base[1], xcd[1])), (name, kern)
        assert torch.equal(yi, D.ref_conv(i["x"], i["w"], i["bias"])), (name, kern)
    assert lib.hpri_get_option(opt) == saved


# ---------------------------------------------------------------------------------------------------------------------------
# ConvTranspose2d(k=2, s=2): forward = 1x1 GEMM + 2x2 scatter (E_D2S, pack mode 2); data gradient = 2x2 gather (A_S2D, mode 3)
# ---------------------------------------------------------------------------------------------------------------------------
def run_d2s(lib, kern, name, x, wt, bias, x_coff=4, y_coff=4):
    """-> the whole hi-res buffer [N, H2, W2, y_cs] (fp64) and the expected one: sentinel everywhere but channels
    [y_coff, y_coff + Cup) of the patch grid."""
    c = D.CONVT_CASES[name]
    N, H, W, Cin, Cup = c["shape"]
    H2, W2, py0, px0 = c["H2"], c["W2"], c["py0"], c["px0"]
    cin_pad, cout, cout_pad = D.rup(Cin, 8), 4 * Cup, D.rup(4 * Cup, 64)
    x_cs, y_cs = x_coff + cin_pad + 4, y_coff + Cup + 4
    xb = _view(N * H * W, x_cs, x_coff, x.reshape(-1, Cin), D.X_PAD_VALUE)
    wp = _pack(lib, kern, wt, 2, Cin, cout, cout_pad, 1, Cup, Cup)
    yb = torch.full((N * H2 * W2, y_cs), D.SENTINEL, device=DEV)
    k, _, wsf = _plan(lib, kern, N, H, W, cin_pad, cout_pad, 1, 0, 1)
    assert k == 1 and wsf == 0
    rc = _launch(lib, kern, xb, x_cs, x_coff, wp, None if bias is None else bias.to(DEV), yb, y_cs, y_coff, None, N, H, W, cin_pad, cout,
                 cout_pad, cout, 1, 0, 1, 0, H2, W2, py0, px0, Cup, None, 0)
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    return yb.cpu().double().reshape(N, H2, W2, y_cs), (py0, px0, 2 * H, 2 * W, y_coff, Cup)


def _d2s_expected(shape, where, ref):
    py0, px0, h, w, coff, cup = where
    want = torch.full(shape, D.SENTINEL, dtype=torch.float64)
    want[:, py0:py0 + h, px0:px0 + w, coff:coff + cup] = ref
    return want


def _convt_opsets():
    out = [(n, "small", k) for n in D.CONVT_CASES for k in D.KERNS]
    out += [(n, o, k) for n in D.CONVT_CASES for o in ("a_wide", "b_wide") for k in ("bf16x3", "bf16x6")]
    out += [(n, o, "bf16x6") for n in D.THIRD_CONVT_CASES for o in ("a_third", "b_third")]
    return out


@pytest.mark.parametrize("name,opset,kern", _convt_opsets() + [(n, o, "bf16x6") for n in D.DEEP_CONVT_CASES for o in ("a_deep", "b_deep")])
def test_integer_transposed_forward_scatter(lib, name, opset, kern):
    """conv_transpose2d(k=2, s=2) placed at (py0, px0) of the hi-res image: equal to fp64 inside the 2H x 2W patch grid, the
    border and every channel outside the view still the sentinel."""
    i = D.convt_inputs(name, opset)
    assert D.convt_budget(i["x"], i["wt"], i["bias"]) < D.LIMIT
    for bias in (i["bias"], None):
        got, where = run_d2s(lib, kern, name, i["x"], i["wt"], bias)
        want = _d2s_expected(got.shape, where, D.ref_convt(i["x"], i["wt"], bias))
        assert torch.equal(got, want), (name, opset, kern, float((got - want).abs().max()))


def run_s2d(lib, kern, name, dy, wt, acc=0, dx0=None, x_coff=4, y_coff=4):
    """The data gradient of the transposed convolution: dx [N*H*W, Cin] gathered from the hi-res gradient dy [N,H2,W2,Cup]; hi-res
    pixels outside the patch grid and channels outside the view hold 1e3 and must not be read."""
    c = D.CONVT_CASES[name]
    N, H, W, Cin, Cup = c["shape"]
    H2, W2, py0, px0 = c["H2"], c["W2"], c["py0"], c["px0"]
    cout_pad, y_cw = D.rup(Cin, 64), D.rup(Cin, 8)
    x_cs, y_cs = x_coff + Cup + 4, y_coff + y_cw + 4
    src = torch.full((N, H2, W2, x_cs), D.X_PAD_VALUE)
    src[:, py0:py0 + 2 * H, px0:px0 + 2 * W, x_coff:x_coff + Cup] = D.convt_patch(dy, H, W, py0, px0)
    xb = src.reshape(-1, x_cs).to(DEV)
    wp = _pack(lib, kern, wt, 3, 4 * Cup, Cin, cout_pad, 1, Cup, Cup)
    yb = torch.full((N * H * W, y_cs), D.SENTINEL)
    if acc & 1:
        yb[:, y_coff:y_coff + y_cw] = 5.0
        yb[:, y_coff:y_coff + Cin] = dx0
    yb = yb.to(DEV)
    k, _, wsf = _plan(lib, kern, N, H, W, 4 * Cup, cout_pad, 1, 1, 0)
    ws = torch.full((max(wsf, 4),), NAN, device=DEV)
    rc = _launch(lib, kern, xb, x_cs, x_coff, wp, None, yb, y_cs, y_coff, None, N, H, W, 4 * Cup, Cin, cout_pad, y_cw, 1, 1, 0, acc,
                 H2, W2, py0, px0, Cup, ws, wsf)
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    full = yb.cpu()
    assert torch.all(full[:, :y_coff] == D.SENTINEL) and torch.all(full[:, y_coff + y_cw:] == D.SENTINEL)
    assert torch.all(full[:, y_coff + Cin:y_coff + y_cw] == (5.0 if acc & 1 else 0.0))
    return full[:, y_coff:y_coff + Cin].double()


@pytest.mark.parametrize("name,opset,kern", _convt_opsets())
def test_integer_transposed_data_gradient_gather(lib, name, opset, kern):
    """Reference: the autograd of conv_transpose2d in fp64, fed the patch grid of the hi-res gradient; then accumulating."""
    c = D.CONVT_CASES[name]
    N, H, W, Cin, Cup = c["shape"]
    i = D.convt_inputs(name, opset)
    dyp = D.convt_patch(i["dy_d"], H, W, c["py0"], c["px0"])
    assert D.convt_grad_budgets(i["x"], i["wt"], dyp, dx0=i["dx0"])[0] < D.LIMIT
    ref, _ = D.ref_convt_grads(i["x"], i["wt"], dyp)
    got = run_s2d(lib, kern, name, i["dy_d"], i["wt"])
    assert torch.equal(got, ref), (name, opset, kern, float((got - ref).abs().max()))
    got = run_s2d(lib, kern, name, i["dy_d"], i["wt"], acc=1, dx0=i["dx0"])
    assert torch.equal(got, ref + i["dx0"].double()), (name, opset, kern)


@pytest.mark.parametrize("name", list(D.CONVT_CASES))
def test_transposed_forward_bf16_plane_output(lib, name):
    """hpri_convt_fwd_bf16_pl: the bf16 plane is the rounding of the very fp32 value the call also writes; without the fp32 view it
    is the same plane.  Random operands, so the rounding matters; the fp32 result against fp64 of the bf16-rounded operands
    under the existing 2e-5 gate."""
    c = D.CONVT_CASES[name]
    N, H, W, Cin, Cup = c["shape"]
    H2, W2, py0, px0 = c["H2"], c["W2"], c["py0"], c["px0"]
    i = D.convt_inputs(name, random=True)
    cin_pad, cout, cout_pad = D.rup(Cin, 8), 4 * Cup, D.rup(4 * Cup, 64)
    x_coff, y_coff, pl_coff = 4, 4, 8
    x_cs, y_cs, pl_cs = x_coff + cin_pad + 4, y_coff + Cup + 4, pl_coff + Cup + 8
    xb = _view(N * H * W, x_cs, x_coff, i["x"].reshape(-1, Cin), D.X_PAD_VALUE)
    wp = _pack(lib, "bf16", i["wt"], 2, Cin, cout, cout_pad, 1, Cup, Cup)
    bias = i["bias"].to(DEV)
    planes = []
    for with_y in (True, False):
        yb = torch.full((N * H2 * W2, y_cs), D.SENTINEL, device=DEV)
        pl = torch.full((N * H2 * W2, pl_cs), D.SENTINEL, dtype=torch.bfloat16, device=DEV)
        rc = lib.hpri_convt_fwd_bf16_pl(P(xb), x_cs, x_coff, P(wp), P(bias), P(yb if with_y else None), y_cs, y_coff, N, H, W, cin_pad, cout,
                                        cout_pad, H2, W2, py0, px0, Cup, P(pl), pl_cs, pl_coff, _st())
        assert rc == 0, lib.hpri_last_error()
        torch.cuda.synchronize()
        planes.append(pl.cpu().reshape(N, H2, W2, pl_cs))
        if with_y:
            y = yb.cpu().reshape(N, H2, W2, y_cs)
    want_pl = torch.full((N, H2, W2, pl_cs), D.SENTINEL, dtype=torch.bfloat16)
    want_pl[:, py0:py0 + 2 * H, px0:px0 + 2 * W, pl_coff:pl_coff + Cup] = y[:, py0:py0 + 2 * H, px0:px0 + 2 * W, y_coff:y_coff + Cup].bfloat16()
    assert torch.equal(planes[0], want_pl) and torch.equal(planes[1], want_pl)
    ref = D.ref_convt(i["x"].bfloat16(), i["wt"].bfloat16(), i["bias"])
    want = _d2s_expected(y.shape, (py0, px0, 2 * H, 2 * W, y_coff, Cup), ref)
    sc = max(1.0, float(ref.abs().max()))
    err = float((y.double() - want).abs().max())
    record_margin(f"direct_bf16/convt_fwd_pl/{name}", err, 2e-5 * sc)
    assert err < 2e-5 * sc


# ---------------------------------------------------------------------------------------------------------------------------
# 2. random operands against fp64 under the project's gates
# ---------------------------------------------------------------------------------------------------------------------------
def _compare_random(kern, tag, got, ref_of, a, b, bias_ref):
    """ref_of(a, b) -> fp64 result without bias; bias_ref is added (None or a broadcastable tensor).  Asserts the family's gate."""
    add = 0.0 if bias_ref is None else bias_ref
    ref = ref_of(a, b) + add
    sc = max(1.0, float(ref.abs().max()))
    err = (got - ref).abs()
    if kern == "f32":
        record_margin(f"direct/fwd/{tag}", float(err.max()), 5e-5 * sc)
        assert float(err.max()) < 5e-5 * sc, (tag, float(err.max()))
    elif kern == "bf16":
        ref16 = ref_of(a.bfloat16(), b.bfloat16()) + add
        sc16 = max(1.0, float(ref16.abs().max()))
        e16 = float((got - ref16).abs().max())
        record_margin(f"direct_bf16/fwd/{tag}", e16, 2e-5 * sc16)
        assert e16 < 2e-5 * sc16, (tag, e16)
    elif kern == "bf16x3":
        bound = ref_of(a.abs(), b.abs()) * 2.0 ** -16 + 5e-5 * sc       # the dropped lo*lo term, per element, plus the fp32 gate
        record_margin(f"direct_bf16/x3/fwd/{tag}", float(err.max()), float(bound.min()))
        assert torch.all(err < bound), (tag, float(err.max()), float((err / bound).max()))
    else:
        record_margin(f"direct_bf16/x6/fwd/{tag}", float(err.max()), 5e-5 * sc)
        assert float(err.max()) < 5e-5 * sc, (tag, float(err.max()))
    return ref


@pytest.mark.parametrize("kern", D.KERNS)
@pytest.mark.parametrize("name", D.RANDOM_FWD_CASES)
def test_random_forward_vs_fp64(lib, name, kern):
    """randn activations, 0.1 * randn weights; forward with bias and BatchNorm partial statistics."""
    i = D.fwd_inputs(name, random=True)
    y, merged, k, tiles = run_direct(lib, kern, i["x"], i["w"], i["bias"], stats=True, x_coff=4, y_coff=8)
    _assert_reached(name, kern, k, tiles)
    ref = _compare_random(kern, f"{kern}/{name}", y, lambda a, b: D.ref_conv(a, b), i["x"], i["w"], i["bias"].double())
    if kern == "bf16":
        ref = D.ref_conv(i["x"].bfloat16(), i["w"].bfloat16(), i["bias"])
    mean, var, cnt = merged
    sc = max(1.0, float(ref.abs().max()))
    assert torch.all(cnt == ref.shape[0])
    if kern in ("f32", "bf16", "bf16x6"):          # bf16x3 has no statistics gate of its own: its values are not fp32-accurate
        em, ev = float((mean - ref.mean(0)).abs().max()), float((var - ref.var(0, unbiased=False)).abs().max())
        record_margin(f"direct/fwd/{kern}/{name}/bn_mean", em, 1e-4 * sc)
        record_margin(f"direct/fwd/{kern}/{name}/bn_var", ev, 1e-4 * sc * sc)
        assert em < 1e-4 * sc and ev < 1e-4 * sc * sc, (name, kern, em, ev)


@pytest.mark.parametrize("kern", D.KERNS)
@pytest.mark.parametrize("name", D.DGRAD_CASES)
def test_random_data_gradient_vs_fp64(lib, name, kern):
    i = D.fwd_inputs(name, random=True)
    y, _, _, _ = run_direct(lib, kern, i["x"], i["w"], None, mode=1)
    _compare_random(kern, f"{kern}/dgrad/{name}", y, lambda a, b: D.ref_conv(a, b), i["x"], i["w"], None)


@pytest.mark.parametrize("kern", D.KERNS)
@pytest.mark.parametrize("name", ("convt_cup8_off10", "convt_cup32"))
def test_random_transposed_forward_and_data_gradient_vs_fp64(lib, name, kern):
    c = D.CONVT_CASES[name]
    N, H, W, Cin, Cup = c["shape"]
    i = D.convt_inputs(name, random=True)
    got, where = run_d2s(lib, kern, name, i["x"], i["wt"], i["bias"])
    py0, px0, h, w, coff, cup = where
    _compare_random(kern, f"{kern}/convt_fwd/{name}", got[:, py0:py0 + h, px0:px0 + w, coff:coff + cup],
                    lambda a, b: D.ref_convt(a, b), i["x"], i["wt"], i["bias"].double())
    dyp = D.convt_patch(i["dy_d"], H, W, c["py0"], c["px0"])
    dx = run_s2d(lib, kern, name, i["dy_d"], i["wt"])
    _compare_random(kern, f"{kern}/convt_dgrad/{name}", dx, lambda a, b: D.ref_convt_grads(torch.zeros(N, H, W, Cin), b, a)[0],
                    dyp, i["wt"], None)


# ---------------------------------------------------------------------------------------------------------------------------
# error returns: a non-zero code and nothing written
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", ("f32", "bf16"))
def test_error_returns_write_nothing(lib, kern):
    name = "splitk3_2x2_bands_8_4"
    N, H, W, Cin, Cout = D.FWD_CASES[name]["shape"]
    i = D.fwd_inputs(name)
    cin_pad, cout_pad = D.rup(Cin, 8), D.rup(Cout, 64)
    xb = _view(N * H * W, cin_pad + 8, 0, i["x"].reshape(-1, Cin), 0.0)
    wp = _pack(lib, kern, i["w"], 0, Cin, Cout, cout_pad, 9, Cin)
    k, tiles, wsf = _plan(lib, kern, N, H, W, cin_pad, cout_pad, 3)
    assert k > 1
    ws = torch.full((wsf,), D.WS_SENTINEL, device=DEV)
    yb = torch.full((4 * N * H * W, Cout + 8), D.SENTINEL, device=DEV)        # big enough for the hi-res forms below
    st = torch.full((tiles * cout_pad * 4,), D.SENTINEL, device=DEV)

    def call(x_cs=cin_pad + 8, cout_pad_=cout_pad, ws_floats=wsf, ks=3, epi=0, stats=None, H2=0, W2=0, cup=0, cout=Cout, y_cw=None):
        return _launch(lib, kern, xb, x_cs, 0, wp, None, yb, Cout + 8, 0, stats, N, H, W, cin_pad, cout, cout_pad_, y_cw or cout, ks, 0, epi,
                       0, H2, W2, 0, 0, cup, ws, ws_floats)

    assert call(ws_floats=wsf - 1) != 0 and b"workspace" in lib.hpri_last_error()      # too small a split-K workspace
    assert call(cout=Cout - 8, y_cw=cout_pad + 8) != 0 and b"y_cw" in lib.hpri_last_error()   # more channels than the grid covers
    assert call(cout_pad_=160) != 0                                                     # Cout_pad not a multiple of 64
    assert call(x_cs=cin_pad + 6) != 0                                                  # x_cs not a multiple of 4
    cup = 16
    assert call(ks=1, epi=1, H2=2 * H - 1, W2=2 * W, cup=cup, cout=4 * cup, cout_pad_=64) != 0    # patch grid exceeds the hi-res image
    assert call(ks=1, epi=1, H2=2 * H, W2=2 * W, cup=cup, cout=4 * cup, cout_pad_=64, stats=st) != 0   # statistics with D2S
    torch.cuda.synchronize()
    assert torch.all(yb == D.SENTINEL) and torch.all(st == D.SENTINEL) and torch.isnan(ws).all()
