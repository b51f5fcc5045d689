"""fp32 Winograd weight gradient (csrc/conv_wino.hip: conv_wino_wgrad_kernel) at the right image edge.  The last 32-column strip of
a strip row hangs over the edge; with plan option "wgrad_skip_edge" = 1 (the default) the kernel runs only the MFMA k-steps that
hold a pixel column of the image, kend = min(8, ceil((W - x0) / 4)), with 0 all 8.  The left-out k-steps multiply by zero-filled
dY, so both settings must give the same BITS -- slabs and reduced gradient -- and the gradient must match fp64 as before.

Called through the C ABI like tests/test_gpu_kernels_r2.py, one 64 x 64 (cin, cout) tile; the fp64 bound (4e-5 of the largest
gradient element, at least 4e-5) is the one that file applies to this entry point.  Needs a real MI355X: ``-m gpu``."""
import ctypes
import functools

import pytest
import torch

from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPT = b"wgrad_skip_edge"

# (N, H, W) -> k-steps of the last strip of a strip row
SHAPES = {(1, 6, 33): 1,      # one valid column
          (1, 6, 36): 1,      # one k-step exactly full
          (1, 6, 37): 2,
          (2, 5, 61): 8,      # 29 valid columns: nothing to skip; odd H, two images
          (1, 4, 57): 7,      # odd
          (1, 4, 64): 8,      # no overhang
          (1, 4, 121): 7,     # the benched 76 x 121 level
          (1, 2, 2): 1}       # a single strip
MUST_SKIP = [(1, 6, 33), (1, 6, 36), (1, 4, 57), (1, 4, 121)]


def P(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _kend(W):
    strips_x = (W + 31) // 32
    x0 = 32 * (strips_x - 1)
    return min(8, (W - x0 + 3) // 4)


def _run(lib, opt, x, dy, N, H, W, cin, cout, x_cvalid, dw0, accumulate):
    """One weight gradient with the option at `opt`: (raw slab workspace, reduced OIHW gradient)."""
    cs, cso = x.shape[1], dy.shape[1]
    sp, cr, nr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib.hpri_wino_wgrad_plan(N, H, W, 64, 64, ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr))
    assert (cr.value, nr.value) == (64, 64)
    ws = torch.full((sp.value * 16 * 64 * 64,), 3.0, device=DEV)
    dw = dw0.clone()
    saved = lib.hpri_get_option(OPT)
    try:
        assert lib.hpri_set_option(OPT, opt) == 0
        rc = lib.hpri_conv_wino_wgrad(P(x), cs, 0, x_cvalid, P(dy), cso, 0, cso, P(ws), ws.numel(), N, H, W, 64, 64, _st())
        assert rc == 0, lib.hpri_last_error()
        assert lib.hpri_wino_wgrad_reduce(P(ws), P(dw), N, H, W, cin, 64, cout, 64, accumulate, _st()) == 0
        torch.cuda.synchronize()
    finally:
        lib.hpri_set_option(OPT, saved)
    return ws, dw


@functools.lru_cache(maxsize=None)
def _case(shape, cin=64, accumulate=0):
    """Inputs, both arms and the fp64 reference of one shape, computed once.  cin < 64: the channels from the next multiple of 4
    on (the entry point takes valid counts in multiples of 4) hold values the kernel must not read."""
    from hyperpri_amd import _lib
    lib = _lib.load()
    N, H, W = shape
    torch.manual_seed(1000 * W + 10 * H + N)
    x = torch.randn(N * H * W, 64, device=DEV)
    x_cvalid = (cin + 3) // 4 * 4
    x[:, cin:x_cvalid] = 0.0
    x[:, x_cvalid:] = 1.0e3
    dy = torch.randn(N * H * W, 64, device=DEV)
    dw0 = torch.randn(64, cin, 3, 3, device=DEV) if accumulate else torch.full((64, cin, 3, 3), 0.5, device=DEV)
    off = _run(lib, 0, x, dy, N, H, W, cin, 64, x_cvalid, dw0, accumulate)
    on = _run(lib, 1, x, dy, N, H, W, cin, 64, x_cvalid, dw0, accumulate)
    xt = x[:, :cin].reshape(N, H, W, cin).permute(0, 3, 1, 2).double().cpu()
    dt = dy.reshape(N, H, W, 64).permute(0, 3, 1, 2).double().cpu()
    ref = torch.nn.grad.conv2d_weight(xt, (64, cin, 3, 3), dt, padding=1)
    if accumulate:
        ref = ref + dw0.double().cpu()
    return off, on, ref


def _assert_same_bits(off, on):
    for a, b in zip(off, on):
        assert torch.equal(a, b)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()          # -0 against +0 and NaN payloads included


def _assert_close(tag, dw, ref):
    sc = max(1.0, float(ref.abs().max()))
    err = float((dw.double().cpu() - ref).abs().max())
    print(f"{tag}: max error {err:.3e}, bound {4e-5 * sc:.3e}")
    record_margin(tag, err, 4e-5 * sc)
    assert err < 4e-5 * sc, (tag, err)


def test_plan_arithmetic_of_the_cases():
    """The cases do reach the skip: from the strip geometry, k-steps of the last strip as listed, fewer than 8 where it matters."""
    for (N, H, W), kend in SHAPES.items():
        assert _kend(W) == kend, (W, _kend(W))
    for shape in MUST_SKIP:
        assert _kend(shape[2]) < 8
    assert [_kend(w) for w in (968, 484, 242, 121, 60)] == [2, 1, 5, 7, 7]      # the benched levels


@pytest.mark.parametrize("shape", list(SHAPES))
def test_skip_gives_the_same_bits(shape):
    off, on, _ = _case(shape)
    if shape in MUST_SKIP:
        assert _kend(shape[2]) < 8
    assert torch.isfinite(on[0]).all() and not torch.any(on[0] == 3.0)          # every slab element was written
    _assert_same_bits(off, on)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_gradient_vs_fp64(shape):
    _, on, ref = _case(shape)
    N, H, W = shape
    _assert_close(f"wino/wgrad_edge/{N}x{H}x{W}", on[1], ref)


def test_partly_valid_input_channels():
    """46 input channels of the 64-channel tile: x_cvalid = 48, the channels beyond hold 1e3 and must not be read."""
    off, on, ref = _case((1, 4, 57), cin=46)
    _assert_same_bits(off, on)
    _assert_close("wino/wgrad_edge/1x4x57/cin46", on[1], ref)


def test_accumulate_into_a_filled_gradient():
    off, on, ref = _case((1, 4, 121), accumulate=1)
    _assert_same_bits(off, on)
    _assert_close("wino/wgrad_edge/1x4x121/accumulate", on[1], ref)
