"""fp32 Winograd weight gradient (csrc/conv_wino.hip: conv_wino_wgrad_kernel), the k-step as the engine launches it.

The k-step reads its operands as 8-byte pairs from ONE per-lane LDS address: lane li of a wave holds input channels 2 li, 2 li + 1
and output channels 2 li, 2 li + 1 of the 64 x 64 block, and the slab is written as channel pairs.  A wrong pairing, a wrong
immediate or a strip that is carried wrongly from unit to unit shows as a wrong gradient, so the whole launch -- hpri_conv_wino_wgrad
plus the reduce, through engine._wgrad -- is compared with an fp64 direct weight gradient on the CPU.  Every launch runs all eight
wave variants (frequency row x column pair).  Shapes: an odd k-step count in the last strip of a strip row (W = 121: 7), a partial
second input-channel block (72 channels) with 7 k-steps (W = 60), and full strips with two output-channel blocks.

Bound: 4e-5 of the largest gradient element, at least 4e-5 -- the one tests/test_gpu_kernels_r2.py and
tests/test_gpu_wino_wgrad_edge.py apply to this kernel.  Both settings of plan option "wgrad_skip_edge" must give the same bits,
and so must two runs of one launch.  Needs a real MI355X: ``-m gpu``."""
import functools

import pytest
import torch

from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPT = b"wgrad_skip_edge"

# (N, H, W, Cin, Cout) -> k-steps of the last strip of a strip row
SHAPES = {(1, 34, 121, 64, 64): 7,
          (2, 36, 60, 72, 64): 7,
          (1, 64, 64, 64, 128): 8}


def _kend(W):
    x0 = 32 * ((W + 31) // 32 - 1)
    return min(8, (W - x0 + 3) // 4)


def _bits(t):
    return t.cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """{option: [dW of run 1, dW of run 2]}, the fp64 reference and the library calls of one launch; computed once per shape."""
    from hyperpri_amd import _lib
    from hyperpri_amd import engine as E
    lib = _lib.load()
    N, H, W, cin, cout = shape
    assert N * H * W >= 4096 and E.WINOGRAD and E.WINO_WGRAD
    torch.manual_seed(100000 * cin + 1000 * W + 10 * H + N)
    x, dy = E.Act.new(N, H, W, cin, DEV), E.Act.new(N, H, W, cout, DEV)
    x.buf.copy_(torch.randn(x.buf.shape, device=DEV))
    dy.buf.copy_(torch.randn(dy.buf.shape, device=DEV))
    assert (x.cs, dy.cs) == (cin, cout)
    calls, real = [], _lib.call

    def spy(name, *args):
        calls.append(name)
        return real(name, *args)

    got = {}
    saved = lib.hpri_get_option(OPT)
    _lib.call = spy
    try:
        for opt in (0, 1):
            assert lib.hpri_set_option(OPT, opt) == 0
            got[opt] = []
            for _ in range(2):
                dw = torch.full((cout, cin, 3, 3), 0.5, device=DEV)
                E._wgrad(x, dy, dw, 0, cin, cout, 3)
                torch.cuda.synchronize()
                got[opt].append(dw)
    finally:
        _lib.call = real
        lib.hpri_set_option(OPT, saved)
    xt = x.buf.reshape(N, H, W, cin).permute(0, 3, 1, 2).double().cpu()
    dt = dy.buf.reshape(N, H, W, cout).permute(0, 3, 1, 2).double().cpu()
    ref = torch.nn.grad.conv2d_weight(xt, (cout, cin, 3, 3), dt, padding=1)
    return got, ref, calls


def test_the_cases_reach_the_paths_they_name():
    for (N, H, W, cin, cout), kend in SHAPES.items():
        assert _kend(W) == kend and N * H * W >= 4096
    assert any(_kend(s[2]) % 2 == 1 for s in SHAPES)                    # an odd trip count
    assert any(s[3] % 64 for s in SHAPES)                               # a partial input-channel block
    assert any(s[4] > 64 for s in SHAPES)                               # two output-channel blocks
    assert any(s[2] % 32 == 0 for s in SHAPES)                          # full strips only


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_winograd_kernel_and_its_reduce_are_what_runs(shape):
    _, _, calls = _case(shape)
    launches = [c for c in calls if "wgrad" in c and not c.endswith("_plan")]
    assert launches == ["hpri_conv_wino_wgrad", "hpri_wino_wgrad_reduce"] * 4, calls       # two options x two runs, no other route


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("opt", [0, 1])
def test_gradient_vs_fp64(shape, opt):
    got, ref, _ = _case(shape)
    N, H, W, cin, cout = shape
    tag = f"wino/wgrad_kstep/{N}x{H}x{W}x{cin}x{cout}/skip_edge_{opt}"
    sc = max(1.0, float(ref.abs().max()))
    err = float((got[opt][0].double().cpu() - ref).abs().max())
    print(f"{tag}: max error {err:.3e}, bound {4e-5 * sc:.3e}")
    record_margin(tag, err, 4e-5 * sc)
    assert err < 4e-5 * sc, (tag, err)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_both_edge_settings_give_the_same_bits(shape):
    got, _, _ = _case(shape)
    assert torch.equal(got[0][0], got[1][0])
    assert _bits(got[0][0]) == _bits(got[1][0])                          # -0 against +0 and NaN payloads included


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("opt", [0, 1])
def test_two_runs_give_the_same_bits(shape, opt):
    got, _, _ = _case(shape)
    assert torch.isfinite(got[opt][0]).all()
    assert _bits(got[opt][0]) == _bits(got[opt][1])
