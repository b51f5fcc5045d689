"""fp32 Winograd weight gradient (csrc/conv_wino.hip: conv_wino_wgrad_kernel), the unit boundary as the engine launches it.

A workgroup walks a run of units (strips of 2 rows x 32 columns).  What describes the next unit -- its strip-column class (first,
middle, last: which lane offsets its pieces take), the rows of its halo that lie outside the image (descriptors of zero records),
its two base pointers (carried from unit to unit by one of three constant steps: next strip, next strip row, next image) and its
k-step count -- is prepared one unit ahead, and its pieces are issued between the MFMAs of the current unit's first k-step.  A wrong
class, a wrong step at a wrap, a row that is not zero-filled or a piece that lands in the wrong unit shows as a wrong gradient, so
the whole launch -- hpri_conv_wino_wgrad plus the reduce, through engine._wgrad -- is compared with an fp64 direct weight gradient
on the CPU.  The shapes and what each reaches: SHAPES below; test_the_cases_reach_the_paths_they_name checks them against a mirror
of the launcher's arithmetic.

Bound: 4e-5 of the largest gradient element, at least 4e-5 -- the one tests/test_gpu_wino_wgrad_kstep.py applies to this kernel.
Both settings of plan option "wgrad_skip_edge" must give the same bits, and so must two runs of one launch.  Needs a real
MI355X: ``-m gpu``."""
import functools

import pytest
import torch

from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPT = b"wgrad_skip_edge"

# (N, H, W, Cin, Cout)
SHAPES = [
    (2, 86, 24, 64, 64),     # one strip column, first and last at once; image wrap; borders every 43 strip rows; 86 units = 10 splits of 9, the last clipped
    (1, 116, 36, 64, 64),    # a last strip with ONE k-step: all pieces of the next unit issue inside a one-k-step unit
    (1, 45, 100, 72, 64),    # first, middle and last classes; odd H; a partial second input-channel block; a last strip with one k-step
    (2, 33, 70, 64, 96),     # half-valid second output-channel block; last strip with two k-steps; odd H with two images
]


def _cdiv(a, b):
    return (a + b - 1) // b


def _plan(N, H, W, cin_pad, cout_pad, reserve):
    """hpri_wino_wgrad_plan and the launcher's strip arithmetic (csrc/conv_wino.hip)."""
    cblk, nblk = _cdiv(cin_pad, 64), _cdiv(cout_pad, 64)
    sx, sy = _cdiv(W, 32), _cdiv(H, 2)
    total, tiles = N * sx * sy, cblk * nblk

    def plan(cus, kmax, tol):
        best, best_eff = 1, 0.0
        for k in range(1, kmax + 1):
            if k > 1 and total // k < 8:
                break
            per_cu = tiles * k / cus
            eff = per_cu if per_cu < 1.0 else per_cu / int(per_cu + 0.999999)
            if eff > best_eff + tol + 1e-9:
                best_eff, best = eff, k
        return best

    splits = plan(256, 512, 0.0)
    if reserve > 0:
        splits = plan(256 - min(reserve, 192), 2 * splits, 0.05)
    per_split = _cdiv(total, splits)
    runs = [(s * per_split, min(total, (s + 1) * per_split)) for s in range(splits)]
    kend_last = min(8, (W - 32 * (sx - 1) + 3) // 4)
    return {"strips_x": sx, "strips_y": sy, "total": total, "splits": splits, "per_split": per_split, "runs": runs,
            "kend_last": kend_last, "cblk": cblk, "nblk": nblk}


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
    return got, ref, calls, (x.cw, dy.cw)


def test_the_cases_reach_the_paths_they_name():
    from hyperpri_amd import _lib
    reserve = _lib.load().hpri_get_option(b"wgrad_cu_reserve")
    p = {s: _plan(s[0], s[1], s[2], s[3], _cdiv(s[4], 64) * 64, reserve) for s in SHAPES}
    for s in SHAPES:
        assert s[0] * s[1] * s[2] >= 4096
        assert all(b - a >= 2 for a, b in p[s]["runs"][:-1])               # every split issues a next unit under its MFMAs
    a, b, c, d = SHAPES
    # a: one strip column (first and last at once), 86 units over 10 splits of 9 with the last one clipped, and the wrap from
    # image 0 to image 1 (unit 43: top border behind a bottom border) inside a split, not at its start
    assert p[a]["strips_x"] == 1 and p[a]["strips_y"] == 43 and p[a]["total"] == 86
    assert (p[a]["splits"], p[a]["per_split"]) == (10, 9)
    assert p[a]["runs"][-1] == (81, 86) and 86 - 81 < p[a]["per_split"]
    assert 43 % p[a]["per_split"] != 0
    # b: two strip columns (first, last; no middle), the last strip runs ONE k-step
    assert p[b]["strips_x"] == 2 and p[b]["kend_last"] == 1
    # c: first, middle and last classes; odd H (one valid dY row in the last strip row); 72 input channels = a second, partial
    # input-channel block; the last strip runs one k-step
    assert p[c]["strips_x"] >= 3 and c[1] % 2 == 1 and p[c]["cblk"] == 2 and c[3] % 64 != 0 and p[c]["kend_last"] == 1
    # d: 96 output channels = a half-valid second output-channel block; the last strip runs two k-steps; odd H, two images
    assert p[d]["nblk"] == 2 and d[4] % 64 == 32 and p[d]["kend_last"] == 2 and d[1] % 2 == 1 and d[0] == 2
    assert p[d]["strips_x"] >= 3
    # strip-row wraps and image wraps happen inside splits somewhere in every multi-split shape
    for s in SHAPES:
        sx, sy = p[s]["strips_x"], p[s]["strips_y"]
        starts = {r[0] for r in p[s]["runs"]}
        assert any(u % sx == 0 and u not in starts for u in range(1, p[s]["total"]))
        if s[0] > 1:
            assert any(u % (sx * sy) == 0 and u not in starts for u in range(1, p[s]["total"]))


@pytest.mark.parametrize("shape", SHAPES)
def test_the_winograd_kernel_and_its_reduce_are_what_runs(shape):
    _, _, calls, widths = _case(shape)
    launches = [c for c in calls if "wgrad" in c and not c.endswith("_plan")]
    assert launches == ["hpri_conv_wino_wgrad", "hpri_wino_wgrad_reduce"] * 4, calls       # two options x two runs, no other route
    assert widths == (shape[3], shape[4])                    # the channel widths the mirror of the plan assumes


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("opt", [0, 1])
def test_gradient_vs_fp64(shape, opt):
    got, ref, _, _ = _case(shape)
    N, H, W, cin, cout = shape
    tag = f"wino/wgrad_units/{N}x{H}x{W}x{cin}x{cout}/skip_edge_{opt}"
    sc = max(1.0, float(ref.abs().max()))
    err = float((got[opt][0].double().cpu() - ref).abs().max())
    print(f"{tag}: max error {err:.3e}, bound {4e-5 * sc:.3e}")
    record_margin(tag, err, 4e-5 * sc)
    assert err < 4e-5 * sc, (tag, err)


@pytest.mark.parametrize("shape", SHAPES)
def test_both_edge_settings_give_the_same_bits(shape):
    got, _, _, _ = _case(shape)
    assert torch.equal(got[0][0], got[1][0])
    assert _bits(got[0][0]) == _bits(got[1][0])                          # -0 against +0 and NaN payloads included


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("opt", [0, 1])
def test_two_runs_give_the_same_bits(shape, opt):
    got, _, _, _ = _case(shape)
    assert torch.isfinite(got[opt][0]).all()
    assert _bits(got[opt][0]) == _bits(got[opt][1])
