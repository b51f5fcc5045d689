"""fp32 Winograd convolution (csrc/conv_wino4.hip: conv_wino4_kernel), its two epilogues.

A workgroup whose 16 x 8 pixels lie inside the image and whose 64 channels are all written takes, in a launch without ReLU and
accumulate, an epilogue without selects and with one address per thread (plan option "wino4_fast_epilogue" = 1, the default); every
other workgroup, and every workgroup with the option at 0, takes the general one.  Both add the same numbers in the same order:
for every case hpri_conv_wino4 (plain | with statistics | accumulate | ReLU) and hpri_conv_wino4_bnred (bn_relu 0 | 1) must give
the same bits of y, of the statistics records and of the partial sums with the option at 1 and at 0, and agree with an fp64 conv2d
on the CPU within the margins tests/test_gpu_kernels_r2.py applies to this kernel: 5e-5 x scale on outputs, 1e-4 on mean and
variance.  The partial sums are also held against fp64 sums of the kernel's own g: 8 pixels per thread, 16 thread rows and up to
three roundings per term, (8 + 16 + 4) x 2^-24 of the summed magnitudes (the bound of tests/test_gpu_bn_kernels.py).
Needs a real MI355X: ``-m gpu``."""
import ctypes
import functools

import pytest
import torch

from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPT = b"wino4_fast_epilogue"
U = 2.0 ** -24

# (N, H, W, Cin, Cout)
SHAPES = [(1, 24, 48, 64, 64),       # 3 x 3 tiles, all interior, two full chunks
          (1, 17, 33, 40, 64),       # interior, right-edge, bottom-edge and corner tiles in one launch; tail chunk
          (2, 8, 16, 8, 128),        # one tile per image, one stage, two channel blocks
          (1, 16, 32, 72, 40),       # channel mask on the only block; three chunks, the last partial
          (1, 9, 17, 16, 320)]       # five channel blocks, the plain (unbanded) item order
VIEW = (1, 17, 33, 40, 64)           # the second shape once more, as channel slices of wider buffers
CASES = [(s, False) for s in SHAPES] + [(VIEW, True)]
FWD = {"plain": (0, False), "stats": (0, True), "accumulate": (1, False), "relu": (2, True)}       # accumulate argument, statistics
IDS = ["x".join(map(str, s)) + ("-view" if v else "") for s, v in CASES]


def rup(x, m):
    return (x + m - 1) // m * m


def P(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.cpu().numpy().tobytes()


def fast_workgroups(shape, view, config):
    """(workgroups that qualify for the fast epilogue, all workgroups) of one launch: the kernel's own conditions."""
    N, H, W, Cin, Cout = shape
    y_cw = _geometry(shape, view)["ycw"]
    if config in ("accumulate", "relu"):
        full_tiles = 0
    else:
        full_tiles = N * (H // 8) * (W // 16)
    full_blocks = sum(1 for nb in range(rup(Cout, 64) // 64) if nb * 64 + 64 <= min(Cout, y_cw))
    return full_tiles * full_blocks, N * -(-H // 8) * -(-W // 16) * (rup(Cout, 64) // 64)


def _geometry(shape, view):
    N, H, W, Cin, Cout = shape
    cinp, cp = rup(Cin, 8), rup(Cout, 64)
    if view:
        return dict(cinp=cinp, cp=cp, xcs=cinp + 16, xoff=8, ycs=136, yoff=64, ycw=Cout, bcs=cp + 8, boff=8)
    return dict(cinp=cinp, cp=cp, xcs=cinp, xoff=0, ycs=rup(Cout, 8), yoff=0, ycw=rup(Cout, 8), bcs=cp, boff=0)


def _chan_stats(stats, tiles, cout_pad, cout):
    """Per-tile (mean, M2, count) records -> per-channel mean and biased variance (Chan merge in fp64)."""
    s = stats.view(tiles, cout_pad, 4).double().cpu()
    n = s[:, :, 2]
    mean = (s[:, :, 0] * n).sum(0) / n.sum(0)
    m2 = (s[:, :, 1] + n * (s[:, :, 0] - mean) ** 2).sum(0)
    return mean[:cout], (m2 / n.sum(0))[:cout], n.sum(0)[:cout]


@functools.lru_cache(maxsize=None)
def _case(shape, view):
    """Every launch of one case with the option at 0 and at 1, and the fp64 references; computed once."""
    from hyperpri_amd import _lib
    lib = _lib.load()
    N, H, W, Cin, Cout = shape
    g = _geometry(shape, view)
    npx = N * H * W
    torch.manual_seed(1000 * W + 10 * H + Cin + (7 if view else 0))
    xb = torch.randn(npx, g["xcs"], device=DEV)
    xb[:, g["xoff"] + Cin:g["xoff"] + g["cinp"]] = 0                        # channels [Cin, Cin_pad) of the view are zero
    xt = xb[:, g["xoff"]:g["xoff"] + Cin].reshape(N, H, W, Cin).permute(0, 3, 1, 2).double().cpu()
    w0 = torch.randn(Cout, Cin, 3, 3, device=DEV) * 0.1                     # forward
    w1 = torch.randn(Cin, Cout, 3, 3, device=DEV) * 0.1                     # data gradient: K = Cin rows of dY, C = Cout columns
    bias = torch.randn(Cout, device=DEV)
    up0 = torch.empty(lib.hpri_wino_packed_floats(Cin, g["cp"]), device=DEV)
    up1 = torch.empty(lib.hpri_wino_packed_floats(Cin, g["cp"]), device=DEV)
    assert lib.hpri_wino4_pack(P(w0), P(up0), P(None), 0, Cin, Cout, g["cp"], Cin, _st()) == 0
    assert lib.hpri_wino4_pack(P(w1), P(up1), P(None), 1, Cin, Cout, g["cp"], Cout, _st()) == 0
    ref = {"fwd": torch.nn.functional.conv2d(xt, w0.double().cpu(), bias.double().cpu(), padding=1).permute(0, 2, 3, 1).reshape(-1, Cout),
           "dgrad": torch.nn.functional.conv2d(xt, w1.double().cpu().permute(1, 0, 2, 3).flip(2, 3), None, padding=1)
           .permute(0, 2, 3, 1).reshape(-1, Cout)}
    # the BatchNorm + ReLU stage of the data gradient: its pre-BN tensor stays 0.25 / invstd away from the mean and |gamma| >= 0.5,
    # so the sign of BN(x) -- the ReLU mask -- does not hang on a rounding
    mean = torch.randn(Cout, device=DEV)
    invstd = torch.rand(Cout, device=DEV) + 0.5
    gamma = (torch.rand(Cout, device=DEV) + 0.5) * torch.where(torch.rand(Cout, device=DEV) < 0.5, -1.0, 1.0)
    scale = gamma * invstd
    shift = 0.0 - mean * scale
    side = torch.where(torch.rand(npx, Cout, device=DEV) < 0.5, -1.0, 1.0)
    bnx = torch.randn(npx, g["bcs"], device=DEV)
    bnx[:, g["boff"]:g["boff"] + Cout] = mean + side * (0.25 + torch.randn(npx, Cout, device=DEV).abs()) / invstd
    tl = ctypes.c_int()
    lib.hpri_conv_wino4_plan(N, H, W, ctypes.byref(tl))
    tiles = tl.value
    got = {}
    saved = lib.hpri_get_option(OPT)
    try:
        for opt in (0, 1):
            assert lib.hpri_set_option(OPT, opt) == 0
            for name, (acc, with_stats) in FWD.items():
                y = torch.full((npx, g["ycs"]), 0.25, device=DEV)
                stats = torch.full((tiles * g["cp"] * 4,), float("nan"), device=DEV) if with_stats else None
                rc = lib.hpri_conv_wino4(P(xb), g["xcs"], g["xoff"], P(up0), P(bias), P(y), g["ycs"], g["yoff"], P(stats), N, H, W, g["cinp"],
                                         Cout, g["cp"], g["ycw"], acc, _st())
                assert rc == 0, lib.hpri_last_error()
                got[(opt, name)] = (y, stats)
            for relu in (0, 1):
                y = torch.full((npx, g["ycs"]), 0.25, device=DEV)
                part = torch.full((tiles, 2, g["cp"]), float("nan"), device=DEV)
                rc = lib.hpri_conv_wino4_bnred(P(xb), g["xcs"], g["xoff"], P(up1), P(y), g["ycs"], g["yoff"], N, H, W, g["cinp"], Cout, g["cp"],
                                               g["ycw"], P(bnx), g["bcs"], g["boff"], P(mean), P(invstd), P(scale), P(shift), relu, P(part),
                                               g["cp"], _st())
                assert rc == 0, lib.hpri_last_error()
                got[(opt, f"bnred{relu}")] = (y, part)
        torch.cuda.synchronize()
    finally:
        lib.hpri_set_option(OPT, saved)
    bn = dict(x=bnx[:, g["boff"]:g["boff"] + Cout].double().cpu(), mean=mean.double().cpu(), invstd=invstd.double().cpu(),
              mask=(side * gamma.sign() > 0).double().cpu())
    return got, ref, bn, tiles, g


CONFIGS = list(FWD) + ["bnred0", "bnred1"]


def test_the_cases_reach_the_paths_they_name():
    f = {(s, v, c): fast_workgroups(s, v, c) for s, v in CASES for c in ("plain", "accumulate", "relu")}
    assert f[(SHAPES[0], False, "plain")] == (9, 9)                          # all interior
    assert f[(SHAPES[1], False, "plain")] == (4, 9)                          # 2 x 2 interior tiles, 2 + 2 edge tiles, 1 corner
    assert f[(SHAPES[2], False, "plain")] == (4, 4)                          # two channel blocks, both full
    assert f[(SHAPES[3], False, "plain")] == (0, 4)                          # 40 of 64 channels: the general epilogue everywhere
    assert f[(SHAPES[4], False, "plain")] == (5, 20) and rup(320, 64) // 64 > 4      # more than four blocks: the plain item order
    assert f[(VIEW, True, "plain")] == (4, 9)
    assert all(f[(s, v, c)][0] == 0 for s, v in CASES for c in ("accumulate", "relu"))
    assert SHAPES[1][3] % 32 and SHAPES[3][3] % 32 and SHAPES[3][3] > 64                # tail chunks; three chunks
    g = _geometry(VIEW, True)
    assert g["xoff"] and g["yoff"] and g["boff"] and g["ycw"] + g["yoff"] < g["ycs"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("config", CONFIGS)
def test_both_epilogues_give_the_same_bits(case, config):
    got, _, _, _, _ = _case(*case)
    (y0, s0), (y1, s1) = got[(0, config)], got[(1, config)]
    assert _bits(y0) == _bits(y1), "y"                                      # -0 against +0 and NaN payloads included
    if s0 is not None:
        assert _bits(s0) == _bits(s1), "statistics records" if config in FWD else "partial sums"


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("opt", [0, 1])
@pytest.mark.parametrize("config", CONFIGS)
def test_output_and_statistics_vs_fp64(case, opt, config):
    got, ref, _, tiles, g = _case(*case)
    shape, view = case
    N, H, W, Cin, Cout = shape
    y, stats = got[(opt, config)]
    want = ref["fwd"] if config in FWD else ref["dgrad"]
    if config == "relu":
        want = want.clamp(min=0)
    if config == "accumulate":
        want = want + 0.25
    tag = f"wino4_lean/{IDS[CASES.index(case)]}/{config}/fast_{opt}"
    out = y[:, g["yoff"]:g["yoff"] + Cout].double().cpu()
    scale = max(1.0, float(want.abs().max()))
    err = float((out - want).abs().max())
    print(f"{tag}: max error {err:.3e}, bound {5e-5 * scale:.3e}")
    record_margin(tag, err, 5e-5 * scale)
    assert err < 5e-5 * scale, (tag, err)
    # outside the written channels: untouched, or (pad channels inside the written width) zero-filled
    assert torch.all(y[:, :g["yoff"]] == 0.25) and torch.all(y[:, g["yoff"] + g["ycw"]:] == 0.25)
    if Cout < g["ycw"]:
        assert float(y[:, g["yoff"] + Cout:g["yoff"] + g["ycw"]].abs().max()) in (0.0, 0.25)
    if config in FWD and stats is not None:
        mean, var, cnt = _chan_stats(stats, tiles, g["cp"], Cout)
        assert torch.all(cnt == N * H * W)
        emean = float((mean - want.mean(0)).abs().max())
        evar = float((var - want.var(0, unbiased=False)).abs().max())
        print(f"{tag}: mean error {emean:.3e} (bound {1e-4 * scale:.3e}), variance error {evar:.3e} (bound {1e-4 * scale * scale:.3e})")
        record_margin(tag + "/mean", emean, 1e-4 * scale)
        record_margin(tag + "/var", evar, 1e-4 * scale * scale)
        assert emean < 1e-4 * scale and evar < 1e-4 * scale * scale, (tag, emean, evar)


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("opt", [0, 1])
@pytest.mark.parametrize("relu", [0, 1])
def test_partial_sums_vs_fp64_sums_of_the_kernels_own_gradient(case, opt, relu):
    got, _, bn, tiles, g = _case(*case)
    shape, view = case
    N, H, W, Cin, Cout = shape
    y, part = got[(opt, f"bnred{relu}")]
    gd = y[:, g["yoff"]:g["yoff"] + Cout].double().cpu()
    if relu:
        gd = gd * bn["mask"]
    xh = (bn["x"] - bn["mean"]) * bn["invstd"]
    pix = torch.arange(N * H * W)
    img, rem = pix // (H * W), pix % (H * W)
    tx, ty = -(-W // 16), -(-H // 8)
    row = img * (tx * ty) + (rem // W // 8) * tx + (rem % W) // 16
    want = torch.zeros(tiles, 4, Cout, dtype=torch.float64)
    for i, t in enumerate((gd, gd * xh, gd.abs(), (gd * xh).abs())):
        want[:, i].index_add_(0, row, t)
    p = part.double().cpu()
    assert torch.isfinite(p).all()
    assert torch.all(p[:, :, Cout:] == 0), "pad columns of the partial rows: exact zeros"
    tag = f"wino4_lean/{IDS[CASES.index(case)]}/bnred{relu}/fast_{opt}"
    for i, name in ((0, "sum_g"), (1, "sum_gxhat")):
        err = (p[:, i, :Cout] - want[:, i]).abs()
        tol = (8 + 16 + 4) * U * want[:, 2 + i] + 1e-30
        worst = float((err / tol).max())
        print(f"{tag}/{name}: worst error / bound {worst:.3f}")
        record_margin(f"{tag}/{name}", worst, 1.0)
        assert worst < 1.0, (tag, name, worst)
