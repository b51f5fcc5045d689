"""Stage 2 of the two-stage column reductions (bn.hip: col_finalize_kernel, col_fold_kernel) and the many-slab Winograd
weight-gradient reduce (conv_wino.hip: wino_wgrad_reduce_wide_kernel<16>), through the existing entry points.

The stage-2 kernels run as workgroups of 8 channels x 32 row slices.  Their summation order is part of the contract (every
gradient downstream is bit-equal whatever the workgroup shape), so the sums are compared BIT FOR BIT with a NumPy float64
restatement of it:

    slice chain   thread (channel c, slice sl) adds the rows b = sl, sl + 32, sl + 64, ... of its range in ascending order, in double
    totals        one thread per channel adds the 32 slice totals in ascending slice order, in double
    rounding      once, to float

col_fold_kernel applies this to each of S row ranges [s * per, min((s + 1) * per, rows)), per = ceil(rows / S), and
col_finalize_kernel applies it to the S folded rows.  Needs a real MI355X: ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_bn_kernels as K           # the helpers and bounds of the BatchNorm kernel tests (the module, not its tests)
from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = K.DEV
NAN = K.NAN
P, _st, rup = K.P, K._st, K.rup


@pytest.fixture(scope="module")
def lib():
    from hyperpri_amd import _lib
    return _lib.load()


def stage2(rows):
    """The documented order on float32 rows [n][...]: float32 [...] (n may be 0: zeros)."""
    rows = np.asarray(rows, dtype=np.float32)
    n, shape = rows.shape[0], rows.shape[1:]
    chain = np.zeros((32,) + shape, dtype=np.float64)
    for b in range(0, n, 32):                      # every slice takes its next row: ascending within each slice
        blk = rows[b:b + 32].astype(np.float64)
        chain[:blk.shape[0]] += blk
    tot = np.zeros(shape, dtype=np.float64)
    for sl in range(32):
        tot += chain[sl]
    return tot.astype(np.float32)


def fold(rows, S):
    """col_fold_kernel: S folded float32 rows of rows [n][...]."""
    n = rows.shape[0]
    per = -(-n // S)
    return np.stack([stage2(rows[min(s * per, n):min((s + 1) * per, n)]) for s in range(S)])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------------
# hpri_col_finalize
# ------------------------------------------------------------------------------------------------------------------------------
FINALIZE_LAYOUTS = [(5, 64), (33, 64), (64, 64), (72, 128), (33, 192)]          # (C, Cpart): Cpart = C rounded up to 64, and one wider


@pytest.mark.parametrize("nblk", [1, 31, 32, 33, 97, 128, 131, 1024])
@pytest.mark.parametrize("C,Cpart", FINALIZE_LAYOUTS)
def test_col_finalize_bit_equal_to_documented_order(lib, C, Cpart, nblk):
    """sums, out1 and out2 of hpri_col_finalize against the restatement, accumulate on and off, zero_out given and null; the
    columns [C, Cpart) of the partial rows hold NaN and must not be read into anything."""
    rng = np.random.default_rng(1000 * C + nblk + Cpart)
    part = np.full((nblk, 2, Cpart), np.nan, dtype=np.float32)
    part[:, :, :C] = (rng.standard_normal((nblk, 2, C)) * np.exp(rng.uniform(-6, 6, (nblk, 2, C)))).astype(np.float32)
    want = stage2(part[:, :, :C])                                                  # [2][C]
    out0 = rng.standard_normal((2, C)).astype(np.float32)
    d_part = torch.from_numpy(part).to(DEV)
    for acc in (0, 1):
        for with_zero in (False, True):
            sums = torch.full((2 * C + 3,), 7.0, device=DEV)
            o1, o2 = torch.from_numpy(out0[0].copy()).to(DEV), torch.from_numpy(out0[1].copy()).to(DEV)
            zero = torch.full((C + 2,), 3.0, device=DEV)
            rc = lib.hpri_col_finalize(P(d_part), nblk, Cpart, C, P(sums), P(o1), P(o2), acc, P(zero if with_zero else None), _st())
            assert rc == 0, lib.hpri_last_error()
            torch.cuda.synchronize()
            got = sums.cpu().numpy()
            assert np.array_equal(_bits(got[:2 * C].reshape(2, C)), _bits(want)), (C, Cpart, nblk, acc, "sums")
            assert np.all(got[2 * C:] == 7.0), "hpri_col_finalize wrote past sums[2][C]"
            w1 = (out0[0] + want[0]) if acc else want[0]                         # float32 + float32: one rounding, as the kernel's
            w2 = (out0[1] + want[1]) if acc else want[1]
            assert np.array_equal(_bits(o1.cpu().numpy()), _bits(w1)), (C, Cpart, nblk, acc, "out1")
            assert np.array_equal(_bits(o2.cpu().numpy()), _bits(w2)), (C, Cpart, nblk, acc, "out2")
            z = zero.cpu().numpy()
            assert np.all(z[:C] == (0.0 if with_zero else 3.0)) and np.all(z[C:] == 3.0), "zero_out: C zeros, or untouched"
    # the optional outputs may all be null
    sums = torch.full((2 * C,), 7.0, device=DEV)
    assert lib.hpri_col_finalize(P(d_part), nblk, Cpart, C, P(sums), P(None), P(None), 0, P(None), _st()) == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(sums.cpu().numpy().reshape(2, C)), _bits(want))


# ------------------------------------------------------------------------------------------------------------------------------
# the fold path: hpri_bn_relu_bwd_fused on synthetic partial rows
# ------------------------------------------------------------------------------------------------------------------------------
# (pixels, C, Cw, partial rows, S): S = min(64, plan rows * plan Cpart / Cpart of the rows); the fold runs for S >= 4 and rows >= 16 S.
# rows = 16 S, 16 S + 1 (S = 4 and 7 do not divide it), and S = 64 with 1040 rows: per = 17, slice 61 holds 3 rows, 62 and 63 none
FOLD_CASES = [(500, 33, 36, 64, 4), (500, 33, 36, 65, 4), (896, 33, 36, 112, 7), (896, 33, 36, 113, 7),
              (8192, 64, 64, 1024, 64), (8192, 64, 64, 1025, 64), (8192, 64, 64, 1040, 64), (8192, 72, 72, 1040, 64)]


@pytest.mark.parametrize("npx,C,Cw,nrows,S_want", FOLD_CASES)
def test_fold_then_finalize_through_bn_relu_bwd_fused(lib, npx, C, Cw, nrows, S_want):
    """The recipe of test_bn_relu_bwd_fused_on_synthetic_rows (rows computed in fp64 and rounded to fp32) at shapes that take the
    folding launch: `sums` is read back from the workspace (after the G * nblk * 2 * Cpart partial rows) and compared bit for bit
    with fold + finalize of the restatement; dx, dgamma and dbeta against fp64 with that test's bounds (rows of one rounding each,
    summed in double: L = 2)."""
    xb = K._tensor(npx, C, Cw, Cw, 0, seed=51)
    g = K._tensor(npx, C, Cw, Cw, 0, seed=52, offset=0.0)
    st = K._stats(xb[:, :C], 1, C, seed=53)
    mask = K._mask_from_forward(lib, xb, Cw, 0, st, npx, npx, C, Cw, 1)
    nblk, cpart_plan, _, _ = K._plan(lib, npx, 1, C)
    cpart = rup(C, 64)
    S = min(64, (nblk * 2 * cpart_plan) // (2 * cpart))
    assert S == S_want and S >= 4 and nrows >= 16 * S, "the case must take the folding launch with the intended slice count"
    row_of = torch.arange(npx, device=DEV) * nrows // npx
    gm = g[:, :C].double() * mask
    xh = (xb[:, :C].double() - st["mean"].double()) * st["invstd"].double()
    s = K._row_sums(gm, xh, row_of, nrows, C)
    part = torch.full((nrows, 2, cpart), NAN, device=DEV)
    part[:, :, :C] = s[:, :2].float()
    dg0, db0, dbias0 = torch.full((C,), 0.5, device=DEV), torch.full((C,), -0.25, device=DEV), torch.full((C,), 2.0, device=DEV)
    dgam, dbet, dbias = dg0.clone(), db0.clone(), dbias0.clone()
    dx = torch.full((npx, Cw), 7.0, device=DEV)
    ws = K._ws(lib, npx, 1, C)
    rc = K._bwd(lib, "fused", g, Cw, 0, xb, Cw, 0, dx, Cw, 0, st, dgam, dbet, 1, dbias, 1, ws, npx, npx, C, Cw, 1, 1,
                part=(part, nrows, cpart))
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    rows = part[:, :, :C].cpu().numpy()
    want = stage2(fold(rows, S))
    off = nblk * 2 * cpart_plan
    got = ws[off:off + 2 * C].cpu().numpy().reshape(2, C)
    assert np.array_equal(_bits(got), _bits(want)), "sums in the workspace differ from fold + finalize in the documented order"
    # the parameter gradients ride along on the finalize launch: accumulated onto their start values with one rounding
    assert np.array_equal(_bits(dbet.cpu().numpy()), _bits(db0.cpu().numpy() + want[0]))
    assert np.array_equal(_bits(dgam.cpu().numpy()), _bits(dg0.cpu().numpy() + want[1]))
    L = 2
    ref = K._bwd_ref(g[:, :C], xb[:, :C], mask, st, 1, C, 1, (L + 8) * K.U)
    K._check_bwd(f"stage2/fold/P{npx}xC{C}/rows{nrows}", lib, (dx[:, :C], dgam, dbet, dbias), ref, 1, C, L, 0, (dg0, db0, dbias0), 1, 1, 1)
    assert torch.all(dx[:, C:Cw] == 0)


# ------------------------------------------------------------------------------------------------------------------------------
# several groups (grid y of the finalize launch, bn_param_grad_kernel) and the plain column sum
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu,ubs,acc", [(1, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1)])
@pytest.mark.parametrize("geom", [(3, 1001, 33, 36, 48, 8, 40, 4), (3, 777, 72, 72, 80, 4, 76, 0)],
                         ids=["G3xP1001xC33", "G3xP777xC72"])
def test_bn_relu_bwd_three_groups_vs_fp64(lib, geom, relu, ubs, acc):
    """hpri_bn_relu_bwd with G = 3: one finalize workgroup column per group, the groups added by bn_param_grad_kernel; eval mode
    (ubs = 0) also takes the second finalize launch for dbias.  Bounds: those of test_bn_relu_bwd_fp32_vs_fp64."""
    K._run_bwd_case(lib, torch.bfloat16, "f32", geom, relu, ubs, acc, 0, True)


@pytest.mark.parametrize("acc", [0, 1])
def test_col_sum_ragged(lib, acc):
    """hpri_col_sum on P = 3001, C = 33 (a sliced source with NaN / inf pad channels), bounds of test_col_sum_vs_fp64."""
    npx, C, cs, coff = 3001, 33, 48, 8
    src = K._tensor(npx, C, rup(C, 4), cs, coff, seed=71, offset=0.2)
    torch.manual_seed(72)
    out0 = torch.randn(C, device=DEV)
    out = out0.clone()
    nblk, cpart, rows, L = K._plan(lib, npx, 1, C)
    ws = torch.full((nblk * 2 * cpart + 2 * C,), NAN, device=DEV)
    rc = lib.hpri_col_sum(P(src), cs, coff, P(out), acc, P(ws), ws.numel(), npx, C, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    v = src[:, coff:coff + C].double()
    want = v.sum(0) + (out0.double() if acc else 0.0)
    tol = (L + 8) * K.U * v.abs().sum(0) + 2 * K.U * (want.abs() + (out0.double().abs() if acc else 0.0))
    K._gate(f"stage2/col_sum/P{npx}xC{C}/acc{acc}", (out.double() - want).abs(), tol)
    # and the stage-2 order itself: the partial rows of stage 1 are still in the workspace
    rows1 = ws[:nblk * 2 * cpart].cpu().numpy().reshape(nblk, 2, cpart)[:, 0, :C]
    w = stage2(rows1)
    w = (out0.cpu().numpy() + w) if acc else w
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(w))


# ------------------------------------------------------------------------------------------------------------------------------
# the many-slab Winograd weight-gradient reduce
# ------------------------------------------------------------------------------------------------------------------------------
def test_wino_wgrad_reduce_wide16_vs_fp64_and_repeatable(lib):
    """The smallest 64 -> 64 layer whose plan reaches 256 slabs (2048 strips of 2 x 32 pixels, 8 per slab), which
    hpri_wino_wgrad_reduce sums with wino_wgrad_reduce_wide_kernel<16>: dW against fp64 with the tolerance of
    test_winograd_weight_gradient_vs_fp64, and two calls bit-equal to each other (the slabs meet in a fixed order)."""
    N, H, W, Cin, Cout = 1, 128, 1024, 64, 64
    torch.manual_seed(23)
    x = torch.randn(N * H * W, Cin, device=DEV)
    dy = torch.randn(N * H * W, Cout, device=DEV)
    sp, cr, nr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.hpri_wino_wgrad_plan(N, H, W, Cin, Cout, ctypes.byref(sp), ctypes.byref(cr), ctypes.byref(nr)) == 0
    assert sp.value >= 256, f"the shape must take the many-slab reduce ({sp.value} slabs)"
    ws = torch.empty(sp.value * 16 * cr.value * nr.value, device=DEV)
    dws = []
    for _ in range(2):
        dw = torch.full((Cout, Cin, 3, 3), 0.5, device=DEV)
        rc = lib.hpri_conv_wino_wgrad(P(x), Cin, 0, Cin, P(dy), Cout, 0, Cout, P(ws), ws.numel(), N, H, W, Cin, Cout, _st())
        assert rc == 0, lib.hpri_last_error()
        assert lib.hpri_wino_wgrad_reduce(P(ws), P(dw), N, H, W, Cin, Cin, Cout, Cout, 0, _st()) == 0, lib.hpri_last_error()
        dws.append(dw)
    torch.cuda.synchronize()
    assert torch.equal(dws[0].view(torch.int32), dws[1].view(torch.int32)), "dW of two calls differs"
    # fp64 reference: dW[o][i][ky][kx] = sum over pixels of dy[p][o] * x[p + (ky - 1, kx - 1)][i], nine products in double
    xp = torch.nn.functional.pad(x.double().reshape(N, H, W, Cin), (0, 0, 1, 1, 1, 1))
    dyt = dy.double().t().contiguous()
    ref = torch.empty(Cout, Cin, 3, 3, dtype=torch.float64, device=DEV)
    for ky in range(3):
        for kx in range(3):
            ref[:, :, ky, kx] = dyt @ xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, Cin)
    sc = max(1.0, float(ref.abs().max()))
    err = float((dws[0].double() - ref).abs().max())
    record_margin(f"stage2/wino_wgrad_wide16/{N}x{H}x{W}x{Cin}x{Cout}", err, 4e-5 * sc)
    assert err < 4e-5 * sc, err
    # accumulate = 1 adds the same sums onto what dW holds, with one more rounding per element
    assert lib.hpri_wino_wgrad_reduce(P(ws), P(dws[1]), N, H, W, Cin, Cin, Cout, Cout, 1, _st()) == 0
    torch.cuda.synchronize()
    err2 = float((dws[1].double() - 2 * ref).abs().max())
    assert err2 < 4e-5 * sc, err2
