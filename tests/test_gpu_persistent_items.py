"""The second and later work items of the persistent kernels (gemm_f32v2.hip, gemm_bf16v3.hip, conv_bf16v3.hip, conv_ingest.hip)
through the C ABI against fp64 references: launches of many tiny images whose work lists give some workgroups two items and some
one (``two_or_one``), or three and two (``three_or_two``, where a registered item queue is drawn from) -- the code behind the
first item: the next item's stages issued under the epilogue, the bias / ticket slots that alternate, the geometry handed over,
the DMA descriptors rebuilt, the statistics record of the right tile, the short last band.  _persistent_cases.py has the work-list
mirror, the cases and the references; test_persistent_cases_cpu.py proves on the CPU what is relied on here.

Operands are small integers, so every fp32 output must equal the fp64 reference bit for bit and every 16-bit output the exact
integer rounded once.  One comparison of the WHOLE output buffer with its expected contents covers the values, completeness (no
SENTINEL left where an item had to write), confinement (prior contents everywhere else) and the pad columns inside the written
width (exact zeros; an accumulating launch of the bf16 kernels adds exact zeros to them, gemm_f32v2 writes zeros there too).  Each launch runs with fixed lists and with a registered queue, twice each (identical bits), and each run is
compared with the reference, never with another run.  A failure names the first wrong item by image, tile, block and the
workgroup and list position the mirror gives it.  Statistics are checked per record.

Measured on an MI355X (256 CUs): the 105 tests of the file take 7 s together, the slowest (g3_rows300 with statistics, 289
images of 300 rows) 0.65 s.  Needs a real MI355X: ``-m gpu``."""
import ctypes

import pytest
import torch

import _persistent_cases as PC
from _persistent_cases import SENTINEL, X_PAD_VALUE, _Queue, rup
from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
REGIME = pytest.mark.parametrize("regime", PC.REGIMES)


def P(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from hyperpri_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def lib16():
    from hyperpri_amd import _lib
    return _lib.load_f16()


@pytest.fixture(scope="module")
def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count       # what hpri_cu_count() reads


def _queue(lib_):
    q = _Queue(lib_)
    yield q
    torch.cuda.synchronize()
    q.off()


@pytest.fixture(scope="module")
def queue(lib):
    yield from _queue(lib)


@pytest.fixture(scope="module")
def queue16(lib16):
    yield from _queue(lib16)


class Buf:
    """One output buffer of a launch: its contents before (CPU), the contents expected after (CPU), and -- for the failure message --
    ``to_items``: the boolean mismatch map of the buffer -> [rows, GEMM columns] of the launch (None: not an item-addressed buffer)."""

    def __init__(self, prior, expected, to_items=None):
        assert prior.shape == expected.shape and prior.dtype == expected.dtype
        self.prior, self.expected, self.to_items = prior, expected, to_items


class Form:
    def __init__(self, name, geom, N, mirror, bufs, launch, stats=None):
        self.name, self.geom, self.g, self.N, self.mirror = name, geom, PC.GEOMS[geom], N, mirror
        self.bufs, self.launch, self.stats = bufs, launch, stats


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _verify(f, got, exp, how):
    for k, b in f.bufs.items():
        if k == "stats":
            continue
        g16 = b.expected.element_size() == 2
        same = torch.equal(_bits(got[k]), _bits(exp[k])) if g16 else torch.equal(got[k], exp[k])
        if same:
            continue
        g, e = got[k].cpu(), b.expected
        wrong = (_bits(g) != _bits(e)) if g16 else (g != e)
        left = int(((g.float() == SENTINEL) & (e.float() != SENTINEL)).sum())
        spilled = int((wrong & (_bits(e) == _bits(b.prior))).sum())
        msg = "%s [%s, %s] buffer %s: %d wrong elements, %d of them a SENTINEL left in the written range, %d where the prior contents had to stay" % (
            f.name, f.mirror.describe(), how, k, int(wrong.sum()), left, spilled)
        if b.to_items is not None:
            msg += "\n" + PC.first_wrong(f.g, f.N, f.mirror, b.to_items(wrong), k)
            if how != "fixed lists" and f.mirror.queue:
                msg += "\n(drawn items: the workgroup and list position are those of the fixed lists; a workgroup draws its band's items in this order)"
        pytest.fail(msg)
    if f.stats is not None:
        _verify_stats(f, got["stats"], how)


def _verify_stats(f, stats, how):
    """Every record on its own: count exact, mean and M2 / count within 1e-4 x scale resp. 1e-4 x scale^2 of fp64 over the rows of
    that tile (the margins test_gpu_kernels_r2.py applies to the merged records), scale = max(1, max |reference|)."""
    key, cp, C, vals = f.stats
    tiles = PC.tile_rows(f.g, f.N)
    s = stats.view(len(tiles), cp, 4).double().cpu()
    sc = max(1.0, float(vals.abs().max()))
    cnt = torch.tensor([float(r.numel()) for r in tiles], dtype=torch.float64)
    mean, var = torch.empty(len(tiles), C, dtype=torch.float64), torch.empty(len(tiles), C, dtype=torch.float64)
    for size in sorted(set(cnt.tolist())):
        sel = torch.nonzero(cnt == size).reshape(-1)
        v = vals[torch.stack([tiles[int(t)] for t in sel])]                    # [tiles of this size, rows, C]
        mean[sel], var[sel] = v.mean(1), v.var(1, unbiased=False)
    where = lambda bad: "record of tile %d, column %d: %s" % (int(bad[0, 0]), int(bad[0, 1]), f.mirror.where(
        int(bad[0, 0]), int(bad[0, 1]) // PC.BLOCK[f.mirror.kernel]))
    bad = torch.nonzero(~(s[:, :C, 2] == cnt[:, None]))
    assert bad.numel() == 0, "%s [%s]: %d records with a wrong count (NaN: never written), first the %s" % (f.name, how, bad.shape[0], where(bad))
    assert bool((s[:, :C, 3] == 0).all())
    e_mean = (s[:, :C, 0] - mean).abs() / (1e-4 * sc)
    e_var = (s[:, :C, 1] / cnt[:, None] - var).abs() / (1e-4 * sc * sc)
    record_margin("persistent_items/%s/record_mean" % key, float(e_mean.max()), 1.0)
    record_margin("persistent_items/%s/record_var" % key, float(e_var.max()), 1.0)
    for what, e in (("mean", e_mean), ("M2 / count", e_var)):
        bad = torch.nonzero(~(e <= 1.0))
        assert bad.numel() == 0, "%s [%s]: %d records with a wrong %s (worst ratio %g), first the %s" % (
            f.name, how, bad.shape[0], what, float(e.nan_to_num(1e30).max()), where(bad))


def _run(lib_, q, regime, f):
    """Fixed lists, then a registered queue; each twice.  Every run is held against the reference."""
    ok, failed = f.mirror.regime_holds(regime)
    assert ok, (f.name, regime, failed, f.mirror.describe())
    steps = sum(v - 1 for v in f.mirror.counts())
    assert f.mirror.tile_changes() == steps and f.mirror.block_changes() == (steps if f.geom in PC.BLOCKS_CHANGE else 0)
    exp = {k: b.expected.to(DEV) for k, b in f.bufs.items()}

    def once():
        bufs = {k: b.prior.to(DEV) for k, b in f.bufs.items()}
        torch.cuda.synchronize()
        with torch.cuda.stream(q.stream):
            rc = f.launch(bufs, q.h)
        assert rc == 0, lib_.hpri_last_error()
        torch.cuda.synchronize()
        return bufs
    try:
        for queued in (False, True):
            how = "registered queue" if queued else "fixed lists"
            q.off()
            if queued:
                q.buf.zero_()
                torch.cuda.synchronize()
                q.on()
            first = once()
            if queued:           # drawn from in three_or_two (one half used, the other zeroed); left alone in two_or_one and by the ingest kernel
                assert q.next_half_is_zero(taken=f.mirror.queue), (f.name, how, "first launch")
            _verify(f, first, exp, how)
            second = once()
            if queued:
                assert q.next_half_is_zero(taken=f.mirror.queue), (f.name, how, "second launch")
            for k in first:
                assert torch.equal(_bits(first[k]), _bits(second[k])), "%s [%s]: buffer %s differs between two identical launches" % (f.name, how, k)
    finally:
        q.off()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _view(buf, coff, width):
    return buf[:, coff:coff + width]


def _rows_to_items(coff, ncols):
    return lambda wrong: wrong[:, coff:coff + ncols]


def _canvas(N, H, W, off):
    py0, px0 = off
    return 2 * H + py0 + (1 if py0 else 0), 2 * W + px0 + (2 if px0 else 0), py0, px0


def _patches_to_items(N, H, W, H2, W2, py0, px0, coff, Cup):
    """mismatch map of a [N*H2*W2, cs] canvas -> [N*H*W, 4*Cup]: GEMM column tap * Cup + co, tap = 2 * row parity + column parity"""
    def f(wrong):
        p = wrong.view(N, H2, W2, -1)[:, py0:py0 + 2 * H, px0:px0 + 2 * W, coff:coff + Cup]
        return p.reshape(N, H, 2, W, 2, Cup).permute(0, 1, 3, 2, 4, 5).reshape(N * H * W, 4 * Cup)
    return f


def _put_patches(canvas, vals, N, H2, W2, py0, px0, coff):
    """vals [N, 2H, 2W, C] into channels [coff, coff + C) of the patch grid of a [N*H2*W2, cs] canvas"""
    canvas.view(N, H2, W2, -1)[:, py0:py0 + vals.shape[1], px0:px0 + vals.shape[2], coff:coff + vals.shape[3]] = vals.to(canvas.dtype)
    return canvas


def _plan_tiles_gemm(lib, N, HW):
    tl = ctypes.c_int()
    assert lib.hpri_gemm_bf16v3_plan(N, HW, ctypes.byref(tl)) == 0
    return tl.value


# ---------------------------------------------------------------------------------------------------------------------------
# gemm_f32v2.hip
# ---------------------------------------------------------------------------------------------------------------------------
def _f2_pack(lib, w, mode, K, ncols, cup, d1):
    ncols_pad = rup(ncols, 64)
    wp = torch.empty(lib.hpri_packed_weight_f32k16_floats(K, ncols_pad), device=DEV)
    assert lib.hpri_pack_weight_f32k16(P(w.to(DEV)), P(wp), mode, K, ncols, ncols_pad, cup, d1, _st()) == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    return wp, ncols_pad


@REGIME
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("geom", ["f2_rows5", "f2_rows300", "f2_rows5_b3"])
def test_gemm_f32v2_rows(lib, queue, ncu, geom, acc, regime):
    """hpri_gemm_f32v2 with a bias into a channel-slice view of a wider buffer, plain and accumulating."""
    g = PC.GEOMS[geom]
    N, m = PC.case_mirror(geom, regime, ncu)
    assert PC.geom_tiles(g) == -(-g["HW"] // 256)
    c = PC.rows_case(geom, N)
    K, C, HW = g["K"], g["C"], g["HW"]
    kpad, rows = rup(K, 16), N * HW
    xcs, xoff = kpad + 8, 4
    x = torch.full((rows, xcs), X_PAD_VALUE)
    x[:, xoff:xoff + kpad] = 0                      # [K, K_pad): "zeros or zero weights"
    x[:, xoff:xoff + K] = c["x"]
    x, bias = x.to(DEV), c["bias"].to(DEV)
    wp, ncp = _f2_pack(lib, c["w"], 0, K, C, 0, K)
    assert ncp == g["ncols_pad"]
    cw, yoff = C + 4, 4                             # four pad columns inside the written width
    ycs = cw + 12
    prior = torch.full((rows, ycs), SENTINEL)
    expected = prior.clone()
    want = c["ref"] + c["bias"].double()
    if acc:
        _view(prior, yoff, C)[:] = c["y0"]
        _view(prior, yoff + C, cw - C)[:] = 5.0
        expected = prior.clone()
        want = want + c["y0"].double()
    _view(expected, yoff + C, cw - C)[:] = 0.0      # "columns >= Ncols: zeros", also of an accumulating launch (gemm_f32v2.hip)
    _view(expected, yoff, C)[:] = want.float()

    def launch(b, st):
        return lib.hpri_gemm_f32v2(P(x), xcs, xoff, P(wp), P(bias), P(b["y"]), ycs, yoff, N, HW, kpad, C, ncp, cw, acc, st)
    _run(lib, queue, regime, Form("gemm_f32v2/%s/acc%d" % (geom, acc), geom, N, m, {"y": Buf(prior, expected, _rows_to_items(yoff, C))}, launch))


@REGIME
@pytest.mark.parametrize("off", [(0, 0), (1, 2)])
def test_convt_fwd_f32v2(lib, queue, ncu, off, regime):
    """hpri_convt_fwd_f32v2: the depth-to-space scatter into a canvas, at the origin and at a pad offset."""
    geom = "f2_convt"
    g = PC.GEOMS[geom]
    N, m = PC.case_mirror(geom, regime, ncu)
    c = PC.convt_case(geom, N)
    H, W, Cin, Cup = g["H"], g["W"], g["Cin"], g["Cup"]
    H2, W2, py0, px0 = _canvas(N, H, W, off)
    kpad = rup(Cin, 16)
    xcs, xoff = kpad + 8, 4
    x = torch.full((N * H * W, xcs), X_PAD_VALUE)
    x[:, xoff:xoff + kpad] = 0
    x[:, xoff:xoff + Cin] = c["x"].reshape(-1, Cin)
    x, bias = x.to(DEV), c["bias"].to(DEV)
    wp, ncp = _f2_pack(lib, c["wt"], 2, Cin, 4 * Cup, Cup, 0)
    assert ncp == g["ncols_pad"]
    ycs, yoff = Cup + 8, 4
    prior = torch.full((N * H2 * W2, ycs), SENTINEL)
    expected = _put_patches(prior.clone(), c["fwd"] + c["bias"].double(), N, H2, W2, py0, px0, yoff)

    def launch(b, st):
        return lib.hpri_convt_fwd_f32v2(P(x), xcs, xoff, P(wp), P(bias), P(b["y"]), ycs, yoff, N, H, W, kpad, Cup, ncp, H2, W2, py0, px0, st)
    _run(lib, queue, regime, Form("convt_fwd_f32v2/off%d%d" % off, geom, N, m,
                                  {"y": Buf(prior, expected, _patches_to_items(N, H, W, H2, W2, py0, px0, yoff, Cup))}, launch))


@REGIME
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("off", [(0, 0), (1, 2)])
def test_convt_dgrad_f32v2(lib, queue, ncu, off, acc, regime):
    """hpri_convt_dgrad_f32v2: K = 4 * Cup gathered from the four parities of a canvas; the canvas around the patch grid and the
    channels beside the gradient's hold values that must not be read."""
    geom = "f2_convt"
    g = PC.GEOMS[geom]
    N, m = PC.case_mirror(geom, regime, ncu, PC.dgrad_ncols_pad(g))
    c = PC.convt_case(geom, N)
    H, W, Cin, Cup = g["H"], g["W"], g["Cin"], g["Cup"]
    H2, W2, py0, px0 = _canvas(N, H, W, off)
    dcs, doff = Cup + 16, 16
    dy = _put_patches(torch.full((N * H2 * W2, dcs), X_PAD_VALUE), c["dy"], N, H2, W2, py0, px0, doff).to(DEV)
    wp, cinp = _f2_pack(lib, c["wt"], 3, 4 * Cup, Cin, Cup, 0)
    assert cinp == PC.dgrad_ncols_pad(g)
    cw, xoff = Cin + 4, 4
    xcs = cw + 8
    prior = torch.full((N * H * W, xcs), SENTINEL)
    want = c["dgrad"]
    if acc:
        _view(prior, xoff, Cin)[:] = c["dx0"]
        _view(prior, xoff + Cin, cw - Cin)[:] = 5.0
        want = want + c["dx0"].double()
    expected = prior.clone()
    _view(expected, xoff + Cin, cw - Cin)[:] = 0.0  # "columns >= Ncols: zeros", also of an accumulating launch (gemm_f32v2.hip)
    _view(expected, xoff, Cin)[:] = want.float()

    def launch(b, st):
        return lib.hpri_convt_dgrad_f32v2(P(dy), dcs, doff, P(wp), P(b["dx"]), xcs, xoff, N, H, W, Cup, Cin, cinp, cw, H2, W2, py0, px0, acc, st)
    _run(lib, queue, regime, Form("convt_dgrad_f32v2/off%d%d/acc%d" % (off + (acc,)), geom, N, m,
                                  {"dx": Buf(prior, expected, _rows_to_items(xoff, Cin))}, launch))


# ---------------------------------------------------------------------------------------------------------------------------
# gemm_bf16v3.hip
# ---------------------------------------------------------------------------------------------------------------------------
def _g3_pack(lib, w, mode, K, ncols, T, d1, cup):
    kp, ncp = rup(K, 32), rup(ncols, 64)
    wp = torch.empty((kp // 32) * T * ncp * 32, dtype=torch.bfloat16, device=DEV)
    assert lib.hpri_pack_weight_bf16(P(w.contiguous().to(DEV)), P(wp), mode, K, ncols, ncp, T, d1, cup, 0, _st()) == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    return wp, ncp


def _planes(vals, cs, coff, kp):
    """bf16 rows of cs elements: vals in [coff, coff + K), zeros up to coff + kp ("zeros or zero weights"), X_PAD_VALUE elsewhere"""
    p = torch.full((vals.shape[0], cs), X_PAD_VALUE, dtype=torch.bfloat16)
    p[:, coff:coff + kp] = 0
    p[:, coff:coff + vals.shape[1]] = vals.to(torch.bfloat16)
    return p.to(DEV)


G3_FORMS = ("f32_stats", "bf16", "relu", "acc32", "acc16")


@REGIME
@pytest.mark.parametrize("form", G3_FORMS)
@pytest.mark.parametrize("geom", ["g3_rows5", "g3_rows300", "g3_rows5_b3"])
def test_gemm_bf16v3_rows(lib, queue, ncu, geom, form, regime):
    """hpri_gemm_bf16v3: fp32 rows with per-tile statistics, bf16 rows, ReLU, accumulate into fp32 rows, accumulate into bf16 rows."""
    g = PC.GEOMS[geom]
    N, m = PC.case_mirror(geom, regime, ncu)
    K, C, HW = g["K"], g["C"], g["HW"]
    assert _plan_tiles_gemm(lib, N, HW) == N * PC.geom_tiles(g) == m.ntiles
    c = PC.rows_case(geom, N)
    rows, kp = N * HW, rup(K, 32)
    xcs, xoff = kp + 16, 8
    xp = _planes(c["x"], xcs, xoff, kp)
    wp, ncp = _g3_pack(lib, c["w"], 0, K, C, 1, K, 0)
    assert ncp == g["ncols_pad"]
    bias = None if form == "acc16" else c["bias"].to(DEV)
    cw, yoff = C + 4, 4
    ycs = cw + 12
    want = c["ref"] + (0 if bias is None else c["bias"].double())
    if form == "relu":
        want = torch.relu(want)
    if form in ("acc32", "acc16"):
        want = want + c["y0"].double()
    dt = torch.bfloat16 if form in ("bf16", "acc16") else torch.float32
    prior = torch.full((rows, ycs), SENTINEL, dtype=dt)
    if form in ("acc32", "acc16"):
        _view(prior, yoff, C)[:] = c["y0"].to(dt)
        _view(prior, yoff + C, cw - C)[:] = 5.0
    expected = prior.clone()
    if form not in ("acc32", "acc16"):
        _view(expected, yoff + C, cw - C)[:] = 0.0
    _view(expected, yoff, C)[:] = want.to(dt)                     # exact integers: fp32 as they are, bf16 rounded once
    bufs = {"y": Buf(prior, expected, _rows_to_items(yoff, C))}
    stats = None
    if form == "f32_stats":
        bufs["stats"] = Buf(torch.full((m.ntiles * ncp * 4,), NAN), torch.full((m.ntiles * ncp * 4,), NAN))
        stats = ("gemm_bf16v3/%s/%s" % (geom, regime), ncp, C, want)
    flags = {"f32_stats": 0, "bf16": 0, "relu": 2, "acc32": 1, "acc16": 1}[form]

    def launch(b, st):
        y32, y16 = (None, b["y"]) if dt == torch.bfloat16 else (b["y"], None)
        return lib.hpri_gemm_bf16v3(P(xp), xcs, xoff, P(wp), P(bias), P(y32), ycs if y32 is not None else 0, yoff if y32 is not None else 0,
                                    P(y16), ycs if y16 is not None else 0, yoff if y16 is not None else 0, P(b.get("stats")),
                                    ncp if stats else 0, N, HW, kp, C, ncp, cw, flags, st)
    _run(lib, queue, regime, Form("gemm_bf16v3/%s/%s" % (geom, form), geom, N, m, bufs, launch, stats))


@REGIME
def test_convt_fwd_bf16v3(lib, queue, ncu, regime):
    """hpri_convt_fwd_bf16v3: the fp32 and the bf16 view of one launch, in a canvas at a pad offset."""
    geom = "g3_convt"
    g = PC.GEOMS[geom]
    N, m = PC.case_mirror(geom, regime, ncu)
    c = PC.convt_case(geom, N)
    H, W, Cin, Cup = g["H"], g["W"], g["Cin"], g["Cup"]
    H2, W2, py0, px0 = _canvas(N, H, W, (1, 2))
    kp = rup(Cin, 32)
    xcs, xoff = kp + 16, 8
    xp = _planes(c["x"].reshape(-1, Cin), xcs, xoff, kp)
    wp, ncp = _g3_pack(lib, c["wt"], 2, Cin, 4 * Cup, 1, Cup, Cup)
    assert ncp == g["ncols_pad"]
    bias = c["bias"].to(DEV)
    ycs, yoff = Cup + 12, 8
    want = c["fwd"] + c["bias"].double()
    bufs = {}
    for k, dt in (("y", torch.float32), ("y16", torch.bfloat16)):
        prior = torch.full((N * H2 * W2, ycs), SENTINEL, dtype=dt)
        bufs[k] = Buf(prior, _put_patches(prior.clone(), want, N, H2, W2, py0, px0, yoff), _patches_to_items(N, H, W, H2, W2, py0, px0, yoff, Cup))

    def launch(b, st):
        return lib.hpri_convt_fwd_bf16v3(P(xp), xcs, xoff, P(wp), P(bias), P(b["y"]), ycs, yoff, P(b["y16"]), ycs, yoff, N, H, W, kp, Cup, ncp,
                                         H2, W2, py0, px0, st)
    _run(lib, queue, regime, Form("convt_fwd_bf16v3", geom, N, m, bufs, launch))


@REGIME
@pytest.mark.parametrize("form", ["acc0", "acc1", "y16"])
def test_convt_dgrad_bf16v3(lib, queue, ncu, form, regime):
    """hpri_convt_dgrad_bf16v3 (plain and accumulating) and hpri_convt_dgrad_bf16v3_y16 (bf16 rows)."""
    geom = "g3_convt"
    g = PC.GEOMS[geom]
    N, m = PC.case_mirror(geom, regime, ncu, PC.dgrad_ncols_pad(g))
    c = PC.convt_case(geom, N)
    H, W, Cin, Cup = g["H"], g["W"], g["Cin"], g["Cup"]
    H2, W2, py0, px0 = _canvas(N, H, W, (1, 2) if form != "acc0" else (0, 0))
    dcs, doff = Cup + 32, 32
    dyp = _put_patches(torch.full((N * H2 * W2, dcs), X_PAD_VALUE, dtype=torch.bfloat16), c["dy"], N, H2, W2, py0, px0, doff).to(DEV)
    wp, cinp = _g3_pack(lib, c["wt"], 3, 4 * Cup, Cin, 1, Cup, Cup)
    assert cinp == PC.dgrad_ncols_pad(g)
    cw, xoff = Cin + 4, 4
    xcs = cw + 8
    dt = torch.bfloat16 if form == "y16" else torch.float32
    prior = torch.full((N * H * W, xcs), SENTINEL, dtype=dt)
    want = c["dgrad"]
    if form == "acc1":
        _view(prior, xoff, Cin)[:] = c["dx0"]
        _view(prior, xoff + Cin, cw - Cin)[:] = 5.0
        want = want + c["dx0"].double()
    expected = prior.clone()
    if form != "acc1":
        _view(expected, xoff + Cin, cw - Cin)[:] = 0.0
    _view(expected, xoff, Cin)[:] = want.to(dt)

    def launch(b, st):
        if form == "y16":
            return lib.hpri_convt_dgrad_bf16v3_y16(P(dyp), dcs, doff, P(wp), P(b["dx"]), xcs, xoff, N, H, W, Cup, Cin, cinp, cw, H2, W2, py0, px0, st)
        return lib.hpri_convt_dgrad_bf16v3(P(dyp), dcs, doff, P(wp), P(b["dx"]), xcs, xoff, N, H, W, Cup, Cin, cinp, cw, H2, W2, py0, px0,
                                           int(form == "acc1"), st)
    _run(lib, queue, regime, Form("convt_dgrad_bf16v3/%s" % form, geom, N, m, {"dx": Buf(prior, expected, _rows_to_items(xoff, Cin))}, launch))


# ---------------------------------------------------------------------------------------------------------------------------
# conv_bf16v3.hip
# ---------------------------------------------------------------------------------------------------------------------------
def _v3_problem(lib, geom, regime, ncu, pack_mode=0):
    g = PC.GEOMS[geom]
    N, m = PC.case_mirror(geom, regime, ncu)
    c = PC.conv_case(geom, N)
    H, W, Cin, Cout = g["H"], g["W"], g["Cin"], g["Cout"]
    cs16, cout_pad = rup(Cin, 32), rup(Cout, 64)
    assert cout_pad == g["ncols_pad"]
    k, tl, wsf = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    assert lib.hpri_conv_bf16v3_plan(N, H, W, cs16, cout_pad, ctypes.byref(k), ctypes.byref(tl), ctypes.byref(wsf)) == 0
    assert k.value == 1 and wsf.value == 0 and tl.value == N * PC.geom_tiles(g) == m.ntiles      # the mirror's tiles are the plan's
    xcs, xoff = cs16 + 16, 8
    xp = _planes(c["x"].reshape(-1, Cin), xcs, xoff, cs16)
    if pack_mode == 0:
        wp, _ = _g3_pack(lib, c["w"], 0, Cin, Cout, 9, Cin, 0)
    else:
        # the data-gradient pack takes the LAYER's weight [its Cout = K][its Cin = columns] and rotates the taps itself:
        # conv_transpose2d(x, wl, padding=1) == conv2d(x, w, padding=1) for wl = w with its first two axes swapped and its taps flipped
        wl = c["w"].permute(1, 0, 2, 3).flip(2, 3)
        wp, _ = _g3_pack(lib, wl, 1, Cin, Cout, 9, Cout, 0)
    return dict(g=g, N=N, m=m, c=c, H=H, W=W, Cin=Cin, Cout=Cout, cs16=cs16, cout_pad=cout_pad, xp=xp, xcs=xcs, xoff=xoff, wp=wp,
                npx=N * H * W, bias=c["bias"].to(DEV))


@REGIME
@pytest.mark.parametrize("geom", ["v3_c72", "v3_c128", "v3_c136", "v3_c512"])
def test_conv_bf16v3_forward_with_statistics(lib, queue, ncu, geom, regime):
    """hpri_conv_bf16v3 forward, bias, one statistics record per tile and channel: the banded item order (Cout 72, 128, and 136 =
    three blocks, so that a workgroup's items change block) and the channel-block-major one (Cout 512)."""
    p = _v3_problem(lib, geom, regime, ncu)
    Cout, npx, cout_pad, N, m = p["Cout"], p["npx"], p["cout_pad"], p["N"], p["m"]
    assert m.nb_major == (geom == "v3_c512")
    cw = min(Cout + 8, cout_pad)                    # eight pad channels inside the written width where the blocks have room
    ycs, yoff = cw + 8, 4
    want = p["c"]["ref"] + p["c"]["bias"].double()
    prior = torch.full((npx, ycs), SENTINEL)
    expected = prior.clone()
    _view(expected, yoff + Cout, cw - Cout)[:] = 0.0
    _view(expected, yoff, Cout)[:] = want.float()
    bufs = {"y": Buf(prior, expected, _rows_to_items(yoff, Cout)),
            "stats": Buf(torch.full((m.ntiles * cout_pad * 4,), NAN), torch.full((m.ntiles * cout_pad * 4,), NAN))}
    ws = torch.empty(4, device=DEV)

    def launch(b, st):
        return lib.hpri_conv_bf16v3(P(p["xp"]), 0, p["xcs"], p["xoff"], P(p["wp"]), P(p["bias"]), P(b["y"]), ycs, yoff, P(b["stats"]), N, p["H"],
                                    p["W"], p["cs16"], Cout, cout_pad, cw, 0, 0, P(ws), ws.numel(), st)
    _run(lib, queue, regime, Form("conv_bf16v3/%s/fwd_stats" % geom, geom, N, m, bufs, launch,
                                  ("conv_bf16v3/%s/%s" % (geom, regime), cout_pad, Cout, want)))


@REGIME
@pytest.mark.parametrize("form", ["dgrad_acc_view", "relu_bias"])
def test_conv_bf16v3_data_gradient_and_relu(lib, queue, ncu, form, regime):
    """hpri_conv_bf16v3 with the mode-1 pack accumulating into a channel-slice view of a gradient buffer; and bias + ReLU."""
    geom = "v3_c136"
    p = _v3_problem(lib, geom, regime, ncu, pack_mode=1)
    Cout, npx, cout_pad, N, m = p["Cout"], p["npx"], p["cout_pad"], p["N"], p["m"]
    cw = min(Cout + 8, cout_pad)                    # eight pad channels inside the written width where the blocks have room
    ycs, yoff = cw + 16, 8
    prior = torch.full((npx, ycs), SENTINEL)
    if form == "dgrad_acc_view":
        _view(prior, yoff, Cout)[:] = p["c"]["y0"]
        _view(prior, yoff + Cout, cw - Cout)[:] = 5.0
        expected = prior.clone()
        _view(expected, yoff, Cout)[:] = (p["c"]["ref"] + p["c"]["y0"].double()).float()
        bias, flags = None, 1
    else:
        expected = prior.clone()
        _view(expected, yoff + Cout, cw - Cout)[:] = 0.0
        _view(expected, yoff, Cout)[:] = torch.relu(p["c"]["ref"] + p["c"]["bias"].double()).float()
        bias, flags = p["bias"], 2
    ws = torch.empty(4, device=DEV)

    def launch(b, st):
        return lib.hpri_conv_bf16v3(P(p["xp"]), 0, p["xcs"], p["xoff"], P(p["wp"]), P(bias), P(b["y"]), ycs, yoff, P(None), N, p["H"], p["W"],
                                    p["cs16"], Cout, cout_pad, cw, flags, 0, P(ws), ws.numel(), st)
    _run(lib, queue, regime, Form("conv_bf16v3/%s/%s" % (geom, form), geom, N, m, {"y": Buf(prior, expected, _rows_to_items(yoff, Cout))}, launch))


@REGIME
@pytest.mark.parametrize("only", [0, 1, 3])
def test_conv_bf16v3_second_output(lib, queue, ncu, only, regime):
    """hpri_conv_bf16v3_y2: channel blocks [64, 192) also (1: only) as bf16 rows; 3: the main output as compact bf16 rows as well."""
    geom = "v3_c192"
    p = _v3_problem(lib, geom, regime, ncu)
    Cout, npx, cout_pad, N, m = p["Cout"], p["npx"], p["cout_pad"], p["N"], p["m"]
    c0, cw2 = 64, 128
    ref = p["c"]["ref"]
    y2cs, y2off = cw2 + 8, 4
    y2p = torch.full((npx, y2cs), SENTINEL, dtype=torch.bfloat16)
    y2e = y2p.clone()
    _view(y2e, y2off, cw2)[:] = ref[:, c0:c0 + cw2].to(torch.bfloat16)
    if only == 3:
        ycs, ycw, dt = c0 + 8, c0, torch.bfloat16
    else:
        ycs, ycw, dt = Cout, Cout, torch.float32
    yp = torch.full((npx, ycs), SENTINEL, dtype=dt)
    ye = yp.clone()
    ye[:, :c0] = ref[:, :c0].to(dt)
    if only == 0:
        ye[:, c0:Cout] = ref[:, c0:].to(dt)
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[0], Cout - t.shape[1], dtype=torch.bool)], 1)
    bufs = {"y": Buf(yp, ye, (lambda w: pad(w[:, :c0])) if only else (lambda w: w)),
            "y2": Buf(y2p, y2e, lambda w: torch.cat([torch.zeros(npx, c0, dtype=torch.bool), w[:, y2off:y2off + cw2]], 1)),
            "stats": Buf(torch.full((m.ntiles * cout_pad * 4,), NAN), torch.full((m.ntiles * cout_pad * 4,), NAN))}

    def launch(b, st):
        return lib.hpri_conv_bf16v3_y2(P(p["xp"]), p["xcs"], p["xoff"], P(p["wp"]), P(None), P(b["y"]), ycs, 0, P(b["stats"]), N, p["H"], p["W"],
                                       p["cs16"], Cout, cout_pad, ycw, P(b["y2"]), y2cs, y2off, c0, cw2, only, st)
    _run(lib, queue, regime, Form("conv_bf16v3_y2/only%d" % only, geom, N, m, bufs, launch,
                                  ("conv_bf16v3_y2/only%d/%s" % (only, regime), cout_pad, Cout, ref)))


# ---------------------------------------------------------------------------------------------------------------------------
# conv_ingest.hip, both libraries
# ---------------------------------------------------------------------------------------------------------------------------
@REGIME
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("geom", ["ig_c64", "ig_c128", "ig_c136"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_conv3x3_ingest_h16(lib, lib16, queue, queue16, ncu, kind, geom, relu, regime):
    """hpri_conv3x3_ingest_h16 over fp32 NCHW cubes of three tiles (32, 32 and 8 wide): a workgroup's consecutive items change tile
    width.  The kernel has no item queue: a registered one stays untouched in both regimes."""
    L, q, dt = (lib, queue, torch.bfloat16) if kind == "bf16" else (lib16, queue16, torch.float16)
    g = PC.GEOMS[geom]
    N, m = PC.case_mirror(geom, regime, ncu)
    assert not m.queue and PC.geom_tiles(g) == 3
    c = PC.conv_case(geom, N)
    H, W, Cin, Cout, cout_pad = g["H"], g["W"], g["Cin"], g["Cout"], g["ncols_pad"]
    x = c["x"].permute(0, 3, 1, 2).contiguous().to(DEV)                      # the caller's NCHW cube
    wp = torch.empty(((Cin + 31) // 32) * 9 * cout_pad * 32, dtype=dt, device=DEV)
    assert L.hpri_pack_weight_bf16(P(c["w"].to(DEV)), P(wp), 0, Cin, Cout, cout_pad, 9, Cin, 0, 0, _st()) == 0, L.hpri_last_error()
    torch.cuda.synchronize()
    bias = c["bias"].to(DEV)
    ycs, yoff = Cout + 8, 4
    want = c["ref"] + c["bias"].double()
    if relu:
        want = torch.relu(want)
    prior = torch.full((N * H * W, ycs), SENTINEL, dtype=dt)
    expected = prior.clone()
    _view(expected, yoff, Cout)[:] = want.to(dt)
    pad = lambda w: torch.cat([w[:, yoff:yoff + Cout], torch.zeros(w.shape[0], cout_pad - Cout, dtype=torch.bool)], 1)

    def launch(b, st):
        return L.hpri_conv3x3_ingest_h16(P(x), P(wp), P(bias), P(b["y"]), ycs, yoff, N, Cin, H, W, Cout, cout_pad, relu, st)
    _run(L, q, regime, Form("conv3x3_ingest_h16/%s/%s/relu%d" % (kind, geom, relu), geom, N, m, {"y": Buf(prior, expected, pad)}, launch))


def test_the_work_lists_these_cases_reach(ncu):
    """The mirror at this device's CU count, per kernel form (printed with -s; the regime predicates themselves are asserted at the
    top of every test above)."""
    for geom in PC.GEOMS:
        for regime in PC.REGIMES:
            N, m = PC.case_mirror(geom, regime, ncu)
            assert m.regime_holds(regime)[0]
            print("%-11s %-12s N = %4d  %s" % (geom, regime, N, m.describe()))
