"""BatchNorm(+ReLU) and column-reduction kernels (bn.hip) called directly through the C ABI (include/hyperpri_hip.h) against a
plain fp64 torch reference of the same operation: forward statistics from per-tile records (hpri_bn_finalize, both kernel forms,
the running-statistics update of one and of several groups), the eval-mode helpers, normalise + ReLU (fp32 / 16-bit input,
16-bit plane outputs), the backward in all its forms (fp32, planes, 16-bit pre-BN tensor, 16-bit gradient, partial sums from
hpri_conv_wino4_bnred), the column sums behind the bias gradients, and the error returns.  Ragged pixel counts, channel counts
that are not a multiple of 4, channel-slice views, one to five groups, NaN / inf in pad channels.  Each backward test feeds the
reference the same fp32 statistics the kernel gets, so every test isolates one stage.  Cases that read or write 16-bit data run
against both product libraries (bf16: libhyperpri_hip.so; IEEE half: libhyperpri_hip_f16.so).  Needs a real MI355X: ``-m gpu``.

Tolerances are stated as multiples of U = 2^-24 (the unit roundoff of fp32) next to each gate.  Sums are gated per channel
relative to the sum of the absolute values of their terms: a sequential fp32 sum of L terms is within (L - 1) U of it, so the
bound is the longest fp32 chain in the kernel (pixels per thread + rows of the workgroup reduction) plus a few roundings of the
terms themselves; the double-precision stages add nothing visible."""
import ctypes

import pytest
import torch

from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24                   # unit roundoff of fp32
U64 = 2.0 ** -53                 # unit roundoff of fp64
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))     # the eps the kernels see (a float argument)
NAN, INF = float("nan"), float("inf")
ERR_ARG, ERR_WORKSPACE = -1, -3


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


@pytest.fixture(scope="module", params=["bf16", "f16"])
def lib16(request):
    """(library, 16-bit torch dtype) of each product library: the "bf16" entry points use the library's own 16-bit type."""
    from hyperpri_amd import _lib
    if request.param == "bf16":
        return _lib.load(), torch.bfloat16
    try:
        return _lib.load_f16(), torch.float16
    except RuntimeError as e:
        pytest.skip(f"the half-precision library is not built ({e})")


def _ratio(err, tol):
    """max err / tol over the elements (0 / 0 counts as 0: an exactly right value where the bound is 0)."""
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return float(r.max()) if r.numel() else 0.0


def _gate(key, err, tol):
    m = _ratio(err, tol)
    record_margin(key, m, 1.0)
    assert m <= 1.0, (key, m)


def _pick_cq(c4, wide):
    cap = 256 if (c4 > 256 and wide) else 64
    q = 1
    while q < c4 and q < cap:
        q <<= 1
    return q


def _plan(lib, ppg, G, C):
    """(nblk, Cpart, rows, L) of the reduction launch: L = the longest fp32 chain of one channel (pixels per thread + the
    workgroup's row reduction)."""
    nblk, cpart = ctypes.c_int(), ctypes.c_int()
    assert lib.hpri_col_reduce_plan(ppg, G, C, ctypes.byref(nblk), ctypes.byref(cpart)) == 0
    rows = 256 // _pick_cq((C + 3) // 4, lib.hpri_get_option(b"bn_wide_cq") != 0)
    per = -(-ppg // nblk.value)
    return nblk.value, cpart.value, rows, -(-per // rows) + rows


class _wide:
    """hpri_set_option("bn_wide_cq", v) for the block, restored afterwards (v None: leave it)."""

    def __init__(self, lib, v):
        self.lib, self.v = lib, v

    def __enter__(self):
        self.old = self.lib.hpri_get_option(b"bn_wide_cq")
        if self.v is not None:
            assert self.lib.hpri_set_option(b"bn_wide_cq", self.v) == 0

    def __exit__(self, *exc):
        self.lib.hpri_set_option(b"bn_wide_cq", self.old)
        return False


# ------------------------------------------------------------------------------------------------------------------------------
# 1. forward statistics
# ------------------------------------------------------------------------------------------------------------------------------
def _records(G, T, Cp, C, ratio, seed):
    """[G][T][Cp] float4 (mean, M2, count, 0) records of tiles with uneven pixel counts (1..199); per-channel mean about `ratio`
    standard deviations away from zero (a conv output over a cube with a DC offset); pad channels [C, Cp) hold NaN (never read)."""
    torch.manual_seed(seed)
    cnt = torch.randint(1, 200, (G, T, 1), device=DEV).float().expand(G, T, C)
    sd = torch.rand(G, 1, C, device=DEV) + 0.5
    mu = (ratio * sd + torch.randn(G, 1, C, device=DEV)) * torch.sign(torch.randn(G, 1, C, device=DEV))
    m = mu + sd * torch.randn(G, T, C, device=DEV) / cnt.sqrt()
    m2 = sd * sd * cnt * (torch.rand(G, T, C, device=DEV) + 0.5)
    rec = torch.full((G, T, Cp, 4), NAN, device=DEV)
    rec[:, :, :C] = torch.stack([m, m2, cnt, torch.zeros_like(m)], -1)
    return rec


def _chan(rec, C):
    """fp64 Chan merge of the records: (mean, biased variance, count, mean of n*m^2 + M2 over the pixels) per [G][C]."""
    r = rec[:, :, :C].double()
    m, m2, n = r[..., 0], r[..., 1], r[..., 2]
    N = n.sum(1)
    mean = (n * m).sum(1) / N
    var = (m2 + n * (m - mean[:, None]) ** 2).sum(1) / N
    a1 = (n * m.abs()).sum(1) / N
    a2 = (m2 + n * m * m).sum(1) / N
    return mean, var, N, a1, a2


FIN_CASES = [(1, 64, 72, 1.0), (97, 5, 8, 1e3), (128, 64, 72, 1e4), (129, 5, 8, 1.0), (511, 64, 72, 1e3), (512, 5, 8, 1e4),
             (513, 64, 72, 1.0), (1024, 5, 8, 1e3), (1025, 64, 72, 1e4), (1793, 5, 8, 1.0), (4600, 64, 72, 1e3), (4637, 33, 36, 1e4),
             (97, 1, 4, 1e4), (97, 3, 8, 1.0), (513, 33, 40, 1e3), (129, 1650, 1664, 1e4), (513, 1650, 1652, 1.0), (1, 3, 4, 1e3)]


@pytest.mark.parametrize("T,C,Cp,ratio", FIN_CASES)
@pytest.mark.parametrize("G", [1, 2])
def test_finalize_statistics_vs_fp64_chan_merge(lib, T, C, Cp, ratio, G):
    """mean, invstd, var_unbiased, scale, shift of both finalize kernels (narrow below 512 tiles, wide from 512 on; tile counts on
    both sides of their 4-way unrolled loop bounds) against the fp64 merge of the same fp32 records, with means up to 1e4
    standard deviations (a sum-of-squares formula in fp32 would lose the variance there)."""
    rec = _records(G, T, Cp, C, ratio, 100 + T + C)
    gamma = torch.randn(C, device=DEV)
    beta = torch.randn(C, device=DEV)
    outs = [torch.full((G * C,), NAN, device=DEV) for _ in range(5)]
    rc = lib.hpri_bn_finalize(P(rec), T, G, Cp, C, P(gamma), P(beta), EPS, 0.1, *(P(o) for o in outs), P(None), P(None), P(None), _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    mean, invstd, varu, scale, shift = (o.view(G, C).double() for o in outs)
    rmean, rvar, N, a1, a2 = _chan(rec, C)
    # double sums: one chain per channel of at most T/32 records + the 32 (or 16) partial sums, then t2/tn - mu^2; the fp32 result
    # is one rounding (U) of the double value
    L = T // 32 + 64
    tol_mean = 2 * U * rmean.abs() + 4 * L * U64 * a1
    dvar = 4 * L * U64 * a2                               # error of the double variance (cancellation against mu^2)
    tol_var = 2 * U * rvar + dvar
    ris = 1.0 / torch.sqrt(rvar + EPS32)
    tol_is = ris * (0.5 * dvar / (rvar + EPS32) + 2 * U)
    rvu = torch.where(N > 1, rvar * N / (N - 1).clamp(min=1), rvar)
    tol_vu = torch.where(N > 1, tol_var * N / (N - 1).clamp(min=1), tol_var)
    g64, b64 = gamma.double(), beta.double()
    rsc = g64 * ris
    tol_sc = g64.abs() * tol_is + 2 * U * rsc.abs()
    rsh = b64 - rmean * rsc
    tol_sh = tol_mean * rsc.abs() + rmean.abs() * tol_sc + 2 * U * (b64.abs() + (rmean * rsc).abs())
    key = f"bn/finalize/T{T}xC{C}xG{G}/r{ratio:g}"
    for got, ref, tol, what in ((mean, rmean, tol_mean, "mean"), (invstd, ris, tol_is, "invstd"), (varu, rvu, tol_vu, "var_unbiased"),
                                (scale, rsc, tol_sc, "scale"), (shift, rsh, tol_sh, "shift")):
        assert torch.isfinite(got).all(), what
        _gate(f"{key}/{what}", (got - ref).abs(), tol)


@pytest.mark.parametrize("G,T,C", [(1, 9, 5), (1, 600, 33), (2, 9, 64), (5, 7, 3), (5, 520, 5)])
def test_finalize_running_statistics_vs_torch_batchnorm(lib, G, T, C):
    """running_mean / running_var (momentum 0.1, unbiased variance) and num_batches_tracked: G = 1 takes the update fused into
    the finalize launch, G > 1 the in-order per-group update (SpectralUNET's per-image loop, models.py:132).  Reference: torch
    nn.BatchNorm1d in float64 called once per group, in group order, on the data the records were made from.  Few pixels per
    group, so that the unbiased and the biased variance differ clearly."""
    torch.manual_seed(7 * G + T)
    Cp = rup(C, 4) + 4
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=0.1).double().train()
    rm0 = torch.randn(C, device=DEV)
    rv0 = torch.rand(C, device=DEV) + 0.2
    with torch.no_grad():
        bn.running_mean.copy_(rm0.double().cpu())
        bn.running_var.copy_(rv0.double().cpu())
        bn.num_batches_tracked.fill_(7)
    rec = torch.full((G, T, Cp, 4), NAN)
    sum_mean, sum_var = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for g in range(G):
        cnt = torch.randint(1, 8, (T,))
        x = torch.randn(int(cnt.sum()), C, dtype=torch.float64) * (torch.rand(C, dtype=torch.float64) + 0.5) + torch.randn(C, dtype=torch.float64)
        x = x.float().double()
        bn(x)
        off = 0
        for t in range(T):
            xs = x[off:off + int(cnt[t])]
            off += int(cnt[t])
            m = xs.mean(0)
            rec[g, t, :C, 0] = m.float()
            rec[g, t, :C, 1] = ((xs - m) ** 2).sum(0).float()
            rec[g, t, :C, 2] = float(cnt[t])
            rec[g, t, :C, 3] = 0.0
        sum_mean += x.mean(0).abs()
        sum_var += x.var(0, unbiased=True) + (x.mean(0).abs() + x.std(0)) ** 2
    rec = rec.to(DEV)
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    gamma, beta = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    outs = [torch.empty(G * C, device=DEV) for _ in range(5)]
    rc = lib.hpri_bn_finalize(P(rec), T, G, Cp, C, P(gamma), P(beta), EPS, 0.1, *(P(o) for o in outs), P(rm), P(rv), P(nbt), _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    assert int(nbt.item()) == 7 + (1 if G == 1 else G)
    assert int(bn.num_batches_tracked) == 7 + G
    # per update three fp32 roundings of terms bounded by the running value and the new statistic; the statistics themselves come
    # from records rounded to fp32 (mean: U relative; variance: about U of (|mean| + sd)^2)
    k = (4 * G + 8) * U
    tol_m = k * (rm0.double().cpu().abs() + sum_mean)
    tol_v = k * (rv0.double().cpu() + sum_var)
    _gate(f"bn/running/G{G}xT{T}xC{C}/mean", (rm.double().cpu() - bn.running_mean).abs(), tol_m)
    _gate(f"bn/running/G{G}xT{T}xC{C}/var", (rv.double().cpu() - bn.running_var).abs(), tol_v)


@pytest.mark.parametrize("C", [5, 64, 1650])
@pytest.mark.parametrize("with_bias", [True, False])
def test_eval_prepare_and_fold_vs_fp64(lib, C, with_bias):
    """hpri_bn_eval_prepare (mean = running_mean, invstd, scale, shift) and hpri_bn_fold (scale, folded bias with and without a
    convolution bias) from running statistics.  Each output is a few fp32 roundings of the fp64 value (correctly rounded division
    and square root): k = 4 U relative on the reciprocal square root, one U per further product or sum."""
    torch.manual_seed(C)
    rm = torch.randn(C, device=DEV) * 3
    rv = torch.rand(C, device=DEV) * 4 + 0.01
    gamma, beta = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    cb = torch.randn(C, device=DEV) if with_bias else None
    mean, invstd, scale, shift = (torch.full((C,), NAN, device=DEV) for _ in range(4))
    assert lib.hpri_bn_eval_prepare(P(rm), P(rv), P(gamma), P(beta), EPS, C, P(mean), P(invstd), P(scale), P(shift), _st()) == 0
    fsc, fb = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    assert lib.hpri_bn_fold(P(rm), P(rv), P(gamma), P(beta), P(cb), EPS, C, P(fsc), P(fb), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(mean, rm)
    rm64, rv64, g64, b64 = rm.double(), rv.double(), gamma.double(), beta.double()
    ris = 1.0 / torch.sqrt(rv64 + EPS32)
    tol_is = 4 * U * ris
    rsc = g64 * ris
    tol_sc = g64.abs() * tol_is + U * rsc.abs()
    rsh = b64 - rm64 * rsc
    tol_sh = rm64.abs() * tol_sc + 2 * U * (b64.abs() + 2 * (rm64 * rsc).abs())
    key = f"bn/eval/C{C}/bias{int(with_bias)}"
    _gate(key + "/invstd", (invstd.double() - ris).abs(), tol_is)
    _gate(key + "/scale", (scale.double() - rsc).abs(), tol_sc)
    _gate(key + "/shift", (shift.double() - rsh).abs(), tol_sh)
    _gate(key + "/fold_scale", (fsc.double() - rsc).abs(), tol_sc)
    d = (cb.double() if with_bias else torch.zeros_like(rm64)) - rm64
    rfb = d * rsc + b64
    tol_fb = d.abs() * tol_sc + 3 * U * ((d * rsc).abs() + d.abs() * rsc.abs() + b64.abs())
    _gate(key + "/fold_bias", (fb.double() - rfb).abs(), tol_fb)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. normalise + ReLU
# ------------------------------------------------------------------------------------------------------------------------------
# (G, pixels per group, C, Cw, x_cs, x_coff, y_cs, y_coff): pixel counts that do not divide a workgroup's rows * 4, one pixel per
# group, C not a multiple of 4, C above 1024 (SpectralUNET-1650), channel-slice views on both sides
GEOM = [
    (1, 1, 5, 8, 8, 0, 8, 0),
    (3, 1, 3, 4, 12, 8, 4, 0),
    (2, 1001, 33, 36, 48, 8, 40, 4),
    (3, 777, 64, 64, 72, 4, 68, 0),
    (1, 50021, 1, 4, 8, 4, 4, 0),
    (1, 4099, 1650, 1652, 1660, 8, 1656, 4),
    (2, 513, 1650, 1652, 1652, 0, 1652, 0),
]


def _geom_params():
    out = []
    for g in GEOM:
        for w in ((1, 0) if g[2] > 1024 else (None,)):
            out.append(pytest.param(g, w, id=f"G{g[0]}xP{g[1]}xC{g[2]}" + ("" if w is None else f"-wide{w}")))
    return out


GEOM_PARAMS = _geom_params()


def _tensor(npx, C, Cw, cs, coff, seed, dt=torch.float32, offset=0.3, ties=None):
    """[npx][cs] view with channels [coff, coff + C) random, pad channels [coff + C, coff + Cw) NaN / +inf / -inf (the kernels must
    not let them through), everything outside the view NaN (never read).  ties = (mean per channel, fraction): that fraction of the
    pixels of every channel set to exactly the mean, the same again to one ulp above and one below it."""
    torch.manual_seed(seed)
    buf = torch.full((npx, cs), NAN, device=DEV)
    v = torch.randn(npx, C, device=DEV) * 1.5 + offset
    if ties is not None:
        mu, frac = ties
        r = torch.rand(npx, C, device=DEV)
        m = mu.view(1, C).expand(npx, C)
        v = torch.where(r < frac, m, v)
        v = torch.where((r >= frac) & (r < 2 * frac), torch.nextafter(m, torch.full_like(m, INF)), v)
        v = torch.where((r >= 2 * frac) & (r < 3 * frac), torch.nextafter(m, torch.full_like(m, -INF)), v)
    buf[:, coff:coff + C] = v
    if Cw > C:
        pat = torch.tensor([NAN, INF, -INF], device=DEV)
        buf[:, coff + C:coff + Cw] = pat[torch.arange(npx * (Cw - C), device=DEV) % 3].view(npx, Cw - C)
    return buf.to(dt)


def _stats(xv, G, C, seed, beta=None):
    """Per-group fp32 mean / invstd / scale / shift of xv [G * ppg][C] (what hpri_bn_finalize would give), [G * C] each."""
    torch.manual_seed(seed)
    x3 = xv.double().reshape(G, -1, C)
    mean = x3.mean(1).float()
    invstd = (1.0 / torch.sqrt(x3.var(1, unbiased=False) + EPS)).float()
    gamma = torch.randn(C, device=DEV) + 0.2
    beta = torch.randn(C, device=DEV) * 0.5 if beta is None else beta
    scale = gamma * invstd
    shift = beta - mean * scale
    return {k: v.reshape(-1).contiguous() for k, v in (("mean", mean), ("invstd", invstd), ("scale", scale), ("shift", shift))}


def _split(y, npl, dt):
    """The planes the kernels must write for fp32 values y: plane k = round-to-nearest-even of the residual after planes 0..k-1."""
    out, r = [], y.clone()
    for _ in range(npl):
        h = r.to(dt)
        out.append(h)
        r = r - h.float()
    return out


def _bits(t):
    return t.contiguous().view(torch.int16)


def _apply(lib, xbuf, xcs, xoff, y, ycs, yoff, st, npx, ppg, C, Cw, relu, planes=None, pl=(0, 0, 0, 0)):
    """One normalise + ReLU launch: hpri_bn_apply_relu_x16 for a 16-bit x, hpri_bn_apply_relu_pl otherwise (pl = plane stride,
    pl_cs, pl_coff, pl_cw; npl from the planes tensor's first dimension)."""
    npl = 0 if planes is None else planes.shape[0]
    fn = lib.hpri_bn_apply_relu_x16 if xbuf.dtype != torch.float32 else lib.hpri_bn_apply_relu_pl
    return fn(P(xbuf), xcs, xoff, P(y), ycs, yoff, P(st["scale"]), P(st["shift"]), npx, ppg, C, Cw, relu, P(planes), *pl, npl, _st())


def _planes(npx, C, Cw, npl, dt):
    pl_coff, pl_cw = 4, Cw + 4
    pl_cs = pl_coff + pl_cw + 4
    buf = torch.full((npl, npx, pl_cs), 3.0, dtype=dt, device=DEV)
    return buf, (npx * pl_cs, pl_cs, pl_coff, pl_cw)


def _check_planes(key, planes, pl, y, C):
    """planes == the RNE split of the kernel's own fp32 output y [npx][C], bit for bit; pad channels [C, pl_cw) exactly zero;
    nothing outside the plane view written."""
    _, pl_cs, pl_coff, pl_cw = pl
    want = _split(y, planes.shape[0], planes.dtype)
    for k in range(planes.shape[0]):
        got = planes[k]
        assert torch.equal(_bits(got[:, pl_coff:pl_coff + C]), _bits(want[k])), (key, "plane", k)
        assert torch.all(got[:, pl_coff + C:pl_coff + pl_cw] == 0), (key, "plane pad", k)
        assert torch.all(got[:, :pl_coff] == 3.0) and torch.all(got[:, pl_coff + pl_cw:] == 3.0), (key, "outside the plane view", k)


def _apply_ref(xv, st, G, C, relu):
    """fp64 y and the gate |y - ref| <= 2 U (|x * scale| + |shift|): at most one rounding of the product and one of the sum
    (none of the product when the compiler fuses them)."""
    x3 = xv.double().reshape(G, -1, C)
    sc, sh = st["scale"].double().view(G, 1, C), st["shift"].double().view(G, 1, C)
    ref = x3 * sc + sh
    tol = 2 * U * ((x3 * sc).abs() + sh.abs())
    if relu:
        ref = ref.clamp(min=0)
    return ref.reshape(-1, C), tol.reshape(-1, C)


@pytest.mark.parametrize("geom,wide", GEOM_PARAMS)
@pytest.mark.parametrize("relu", [1, 0])
def test_apply_relu_fp32_vs_fp64(lib, geom, wide, relu):
    """hpri_bn_apply_relu: y = relu(x * scale + shift) per group, elementwise against fp64; pad channels [C, Cw) of y exactly zero
    although x holds NaN / inf there (the header's contract); nothing outside y's view written."""
    G, ppg, C, Cw, xcs, xoff, ycs, yoff = geom
    npx = G * ppg
    xb = _tensor(npx, C, Cw, xcs, xoff, seed=C + ppg)
    xv = xb[:, xoff:xoff + C]
    st = _stats(xv, G, C, seed=3)
    y = torch.full((npx, ycs), 7.0, device=DEV)
    with _wide(lib, wide):
        rc = lib.hpri_bn_apply_relu(P(xb), xcs, xoff, P(y), ycs, yoff, P(st["scale"]), P(st["shift"]), npx, ppg, C, Cw, relu, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    ref, tol = _apply_ref(xv, st, G, C, relu)
    _gate(f"bn/apply/f32/G{G}xP{ppg}xC{C}/relu{relu}", (y[:, yoff:yoff + C].double() - ref).abs(), tol)
    assert torch.all(y[:, yoff + C:yoff + Cw] == 0), "pad channels of y must be zeros"
    assert torch.all(y[:, :yoff] == 7.0) and torch.all(y[:, yoff + Cw:] == 7.0)


# (npl, y written or planes only, x stored as 16-bit, relu)
APPLY16 = [(1, True, False, 1), (2, False, False, 0), (3, True, True, 1), (2, False, True, 1), (1, True, True, 0)]


@pytest.mark.parametrize("geom,wide", GEOM_PARAMS)
@pytest.mark.parametrize("npl,with_y,x16,relu", APPLY16)
def test_apply_relu_planes_and_16bit_input(lib16, geom, wide, npl, with_y, x16, relu):
    """hpri_bn_apply_relu_pl / _x16 with plane outputs (pl_cw > Cw, pl_coff > 0) and the planes-only form (y == NULL): y against
    fp64 (for a 16-bit x the reference takes the stored values widened exactly), planes bit for bit the split of y."""
    lib, dt = lib16
    G, ppg, C, Cw, xcs, xoff, ycs, yoff = geom
    npx = G * ppg
    xb = _tensor(npx, C, Cw, xcs, xoff, seed=C + ppg + 1, dt=dt if x16 else torch.float32)
    xv = xb[:, xoff:xoff + C]
    st = _stats(xv.float(), G, C, seed=4)
    y = torch.full((npx, ycs), 7.0, device=DEV)
    planes, pl = _planes(npx, C, Cw, npl, dt)
    with _wide(lib, wide):
        if with_y:
            rc = _apply(lib, xb, xcs, xoff, y, ycs, yoff, st, npx, ppg, C, Cw, relu, planes, pl)
        else:
            rc = _apply(lib, xb, xcs, xoff, y, ycs, yoff, st, npx, ppg, C, Cw, relu)
            assert rc == 0, lib.hpri_last_error()
            rc = _apply(lib, xb, xcs, xoff, None, ycs, yoff, st, npx, ppg, C, Cw, relu, planes, pl)
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    key = f"bn/apply/{dt}/G{G}xP{ppg}xC{C}/npl{npl}/y{int(with_y)}/x16{int(x16)}/relu{relu}"
    ref, tol = _apply_ref(xv, st, G, C, relu)
    yv = y[:, yoff:yoff + C]
    _gate(key, (yv.double() - ref).abs(), tol)
    assert torch.all(y[:, yoff + C:yoff + Cw] == 0), "pad channels of y must be zeros"
    _check_planes(key, planes, pl, yv, C)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. backward
# ------------------------------------------------------------------------------------------------------------------------------
def _bwd(lib, kind, dyb, dycs, dyoff, xb, xcs, xoff, dx, dxcs, dxoff, st, dgam, dbet, acc_pg, dbias, acc_db, ws, npx, ppg, C, Cw,
         relu, ubs, planes=None, pl=(0, 0, 0, 0), part=None):
    """One BatchNorm(+ReLU) backward launch.  kind: "f32" hpri_bn_relu_bwd, "pl" hpri_bn_relu_bwd_pl, "x16" hpri_bn_relu_bwd_x16,
    "x16dy16" hpri_bn_relu_bwd_x16_dy16, "fused" hpri_bn_relu_bwd_fused (part = (rows, nrows, cpart))."""
    npl = 0 if planes is None else planes.shape[0]
    head = (P(dyb), dycs, dyoff, P(xb), xcs, xoff, P(dx), dxcs, dxoff, P(st["mean"]), P(st["invstd"]), P(st["scale"]),
            P(st["shift"]), P(dgam), P(dbet), acc_pg, P(dbias), acc_db, P(ws), 0 if ws is None else ws.numel(), npx, ppg, C, Cw, relu, ubs)
    tail = (P(planes), *pl, npl, _st())
    if kind == "f32":
        return lib.hpri_bn_relu_bwd(*head, _st())
    if kind == "fused":
        return lib.hpri_bn_relu_bwd_fused(P(part[0]), part[1], part[2], *head, *tail)
    return getattr(lib, {"pl": "hpri_bn_relu_bwd_pl", "x16": "hpri_bn_relu_bwd_x16", "x16dy16": "hpri_bn_relu_bwd_x16_dy16"}[kind])(*head, *tail)


def _ws(lib, ppg, G, C, extra=0):
    nblk, cpart, _, _ = _plan(lib, ppg, G, C)
    return torch.full((2 * (G * nblk * 2 * cpart + G * 2 * C) + extra,), NAN, device=DEV)


def _bwd_ref(dy, xv, mask, st, G, C, ubs, tol_rel):
    """fp64 backward of y = relu(x * scale + shift) with the batch statistics of each group: g = dy * mask, dx = scale * (g - mean(g)
    - xhat * mean(g * xhat)) (eval form: scale * g); dgamma = sum g * xhat, dbeta = sum g over all groups.  Returns the references
    and elementwise bounds: the two sums within tol_rel of the sums of the absolute values of their terms (kernel chain length),
    then three fp32 roundings of each k = sum / Np, four of each term of dx."""
    g = (dy.double() * mask).reshape(G, -1, C)
    x3 = xv.double().reshape(G, -1, C)
    mu, istd, sc = (st[k].double().view(G, 1, C) for k in ("mean", "invstd", "scale"))
    xh = (x3 - mu) * istd
    Np = g.shape[1]
    s1, s2 = g.sum(1), (g * xh).sum(1)
    a1, a2 = g.abs().sum(1), (g * xh).abs().sum(1)
    if ubs:
        k1, k2 = (s1 / Np)[:, None], (s2 / Np)[:, None]
        d1 = tol_rel * (a1 / Np)[:, None] + 3 * U * k1.abs()
        d2 = tol_rel * (a2 / Np)[:, None] + 3 * U * k2.abs()
        dx = sc * (g - k1 - xh * k2)
        tol = sc.abs() * (4 * U * (g.abs() + k1.abs() + 2 * (xh * k2).abs()) + d1 + xh.abs() * d2)
    else:
        dx = sc * g
        tol = 2 * U * dx.abs()          # one rounding (< U relative); k = 2 leaves room for an extra one in the same formula
    return dict(dx=dx.reshape(-1, C), tol_dx=tol.reshape(-1, C), dgamma=s2.sum(0), dbeta=s1.sum(0), a_gamma=a2.sum(0), a_beta=a1.sum(0))


def _mask_from_forward(lib, xb, xcs, xoff, st, npx, ppg, C, Cw, relu):
    """[y > 0] of the forward kernel's own output (hpri_bn_apply_relu(_x16)): the backward must pass the gradient exactly there."""
    if not relu:
        return torch.ones(npx, C, dtype=torch.bool, device=DEV)
    y = torch.empty(npx, rup(Cw, 4), device=DEV)
    assert _apply(lib, xb, xcs, xoff, y, y.shape[1], 0, st, npx, ppg, C, Cw, 1) == 0, lib.hpri_last_error()
    return y[:, :C] > 0


def _check_bwd(key, lib, res, ref, G, C, L, rows, init, acc_pg, acc_db, ubs, dbias_ref=None):
    """dx (when written), dgamma / dbeta with the accumulate flag, and dbias: training mode -> exact zeros, or unchanged when
    accumulating; eval mode -> the column sum of dx."""
    dx, dgam, dbet, dbias = res
    dg0, db0, dbias0 = init
    if dx is not None:
        _gate(key + "/dx", (dx.double() - ref["dx"]).abs(), ref["tol_dx"])
    # fp32 chains of the reduction, then G fp32 additions of the group sums (bn_param_grad_kernel), then the accumulate rounding
    tol_rel = (L + G + 8) * U
    for got, name, a, base in ((dgam, "dgamma", ref["a_gamma"], dg0), (dbet, "dbeta", ref["a_beta"], db0)):
        want = ref[name] + (base.double() if acc_pg else 0.0)
        tol = tol_rel * a + 2 * U * (want.abs() + (base.double().abs() if acc_pg else 0.0))
        _gate(f"{key}/{name}", (got.double() - want).abs(), tol)
    if ubs:
        want = dbias0 if acc_db else torch.zeros_like(dbias0)
        assert torch.equal(dbias, want), "training mode: dbias is exact zeros, or unchanged when accumulating"
    else:
        s, a = dbias_ref
        want = s + (dbias0.double() if acc_db else 0.0)
        tol = tol_rel * a + 2 * U * (want.abs() + (dbias0.double().abs() if acc_db else 0.0))
        _gate(f"{key}/dbias", (dbias.double() - want).abs(), tol)


# (kind, relu, use_batch_stats, accumulate both, npl, dx written)
BWD32 = [("f32", 1, 1, 0, 0, True), ("f32", 0, 1, 1, 0, True), ("f32", 1, 0, 0, 0, True), ("f32", 1, 0, 1, 0, True)]
BWD16 = [("pl", 1, 1, 0, 2, True), ("pl", 1, 0, 1, 3, False), ("x16", 1, 1, 1, 1, True), ("x16dy16", 1, 1, 0, 0, True),
         ("x16dy16", 0, 0, 0, 2, False)]


def _run_bwd_case(lib, dt, kind, geom, relu, ubs, acc, npl, with_dx):
    G, ppg, C, Cw, xcs, xoff, dxcs, dxoff = geom
    dycs, dyoff = Cw + 12, 8
    npx = G * ppg
    x16 = kind in ("x16", "x16dy16")
    xb = _tensor(npx, C, Cw, xcs, xoff, seed=C + ppg + 2, dt=dt if x16 else torch.float32)
    dyb = _tensor(npx, C, Cw, dycs, dyoff, seed=C + ppg + 3, dt=dt if kind == "x16dy16" else torch.float32, offset=0.0)
    xv, dyv = xb[:, xoff:xoff + C], dyb[:, dyoff:dyoff + C]
    st = _stats(xv.float(), G, C, seed=5)
    mask = _mask_from_forward(lib, xb, xcs, xoff, st, npx, ppg, C, Cw, relu)
    torch.manual_seed(9)
    dg0, db0, dbias0 = torch.randn(C, device=DEV), torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    dgam, dbet, dbias = dg0.clone(), db0.clone(), dbias0.clone()
    dx = torch.full((npx, dxcs), 7.0, device=DEV)
    planes, pl = _planes(npx, C, Cw, npl, dt) if npl else (None, (0, 0, 0, 0))
    ws = _ws(lib, ppg, G, C)
    rc = _bwd(lib, kind, dyb, dycs, dyoff, xb, xcs, xoff, dx, dxcs, dxoff, st, dgam, dbet, acc, dbias, acc, ws, npx, ppg, C, Cw,
              relu, ubs, planes, pl)
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    _, _, rows, L = _plan(lib, ppg, G, C)
    ref = _bwd_ref(dyv.float(), xv.float(), mask, st, G, C, ubs, (L + 8) * U)
    key = f"bn/bwd/{kind}/{dt}/G{G}xP{ppg}xC{C}/relu{relu}/ubs{ubs}/acc{acc}"
    dxv = dx[:, dxoff:dxoff + C]
    dbias_ref = (ref["dx"].sum(0), ref["dx"].abs().sum(0)) if not ubs else None
    _check_bwd(key, lib, (dxv, dgam, dbet, dbias), ref, G, C, L, rows, (dg0, db0, dbias0), acc, acc, ubs, dbias_ref)
    assert torch.all(dx[:, dxoff + C:dxoff + Cw] == 0), "pad channels of dx must be zeros"
    assert torch.all(dx[:, :dxoff] == 7.0) and torch.all(dx[:, dxoff + Cw:] == 7.0)
    if planes is None:
        return
    _check_planes(key, planes, pl, dxv, C)
    if not with_dx:
        # the planes-only form (dx == NULL) writes the same planes
        p2, _ = _planes(npx, C, Cw, npl, dt)
        rc = _bwd(lib, kind, dyb, dycs, dyoff, xb, xcs, xoff, None, dxcs, dxoff, st, None, None, 0, None, 0, ws, npx, ppg, C, Cw,
                  relu, ubs, p2, pl)
        assert rc == 0, lib.hpri_last_error()
        torch.cuda.synchronize()
        assert torch.equal(_bits(p2), _bits(planes)), "planes-only backward differs from the planes written beside dx"


@pytest.mark.parametrize("geom,wide", GEOM_PARAMS)
@pytest.mark.parametrize("kind,relu,ubs,acc,npl,with_dx", BWD32)
def test_bn_relu_bwd_fp32_vs_fp64(lib, geom, wide, kind, relu, ubs, acc, npl, with_dx):
    with _wide(lib, wide):
        _run_bwd_case(lib, torch.bfloat16, kind, geom, relu, ubs, acc, npl, with_dx)


@pytest.mark.parametrize("geom,wide", GEOM_PARAMS)
@pytest.mark.parametrize("kind,relu,ubs,acc,npl,with_dx", BWD16)
def test_bn_relu_bwd_16bit_forms_vs_fp64(lib16, geom, wide, kind, relu, ubs, acc, npl, with_dx):
    """hpri_bn_relu_bwd_pl / _x16 / _x16_dy16: planes (also planes only), a 16-bit pre-BN tensor and a 16-bit incoming gradient
    (the reference reads the stored values widened exactly)."""
    lib, dt = lib16
    with _wide(lib, wide):
        _run_bwd_case(lib, dt, kind, geom, relu, ubs, acc, npl, with_dx)


# CubeNET's full-size layer: two 608 x 968 cubes, 64 channels (the plan: 1024 blocks of ~575 pixels, the longest fp32 chains)
FULL = (2, 608, 968, 64)


def test_bn_relu_bwd_full_size_layer_vs_fp64(lib):
    N, H, W, C = FULL
    npx = N * H * W
    xb = _tensor(npx, C, C, C, 0, seed=21)
    dyb = _tensor(npx, C, C, C, 0, seed=22, offset=0.0)
    st = _stats(xb, 1, C, seed=23)
    mask = _mask_from_forward(lib, xb, C, 0, st, npx, npx, C, C, 1)
    dg0, db0, dbias0 = torch.randn(C, device=DEV), torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    dgam, dbet, dbias = dg0.clone(), db0.clone(), dbias0.clone()
    dx = torch.empty(npx, C, device=DEV)
    ws = _ws(lib, npx, 1, C)
    rc = _bwd(lib, "f32", dyb, C, 0, xb, C, 0, dx, C, 0, st, dgam, dbet, 1, dbias, 0, ws, npx, npx, C, C, 1, 1)
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    nblk, _, rows, L = _plan(lib, npx, 1, C)
    assert nblk == 1024
    ref = _bwd_ref(dyb, xb, mask, st, 1, C, 1, (L + 8) * U)
    _check_bwd("bn/bwd/f32/full", lib, (dx, dgam, dbet, dbias), ref, 1, C, L, rows, (dg0, db0, dbias0), 1, 0, 1)


@pytest.mark.parametrize("G,ppg,C,Cw", [(1, 3001, 5, 8), (2, 1500, 64, 64), (1, 2000, 33, 36)])
def test_backward_mask_matches_forward_at_ties(lib16, G, ppg, C, Cw):
    """Pixels where x * scale + shift is exactly 0 or within an ulp of it (x == mean and beta = 0, x one ulp either side of the mean;
    half the channels have a scale of few bits, where the product is exact and the tie is exact): the backward (eval form: dx =
    scale * g, so dx != 0 exactly where the mask passes) must pass the gradient exactly where the forward kernel's y > 0 -- fp32
    and 16-bit x, bit for bit.  Training form: the reduction sweep's mask agrees too (sums within the chain bound of the fp64 sums
    taken with the forward mask; one flipped tie would move them by a whole gradient value)."""
    lib, dt = lib16
    npx = G * ppg
    torch.manual_seed(31)
    mean = (torch.randint(-64, 64, (G, C), device=DEV).float() + 0.5) / 16       # exactly representable in both 16-bit types
    invstd = torch.rand(G, C, device=DEV) + 0.5
    gamma = torch.randn(C, device=DEV)
    few = torch.arange(C, device=DEV) % 2 == 0
    invstd = torch.where(few, torch.full_like(invstd, 0.5), invstd)
    gamma = torch.where(few, (torch.randint(1, 16, (C,), device=DEV).float() / 8), gamma)
    scale = gamma * invstd
    shift = 0.0 - mean * scale
    st = {k: v.reshape(-1).contiguous() for k, v in (("mean", mean), ("invstd", invstd), ("scale", scale), ("shift", shift))}
    for x16 in (False, True):
        xbs = []
        for g in range(G):
            xbs.append(_tensor(ppg, C, Cw, Cw, 0, seed=40 + g, ties=(mean[g], 0.15)))
        xb = torch.cat(xbs)
        if x16:
            xb = xb.to(dt)
        xv = xb[:, :C]
        y = torch.empty(npx, Cw, device=DEV)
        assert _apply(lib, xb, Cw, 0, y, Cw, 0, st, npx, ppg, C, Cw, 1) == 0, lib.hpri_last_error()
        dyb = torch.rand(npx, Cw, device=DEV) + 0.5
        kind = "x16" if x16 else "pl"
        dx = torch.empty(npx, Cw, device=DEV)
        ws = _ws(lib, ppg, G, C)
        rc = _bwd(lib, kind, dyb, Cw, 0, xb, Cw, 0, dx, Cw, 0, st, None, None, 0, None, 0, ws, npx, ppg, C, Cw, 1, 0)
        assert rc == 0, lib.hpri_last_error()
        torch.cuda.synchronize()
        fwd = y[:, :C] > 0
        on_tie = (xv.float() == mean.repeat_interleave(ppg, 0)).sum()
        assert int(on_tie) > 0
        assert torch.equal(dx[:, :C] != 0, fwd), f"x16={x16}: backward mask differs from the forward's y > 0"
        dgam, dbet = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        rc = _bwd(lib, kind, dyb, Cw, 0, xb, Cw, 0, dx, Cw, 0, st, dgam, dbet, 0, None, 0, ws, npx, ppg, C, Cw, 1, 1)
        assert rc == 0, lib.hpri_last_error()
        torch.cuda.synchronize()
        _, _, rows, L = _plan(lib, ppg, G, C)
        ref = _bwd_ref(dyb[:, :C], xv.float(), fwd, st, G, C, 1, (L + 8) * U)
        _check_bwd(f"bn/ties/{dt}/G{G}xC{C}/x16{int(x16)}", lib, (dx[:, :C], dgam, dbet, torch.zeros(C, device=DEV)), ref, G, C, L,
                   rows, (torch.zeros(C, device=DEV),) * 3, 0, 0, 1)


def _row_sums(g, xh, row_of, nrows, C):
    """fp64 sums of g and g * xhat per partial row (row_of: row index of every pixel) and the sums of their absolute values."""
    s = torch.zeros(nrows, 4, C, dtype=torch.float64, device=DEV)
    gx = g * xh
    s[:, 0].index_add_(0, row_of, g)
    s[:, 1].index_add_(0, row_of, gx)
    s[:, 2].index_add_(0, row_of, g.abs())
    s[:, 3].index_add_(0, row_of, gx.abs())
    return s


def _fused_vs_unfused(lib, key, part, nrows, cpart, g, xb, st, mask, npx, C, Cw, L_fused):
    """hpri_bn_relu_bwd_fused on partial rows against fp64 and against hpri_bn_relu_bwd_pl doing its own sweeps on the same
    inputs (with planes, so both plane paths are compared too)."""
    outs = []
    for fused in (True, False):
        dg0, db0, dbias0 = torch.full((C,), 0.5, device=DEV), torch.full((C,), -0.25, device=DEV), torch.full((C,), 2.0, device=DEV)
        dgam, dbet, dbias = dg0.clone(), db0.clone(), dbias0.clone()
        dx = torch.full((npx, Cw), 7.0, device=DEV)
        planes, pl = _planes(npx, C, Cw, 1, torch.bfloat16)
        ws = _ws(lib, npx, 1, C)
        rc = _bwd(lib, "fused" if fused else "pl", g, Cw, 0, xb, xb.shape[1], 0, dx, Cw, 0, st, dgam, dbet, 1, dbias, 1, ws, npx, npx, C,
                  Cw, 1, 1, planes, pl, part=(part, nrows, cpart))
        assert rc == 0, lib.hpri_last_error()
        torch.cuda.synchronize()
        _, _, rows, L = _plan(lib, npx, 1, C)
        L = L_fused if fused else L
        ref = _bwd_ref(g[:, :C], xb[:, :C], mask, st, 1, C, 1, (L + 8) * U)
        _check_bwd(f"{key}/{'fused' if fused else 'unfused'}", lib, (dx[:, :C], dgam, dbet, dbias), ref, 1, C, L, rows, (dg0, db0, dbias0),
                   1, 1, 1)
        assert torch.all(dx[:, C:Cw] == 0)
        _check_planes(key, planes, pl, dx[:, :C], C)
        tol_g = (L + 9) * U * ref["a_gamma"] + 2 * U * (dgam.double().abs() + 0.5)
        tol_b = (L + 9) * U * ref["a_beta"] + 2 * U * (dbet.double().abs() + 0.25)
        outs.append((dx[:, :C].double(), dgam.double(), dbet.double(), ref["tol_dx"], tol_g, tol_b))
    a, b = outs
    for i, what in ((0, "dx"), (1, "dgamma"), (2, "dbeta")):     # each within its own bound of fp64, so within the sum of each other
        _gate(f"{key}/fused_vs_unfused_{what}", (a[i] - b[i]).abs(), a[3 + i] + b[3 + i])


@pytest.mark.parametrize("npx,C,Cw,nrows", [(3001, 33, 36, 7), (FULL[0] * FULL[1] * FULL[2], FULL[3], FULL[3], 9272)])
def test_bn_relu_bwd_fused_on_synthetic_rows(lib, npx, C, Cw, nrows):
    """hpri_bn_relu_bwd_fused fed partial rows [rows][2][cpart] computed in fp64 and rounded to fp32: a small layer that skips the
    folding launch (col_fold_kernel: S >= 4 and rows >= 16 S) and the full-size layer (9272 rows) that takes it."""
    xb = _tensor(npx, C, Cw, Cw, 0, seed=51)
    g = _tensor(npx, C, Cw, Cw, 0, seed=52, offset=0.0)
    st = _stats(xb[:, :C], 1, C, seed=53)
    mask = _mask_from_forward(lib, xb, Cw, 0, st, npx, npx, C, Cw, 1)
    nblk, cpart_plan, _, _ = _plan(lib, npx, 1, C)
    cpart = rup(C, 64)
    S = min(64, (nblk * 2 * cpart_plan) // (2 * cpart))
    assert (S >= 4 and nrows >= 16 * S) == (nrows > 1000)
    row_of = torch.arange(npx, device=DEV) * nrows // npx
    gm = g[:, :C].double() * mask
    xh = (xb[:, :C].double() - st["mean"].double()) * st["invstd"].double()
    s = _row_sums(gm, xh, row_of, nrows, C)
    part = torch.full((nrows, 2, cpart), NAN, device=DEV)
    part[:, :, :C] = s[:, :2].float()
    # the rows are single roundings of exact sums (U each), summed in double
    _fused_vs_unfused(lib, f"bn/fused/synthetic/P{npx}xC{C}", part, nrows, cpart, g, xb, st, mask, npx, C, Cw, 2)


@pytest.mark.parametrize("N,H,W,K,C", [(1, 37, 45, 24, 40), (FULL[0], FULL[1], FULL[2], 64, FULL[3])])
def test_wino4_bnred_rows_and_fused_chain(lib, N, H, W, K, C):
    """hpri_conv_wino4_bnred: the data gradient g of a 3x3 layer plus, per 16 x 8-pixel tile, sum g * [BN(x) > 0] and
    sum g * [BN(x) > 0] * xhat of the BatchNorm + ReLU stage whose pre-BN tensor x sits at g's positions.  The rows against fp64
    sums of the kernel's own g, with the mask of hpri_bn_apply_relu (x holds exact and one-ulp ties: the two kernels must agree
    on them); then the chain into hpri_bn_relu_bwd_fused against the fp64 backward and the unfused kernel.  Ragged tiles on the
    small shape; the full-size layer takes the folding launch."""
    npx = N * H * W
    Kp, Cp = rup(K, 8), rup(C, 64)
    Cw = rup(C, 4)
    torch.manual_seed(61)
    d = torch.zeros(npx, Kp, device=DEV)
    d[:, :K] = torch.randn(npx, K, device=DEV)
    w = torch.randn(K, C, 3, 3, device=DEV) * 0.1
    up = torch.empty(lib.hpri_wino_packed_floats(K, Cp), device=DEV)
    assert lib.hpri_wino4_pack(P(w), P(up), P(None), 1, K, C, Cp, C, _st()) == 0
    mean = (torch.randint(-64, 64, (C,), device=DEV).float() + 0.5) / 16
    xb = torch.zeros(npx, Cp, device=DEV)
    xb[:, :C] = _tensor(npx, C, C, C, 0, seed=62, ties=(mean, 0.1))
    invstd = torch.rand(C, device=DEV) + 0.5
    gamma = torch.randn(C, device=DEV)
    scale = gamma * invstd
    shift = 0.0 - mean * scale
    st = {"mean": mean, "invstd": invstd, "scale": scale, "shift": shift}
    tl = ctypes.c_int()
    lib.hpri_conv_wino4_plan(N, H, W, ctypes.byref(tl))
    tiles_x, tiles_y = -(-W // 16), -(-H // 8)
    nrows = tl.value                                      # tiles of all N images
    assert nrows == N * tiles_x * tiles_y
    part = torch.full((nrows, 2, Cp), NAN, device=DEV)
    g = torch.full((npx, Cw), NAN, device=DEV)
    rc = lib.hpri_conv_wino4_bnred(P(d), Kp, 0, P(up), P(g), Cw, 0, N, H, W, Kp, C, Cp, Cw, P(xb), Cp, 0, P(mean), P(invstd), P(scale),
                                   P(shift), 1, P(part), Cp, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(g).all()
    mask = _mask_from_forward(lib, xb, Cp, 0, st, npx, npx, C, Cw, 1)
    pix = torch.arange(npx, device=DEV)
    img, rem = pix // (H * W), pix % (H * W)
    row_of = img * (tiles_x * tiles_y) + (rem // W // 8) * tiles_x + (rem % W) // 16
    gm = g[:, :C].double() * mask
    xh = (xb[:, :C].double() - mean.double()) * invstd.double()
    s = _row_sums(gm, xh, row_of, nrows, C)
    got = part[:, :, :C].double()
    assert torch.isfinite(got).all()
    # per tile: 8 pixels per thread, then 16 thread rows, all fp32; the terms carry up to three roundings (xhat and the product)
    tol_rel = (8 + 16 + 4) * U
    key = f"bn/wino4_bnred/{N}x{H}x{W}x{K}x{C}"
    _gate(key + "/rows_sum_g", (got[:, 0] - s[:, 0]).abs(), tol_rel * s[:, 2])
    _gate(key + "/rows_sum_gxhat", (got[:, 1] - s[:, 1]).abs(), tol_rel * s[:, 3])
    assert torch.all(part[:, :, C:] == 0), "pad columns of the partial rows: exact zeros"
    # the rows are fp32 chains of 8 + 16; folding and finalize sum them in double
    _fused_vs_unfused(lib, key, part, nrows, Cp, g, xb, st, mask, npx, C, Cw, 8 + 16 + 4)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. column sums
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npx,C,cs,coff", [(1, 1, 4, 0), (1001, 33, 48, 8), (4099, 5, 12, 4), (77777, 1650, 1660, 8), (300001, 64, 72, 4)])
@pytest.mark.parametrize("acc", [0, 1])
def test_col_sum_vs_fp64(lib, npx, C, cs, coff, acc):
    """hpri_col_sum: out[c] (+)= sum over the pixels of src[p][coff + c], ragged pixel counts, C not a multiple of 4, a sliced source
    whose pad channels hold NaN / inf (they must not reach out)."""
    src = _tensor(npx, C, rup(C, 4), cs, coff, seed=71, offset=0.2)
    torch.manual_seed(72)
    out0 = torch.randn(C, device=DEV)
    out = out0.clone()
    nblk, cpart, rows, L = _plan(lib, npx, 1, C)
    ws = torch.full((nblk * 2 * cpart + 2 * C,), NAN, device=DEV)
    rc = lib.hpri_col_sum(P(src), cs, coff, P(out), acc, P(ws), ws.numel(), npx, C, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    v = src[:, coff:coff + C].double()
    want = v.sum(0) + (out0.double() if acc else 0.0)
    tol = (L + 8) * U * v.abs().sum(0) + 2 * U * (want.abs() + (out0.double().abs() if acc else 0.0))
    _gate(f"bn/col_sum/P{npx}xC{C}/acc{acc}", (out.double() - want).abs(), tol)


@pytest.mark.parametrize("tiles,Cpad,c0,C", [(1, 64, 4, 7), (333, 72, 8, 61), (9272, 128, 64, 64), (4600, 1664, 12, 1650), (517, 8, 4, 3)])
@pytest.mark.parametrize("acc", [0, 1])
def test_colsum_from_stats_vs_fp64(lib, tiles, Cpad, c0, C, acc):
    """hpri_colsum_from_stats: out[c] (+)= sum over tiles of mean * count of channel c0 + c, tiles with uneven counts; records of
    the other channels hold NaN (never read).  Double accumulation: one rounding to fp32 (and one for the accumulate)."""
    torch.manual_seed(81 + tiles)
    rec = torch.full((tiles, Cpad, 4), NAN, device=DEV)
    cnt = torch.randint(1, 129, (tiles, 1), device=DEV).float().expand(tiles, C)
    rec[:, c0:c0 + C, 0] = torch.randn(tiles, C, device=DEV) + 0.1
    rec[:, c0:c0 + C, 1] = torch.rand(tiles, C, device=DEV)
    rec[:, c0:c0 + C, 2] = cnt
    rec[:, c0:c0 + C, 3] = 0.0
    out0 = torch.randn(C, device=DEV)
    out = out0.clone()
    rc = lib.hpri_colsum_from_stats(P(rec), tiles, Cpad, c0, C, P(out), acc, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    t = rec[:, c0:c0 + C, 0].double() * rec[:, c0:c0 + C, 2].double()
    want = t.sum(0) + (out0.double() if acc else 0.0)
    tol = (tiles // 64 + 128) * U64 * t.abs().sum(0) + 2 * U * (want.abs() + (out0.double().abs() if acc else 0.0))
    _gate(f"bn/colsum_from_stats/T{tiles}xC{C}/acc{acc}", (out.double() - want).abs(), tol)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. error returns
# ------------------------------------------------------------------------------------------------------------------------------
def test_error_returns_launch_nothing(lib16):
    """Every refused call returns its HPRI_ERR_* and leaves every output as it was (nothing launched)."""
    lib, dt = lib16
    G, ppg, C, Cw = 2, 100, 6, 8
    npx = G * ppg
    xb = torch.randn(npx, Cw, device=DEV)
    xw = torch.randn(npx, 16, device=DEV)                 # room for a view at channel offset 2
    dyb = torch.randn(npx, Cw, device=DEV)
    st = _stats(xb[:, :C], G, C, seed=91)
    outs = {k: torch.full((G * C,), 5.0, device=DEV) for k in ("m", "i", "v", "s", "h")}
    y = torch.full((npx, Cw), 5.0, device=DEV)
    dx = torch.full((npx, Cw), 5.0, device=DEV)
    dgam, dbet, dbias = (torch.full((C,), 5.0, device=DEV) for _ in range(3))
    col = torch.full((C,), 5.0, device=DEV)
    planes, pl = _planes(npx, C, Cw, 1, dt)
    rec = torch.zeros(8, Cw, 4, device=DEV)                # (4 tiles are passed: room beyond them)
    gamma = torch.ones(C, device=DEV)
    ws = _ws(lib, ppg, G, C)
    ws_small = ws[:ws.numel() - 1]
    x16 = torch.zeros(npx * Cw + 8, dtype=dt, device=DEV)
    x16m = x16[1:]                                         # 2-byte offset: not 8-byte aligned
    nblk, cpart, _, _ = _plan(lib, npx, 1, C)
    ws_col = torch.zeros(nblk * 2 * cpart + 2 * C, device=DEV)
    part = torch.zeros(4, 2, 64, device=DEV)

    def bwd(kind="pl", dyb_=dyb, xb_=xb, xcs=Cw, xoff=0, ws_=ws, P_=npx, ppg_=ppg, Cw_=Cw, part_=None):
        return _bwd(lib, kind, dyb_, Cw, 0, xb_, xcs, xoff, dx, Cw, 0, st, dgam, dbet, 0, dbias, 0, ws_, P_, ppg_, C, Cw_, 1, 1, planes, pl,
                    part=part_)

    cases = [
        ("finalize: null mean", ERR_ARG, lambda: lib.hpri_bn_finalize(P(rec), 4, 1, Cw, C, P(gamma), P(gamma), EPS, 0.1, P(None), P(outs["i"]),
                                                                      P(outs["v"]), P(outs["s"]), P(outs["h"]), P(None), P(None), P(None), _st())),
        ("apply: null x", ERR_ARG, lambda: lib.hpri_bn_apply_relu(P(None), Cw, 0, P(y), Cw, 0, P(st["scale"]), P(st["shift"]), npx, ppg, C, Cw, 1, _st())),
        ("apply: Cw % 4", ERR_ARG, lambda: lib.hpri_bn_apply_relu(P(xb), Cw, 0, P(y), Cw, 0, P(st["scale"]), P(st["shift"]), npx, ppg, C, 6, 1, _st())),
        ("apply: x_coff % 4", ERR_ARG, lambda: lib.hpri_bn_apply_relu(P(xw), 16, 2, P(y), Cw, 0, P(st["scale"]), P(st["shift"]), npx, ppg, C, Cw, 1, _st())),
        ("apply: P % ppg", ERR_ARG, lambda: lib.hpri_bn_apply_relu(P(xb), Cw, 0, P(y), Cw, 0, P(st["scale"]), P(st["shift"]), npx, 99, C, Cw, 1, _st())),
        ("apply_x16: misaligned", ERR_ARG, lambda: _apply(lib, x16m.view(-1), Cw, 0, y, Cw, 0, st, npx, ppg, C, Cw, 1, planes, pl)),
        ("bwd: null dy", ERR_ARG, lambda: bwd(dyb_=None)),
        ("bwd: Cw % 4", ERR_ARG, lambda: bwd(Cw_=6)),
        ("bwd: x_coff % 4", ERR_ARG, lambda: bwd(xb_=xw, xcs=16, xoff=2)),
        ("bwd: P % ppg", ERR_ARG, lambda: bwd(ppg_=99)),
        ("bwd: workspace one float short", ERR_WORKSPACE, lambda: bwd(ws_=ws_small)),
        ("bwd_x16: misaligned x", ERR_ARG, lambda: bwd(kind="x16", xb_=x16m)),
        ("bwd_x16_dy16: misaligned dy", ERR_ARG, lambda: bwd(kind="x16dy16", dyb_=x16m, xb_=x16[:npx * Cw])),
        ("bwd_fused: cpart < C", ERR_ARG, lambda: _bwd(lib, "fused", dyb, Cw, 0, xb, Cw, 0, dx, Cw, 0, st, dgam, dbet, 0, dbias, 0,
                                                       _ws(lib, npx, 1, C), npx, npx, C, Cw, 1, 1, planes, pl, part=(part, 4, 4))),
        ("bwd_fused: null rows", ERR_ARG, lambda: _bwd(lib, "fused", dyb, Cw, 0, xb, Cw, 0, dx, Cw, 0, st, dgam, dbet, 0, dbias, 0,
                                                       _ws(lib, npx, 1, C), npx, npx, C, Cw, 1, 1, planes, pl, part=(None, 4, 64))),
        ("col_sum: null src", ERR_ARG, lambda: lib.hpri_col_sum(P(None), Cw, 0, P(col), 0, P(ws_col), ws_col.numel(), npx, C, _st())),
        ("col_sum: coff % 4", ERR_ARG, lambda: lib.hpri_col_sum(P(xw), 16, 2, P(col), 0, P(ws_col), ws_col.numel(), npx, C, _st())),
        ("col_sum: workspace one float short", ERR_WORKSPACE,
         lambda: lib.hpri_col_sum(P(xb), Cw, 0, P(col), 0, P(ws_col), ws_col.numel() - 1, npx, C, _st())),
        ("colsum_from_stats: null", ERR_ARG, lambda: lib.hpri_colsum_from_stats(P(None), 4, Cw, 0, C, P(col), 0, _st())),
        ("colsum_from_stats: c0 + C > Cpad", ERR_ARG, lambda: lib.hpri_colsum_from_stats(P(rec), 4, Cw, 4, C, P(col), 0, _st())),
    ]
    snap = [t.clone() for t in (*outs.values(), y, dx, dgam, dbet, dbias, col, planes)]
    for name, code, call in cases:
        rc = call()
        assert rc == code, (name, rc, lib.hpri_last_error())
    torch.cuda.synchronize()
    for a, b in zip(snap, (*outs.values(), y, dx, dgam, dbet, dbias, col, planes)):
        assert torch.equal(_bits(a) if a.dtype != torch.float32 else a, _bits(b) if b.dtype != torch.float32 else b)
