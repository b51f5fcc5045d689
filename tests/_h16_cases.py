"""Cases, fp64 references and elementwise bounds shared by test_h16_cases_cpu.py and test_gpu_h16_kernels.py: the 16-bit MFMA kernels
(gemm_bf16v3.hip, conv_bf16v3.hip, conv_wgrad_bf16v2.hip, wgrad_bf16v3.hip), the x16 head and pooling kernels and the 16-bit weight
packers, for BOTH product libraries (``LIBS``: h16_t = bf16, and IEEE half in the -DHPRI_H16_F16 build).  Everything here runs on the
CPU, is seeded and cached.

A case is a bilinear form ``ref = product(form, a, b)`` of two operands that are exact in the library's 16-bit type (``FORMS``):

  rows         a = x [P, K],          b = w [C, K]            -> [P, C]              n = K terms per element
  conv         a = x [N, H, W, Cin],  b = w [Cout, Cin, 3, 3] -> [N H W, Cout]       n = 9 Cin
  convt_fwd    a = x [N, H, W, Cin],  b = wt [Cin, Cup, 2, 2] -> [N, 2H, 2W, Cup]    n = Cin
  convt_dgrad  a = dy [N, 2H, 2W, Cup], b = wt                -> [N H W, Cin]        n = 4 Cup
  wgrad1x1     a = x [P, Cin],        b = dy [P, Cout]        -> [Cout, Cin]         n = P
  wgrad_conv   a = x [N, H, W, Cin],  b = dy [N, H, W, Cout]  -> [Cout, Cin, 3, 3]   n = N H W
  wgrad_convt  a = x [N, H, W, Cin],  b = dy [N, 2H, 2W, Cup] -> [Cin, Cup, 2, 2]    n = N H W

Three kinds of operands:

``int``   integers in [-3, 3] (bias and prior contents in [-8, 8]): exact in bf16 and in half, every partial sum an integer below
          2^24, so any summation order gives the same fp32 result.  fp32 outputs must equal ``ref`` bit for bit, 16-bit outputs
          ``round16(ref)``.
``real``  Gaussians rounded by torch to the 16-bit type.  A product of two 16-bit values is exact in fp32 (8 + 8 significand bits for
          bf16, 11 + 11 for half, exponents far inside fp32's range), so the only error of a kernel is its fp32 accumulation: with
          round-to-nearest adds, in any order, |got - ref| <= (n + 2) u (sum |a||b| + |bias| + |prior|) per element, u = 2^-24 (n - 1
          adds of the products, one for the bias, one for the prior contents, one spare).  ``bound`` is that array.  The form
          test_gpu_spectral.py uses for its MFMA chain.
``edge``  range tables (``edge_problem``): a selector second operand -- at most two non-zeros per output column, each a power of two
          -- makes every fp32 output an exactly known value x 2^s or x1 2^a + x2 2^b; the first operand walks the roundings, the
          subnormals and the overflow threshold of the 16-bit type (built from torch.finfo, so one table serves both types).  The
          expected 16-bit bits are torch's own ``y64.float().to(dtype)``.

test_h16_cases_cpu.py proves the premises (exactness, budgets, lossless edge outputs, classes present) and that the real-valued
bound is not vacuous: a dropped k-step of 32, an input shifted by one pixel and two swapped output channels (``mutations``) each
exceed it, while fp32 emulations of the same sums (``emulations``) stay inside."""
import functools

import torch

from _direct_cases import LIMIT, SENTINEL, X_PAD_VALUE, _ints, cdiv, rup
from _persistent_cases import PRIOR, SMALL, _gen, round16

__all__ = ["LIMIT", "SENTINEL", "X_PAD_VALUE", "cdiv", "rup", "round16"]

F = torch.nn.functional
U = 2.0 ** -24
LIBS = ("bf16", "f16")
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
FORMS = ("rows", "conv", "convt_fwd", "convt_dgrad", "wgrad1x1", "wgrad_conv", "wgrad_convt")

# The shapes of test_gpu_h16_kernels.py: the smallest that still reach each kernel's edges.
GEMM_FWD = [(1, 5, 8, 4), (2, 300, 40, 24), (2, 129, 238, 150), (3, 257, 64, 330)]        # N, HW, K, C
GEMM_DGRAD = [(2, 129, 150, 238), (1, 300, 64, 96)]                                      # N, HW, K = out features, C = in features
CONVT = [(2, 5, 7, 96, 48, 0, 1), (1, 19, 30, 64, 32, 1, 1), (2, 9, 15, 128, 64, 0, 0)]  # N, H, W, Cin, Cup, canvas offset (y, x)
CONV = [(1, 4, 32, 64, 64), (1, 17, 23, 40, 64), (1, 33, 31, 238, 64), (2, 36, 50, 64, 64)]   # N, H, W, Cin, Cout
CONV_Y2 = (2, 19, 30, 32, 192)                                                           # second output over channels [128, 192)
WGRAD_CONV = [(1, 17, 23, 5, 7), (1, 4, 32, 64, 64), (2, 36, 50, 64, 64)]
WGRAD_1X1 = [(33, 8, 8), (300, 40, 24), (5000, 238, 150)]                                # P, Cin, Cout
WGRAD_CONVT = [(2, 9, 15, 128, 64, 0, 0), (1, 19, 30, 96, 64, 1, 1)]
HEAD = [(1, 50, 6, 1, 0), (1, 333, 64, 1, 32), (1, 211, 40, 3, 0), (2, 129, 1650, 1, 1664)]   # N, HW, C, K, channel offset of x
POOL = [(1, 9, 7, 32), (2, 8, 10, 64)]                                                   # N, H, W, C


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def product(form, a, b, dtype=torch.float64):
    """The bilinear form in ``dtype`` (fp64: the reference; fp32: an emulation of a kernel's accumulation)."""
    a, b = a.to(dtype), b.to(dtype)
    if form == "rows":
        return a @ b.t()
    if form == "conv":
        return F.conv2d(_nchw(a), b, padding=1).permute(0, 2, 3, 1).reshape(-1, b.shape[0])
    if form == "convt_fwd":
        return F.conv_transpose2d(_nchw(a), b, stride=2).permute(0, 2, 3, 1).contiguous()
    if form == "convt_dgrad":
        return F.conv2d(_nchw(a), b, stride=2).permute(0, 2, 3, 1).reshape(-1, b.shape[0])
    if form == "wgrad1x1":
        return b.t() @ a
    if form == "wgrad_conv":
        return torch.nn.grad.conv2d_weight(_nchw(a), (b.shape[3], a.shape[3], 3, 3), _nchw(b), padding=1)
    if form == "wgrad_convt":
        out = torch.empty(a.shape[3], b.shape[3], 2, 2, dtype=dtype)
        for i in range(2):
            for j in range(2):
                out[:, :, i, j] = torch.einsum("nhwc,nhwk->ck", a, b[:, i::2, j::2])
        return out
    raise AssertionError(form)


def terms(form, a, b):
    """n: the number of products summed into one output element."""
    if form == "rows":
        return a.shape[1]
    if form == "conv":
        return 9 * a.shape[3]
    if form == "convt_fwd":
        return a.shape[3]
    if form == "convt_dgrad":
        return 4 * a.shape[3]
    if form == "wgrad1x1":
        return a.shape[0]
    return a.shape[0] * a.shape[1] * a.shape[2]


def shapes(form, shape):
    """(shape of a, shape of b) of ``form`` for a shape tuple of the tables above."""
    if form == "rows":
        N, HW, K, C = shape
        return (N * HW, K), (C, K)
    if form == "wgrad1x1":
        Pn, Cin, Cout = shape
        return (Pn, Cin), (Pn, Cout)
    N, H, W, Cin, Co = shape[:5]
    if form == "conv":
        return (N, H, W, Cin), (Co, Cin, 3, 3)
    if form == "convt_fwd":
        return (N, H, W, Cin), (Cin, Co, 2, 2)
    if form == "convt_dgrad":
        return (N, 2 * H, 2 * W, Co), (Cin, Co, 2, 2)
    if form == "wgrad_conv":
        return (N, H, W, Cin), (N, H, W, Co)
    if form == "wgrad_convt":
        return (N, H, W, Cin), (N, 2 * H, 2 * W, Co)
    raise AssertionError(form)


def _operand(kind, dt, gen, shape, scale=1.0):
    if kind == "int":
        return _ints(gen, shape, SMALL)
    return (torch.randn(shape, generator=gen) * scale).to(dt).float()          # rounded by torch: exact in the 16-bit type


def _fan_in(form, sa, sb):
    return {"rows": sb[1], "conv": 9 * sb[1], "convt_fwd": sb[0], "convt_dgrad": 4 * sb[1]}.get(form, 1)


@functools.lru_cache(maxsize=None)
def case(form, kind, lib, shape):
    """dict(a, b, bias, prior, ref, mag, n): ``ref`` = product(a, b) in fp64 (no bias, no prior), ``mag`` = product(|a|, |b|), bias
    per output channel, prior of the shape of ref (fp32 values; a test that accumulates into 16-bit rows rounds it itself)."""
    dt = DTYPES[lib]
    gen = _gen("h16", form, kind, lib, *shape)
    sa, sb = shapes(form, shape)
    a = _operand(kind, dt, gen, sa)
    b = _operand(kind, dt, gen, sb, _fan_in(form, sa, sb) ** -0.5 if form in ("rows", "conv", "convt_fwd", "convt_dgrad") else 1.0)
    ref = product(form, a, b)
    mag = product(form, a.abs(), b.abs())
    nb = {"rows": sb[0], "conv": sb[0], "convt_fwd": sb[1], "convt_dgrad": sb[0]}.get(form, 1)
    if kind == "int":
        bias, prior = _ints(gen, (nb,), PRIOR), _ints(gen, tuple(ref.shape), PRIOR)
    else:
        bias, prior = torch.randn(nb, generator=gen), torch.randn(tuple(ref.shape), generator=gen)
    return dict(form=form, kind=kind, lib=lib, shape=shape, a=a, b=b, bias=bias, prior=prior, ref=ref, mag=mag, n=terms(form, a, b))


def bound(c, extra=0.0):
    """(n + 2) u (sum |a||b| + extra) per element; ``extra`` = |bias| + |prior| as far as the launch adds them (broadcastable)."""
    return (c["n"] + 2) * U * (c["mag"] + extra)


def budget(c):
    """The largest partial sum an integer case can reach: every term, the bias and the prior contents with the same sign."""
    return float(c["mag"].max()) + float(c["bias"].abs().max()) + float(c["prior"].abs().max())


# ---------------------------------------------------------------------------------------------------------------------------
# Mutations (what a subtly wrong kernel computes) and fp32 emulations (what a right one may compute)
# ---------------------------------------------------------------------------------------------------------------------------
def _drop_last_kstep(form, a, b):
    """The last 32 of the summed index contribute nothing: a lost k-step at the end of the reduction."""
    a, b = a.clone(), b.clone()
    if form == "rows":
        a[:, -32:] = 0
    elif form == "conv":
        b[:, -32:, 2, 2] = 0                       # k = tap * Cin + ci: the last tap's last channels
    elif form == "convt_fwd":
        a[..., -32:] = 0
    elif form == "convt_dgrad":
        b[:, -32:, 1, 1] = 0                       # k = tap * Cup + co
    elif form == "wgrad1x1":
        a[-32:] = 0                                # the summed index is the pixel
    else:
        a.view(-1, a.shape[-1])[-32:] = 0
    return a, b


def _shift_input(form, a):
    """The first operand read one pixel off."""
    if form in ("rows", "wgrad1x1"):
        return a.roll(1, 0)
    return a.roll(1, 2)


def _swap_channels(form, ref):
    """Two output channels swapped: the last axis of the activations, the first of the weight gradients (a one-channel output: two
    pixels)."""
    out = ref.clone()
    first = (form.startswith("wgrad") and ref.shape[0] > 1) or ref.shape[-1] == 1
    if first:
        out[[0, 1]] = ref[[1, 0]]
    else:
        out[..., [0, 1]] = ref[..., [1, 0]]
    return out


def mutations(c):
    """{name: fp64 reference of the mutated computation}."""
    form, a, b = c["form"], c["a"], c["b"]
    return {"last k-step dropped": product(form, *_drop_last_kstep(form, a, b)),
            "input shifted by one pixel": product(form, _shift_input(form, a), b),
            "two output channels swapped": _swap_channels(form, c["ref"])}


def emulations(c):
    """fp32 evaluations of the unmutated sums in two orders: torch's own, and with the summed index reversed."""
    form, a, b = c["form"], c["a"], c["b"]
    plain = product(form, a, b, torch.float32)
    if form == "rows":
        rev = product(form, a.flip(1), b.flip(1), torch.float32)
    elif form == "conv":
        rev = product(form, a.flip(3), b.flip(1), torch.float32)
    elif form == "convt_fwd":
        rev = product(form, a.flip(3), b.flip(0), torch.float32)
    elif form == "convt_dgrad":
        rev = product(form, a.flip(3), b.flip(1), torch.float32)
    elif form == "wgrad1x1":
        rev = product(form, a.flip(0), b.flip(0), torch.float32)
    else:
        rev = product(form, a.flip(0), b.flip(0), torch.float32)               # the images in reverse order
    return {"fp32": plain.double(), "fp32, reversed": rev.double()}


# ---------------------------------------------------------------------------------------------------------------------------
# The x16 head (1x1 output layer over 16-bit rows) and max-pooling
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_case(kind, lib, shape):
    """x [N HW, C] (16-bit rows), w [K, C] and b [K] (fp32 arguments holding 16-bit-exact values, so that every product is exact in
    fp32), dy [N HW, K] likewise; as three bilinear cases: ``fwd`` = rows(x, w) -> logits [N HW, K], ``dx`` = rows(dy, w^T) ->
    [N HW, C], ``dw`` = wgrad1x1(x, dy) -> [K, C]; db = the column sums of dy (``db``, ``db_mag``; n = N HW terms, no products)."""
    N, HW, C, K, _ = shape
    dt = DTYPES[lib]
    gen = _gen("h16", "head", kind, lib, *shape)
    x = _operand(kind, dt, gen, (N * HW, C))
    w = _operand(kind, dt, gen, (K, C), C ** -0.5)
    dy = _operand(kind, dt, gen, (N * HW, K))
    out = {}
    for name, form, a, b in (("fwd", "rows", x, w), ("dx", "rows", dy, w.t().contiguous()), ("dw", "wgrad1x1", x, dy)):
        ref = product(form, a, b)
        if kind == "int":
            bias, prior = _ints(gen, (ref.shape[1] if form == "rows" else 1,), PRIOR), _ints(gen, tuple(ref.shape), PRIOR)
        else:
            bias, prior = torch.randn(ref.shape[1] if form == "rows" else 1, generator=gen), torch.randn(tuple(ref.shape), generator=gen)
        out[name] = dict(form=form, kind=kind, lib=lib, shape=shape, a=a, b=b, bias=bias, prior=prior, ref=ref,
                         mag=product(form, a.abs(), b.abs()), n=terms(form, a, b))
    out["db"], out["db_mag"] = dy.double().sum(0), dy.double().abs().sum(0)
    out["db_prior"] = _ints(gen, (K,), PRIOR) if kind == "int" else torch.randn(K, generator=gen)
    return out


@functools.lru_cache(maxsize=None)
def pool_case(kind, lib, shape):
    """MaxPool2d(2) over x [N, H, W, C] (16-bit-exact values with ties inside windows: a repeated value, and in ``int`` the small
    range itself) and its gradient for dy [N, H/2, W/2, C]: ``fwd`` [N, H/2, W/2, C] and ``routed`` [N, H, W, C] (dy at the FIRST
    maximum of each window in scan order, zero elsewhere and in an odd last row / column) -- exact selections, no rounding."""
    N, H, W, C = shape
    dt = DTYPES[lib]
    gen = _gen("h16", "pool", kind, lib, *shape)
    x = _operand(kind, dt, gen, (N, H, W, C))
    x[:, :H // 2 * 2:2, 1:W // 2 * 2:2] = x[:, :H // 2 * 2:2, :W // 2 * 2:2]           # the top pair of every window ties
    x[:, 1::4] = x[:, 1::4].round() + 0.0                                             # (+ 0.0: no -0 goes in)
    dy = _operand(kind, dt, gen, (N, H // 2, W // 2, C)) if kind == "int" else torch.randn((N, H // 2, W // 2, C), generator=gen)
    xr = _nchw(x).double().requires_grad_(True)
    y = F.max_pool2d(xr, 2)
    y.backward(_nchw(dy).double())
    prior = _ints(gen, (N, H, W, C), PRIOR) if kind == "int" else torch.randn((N, H, W, C), generator=gen)
    return dict(x=x, dy=dy, fwd=y.detach().permute(0, 2, 3, 1).contiguous(), routed=xr.grad.permute(0, 2, 3, 1).contiguous(), prior=prior)


# ---------------------------------------------------------------------------------------------------------------------------
# Range tables
# ---------------------------------------------------------------------------------------------------------------------------
# (rows, K, ncols, single_term) of the range-table launch of each form: rows GEMM K = C = 32 on 8 rows; conv 1 x 4 x 32 with 32 -> 64
# channels (and -> 128 for the second-output form); transposed convolution 1 x 2 x 3 with 32 -> 32 channels (forward: 4 x 32 columns,
# data gradient: K = 4 x 32); weight gradients: rows = output channels of dY (x taps), K = pixels, columns = input channels
EDGE = {"rows": (8, 32, 32, False), "conv": (128, 32, 64, False), "conv_y2": (128, 32, 128, False), "convt_fwd": (6, 32, 128, False),
        "convt_dgrad": (6, 128, 32, False), "wgrad1x1": (32, 64, 32, False), "wgrad_conv": (64, 128, 32, True),
        "wgrad_convt": (256, 64, 32, True)}
CLASSES = ("exact", "tie rounded down", "tie rounded up", "subnormal", "subnormal operand", "inf")


def edge_entries(dt):
    """[(x1, a, x2, b, class)]: the fp32 output is x1 2^a + x2 2^b, every x a value of the 16-bit type.  Both signs of every row."""
    fi = torch.finfo(dt)
    eps = fi.eps
    rows = [(1.0, 0, eps, -1, "tie rounded down"),                    # 1 + eps/2 -> 1 (tie to even)
            (1.0 + eps, 0, eps, -1, "tie rounded up")]                # 1 + 3 eps/2 -> 1 + 2 eps
    rows += [(v, 0, 0.0, 0, "exact") for v in (1.0, 1.0 + eps, 2.0 - eps, 3.5, 0.375, fi.smallest_normal)]
    if dt == torch.float16:
        sub = fi.smallest_normal * eps                                 # the smallest subnormal, 2^-24
        rows += [(sub, 10, 0.0, 0, "subnormal operand"),               # 2^-24 2^10 = 2^-14: the operand is consumed at its value
                 (sub, -1, 0.0, 0, "tie rounded down"),                # 2^-25 -> 0
                 (3 * sub, -1, 0.0, 0, "tie rounded up"),              # 3 2^-25 -> 2^-23
                 (1023 * sub, 0, 0.0, 0, "subnormal"),                 # the largest subnormal is kept
                 (5 * sub, 0, 0.0, 0, "subnormal"),
                 (2.0 ** -14, 0, 0.0, 0, "exact"),
                 (fi.max, 0, 0.0, 0, "exact"),                         # 65504 is kept
                 (fi.max, 0, 15.0, 0, "tie rounded down"),             # 65519 -> 65504 (below the tie at 65520)
                 (fi.max, 0, 16.0, 0, "inf"),                          # 65520 -> inf (tie to even)
                 (fi.max, 1, 0.0, 0, "inf")]                           # 131008 -> inf
    return rows + [(-x1, a, -x2 if x2 else 0.0, b, k) for x1, a, x2, b, k in rows]


@functools.lru_cache(maxsize=None)
def edge_problem(lib, rows, K, ncols, single_term=False):
    """A [rows, K] (first operand), B [ncols, K] (selector), y64 = A B^T [rows, ncols], cls [rows, ncols] (index into CLASSES).
    Column j multiplies slot 2 j' by 2^a and slot 2 j' + 1 by 2^b (j' = j mod the number of patterns); the entries with that (a, b)
    fill its rows cyclically, a group larger than ``rows`` takes several patterns.  ``single_term``: one non-zero per column (the
    two-term entries are left out) -- for forms whose other taps would pair the terms differently.  Slots no column selects hold
    3.0 and meet zero weights."""
    dt = DTYPES[lib]
    groups = {}
    for x1, a, x2, b, k in edge_entries(dt):
        if single_term and x2 != 0.0:
            continue
        groups.setdefault((a, b), []).append((x1, x2, k))
    pats = [(a, b, ent[i:i + rows]) for (a, b), ent in sorted(groups.items()) for i in range(0, len(ent), rows)]
    assert 2 * len(pats) <= K and len(pats) <= ncols, (len(pats), K, ncols)
    A = torch.full((rows, K), 3.0)
    B = torch.zeros(ncols, K)
    cls = torch.zeros(rows, ncols, dtype=torch.long)
    for j, (a, b, ent) in enumerate(pats):
        for r in range(rows):
            x1, x2, k = ent[r % len(ent)]
            A[r, 2 * j], A[r, 2 * j + 1] = x1, x2
    for j in range(ncols):
        jp = j % len(pats)
        a, b, ent = pats[jp]
        B[j, 2 * jp] = 2.0 ** a
        if not single_term:
            B[j, 2 * jp + 1] = 2.0 ** b
        cls[:, j] = torch.tensor([CLASSES.index(ent[r % len(ent)][2]) for r in range(rows)])
    y64 = A.double() @ B.double().t()
    return dict(A=A, B=B, y64=y64, cls=cls, bits=round16(y64.float(), dt))


# ---------------------------------------------------------------------------------------------------------------------------
# Every bilinear case of test_gpu_h16_kernels.py, by name
# ---------------------------------------------------------------------------------------------------------------------------
def sid(shape):
    return "x".join(str(v) for v in shape)


def bilinear_cases(kind, lib):
    """(name, case) of every bilinear case the GPU module runs with ``kind`` operands on ``lib``."""
    for s in GEMM_FWD:
        yield "gemm_fwd/" + sid(s), case("rows", kind, lib, s)
    for s in GEMM_DGRAD:
        yield "gemm_dgrad/" + sid(s), case("rows", kind, lib, s)
    for s in CONVT:
        yield "convt_fwd/" + sid(s), case("convt_fwd", kind, lib, s)
        if s[4] % 32 == 0:
            yield "convt_dgrad/" + sid(s), case("convt_dgrad", kind, lib, s)
    for s in CONV + [CONV_Y2]:
        yield "conv/" + sid(s), case("conv", kind, lib, s)
    for s in WGRAD_CONV:
        yield "wgrad_conv/" + sid(s), case("wgrad_conv", kind, lib, s)
    for s in WGRAD_1X1:
        yield "wgrad1x1/" + sid(s), case("wgrad1x1", kind, lib, s)
    for s in WGRAD_CONVT:
        yield "wgrad_convt/" + sid(s), case("wgrad_convt", kind, lib, s)
    for s in HEAD:
        h = head_case(kind, lib, s)
        for part in ("fwd", "dx", "dw"):
            yield "head_%s/%s" % (part, sid(s)), h[part]
