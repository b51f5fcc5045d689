"""Case tables, input builders and fp64 references shared by test_direct_cases_cpu.py, test_gpu_direct_conv.py,
test_gpu_direct_wgrad.py and test_gpu_pack_weight.py: the implicit-GEMM convolution (csrc/conv_fwd.hip), the pixel-reduction
weight gradient (csrc/conv_wgrad.hip) and the weight packers (csrc/pack.hip), called through the C ABI.

Everything here runs on the CPU.  The inputs are built on the CPU from a seeded generator, so the CPU test proves the exactness
budget of the very tensors the GPU tests then upload.

Integer operands: with small-integer operands every product and every partial sum of a convolution is an integer below 2^24, i.e.
an exactly representable fp32 value, so the result does not depend on summation order, split-K, slab order or the MFMA k-permutation
and must equal the fp64 reference bit for bit.  The condition is on the inputs: per output element sum|x||w| + |bias| + |y0| < 2^24
(weight gradient: sum|x||dy| + |dw0| < 2^24), computed in fp64 as the same convolution of absolute values (``*_budget``).

Operand sets (bias and the prior contents of y / dW are always integers in [-8, 8]):
  small   both operands integers in [-3, 3]: bf16-exact, the lo / mid planes of the split kernels are zero
  a_wide  first operand (x) integers in [-1000, 1000] (needs hi + lo), second in [-2, 2] (lo plane zero, so the dropped lo*lo is 0)
  b_wide  the same with the second operand (w; dy for the weight gradient) wide
  a_third first operand integers below 2^17 in magnitude (needs hi + mid + lo), second in {-1, 0, 1}
  b_third the same with the second operand wide
  a_deep / b_deep  one operand integers below 2^19 in magnitude, the other in {-1, 0, 1}.  Round-to-nearest planes carry a sign, so
          two planes already hold every integer below 2^17 (test_direct_cases_cpu.py asserts it): the *_third sets exercise
          the mid plane of the bf16x6 kernels and the products with it, and only these deeper ones put non-zero values into the
          lo plane (a third of their elements).  They need Cin * KS^2 <= 31 resp. N*H*W <= 31.
Both split kernels build their planes as the packer does (plane = bf16(rest), rest -= plane: conv_fwd.hip STORE_A, conv_wgrad.hip
LOAD_UNIT, pack.hip pack_weight_bf16_kernel), so hi + lo resp. hi + mid + lo reproduce these integers exactly in either operand."""
import torch

LIMIT = float(1 << 24)
X_PAD_VALUE = 1.0e3          # operand channels the kernel must not read (or that meet zero weights)
SENTINEL = 7.5               # no integer result can equal it
WS_SENTINEL = float("nan")   # workspaces: no result, integer or random, is NaN

OPSETS = {  # name -> ((lo, hi) of the first operand, (lo, hi) of the second)
    "small": ((-3, 3), (-3, 3)),
    "a_wide": ((-1000, 1000), (-2, 2)),
    "b_wide": ((-2, 2), (-1000, 1000)),
    "a_third": ((-(1 << 17) + 1, (1 << 17) - 1), (-1, 1)),
    "b_third": ((-1, 1), (-(1 << 17) + 1, (1 << 17) - 1)),
    "a_deep": ((-(1 << 19) + 1, (1 << 19) - 1), (-1, 1)),
    "b_deep": ((-1, 1), (-(1 << 19) + 1, (1 << 19) - 1)),
}
KERNS = ("f32", "bf16", "bf16x3", "bf16x6")        # hpri_conv_fwd | hpri_conv_fwd_bf16 with split 0, 1, 2 (same for the wgrad)


def rup(x, m):
    return (x + m - 1) // m * m


def cdiv(a, b):
    return (a + b - 1) // b


def split_of(kern):
    return KERNS.index(kern) - 1


# ---------------------------------------------------------------------------------------------------------------------------
# Forward geometries: (N, H, W, Cin, Cout), KS; what the plan must show for the fp32 kernel (asserted from hpri_conv_fwd_plan):
#   seg     stat_tiles differs from the plain count N * ceil(H / TH) * ceil(W / 32): the width was cut into column bands
#   ksplit  the split-K factor (None: do not care; 1: must not split)
#   tiles   stat_tiles where the case names it
# ---------------------------------------------------------------------------------------------------------------------------
FWD_CASES = {
    "bands_32_16_8_4": dict(shape=(1, 32, 60, 8, 128), ks=3, seg=True, ksplit=1, tiles=15),
    "bands_32_16_4": dict(shape=(1, 16, 52, 12, 128), ks=3, seg=True, ksplit=1),
    "bands_32_4": dict(shape=(1, 8, 36, 8, 128), ks=3, seg=True, ksplit=1),
    "4x1_bands_32_8": dict(shape=(1, 32, 41, 8, 64), ks=3, seg=True, ksplit=1),
    "4x1_bands_ragged_rows": dict(shape=(1, 19, 40, 40, 64), ks=3, seg=True, ksplit=1),
    "plain_odd_2x2": dict(shape=(1, 33, 61, 8, 128), ks=3, seg=False, ksplit=1),
    "plain_odd_two_images": dict(shape=(2, 17, 23, 5, 7), ks=3, seg=False, ksplit=1),
    "one_pixel": dict(shape=(1, 1, 1, 8, 8), ks=3, seg=False, ksplit=1),
    "tiny_image": dict(shape=(1, 2, 3, 3, 1), ks=3, seg=False, ksplit=1),
    "splitk2_partial_chunk": dict(shape=(1, 9, 11, 260, 64), ks=3, seg=None, ksplit=2),
    "splitk3_2x2_bands_8_4": dict(shape=(1, 9, 11, 392, 128), ks=3, seg=None, ksplit=3),
    "k1_splitk4": dict(shape=(2, 7, 13, 520, 64), ks=1, seg=None, ksplit=4),
    "k1_no_split": dict(shape=(1, 5, 9, 264, 64), ks=1, seg=None, ksplit=1),
    "k1_4x1_three_blocks": dict(shape=(1, 6, 35, 24, 192), ks=1, seg=None, ksplit=1),
    "k1_2x2_two_blocks": dict(shape=(1, 6, 35, 24, 256), ks=1, seg=None, ksplit=1),
}
# the XCD-aware 1-D grid ("conv_nbx_min" = 2); both tile counts are not multiples of 8, so blocks of the last round return early
XCD_FWD_CASES = {
    "xcd_4x1_three_blocks": dict(shape=(1, 19, 40, 8, 192), ks=3),
    "xcd_2x2_two_blocks": dict(shape=(1, 32, 60, 8, 256), ks=3),
}
EPILOGUE_CASES = ("bands_32_16_8_4", "splitk3_2x2_bands_8_4", "4x1_bands_ragged_rows", "splitk2_partial_chunk")   # 2x2, 2x2, 4x1, 4x1
DGRAD_CASES = ("bands_32_16_4", "plain_odd_two_images")                 # pack mode 1
RANDOM_FWD_CASES = ("bands_32_16_8_4", "4x1_bands_ragged_rows", "plain_odd_two_images", "splitk2_partial_chunk",
                    "splitk3_2x2_bands_8_4", "k1_splitk4", "k1_4x1_three_blocks")
# second plane: Cin * KS^2 * 2000 + 16 < 2^24 holds for every geometry of the table; a subset that covers bands, both workgroup
# shapes, split-K and the 1x1 form.  Third plane: Cin * KS^2 <= 96.
WIDE_FWD_CASES = ("bands_32_16_8_4", "4x1_bands_ragged_rows", "plain_odd_two_images", "splitk2_partial_chunk", "k1_splitk4")
THIRD_FWD_CASES = ("bands_32_16_8_4", "4x1_bands_32_8", "plain_odd_two_images", "tiny_image")
DEEP_FWD_CASES = ("tiny_image", "k1_4x1_three_blocks", "k1_2x2_two_blocks")                         # Cin * KS^2 <= 31

# ConvTranspose2d(k=2, s=2): (N, H, W, Cin, Cup), hi-res image H2 x W2, pad offsets (py0, px0)
CONVT_CASES = {
    "convt_cup8_off01": dict(shape=(1, 5, 7, 16, 8), H2=11, W2=15, py0=0, px0=1),
    "convt_cup8_off10": dict(shape=(1, 5, 7, 16, 8), H2=11, W2=15, py0=1, px0=0),
    "convt_cup32": dict(shape=(2, 6, 33, 40, 32), H2=13, W2=68, py0=1, px0=2),
}
THIRD_CONVT_CASES = ("convt_cup8_off01",)                                # Cin <= 96 (forward); N*H*W <= 96 (weight gradient)
DEEP_CONVT_CASES = ("convt_cup8_off01",)                                 # forward only: Cin = 16; 4 * Cup and N*H*W exceed 31

# Weight gradient: (N, H, W, Cin, Cout), KS
WGRAD_CASES = {
    "one_strip": dict(shape=(1, 2, 2, 4, 4), ks=3),
    "one_column_in_second_strip": dict(shape=(1, 6, 33, 8, 8), ks=3),
    "two_images_odd": dict(shape=(2, 5, 61, 40, 64), ks=3),
    "cvalid_8": dict(shape=(1, 17, 23, 5, 7), ks=3),
    "blocks_2x3": dict(shape=(1, 9, 40, 72, 136), ks=3),
    "k1_ragged_blocks": dict(shape=(1, 7, 13, 130, 70), ks=1),
    "k1_two_n_blocks": dict(shape=(1, 3, 9, 12, 134), ks=1),
    "k1_wide_rows": dict(shape=(2, 3, 100, 8, 8), ks=1),
}
XCD_WGRAD_CASE = "blocks_2x3"
RANDOM_WGRAD_CASES = ("one_column_in_second_strip", "two_images_odd", "cvalid_8", "blocks_2x3", "k1_ragged_blocks", "k1_wide_rows")
WIDE_WGRAD_CASES = ("one_column_in_second_strip", "cvalid_8", "blocks_2x3", "k1_ragged_blocks")      # N*H*W <= 4096 everywhere
THIRD_WGRAD_CASES = ("one_strip", "k1_ragged_blocks")                                                 # N*H*W <= 96
DEEP_WGRAD_CASES = ("one_strip", "k1_two_n_blocks")                                                   # N*H*W <= 31


def _gen(*key):
    """A generator seeded from the case key (not hash(): that differs between processes)."""
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(map(str, key)))))
    return g


def _ints(g, shape, lohi):
    return torch.randint(lohi[0], lohi[1] + 1, shape, generator=g).float()


# ---------------------------------------------------------------------------------------------------------------------------
# Input builders.  Activations are NHWC fp32 (the library's layout), weights in the nn.Parameter layouts.
# ---------------------------------------------------------------------------------------------------------------------------
def fwd_inputs(name, opset="small", random=False):
    """x [N,H,W,Cin], w [Cout,Cin,KS,KS] (the EFFECTIVE forward weight: the data-gradient tests pack its transposed, flipped
    form with mode 1), bias [Cout], y0 [N*H*W, Cout]."""
    c = FWD_CASES.get(name) or XCD_FWD_CASES[name]
    N, H, W, Cin, Cout = c["shape"]
    ks = c["ks"]
    g = _gen("fwd", name, opset, random)
    if random:
        return dict(x=torch.randn(N, H, W, Cin, generator=g), w=torch.randn(Cout, Cin, ks, ks, generator=g) * 0.1,
                    bias=torch.randn(Cout, generator=g), y0=torch.randn(N * H * W, Cout, generator=g))
    a, b = OPSETS[opset]
    return dict(x=_ints(g, (N, H, W, Cin), a), w=_ints(g, (Cout, Cin, ks, ks), b), bias=_ints(g, (Cout,), (-8, 8)),
                y0=_ints(g, (N * H * W, Cout), (-8, 8)))


def convt_inputs(name, opset="small", random=False):
    """x [N,H,W,Cin], wt [Cin,Cup,2,2], bias [Cup]; dy_d and dy_w [N,H2,W2,Cup]: gradients of the whole hi-res image (the kernels
    read only the 2H x 2W patch grid at the offset) -- dy_d, in the first operand's range, meets wt in the data gradient; dy_w, in
    the second operand's range, meets x in the weight gradient; dx0 [N*H*W, Cin] and dw0 [Cin,Cup,2,2]: prior contents for the
    accumulate forms."""
    c = CONVT_CASES[name]
    N, H, W, Cin, Cup = c["shape"]
    g = _gen("convt", name, opset, random)
    if random:
        return dict(x=torch.randn(N, H, W, Cin, generator=g), wt=torch.randn(Cin, Cup, 2, 2, generator=g) * 0.1,
                    bias=torch.randn(Cup, generator=g), dy_d=torch.randn(N, c["H2"], c["W2"], Cup, generator=g),
                    dy_w=torch.randn(N, c["H2"], c["W2"], Cup, generator=g),
                    dx0=torch.randn(N * H * W, Cin, generator=g), dw0=torch.randn(Cin, Cup, 2, 2, generator=g))
    a, b = OPSETS[opset]
    return dict(x=_ints(g, (N, H, W, Cin), a), wt=_ints(g, (Cin, Cup, 2, 2), b), bias=_ints(g, (Cup,), (-8, 8)),
                dy_d=_ints(g, (N, c["H2"], c["W2"], Cup), a), dy_w=_ints(g, (N, c["H2"], c["W2"], Cup), b),
                dx0=_ints(g, (N * H * W, Cin), (-8, 8)), dw0=_ints(g, (Cin, Cup, 2, 2), (-8, 8)))


def wgrad_inputs(name, opset="small", random=False):
    """x [N,H,W,Cin], dy [N,H,W,Cout], dw0 [Cout,Cin,KS,KS]."""
    c = WGRAD_CASES[name]
    N, H, W, Cin, Cout = c["shape"]
    ks = c["ks"]
    g = _gen("wgrad", name, opset, random)
    if random:
        return dict(x=torch.randn(N, H, W, Cin, generator=g), dy=torch.randn(N, H, W, Cout, generator=g),
                    dw0=torch.randn(Cout, Cin, ks, ks, generator=g))
    a, b = OPSETS[opset]
    return dict(x=_ints(g, (N, H, W, Cin), a), dy=_ints(g, (N, H, W, Cout), b), dw0=_ints(g, (Cout, Cin, ks, ks), (-8, 8)))


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 references (torch's own operators on the CPU) and the exactness budgets (the same operators on absolute values)
# ---------------------------------------------------------------------------------------------------------------------------
def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _rows(t):
    """[N, C, H, W] -> [N*H*W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def ref_conv(x, w, bias=None):
    """conv2d(k = 1 | 3, padding = k // 2) -> [N*H*W, Cout] in fp64."""
    return _rows(torch.nn.functional.conv2d(_nchw(x), w.double(), None if bias is None else bias.double(), padding=w.shape[2] // 2))


def fwd_budget(x, w, bias=None, y0=None):
    b = ref_conv(x.abs(), w.abs(), None if bias is None else bias.abs())
    if y0 is not None:
        b = b + y0.double().abs()
    return float(b.max())


def ref_convt(x, wt, bias=None):
    """conv_transpose2d(k=2, s=2) -> [N, 2H, 2W, Cup] in fp64."""
    y = torch.nn.functional.conv_transpose2d(_nchw(x), wt.double(), None if bias is None else bias.double(), stride=2)
    return y.permute(0, 2, 3, 1).contiguous()


def convt_budget(x, wt, bias=None):
    return float(ref_convt(x.abs(), wt.abs(), None if bias is None else bias.abs()).max())


def convt_patch(dy, H, W, py0, px0):
    """The 2H x 2W patch grid of a hi-res [N, H2, W2, C] tensor at the pad offset."""
    return dy[:, py0:py0 + 2 * H, px0:px0 + 2 * W, :]


def ref_convt_grads(x, wt, dy_patch):
    """Autograd of conv_transpose2d(k=2, s=2) in fp64: (dx [N*H*W, Cin], dw [Cin, Cup, 2, 2])."""
    xr = _nchw(x).clone().requires_grad_(True)
    wr = wt.double().clone().requires_grad_(True)
    y = torch.nn.functional.conv_transpose2d(xr, wr, None, stride=2)
    y.backward(_nchw(dy_patch))
    return _rows(xr.grad), wr.grad


def convt_grad_budgets(x, wt, dy_patch, dx0=None, dw0=None):
    dx, dw = ref_convt_grads(x.abs(), wt.abs(), dy_patch.abs())
    if dx0 is not None:
        dx = dx + dx0.double().abs()
    if dw0 is not None:
        dw = dw + dw0.double().abs()
    return float(dx.max()), float(dw.max())


def ref_wgrad(x, dy, ks):
    """conv2d_weight(padding = ks // 2) -> [Cout, Cin, ks, ks] in fp64."""
    Cout, Cin = dy.shape[3], x.shape[3]
    return torch.nn.grad.conv2d_weight(_nchw(x), (Cout, Cin, ks, ks), _nchw(dy), padding=ks // 2)


def wgrad_budget(x, dy, ks, dw0=None):
    b = ref_wgrad(x.abs(), dy.abs(), ks)
    if dw0 is not None:
        b = b + dw0.double().abs()
    return float(b.max())


# ---- index-by-index restatements, for the cross-check of the references above (test_direct_cases_cpu.py) ----
def naive_conv(x, w, bias=None):
    N, H, W, Cin = x.shape
    Cout, _, ks, _ = w.shape
    p = ks // 2
    xp = torch.zeros(N, H + 2 * p, W + 2 * p, Cin, dtype=torch.float64)
    xp[:, p:p + H, p:p + W] = x.double()
    y = torch.zeros(N, H, W, Cout, dtype=torch.float64)
    for dy in range(ks):
        for dx in range(ks):
            y += xp[:, dy:dy + H, dx:dx + W] @ w[:, :, dy, dx].double().t()
    if bias is not None:
        y += bias.double()
    return y.reshape(-1, Cout)


def naive_wgrad(x, dy, ks):
    N, H, W, Cin = x.shape
    Cout = dy.shape[3]
    p = ks // 2
    xp = torch.zeros(N, H + 2 * p, W + 2 * p, Cin, dtype=torch.float64)
    xp[:, p:p + H, p:p + W] = x.double()
    dw = torch.zeros(Cout, Cin, ks, ks, dtype=torch.float64)
    d = dy.double().reshape(-1, Cout)
    for a in range(ks):
        for b in range(ks):
            dw[:, :, a, b] = d.t() @ xp[:, a:a + H, b:b + W].reshape(-1, Cin)
    return dw


def naive_convt(x, wt, bias=None):
    N, H, W, Cin = x.shape
    Cup = wt.shape[1]
    y = torch.zeros(N, 2 * H, 2 * W, Cup, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            y[:, a::2, b::2] = x.double() @ wt[:, :, a, b].double()
    if bias is not None:
        y += bias.double()
    return y


# ---------------------------------------------------------------------------------------------------------------------------
# Plan arithmetic the tests compare the library's plan queries with
# ---------------------------------------------------------------------------------------------------------------------------
def plain_tiles(N, H, W, cout_pad, narrow=False):
    """Tiles of the un-banded grid: N * ceil(H / TH) * ceil(W / 32); TH = 4 for the 2x2-wave workgroup (and the narrow bf16x6
    one), 8 for 4x1."""
    th = 4 if (cout_pad % 128 == 0 or narrow) else 8
    return N * cdiv(H, th) * cdiv(W, 32)


def chan_merge(stats, tiles, cout_pad, cout):
    """Per-tile (mean, M2, count, 0) records -> per-channel mean, biased variance and count (Chan merge in fp64)."""
    s = stats.reshape(tiles, cout_pad, 4).double()
    n = s[:, :, 2]
    mean = (s[:, :, 0] * n).sum(0) / n.sum(0)
    m2 = (s[:, :, 1] + n * (s[:, :, 0] - mean) ** 2).sum(0)
    return mean[:cout], (m2 / n.sum(0))[:cout], n.sum(0)[:cout]


# ---------------------------------------------------------------------------------------------------------------------------
# numpy restatement of the packed layouts documented at the top of pack.hip
# ---------------------------------------------------------------------------------------------------------------------------
def pack_source_index(mode, k, col, t, T, src_d1, Cup):
    """Flat index into the source weight of packed element (k, col) of tap t; the caller has checked k < K and col < Ncols."""
    if mode == 0:
        return (col * src_d1 + k) * T + t                    # W[n = col][c = k][t]
    if mode == 1:
        return (k * src_d1 + col) * T + (T - 1 - t)          # W[n = k][c = col][flipped t]
    if mode == 2:
        tap, co = divmod(col, Cup)
        return (k * Cup + co) * 4 + tap                      # Wt[ci = k][co][tap]
    tap, co = divmod(k, Cup)
    return (col * Cup + co) * 4 + tap                        # Wt[ci = col][co][tap]


def pack_expected(w, mode, K, Ncols, Ncols_pad, T, src_d1, Cup, colscale=None, gap_at=0, gap_len=0):
    """The values of the packed panel as [chunks][T][32][Ncols_pad] fp32 (the fp32 packer's own layout; the bf16 packers hold
    the same values as [chunks][T][plane][Ncols_pad][32]), index by index in numpy."""
    import numpy as np
    src = w.detach().cpu().numpy().reshape(-1).astype(np.float32)
    chunks = cdiv(K, 32)
    out = np.zeros((chunks, T, 32, Ncols_pad), dtype=np.float32)
    for k in range(K):
        for col in range(Ncols):
            ks, cs = k, col
            if gap_len:
                ax = k if mode == 0 else col                  # the input-channel axis carries the gap
                if gap_at <= ax < gap_at + gap_len:
                    continue
                if ax >= gap_at + gap_len:
                    ax -= gap_len
                ks, cs = (ax, col) if mode == 0 else (k, ax)
            for t in range(T):
                v = src[pack_source_index(mode, ks, cs, t, T, src_d1, Cup)]
                if colscale is not None:
                    v = np.float32(v) * np.float32(colscale[col])
                out[k // 32, t, k % 32, col] = v
    return out
