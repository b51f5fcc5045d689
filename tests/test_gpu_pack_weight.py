"""The weight packers (csrc/pack.hip) against an index-by-index numpy restatement of the layouts documented at the top of that
file (tests/_direct_cases.py: pack_expected) -- exactly: they are copies, roundings to nearest-even bf16 and one fp32 multiply.
hpri_pack_weight modes 0-3, hpri_pack_weight_scaled, hpri_pack_weight_bf16 with split 0 / 1 / 2 in all modes,
hpri_pack_weight_bf16_scaled and hpri_pack_weight_bf16_gap; K = 5, 32 and 40 (a partial chunk, one whole chunk, one and a
quarter), Ncols = 7 and 70 padded to 64 and 128.  The destination starts as NaN, so pad rows and columns must have been written,
as exact zeros.  Needs a real MI355X: ``-m gpu``."""
import ctypes
import functools

import pytest
import torch

import _direct_cases as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = (5, 32, 40)
NCOLS = ((7, 64), (70, 128))


def P(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    from hyperpri_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _case(mode, K, ncols, ncols_pad, T, scaled=False):
    """Source weight in its nn.Parameter layout, the packer's (src_d1, Cup) and the expected panel values
    [chunks][T][32][ncols_pad]."""
    g = torch.Generator().manual_seed(1000 * mode + 10 * K + ncols + T)
    cup = 0
    if mode == 0:
        w, d1 = torch.randn(ncols, K, T, generator=g), K
    elif mode == 1:
        w, d1 = torch.randn(K, ncols, T, generator=g), ncols
    elif mode == 2:
        cup = D.cdiv(ncols, 4)
        w, d1 = torch.randn(K, cup, 4, generator=g), cup
    else:
        cup = D.cdiv(K, 4)
        w, d1 = torch.randn(ncols, cup, 4, generator=g), cup
    scale = (torch.rand(ncols, generator=g) + 0.5) if scaled else None
    want = D.pack_expected(w, mode, K, ncols, ncols_pad, T, d1, cup, None if scale is None else scale.numpy())
    return w, d1, cup, scale, torch.from_numpy(want)


def _planes(want, split):
    """[chunks][T][32][ncols_pad] fp32 -> the bf16 packers' [chunks][T][plane][ncols_pad][32]: plane p = bf16(rest), rest -= plane."""
    rest = want.permute(0, 1, 3, 2).contiguous()
    out = []
    for _ in range(split + 1):
        h = rest.bfloat16()
        out.append(h)
        rest = rest - h.float()
    return torch.stack(out, 2)


def _cases():
    return [(m, K, n, npad, T) for m in (0, 1, 2, 3) for K in KS for (n, npad) in NCOLS for T in ((9, 1) if m < 2 and K == 5 else (9,) if m < 2 else (1,))]


@pytest.mark.parametrize("mode,K,ncols,ncols_pad,T", _cases())
def test_pack_weight_fp32_layout(lib, mode, K, ncols, ncols_pad, T):
    w, d1, cup, _, want = _case(mode, K, ncols, ncols_pad, T)
    n = lib.hpri_packed_weight_floats(K, ncols_pad, T)
    assert n == want.numel()
    wd, wp = w.to(DEV), torch.full((n,), float("nan"), device=DEV)
    assert lib.hpri_pack_weight(P(wd), P(wp), mode, K, ncols, ncols_pad, T, cup, w.shape[0], d1, _st()) == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    got = wp.cpu().reshape(want.shape)
    assert torch.equal(got, want)
    assert float(got[:, :, :, ncols:].abs().max()) == 0.0                               # pad columns
    if K % 32:
        assert float(got[-1, :, K % 32:, :].abs().max()) == 0.0                          # pad rows of the last chunk


@pytest.mark.parametrize("split", (0, 1, 2))
@pytest.mark.parametrize("mode,K,ncols,ncols_pad,T", _cases())
def test_pack_weight_bf16_layout_and_planes(lib, mode, K, ncols, ncols_pad, T, split):
    """Same values as the fp32 pack, k contiguous per column, split + 1 planes per tap.  The planes reproduce w to the precision
    pack.hip and conv_fwd.hip claim: hi + lo carries 16 mantissa bits (|w - hi - lo| <= 2^-17 |w|), hi + mid + lo is w exactly."""
    w, d1, cup, _, want = _case(mode, K, ncols, ncols_pad, T)
    wantp = _planes(want, split)
    wd, wp = w.to(DEV), torch.full((wantp.numel(),), float("nan"), dtype=torch.bfloat16, device=DEV)
    rc = lib.hpri_pack_weight_bf16(P(wd), P(wp), mode, K, ncols, ncols_pad, T, d1, cup, split, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    got = wp.cpu().reshape(wantp.shape)
    assert torch.equal(got.float(), wantp.float()) and not torch.isnan(got.float()).any()
    total = got.double().sum(2)                                                       # the plane sum, [chunks][T][ncols_pad][32]
    src = want.permute(0, 1, 3, 2).double()
    if split == 1:
        assert torch.all((total - src).abs() <= 2.0 ** -17 * src.abs())
        assert float((total - src).abs().max()) > 0.0                                 # ... and two planes are not the fp32 value
    if split == 2:
        assert torch.equal(total, src)
    assert float(got[:, :, :, ncols:, :].float().abs().max()) == 0.0
    if K % 32:
        assert float(got[-1, :, :, :, K % 32:].float().abs().max()) == 0.0


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("ncols,ncols_pad", NCOLS)
def test_pack_weight_scaled(lib, K, ncols, ncols_pad):
    """Mode 0 with a per-output-channel scale (the eval-mode BatchNorm fold): one fp32 multiply, then -- in the bf16 layouts --
    the rounding / plane split of the product."""
    w, d1, _, scale, want = _case(0, K, ncols, ncols_pad, 9, scaled=True)
    wd, sd = w.to(DEV), scale.to(DEV)
    wp = torch.full((want.numel(),), float("nan"), device=DEV)
    assert lib.hpri_pack_weight_scaled(P(wd), P(wp), P(sd), K, ncols, ncols_pad, 9, d1, _st()) == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    assert torch.equal(wp.cpu().reshape(want.shape), want)
    plain = _case(0, K, ncols, ncols_pad, 9)[4]
    assert not torch.equal(want, plain) and torch.equal(want == 0, plain == 0)
    for split in (0, 1, 2):
        wantp = _planes(want, split)
        wpb = torch.full((wantp.numel(),), float("nan"), dtype=torch.bfloat16, device=DEV)
        assert lib.hpri_pack_weight_bf16_scaled(P(wd), P(wpb), P(sd), K, ncols, ncols_pad, 9, d1, split, _st()) == 0, lib.hpri_last_error()
        torch.cuda.synchronize()
        assert torch.equal(wpb.cpu().reshape(wantp.shape).float(), wantp.float()), split


@pytest.mark.parametrize("mode,K,ncols,ncols_pad,gap_at,gap_len", [(0, 40, 7, 64, 5, 27), (0, 40, 70, 128, 5, 27), (0, 32, 70, 128, 0, 3),
                                                                   (1, 40, 70, 128, 7, 25), (1, 5, 7, 64, 2, 3), (1, 32, 70, 128, 45, 25)])
def test_pack_weight_bf16_gap(lib, mode, K, ncols, ncols_pad, gap_at, gap_len):
    """The input-channel axis (k in mode 0, the columns in mode 1) carries gap_len structural zeros from gap_at on; the weight
    tensor has the unpadded width."""
    T = 9
    width = (K if mode == 0 else ncols) - gap_len
    g = torch.Generator().manual_seed(77 + gap_at)
    w = torch.randn(ncols, width, T, generator=g) if mode == 0 else torch.randn(K, width, T, generator=g)
    want = torch.from_numpy(D.pack_expected(w, mode, K, ncols, ncols_pad, T, width, 0, None, gap_at, gap_len))
    wantp = _planes(want, 0)
    wd, wp = w.to(DEV), torch.full((wantp.numel(),), float("nan"), dtype=torch.bfloat16, device=DEV)
    rc = lib.hpri_pack_weight_bf16_gap(P(wd), P(wp), mode, K, ncols, ncols_pad, T, width, gap_at, gap_len, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    got = wp.cpu().reshape(wantp.shape).float()
    assert torch.equal(got, wantp.float())
    gap = got[0, :, 0, :, gap_at:gap_at + gap_len] if mode == 0 and gap_at + gap_len <= 32 else got[:, :, 0, gap_at:gap_at + gap_len, :]
    assert float(gap.abs().max()) == 0.0 and int((wantp.float() != 0).sum()) == w.numel()          # every weight landed, once
    # the gap must fit the padded axis and leave the weight's own width
    assert lib.hpri_pack_weight_bf16_gap(P(wd), P(wp), mode, K, ncols, ncols_pad, T, width + 1, gap_at, gap_len, _st()) != 0
