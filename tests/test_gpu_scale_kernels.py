"""The loss-scale and multi-tensor scaling kernels of step.hip called directly through the C ABI (include/hyperpri_hip.h) against a
plain host reference: hpri_loss_scale_pick (the rule s = min(static, 2^floor(log2(2 / max|g|))) the whole f16 mode rests on),
hpri_scale_tensors, hpri_scale_tensors_dev and hpri_unscale_accumulate.  Everything here is exact: the maximum of |g| is
order-free, the picked scale is a power of two, a product with a power of two is exact away from underflow, so the gates are bit
comparisons (recorded as the number of wrong elements against a bound of 0; U = 2^-24 appears only where a comment says why no
tolerance is needed).  Every destination sits inside a larger buffer of random "prior" data whose other elements must come back
bit for bit; the elements next to every source are NaN / inf, which a kernel that read past its tensor would carry into the
result.  Needs a real MI355X: ``-m gpu``."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import record_margin
from test_gpu_step import SIZES            # 58 tensors: two launches of 48 + 10, block edges at 4096 and 4097

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24                   # unit roundoff of fp32
NAN, INF = float("nan"), float("inf")
ERR_ARG = -1
GUARD = 16                       # floats of prior data in front of and behind every tensor
LS_BLOCKS, LS_PER_BLOCK = 256, 256 * 16
F32 = np.float32


def P(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    from hyperpri_amd import _lib
    return _lib.load()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Bit for bit (signed zeros and NaN payloads included)."""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _exact(key, got, want):
    """Bit for bit; the number of differing elements goes to the margins file against a bound of 0."""
    assert got.shape == want.shape, (key, got.shape, want.shape)
    bad = int((_bits(got) != _bits(want)).sum())
    record_margin(key, bad, 0)
    assert bad == 0, (key, bad, "elements differ")


# ------------------------------------------------------------------------------------------------------------------------------
# hpri_loss_scale_pick
# ------------------------------------------------------------------------------------------------------------------------------
def _expected_scale(m, stat):
    """s = min(stat, 2^max(floor(log2(2 / m)), -126)) with 2 / m the correctly rounded fp32 quotient; s = stat when m is 0 or not
    finite, or when the quotient overflows (m subnormal).  floor(log2 t) from math.frexp: t = f * 2^e, f in [0.5, 1)."""
    m, stat = F32(m), F32(stat)
    if not np.isfinite(m) or m == 0:
        return stat
    with np.errstate(over="ignore", under="ignore"):
        t = F32(2.0) / m
    if not (t > 0 and np.isfinite(t)):
        return stat
    _, e = math.frexp(float(t))
    return min(stat, F32(2.0 ** max(e - 1, -126)))


def _ls_nblk(n):
    return min((n + LS_PER_BLOCK - 1) // LS_PER_BLOCK, LS_BLOCKS)


def _pick(lib, x, n, stat, prior_slot):
    slot = prior_slot.clone()
    rc = lib.hpri_loss_scale_pick(P(x), n, float(stat), P(slot), _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    return slot.cpu()


def _check_slot(key, got, prior, n, s):
    """slot[0] == s and slot[1] == 1 / s exactly (s a power of two: the quotient is exact; otherwise the correctly rounded fp32
    quotient); the entries behind the nblk block maxima are the prior ones."""
    nblk = _ls_nblk(n)
    with np.errstate(over="ignore"):
        inv = F32(1.0) / F32(s)
    bad = int(got[0].item() != float(s)) + int(got[1].item() != float(inv)) + int((_bits(got[2 + nblk:]) != _bits(prior[2 + nblk:])).sum())
    record_margin(f"loss_scale_pick/n{n}/wrong_slot_entries", bad, 0)
    assert got[0].item() == float(s) and got[1].item() == float(inv), (key, got[0].item(), got[1].item(), float(s), float(inv))
    assert _same(got[2 + nblk:], prior[2 + nblk:]), (key, "slot entries past 2 + nblk")


M_VALUES = [("2^-3", F32(2.0 ** -3)), ("2^-3-", np.nextafter(F32(2.0 ** -3), F32(-INF))), ("2^-3+", np.nextafter(F32(2.0 ** -3), F32(INF))),
            ("1", F32(1.0)), ("3e38", F32(3e38)), ("subnormal", F32(1e-40))]


def test_expected_scale_reference():
    """The host rule itself at the values whose answer can be written down: 2 / 2^-3 = 16; one ulp below 2^-3 the quotient is just
    above 16, one ulp above it just below (2^3); at 3e38 the exponent clamps at -126; a subnormal and zero keep the static scale."""
    stat = 65536.0
    want = [16.0, 16.0, 8.0, 2.0, 2.0 ** -126, stat]
    assert [float(_expected_scale(m, stat)) for _, m in M_VALUES] == want
    assert float(_expected_scale(0.0, stat)) == stat and float(_expected_scale(INF, stat)) == stat
    assert float(_expected_scale(2.0 ** -3, 4.0)) == 4.0
    assert float(F32(1.0) / F32(2.0 ** -126)) == 2.0 ** 126


@pytest.mark.parametrize("n", [1, 4096, 4097, 256 * 4096 + 5])
def test_loss_scale_pick_rule(lib, n):
    """Every value of the maximum, at the first element, the last element and an element the last block reaches in its SECOND
    stride (n = 256 * 4096 + 5 makes the partial kernel stride), with either sign; the data behind element n - 1 is inf / NaN."""
    assert lib.hpri_loss_scale_slot_floats() == 2 + LS_BLOCKS
    nblk = _ls_nblk(n)
    g = torch.Generator().manual_seed(n)
    unit = (torch.rand(n, generator=g) * 2 - 1).to(DEV)
    buf = torch.full((GUARD + n + GUARD,), NAN, device=DEV)
    buf[GUARD + n:] = torch.tensor([INF, -INF, NAN, 3e38] * (GUARD // 4), device=DEV)
    x = buf[GUARD:GUARD + n]
    prior = (torch.rand(2 + LS_BLOCKS + 8, generator=g) + 0.5)
    prior_dev = prior.to(DEV)
    positions = sorted({0, n - 1, min(n - 1, (nblk - 1) * 256 + 7 + nblk * 256)})
    stat = 65536.0
    checked = 0
    for name, m in M_VALUES:
        for pos in positions:
            for sign in (1.0, -1.0):
                x.copy_(unit * (float(m) * 0.5))              # everything else below the maximum
                x[pos] = sign * float(m)
                got = _pick(lib, x, n, stat, prior_dev)
                _check_slot((n, name, pos, sign), got, prior, n, _expected_scale(m, stat))
                if float(m) >= 2.0 ** -126:                   # (fp32 subnormals may or may not survive the comparison chain)
                    assert float(got[2:2 + nblk].max()) == float(m), (n, name, pos, "block maxima")
                checked += 1
    # the block maxima one by one: block b owns the elements i with (i / 256) % nblk == b
    x.copy_(unit)
    got = _pick(lib, x, n, stat, prior_dev)
    pad = torch.zeros(-(-n // (256 * nblk)) * 256 * nblk)
    pad[:n] = unit.cpu().abs()
    _exact(f"loss_scale_pick/n{n}/block_maxima", got[2:2 + nblk], pad.view(-1, nblk, 256).amax(dim=(0, 2)))
    _check_slot((n, "unit"), got, prior, n, _expected_scale(float(pad.max()), stat))
    # all zeros: the static scale
    x.zero_()
    _check_slot((n, "zeros"), _pick(lib, x, n, stat, prior_dev), prior, n, F32(stat))
    # one NaN / +inf / -inf anywhere: the static scale
    for bad in (NAN, INF, -INF):
        for pos in positions:
            x.copy_(unit)
            x[pos] = bad
            _check_slot((n, bad, pos), _pick(lib, x, n, stat, prior_dev), prior, n, F32(stat))
    # a static scale below the picked power wins; one that is no power of two comes back as it is, with its rounded reciprocal
    x.copy_(unit * 0.0625)
    x[n - 1] = -0.125
    _check_slot((n, "stat 4"), _pick(lib, x, n, 4.0, prior_dev), prior, n, F32(4.0))
    _check_slot((n, "stat 3"), _pick(lib, x, n, 3.0, prior_dev), prior, n, F32(3.0))
    _check_slot((n, "stat 1000"), _pick(lib, x, n, 1000.0, prior_dev), prior, n, F32(16.0))
    assert checked == len(M_VALUES) * len(positions) * 2


def test_loss_scale_pick_error_returns(lib):
    x = torch.ones(64, device=DEV)
    slot = torch.zeros(2 + LS_BLOCKS, device=DEV)
    assert lib.hpri_loss_scale_pick(P(x), 64, 0.0, P(slot), _st()) == ERR_ARG
    assert lib.hpri_loss_scale_pick(P(x), 64, -1.0, P(slot), _st()) == ERR_ARG
    assert lib.hpri_loss_scale_pick(P(x), 0, 1.0, P(slot), _st()) == ERR_ARG
    assert lib.hpri_loss_scale_pick(P(x), -5, 1.0, P(slot), _st()) == ERR_ARG
    assert lib.hpri_loss_scale_pick(P(None), 64, 1.0, P(slot), _st()) == ERR_ARG
    assert lib.hpri_loss_scale_pick(P(x), 64, 1.0, P(None), _st()) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.all(slot == 0)


# ------------------------------------------------------------------------------------------------------------------------------
# hpri_scale_tensors / hpri_scale_tensors_dev / hpri_unscale_accumulate
# ------------------------------------------------------------------------------------------------------------------------------
def _sizes(zeros):
    """SIZES as it is (a tensor with elements opens each chunk), or with zero-numel tensors at the first, a middle and the last
    position of the first chunk of 48, at the first position of the second chunk and at the very end."""
    s = list(SIZES)
    if not zeros:
        return s
    for pos in (0, 20, 47, 48):
        s.insert(pos, 0)
    return s + [0]


def _arena(sizes, seed, bait=False):
    """One buffer that holds every tensor between GUARD floats on either side; values in +-[0.5, 2) (far from underflow for every
    factor used here).  bait: the guard floats are NaN / inf (a source: nothing outside a tensor may be read into a result)."""
    g = torch.Generator().manual_seed(seed)
    offs, total = [], GUARD
    for n in sizes:
        offs.append(total)
        total += n + GUARD
    buf = (torch.rand(total, generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, (total,), generator=g) * 2 - 1).float()
    if bait:
        keep = torch.zeros(total, dtype=torch.bool)
        for o, n in zip(offs, sizes):
            keep[o:o + n] = True
        pat = torch.tensor([NAN, INF, -INF])[torch.arange(total) % 3]
        buf = torch.where(keep, buf, pat)
    return buf, offs


def _ptr_array(buf, offs, sizes):
    """Zero-numel tensors carry a null pointer (allowed by the ABI)."""
    return (ctypes.c_void_p * len(sizes))(*[(buf.data_ptr() + 4 * o) if n else None for o, n in zip(offs, sizes)])


def _numel_array(sizes):
    return (ctypes.c_longlong * len(sizes))(*sizes)


def _scaled(buf, offs, sizes, factor, add=None):
    """buf with every tensor multiplied by the fp32 ``factor`` (one rounding) -- or, with ``add``, add's tensors times factor added
    onto buf's (the product exact, one rounding in the sum) -- and everything between the tensors left alone."""
    f = torch.tensor(float(factor), dtype=torch.float32)
    want = buf.clone()
    for o, n in zip(offs, sizes):
        if add is None:
            want[o:o + n] = buf[o:o + n] * f
        else:
            want[o:o + n] = buf[o:o + n] + add[o:o + n] * f
    return want


@pytest.mark.parametrize("zeros", [0, 1])
@pytest.mark.parametrize("factor", [2.0 ** -7, 0.3, 1024.0])
def test_scale_tensors_bit_exact(lib, factor, zeros):
    """t *= factor: one fp32 product per element, so torch's fp32 product bit for bit -- for a power of two and for a factor that
    is none; the guard floats between the tensors untouched (a block that looked up the wrong tensor or ran past numel)."""
    sizes = _sizes(zeros)
    buf, offs = _arena(sizes, 3)
    d = buf.to(DEV)
    rc = lib.hpri_scale_tensors(_ptr_array(d, offs, sizes), _numel_array(sizes), len(sizes), float(F32(factor)), _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    _exact(f"scale_tensors/{factor:g}/zeros{zeros}", d.cpu(), _scaled(buf, offs, sizes, F32(factor)))


@pytest.mark.parametrize("zeros", [0, 1])
@pytest.mark.parametrize("s", [1024.0, 1000.0])
@pytest.mark.parametrize("invert", [0, 1])
def test_scale_tensors_dev_bit_exact(lib, s, invert, zeros):
    """The same with the factor read from the loss-scale slot: slot[0], or slot[1] = 1 / slot[0] with ``invert``."""
    sizes = _sizes(zeros)
    buf, offs = _arena(sizes, 4)
    d = buf.to(DEV)
    inv = F32(1.0) / F32(s)
    slot = torch.tensor([s, float(inv), NAN, NAN], device=DEV)
    rc = lib.hpri_scale_tensors_dev(_ptr_array(d, offs, sizes), _numel_array(sizes), len(sizes), P(slot), invert, _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    _exact(f"scale_tensors_dev/{s:g}/inv{invert}/zeros{zeros}", d.cpu(), _scaled(buf, offs, sizes, inv if invert else F32(s)))


@pytest.mark.parametrize("zeros", [0, 1])
def test_unscale_accumulate_bit_exact(lib, zeros):
    """dst += src * slot[1] with a power-of-two slot: the product is exact (values in +-[0.5, 2) * 2^-10), so whether or not the
    compiler fuses it into the sum there is ONE rounding -- torch's fp32 dst + src * inv bit for bit.  The source's guards are
    NaN / inf; the destination's guards must come back untouched."""
    sizes = _sizes(zeros)
    dbuf, offs = _arena(sizes, 5)
    sbuf, _ = _arena(sizes, 6, bait=True)
    d, s = dbuf.to(DEV), sbuf.to(DEV)
    slot = torch.tensor([1024.0, 2.0 ** -10, NAN, NAN], device=DEV)
    rc = lib.hpri_unscale_accumulate(_ptr_array(d, offs, sizes), _ptr_array(s, offs, sizes), _numel_array(sizes), len(sizes), P(slot), _st())
    assert rc == 0, lib.hpri_last_error()
    torch.cuda.synchronize()
    _exact(f"unscale_accumulate/zeros{zeros}", d.cpu(), _scaled(dbuf, offs, sizes, 2.0 ** -10, add=sbuf))
    assert _same(s.cpu(), sbuf)


def test_scale_kernels_error_returns(lib):
    """A null tensor pointer with numel > 0, a null table, ntensors = 0 and a null slot are error returns; nothing is written."""
    sizes = [5, 0, 7]
    buf, offs = _arena(sizes, 7)
    d = buf.to(DEV)
    slot = torch.tensor([2.0, 0.5], device=DEV)
    ptrs, n = _ptr_array(d, offs, sizes), _numel_array(sizes)
    null_t = (ctypes.c_void_p * 3)(d.data_ptr() + 4 * offs[0], None, None)          # tensor 2 has 7 elements and no pointer
    neg = (ctypes.c_longlong * 3)(5, -1, 7)
    for call in (lambda p, m, k: lib.hpri_scale_tensors(p, m, k, 2.0, _st()),
                 lambda p, m, k: lib.hpri_scale_tensors_dev(p, m, k, P(slot), 0, _st()),
                 lambda p, m, k: lib.hpri_unscale_accumulate(p, p, m, k, P(slot), _st())):
        assert call(null_t, n, 3) == ERR_ARG
        assert call(None, n, 3) == ERR_ARG
        assert call(ptrs, None, 3) == ERR_ARG
        assert call(ptrs, n, 0) == ERR_ARG
        assert call(ptrs, neg, 3) == ERR_ARG
    assert lib.hpri_scale_tensors_dev(ptrs, n, 3, P(None), 0, _st()) == ERR_ARG
    assert lib.hpri_unscale_accumulate(ptrs, ptrs, n, 3, P(None), _st()) == ERR_ARG
    assert lib.hpri_unscale_accumulate(ptrs, null_t, n, 3, P(slot), _st()) == ERR_ARG
    torch.cuda.synchronize()
    assert _same(d.cpu(), buf)
