"""Augmenting gather of the cube cache on the device (csrc/cache_warp.hip through hyperpri_amd/cache.py): identity and quarter
turns are bit-exact against the plain gather, every other geometry matches the fp64 restatement of
tests/test_cube_warp_cpu.py (which that file checks against ``grid_sample``) within a tolerance computed from the inputs,
masks are exact, gain / offset / band drop / pad channels behave as documented, the networks consume a warped batch in place,
and epochs reproduce the host planner.  Needs a real MI355X: ``-m gpu``."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import record_margin
from oracle import hyperpri_oracle as O
from test_cube_warp_cpu import FLIPS, GEOMETRIES, PARAMS, case_entries, centre_shift, coords64, entry_fields, restate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BANDS = [(299, 25, 263), (13, 12, 13), (11, 2, 9)]          # rows of several work items; cs = 8 with 7 and with 1 pad channels
STORES = [torch.float32, torch.float16]
_CACHES = {}


def _u(seed, shape):
    return torch.from_numpy(O._u(seed, int(np.prod(shape))).reshape(shape).copy())


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _setup(Hs, Ws, band, store, classes=2, n=3):
    """A filled cache of ``n`` cubes (one per key, shared by the tests), the slots' stored values as fp64 (rounded once to half
    for fp16 slots) and the masks."""
    key = (Hs, Ws, band, store, classes, n)
    if key not in _CACHES:
        from hyperpri_amd.cache import CubeCache
        B, lo, hi = band
        cubes = [_u(300 + k + 10 * Hs, (Hs, Ws, B)) for k in range(n)]
        masks = [(_u(400 + k + 10 * Hs, (Hs, Ws)) * classes).to(torch.uint8) for k in range(n)]
        cache = CubeCache(n, Hs, Ws, B, hsi_lo=lo, hsi_hi=hi, device=DEV, store_dtype=store, out_slots=1)
        cache.fill((cubes[k], masks[k], f"box{k}") for k in range(n))
        stored = [(c.half().float() if store == torch.float16 else c)[..., lo:hi].double().numpy() for c in cubes]
        _CACHES[key] = (cache, stored, [m.numpy() for m in masks])
    return _CACHES[key]


def _underlying(x, cs):
    """The padded (N, h, w, cs) buffer behind a batch's image."""
    x4 = x.squeeze(1) if x.dim() == 5 else x
    N, _, h, w = x4.shape
    return torch.as_strided(x4, (N, h, w, cs), (h * w * cs, w * cs, cs, 1))


def _poison(cache):
    cache._out[0].fill_(float("nan"))
    cache._mout[0].fill_(float("nan"))


def _clone(out, cs):
    return out["image"].clone(), out["mask"].clone(), _underlying(out["image"], cs).clone()


def _check_against_restatement(key, out, entries, stored, masks, C, cs, h, w, check_mask=True):
    """Image within the per-sample tolerance on every channel of the padded buffer (dropped and pad channels are exact zeros in
    the restatement and must be exact zeros here), mask exact; returns the largest error / tolerance ratio."""
    want, want_m, tols, margin = restate(entries, stored, masks, C, cs, h, w)
    assert margin >= 1e-3, (key, margin)                         # no coordinate sits where the nearest pixel switches
    got = _underlying(out["image"], cs).double().cpu().numpy()
    assert got.shape == want.shape and not np.isnan(got).any(), key
    worst = 0.0
    for i, tol in enumerate(tols):
        err = float(np.abs(got[i] - want[i]).max())
        print(f"{key} sample {i}: max error {err:.3e}, tolerance {tol:.3e}")
        record_margin(f"cube_warp/{key}", err, tol)
        assert err <= tol, (key, i, err, tol)
        worst = max(worst, err / tol)
        _, dlo, dn, _ = entry_fields(entries[i])
        assert not got[i][..., C:].any() and not got[i][..., dlo:dlo + dn].any(), (key, i)
    if check_mask:
        assert out["mask"].dtype == torch.float32 and np.array_equal(out["mask"].double().cpu().numpy(), want_m), key
    return worst


# ---- 1. identity, quarter and half turns are exact -----------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("band", BANDS)
def test_identity_through_the_warp_kernel_is_bit_exact(band, store):
    C = band[2] - band[1]
    cs = (C + 7) // 8 * 8
    for geom in GEOMETRIES:
        Hs, Ws, h, w = geom
        cache, _, _ = _setup(Hs, Ws, band, store)
        for top, left in {((Hs - h) // 2, (Ws - w) // 2), (0, Ws - w), (Hs - h, 0)}:
            for fh, fw in FLIPS:
                kw = dict(top=top, left=left, flip_h=fh, flip_w=fw, patch=(h, w))
                plain = cache.batch([2, 0], **kw)
                stride = plain["image"].stride()
                x, m, under = _clone(plain, cs)
                _poison(cache)
                out = cache.batch([2, 0], _force_warp=True, **kw)
                assert tuple(out["image"].shape) == tuple(x.shape) and out["image"].stride() == stride
                assert getattr(out["image"], "_hpri_zero_padded", False) and out["index"] == ["box2", "box0"]
                assert torch.equal(out["image"], x) and torch.equal(out["mask"], m), (geom, top, left, fh, fw)
                assert torch.equal(_underlying(out["image"], cs), under)
                assert torch.count_nonzero(under[..., C:]) == 0


@pytest.mark.parametrize("store", STORES)
def test_quarter_and_half_turns_are_bit_exact(store):
    band = BANDS[0]
    cache, _, _ = _setup(16, 24, band, store, classes=4)
    for top, left in [(4, 8), (0, 16), (8, 3)]:
        kw = dict(top=top, left=left, patch=(8, 8))
        x, m, _ = _clone(cache.batch([1, 2], **kw), 240)
        for k in (1, 2, 3):
            _poison(cache)
            out = cache.batch([1, 2], angle=90.0 * k, **kw)
            assert torch.equal(out["image"], torch.rot90(x, k, (-2, -1))), (top, left, k)
            assert torch.equal(out["mask"], torch.rot90(m, k, (-2, -1)))
            assert torch.count_nonzero(_underlying(out["image"], 240)[..., 238:]) == 0
        x2, m2, _ = _clone(cache.batch([1, 2], flip_h=1, flip_w=1, **kw), 240)
        assert torch.equal(x2, torch.rot90(x, 2, (-2, -1)))
        _poison(cache)
        out = cache.batch([1, 2], angle=180.0, **kw)
        assert torch.equal(out["image"], x2) and torch.equal(out["mask"], m2)
        _poison(cache)
        out = cache.batch([1, 2], angle=[90.0, -90.0], flip_h=[1, 0], flip_w=[0, 1], **kw)        # a flip composes with the turn
        want = torch.stack([torch.flip(torch.rot90(x[0], 1, (-2, -1)), (-2,)), torch.flip(torch.rot90(x[1], 3, (-2, -1)), (-1,))])
        assert torch.equal(out["image"], want)


# ---- 2 + 3. bilinear parity within the computed tolerance, masks exact -----------------------------------------------------
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("band", BANDS)
def test_bilinear_and_mask_parity_with_the_restatement(band, store):
    """Every parameter set (one sample each, nine to a batch) x geometry x flip pair; no sample is exempt.  On an MI355X the
    tolerances computed here run from 1e-5 to 8e-5 and the largest error is 0.07 of its tolerance."""
    C = band[2] - band[1]
    cs = (C + 7) // 8 * 8
    slots = [i % 3 for i in range(len(PARAMS))]
    worst = 0.0
    for gi, geom in enumerate(GEOMETRIES):
        Hs, Ws, h, w = geom
        cache, stored, masks = _setup(Hs, Ws, band, store, classes=4 if gi == 0 else 2)
        sh = [centre_shift(geom, p[2], p[3]) for p in PARAMS]
        cache.batch(slots, patch=(h, w))                         # a first tenant of the output buffer, then poison
        for fh, fw in FLIPS:
            _poison(cache)
            out = cache.batch(slots, patch=(h, w), flip_h=fh, flip_w=fw, angle=[p[0] for p in PARAMS], zoom=[p[1] for p in PARAMS],
                              shift=sh)
            entries = case_entries(geom, slots, PARAMS, fh, fw)
            key = f"{band[2] - band[1]}b/{'f16' if store == torch.float16 else 'f32'}/{Hs}x{Ws}:{h}x{w}/flip{fh}{fw}"
            worst = max(worst, _check_against_restatement(key, out, entries, stored, masks, C, cs, h, w))
            assert tuple(out["image"].shape) == (len(PARAMS), 1, C, h, w)
    print(f"largest error / tolerance: {worst:.3f}")


# ---- 4. gain, offset, dropped bands, pad channels --------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("band,drop", [(BANDS[0], (3, 5)), (BANDS[2], (0, 1)), (BANDS[2], (6, 1)), (BANDS[0], (237, 1))])
def test_gain_offset_band_drop_and_pad_channels(band, drop, store):
    C = band[2] - band[1]
    cs = (C + 7) // 8 * 8
    slots = [i % 3 for i in range(len(PARAMS))]
    for geom in (GEOMETRIES[0], GEOMETRIES[1], GEOMETRIES[3]):
        Hs, Ws, h, w = geom
        cache, stored, masks = _setup(Hs, Ws, band, store)
        sh = [centre_shift(geom, p[2], p[3]) for p in PARAMS]
        geo = dict(patch=(h, w), flip_h=0, flip_w=1, angle=[p[0] for p in PARAMS], zoom=[p[1] for p in PARAMS], shift=sh)
        plain_mask = cache.batch(slots, **geo)["mask"].clone()
        _poison(cache)
        out = cache.batch(slots, gain=1.7, offset=0.3, band_drop=drop, **geo)
        entries = case_entries(geom, slots, PARAMS, 0, 1, gain=1.7, offset=0.3, drop=drop)
        _check_against_restatement(f"photometric/{C}b/{'f16' if store == torch.float16 else 'f32'}/{Hs}x{Ws}:{h}x{w}/drop{drop}", out,
                                   entries, stored, masks, C, cs, h, w)
        under = _underlying(out["image"], cs)
        assert not torch.isnan(under).any()
        assert torch.count_nonzero(under[..., drop[0]:drop[0] + drop[1]]) == 0           # dropped bands: exactly 0, not the offset
        assert torch.count_nonzero(under[..., C:]) == 0                                  # pad channels: exactly 0, not the offset
        kept = [c for c in range(C) if not drop[0] <= c < drop[0] + drop[1]]
        assert bool((under[..., kept] >= 0.3).all())                                     # (the offset did reach every other band)
        assert torch.equal(out["mask"], plain_mask)                                      # untouched by gain / offset / drop
    # identity geometry with gain / offset only is a warp batch too
    from hyperpri_amd.cache import warp_entries
    cache, stored, masks = _setup(12, 20, band, store)
    cache.batch([1], patch=(5, 7))
    _poison(cache)
    out = cache.batch([1], patch=(5, 7), gain=1.7, offset=0.3)
    entries = warp_entries([1], [3], [6], [0], [0], (5, 7), [0.0], [1.0], [0.0], [0.0], [1.7], [0.3], [0], [0]).numpy()
    _check_against_restatement(f"photometric/{C}b/identity", out, entries, stored, masks, C, cs, 5, 7)


# ---- 5. a warped and an identity sample in one batch -----------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_mixed_batch_identity_sample_stays_bit_exact(store):
    band = BANDS[0]
    geom = (12, 20, 5, 7)
    cache, stored, masks = _setup(12, 20, band, store)
    kw = dict(patch=(5, 7), flip_h=[0, 1], flip_w=[1, 0])
    x, m, _ = _clone(cache.batch([0, 2], **kw), 240)
    sh = centre_shift(geom, PARAMS[0][2], PARAMS[0][3])
    _poison(cache)
    out = cache.batch([0, 2], angle=[PARAMS[0][0], 0.0], zoom=[PARAMS[0][1], 1.0], shift=[sh, (0.0, 0.0)], **kw)
    assert torch.equal(out["image"][1], x[1]) and torch.equal(out["mask"][1], m[1])          # the identity sample: the stored bits
    assert not torch.equal(out["image"][0], x[0])
    from hyperpri_amd.cache import warp_entries
    entries = warp_entries([0, 2], [3, 3], [6, 6], [0, 1], [1, 0], (5, 7), [PARAMS[0][0], 0.0], [PARAMS[0][1], 1.0], [sh[0], 0.0],
                           [sh[1], 0.0], [1.0, 1.0], [0.0, 0.0], [0, 0], [0, 0]).numpy()
    _check_against_restatement(f"mixed/{'f16' if store == torch.float16 else 'f32'}", out, entries, stored, masks, 238, 240, 5, 7)


# ---- 6. the networks consume a warped batch in place -----------------------------------------------------------------------
def _step(net, x, mask, log_calls=False):
    import hyperpri_amd.engine as E
    calls = []
    orig = E._lib.call
    if log_calls:
        E._lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        logits = net(x)
        loss = torch.nn.BCEWithLogitsLoss()(logits, mask)
        loss.backward()
    finally:
        E._lib.call = orig
    grads = [p.grad.clone() for p in net.parameters()]
    for p in net.parameters():
        p.grad = None
    return loss.detach().clone(), logits.detach().clone(), grads, calls


def _tiny_cubenet():
    import hyperpri_amd as H
    net = H.CubeNET(6, 1, first_depth=64, bilinear=False)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())
    net.load_state_dict(O.synth_state_dict(shapes))
    return net.to(DEV).train()


def _tiny_cache(n=2, **kw):
    from hyperpri_amd.cache import CubeCache
    cubes = [_u(1235 + k, (36, 50, 9)) for k in range(n)]                # 9 bands on "disk", the net takes [2:8]
    masks = [(_u(4321 + k, (36, 50)) > 0.9).to(torch.uint8) for k in range(n)]
    cache = CubeCache(n, 36, 50, 9, hsi_lo=2, hsi_hi=8, device=DEV, **kw)
    assert cache.fill((cubes[k].numpy(), masks[k].numpy(), f"box{k}") for k in range(n)) == n
    return cache, [c[..., 2:8].double().numpy() for c in cubes], [m.numpy() for m in masks]


WARP_KW = dict(angle=[12.0, -20.0], zoom=[1.1, 0.9], shift=[(0.3, -0.7), (-1.2, 0.4)], gain=[1.2, 0.9], offset=[0.05, -0.02],
               band_drop=[(1, 2), (0, 0)])


def test_cubenet_consumes_a_warped_batch_in_place_bit_identical():
    cache, _, _ = _tiny_cache()
    out = cache.batch([1, 0], flip_w=[1, 0], **WARP_KW)
    assert getattr(out["image"], "_hpri_zero_padded", False) and tuple(out["image"].shape) == (2, 1, 6, 36, 50)
    x_ref, m_ref = out["image"].contiguous().clone(), out["mask"].clone()               # the same values, (N,1,C,H,W) contiguous
    assert not hasattr(x_ref, "_hpri_zero_padded") and x_ref.is_contiguous()
    assert torch.count_nonzero(x_ref[0, 0, 1:3]) == 0 and torch.count_nonzero(x_ref[1]) > 0 and float(x_ref.std()) > 0.1
    loss, logits, grads, _ = _step(_tiny_cubenet(), x_ref, m_ref)
    loss2, logits2, grads2, calls = _step(_tiny_cubenet(), out["image"], out["mask"], log_calls=True)
    assert calls and not any(c.startswith("hpri_nchw_to_nhwc") for c in calls)            # consumed in place
    assert torch.equal(loss2, loss) and torch.equal(logits2, logits)
    assert len(grads) == len(grads2) and all(torch.equal(a, b) for a, b in zip(grads2, grads))


def test_spectral_unet_consumes_a_warped_4d_batch_in_place_bit_identical():
    import hyperpri_amd as H
    from hyperpri_amd.cache import CubeCache

    def mk():
        net = H.SpectralUNET(22, 1, 48)
        shapes = OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())
        net.load_state_dict(O.synth_state_dict(shapes))
        return net.to(DEV).train()
    cubes = [_u(1238 + k, (12, 20, 22)) for k in range(2)]
    masks = [(_u(77 + k, (12, 20)) > 0.8).to(torch.uint8) for k in range(2)]
    cache = CubeCache(2, 12, 20, 22, device=DEV, unsqueeze_hsi=False)
    cache.fill((cubes[k], masks[k], k) for k in range(2))
    out = cache.batch([0, 1], **dict(WARP_KW, band_drop=[(20, 2), (0, 3)]))
    assert tuple(out["image"].shape) == (2, 22, 12, 20) and getattr(out["image"], "_hpri_zero_padded", False)
    a = _step(mk(), out["image"].contiguous().clone(), out["mask"].clone())
    b = _step(mk(), out["image"], out["mask"], log_calls=True)
    assert not any(c.startswith("hpri_nchw_to_nhwc") for c in b[3])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))


# ---- 7. epochs ---------------------------------------------------------------------------------------------------------------
EPOCH_KW = dict(patch=(20, 31), shuffle=True, random_crop=True, flips=True)


def _spy(fn):
    from hyperpri_amd import _lib
    calls, orig = [], _lib.call
    _lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        return fn(), calls
    finally:
        _lib.call = orig


def test_augmented_epoch_reproduces_the_host_plan():
    from hyperpri_amd.cache import CubeAugment, plan_epoch_augmented
    cache, stored, masks = _tiny_cache(7)
    aug = CubeAugment(p=0.6, rotate=20.0, zoom=(0.8, 1.25), shift=2.0, gain=(0.9, 1.1), offset=(-0.05, 0.05), band_drop=(0.5, 2))
    plan = plan_epoch_augmented(7, 3, (36, 50), 6, aug, generator=_gen(5), **EPOCH_KW)
    got, calls = _spy(lambda: [(_underlying(b["image"], 8).clone(), b["mask"].clone(), b["index"], b["image"].shape)
                               for b in cache.epoch(3, generator=_gen(5), augment=aug, **EPOCH_KW)])
    assert torch.equal(cache.last_plan.entries, plan.entries) and torch.equal(cache.last_plan.table, plan.table)
    assert [tuple(s) for _, _, _, s in got] == [(3, 1, 6, 20, 31), (3, 1, 6, 20, 31), (1, 1, 6, 20, 31)] and all(plan.warped)
    assert calls == ["hpri_cube_warp", "hpri_mask_warp"] * 3
    for (under, m, names, _), (s, e) in list(zip(got, plan.batches))[:2]:
        entries = plan.entries[s:e].numpy()
        want, want_m, tols, _ = restate(entries, stored, masks, 6, 8, 20, 31)
        g = under.double().cpu().numpy()
        for i, tol in enumerate(tols):
            err = float(np.abs(g[i] - want[i]).max())
            record_margin("cube_warp/epoch", err, tol)
            assert err <= tol, (s, i, err, tol)
        # random draws may land a coordinate on a k + 1/2, where fp32 and fp64 may pick different pixels: compare the rest
        sure = np.ones((e - s, 1, 20, 31), dtype=bool)
        for i, row in enumerate(entries):
            sx, sy, _ = coords64(entry_fields(row)[3], 20, 31)
            sure[i, 0] = (np.abs(sx - np.floor(sx) - 0.5) >= 1e-3) & (np.abs(sy - np.floor(sy) - 0.5) >= 1e-3)
        assert sure.mean() > 0.98 and np.array_equal(m.double().cpu().numpy()[sure], want_m[sure])
        assert names == [f"box{r}" for r in plan.table[s:e, 0].tolist()]
    assert (plan.entries[:, 2] > 0).any() and not torch.equal(got[0][0], got[1][0])


def test_neutral_augmentation_is_the_plain_epoch_bit_for_bit():
    from hyperpri_amd.cache import CubeAugment
    cache, _, _ = _tiny_cache(7)

    def run(**kw):
        return _spy(lambda: [(b["image"].clone(), b["mask"].clone(), b["index"]) for b in cache.epoch(3, generator=_gen(5), **EPOCH_KW, **kw)])
    plain, calls0 = run()
    table = cache.last_plan.table.clone()
    for aug in (None, CubeAugment(), CubeAugment(p=0.0, rotate=30.0, zoom=(0.5, 2.0), shift=3.0)):
        got, calls = run(augment=aug)
        assert torch.equal(cache.last_plan.table, table)
        assert calls == calls0 == ["hpri_cube_gather", "hpri_mask_gather"] * 3            # the unchanged kernels serve it
        assert len(got) == len(plain) == 3
        for (x, m, names), (x0, m0, names0) in zip(got, plain):
            assert torch.equal(x, x0) and torch.equal(m, m0) and names == names0
    # a plan that warps only some batches sends the others through the plain gather
    some, calls = run(augment=CubeAugment(p=0.3, rotate=15.0))
    flags = cache.last_plan.warped
    assert any(flags) and not all(flags)
    assert calls == [c for f in flags for c in (("hpri_cube_warp", "hpri_mask_warp") if f else ("hpri_cube_gather", "hpri_mask_gather"))]
    for f, (x, m, _), (x0, m0, _) in zip(flags, some, plain):
        assert f or (torch.equal(x, x0) and torch.equal(m, m0))


@pytest.mark.parametrize("out_slots", [1, 2])
def test_warped_output_buffers_rotate_without_host_synchronisation(out_slots):
    """Six consecutive training steps over one augmented epoch, nothing between them but stream order: every step's gradients
    equal those of a run that synchronises and clones each batch first."""
    from hyperpri_amd.cache import CubeAugment
    cache, _, _ = _tiny_cache(12, out_slots=out_slots)
    aug = CubeAugment(p=1.0, rotate=25.0, zoom=(0.8, 1.25), shift=2.0, gain=(0.9, 1.1), offset=(-0.05, 0.05), band_drop=(0.5, 2))
    kw = dict(batch_size=2, shuffle=True, patch=(32, 48), random_crop=True, flips=True, augment=aug)
    net = _tiny_cubenet()
    fast, slots = [], []
    for batch in cache.epoch(generator=_gen(21), **kw):
        slots.append(batch["image"]._hpri_slot)
        fast.append(_step(net, batch["image"], batch["mask"])[2])
    assert len(fast) == 6 and all(cache.last_plan.warped)
    assert slots == [i % out_slots for i in range(6)]
    torch.cuda.synchronize()
    net = _tiny_cubenet()
    slow = []
    for batch in cache.epoch(generator=_gen(21), **kw):
        torch.cuda.synchronize()
        x, m = batch["image"].contiguous().clone(), batch["mask"].clone()
        torch.cuda.synchronize()
        slow.append(_step(net, x, m)[2])
        torch.cuda.synchronize()
    for ga, gb in zip(fast, slow):
        assert all(torch.equal(a, b) for a, b in zip(ga, gb))
    assert not all(torch.equal(a, b) for a, b in zip(fast[0], fast[1]))          # (the steps do see different data)
