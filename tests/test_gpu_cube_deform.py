"""Deforming gather of the cube cache on the device (csrc/cache_warp.hip, csrc/cache_deform.hip through hyperpri_amd/cache.py): neutral entries give the
warp kernels' bits, the elastic field matches its fp64 restatement, deformed images lie within the warp test's tolerance and masks
are exact, the noise is the documented Philox / Box-Muller stream, CutMix is a bit-exact ``torch.where`` of unmixed outputs, and
epochs reproduce the host planner.  The restatement is tests/_deform_ref.py (checked by tests/test_cube_deform_cpu.py).
Needs a real MI355X: ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

import _deform_ref as R
from conftest import record_margin
from test_cube_warp_cpu import centre_shift
from test_gpu_cube_warp import BANDS, STORES, _clone, _gen, _setup, _spy, _step, _tiny_cache, _tiny_cubenet, _underlying

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _poison(cache):
    """NaN into the output, mask and field buffers before a call: whatever the kernels do not write shows."""
    cache._out[0].fill_(float("nan"))
    cache._mout[0].fill_(float("nan"))
    for f in cache._fout:
        if f is not None:
            f.fill_(float("nan"))


def _name(band, store):
    return f"{band[2] - band[1]}b/{'f16' if store == torch.float16 else 'f32'}"


def _case_kw(case, fh=0, fw=0):
    """``cache.batch`` arguments of an elastic case's three samples (tests/_deform_ref.py: ``case_warp_entries`` are their entries)."""
    geom = case[0]
    return dict(patch=(geom[2], geom[3]), flip_h=fh, flip_w=fw, angle=[p[0] for p in R.CASE_PARAMS], zoom=[p[1] for p in R.CASE_PARAMS],
                shift=[centre_shift(geom, p[2], p[3]) for p in R.CASE_PARAMS], gain=R.CASE_GAINS, offset=R.CASE_OFFSETS)


def _deform_rows(n, h, w, pitch=None, noise=None, cutmix=None):
    """The deform entries ``cache.batch`` builds for these arguments (lattices back to back in the node table)."""
    from hyperpri_amd.cache import deform_entries, elastic_lattice
    gy, gx = elastic_lattice(h, w, pitch) if pitch else (0, 0)
    nz = noise or [(0.0, 0, 0)] * n
    cm = cutmix or [(-1, 0, 0, 0, 0)] * n
    return deform_entries([c[0] for c in cm], [c[1] for c in cm], [c[2] for c in cm], [c[3] for c in cm], [c[4] for c in cm],
                          [j * 2 * gy * gx if pitch else -1 for j in range(n)], [gy] * n, [gx] * n, [1 / pitch if pitch else 0.0] * n,
                          [z[0] for z in nz], [z[1] for z in nz], [z[2] for z in nz]).numpy()


# ---- 1. neutral entries: the warp kernels' bits -------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("band", BANDS)
def test_neutral_deform_is_the_warp_kernel_bit_for_bit(band, store):
    from hyperpri_amd.cache import elastic_lattice
    C = band[2] - band[1]
    cs = (C + 7) // 8 * 8
    variants = [dict(), dict(flip_h=1), dict(flip_w=1), dict(flip_h=1, flip_w=1), dict(flip_h=[0, 1], flip_w=[1, 0]), dict(angle=90.0),
                dict(angle=[17.0, -33.0], zoom=[1.25, 0.8], shift=[(0.54, 0.36), (-0.2, 0.11)], gain=1.7, offset=0.3, band_drop=(0, 1))]
    for geom in R.GEOMS:
        Hs, Ws, h, w = geom
        cache, _, _ = _setup(Hs, Ws, band, store)
        zero = np.zeros((2,) + elastic_lattice(h, w, 4.0) + (2,))
        for kw in variants:
            kw = dict(kw, patch=(h, w))
            x, m, under = _clone(cache.batch([2, 0], _force_warp=True, **kw), cs)
            for extra in (dict(_force_deform=True), dict(_force_deform=True, elastic=(zero, 4.0))):
                _poison(cache)
                out, calls = _spy(lambda: cache.batch([2, 0], **kw, **extra))
                assert calls == (["hpri_elastic_field"] if "elastic" in extra else []) + ["hpri_cube_deform", "hpri_mask_deform"]
                assert getattr(out["image"], "_hpri_zero_padded", False) and out["index"] == ["box2", "box0"]
                assert torch.equal(out["image"], x) and torch.equal(out["mask"], m), (geom, kw, list(extra))
                assert torch.equal(_underlying(out["image"], cs), under)
                if "elastic" in extra:
                    f = cache._fout[0][:2]
                    assert torch.count_nonzero(f) == 0 and not torch.signbit(f).any()          # exact +0
    # neutral values without the force flag keep the old paths
    _, calls = _spy(lambda: cache.batch([2, 0], noise=(0.0, 5, 6), cutmix=[(-1, 0, 3, 0, 3), (1, 0, 3, 0, 3)]))   # none, and its own index
    assert calls == ["hpri_cube_gather", "hpri_mask_gather"]
    _, calls = _spy(lambda: cache.batch([2, 0], gain=1.1, noise=[(-1.0, 5, 6), (0.0, 1, 2)], cutmix=(1, 4, 4, 0, 3)))        # an empty rectangle
    assert calls == ["hpri_cube_warp", "hpri_mask_warp"]


# ---- 2. the field -------------------------------------------------------------------------------------------------------------
def test_elastic_field_matches_the_restatement_and_bad_descriptors_give_zeros():
    from hyperpri_amd import _lib
    from hyperpri_amd.cache import deform_entries
    from hyperpri_amd.engine import _p
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for case in R.ELASTIC_CASES + [((0, 0, 33, 70), 7.5, 3.0, 21)]:         # (and a pitch that is no power of two)
        (_, _, h, w), pitch, _, _ = case
        nodes = R.case_nodes(case)
        gy, gx = nodes.shape[1:3]
        cell = 2 * gy * gx
        flat = nodes.ravel()
        # samples 0..2: their lattices (the last one ends exactly at the table's end); 3: none; 4: starts inside, ends past the end;
        # 5: starts past the end; 6: gy < 4; 7: gx < 4; 8: a descriptor whose 2 * gy * gx overflows 64 bits
        off = [0, cell, 2 * cell, -1, 2 * cell + 2, 3 * cell, 0, 0, 0]
        gys = [gy] * 6 + [3, gy, 2 ** 31 - 1]
        gxs = [gx] * 6 + [gx, 3, 2 ** 31 - 1]
        n = len(off)
        rows = deform_entries([-1] * n, [0] * n, [0] * n, [0] * n, [0] * n, off, gys, gxs, [1 / pitch] * n, [0.0] * n, [0] * n, [0] * n)
        want = R.fields64(rows.numpy(), flat, h, w)
        assert want[:3].any() and not want[3:].any()
        d_rows, d_nodes = rows.to(DEV), torch.from_numpy(flat).to(DEV)
        field = torch.full((n, h, w, 2), float("nan"), device=DEV)
        _lib.call("hpri_elastic_field", _p(d_nodes), d_nodes.numel(), _p(d_rows), n, h, w, _p(field), stream)
        got = field.double().cpu().numpy()
        tol = 2.0 ** -18 * float(np.abs(nodes).max())
        err = float(np.abs(got[:3] - want[:3]).max())
        print(f"field {h}x{w} pitch {pitch}: max error {err:.3e}, tolerance {tol:.3e}")
        record_margin(f"cube_deform/field/{h}x{w}", err, tol)
        assert err <= tol
        assert torch.count_nonzero(field[3:]) == 0 and not torch.signbit(field[3:]).any()       # exact +0, and no fault
        # an empty node table: every sample gets zeros
        field.fill_(float("nan"))
        _lib.call("hpri_elastic_field", ctypes.c_void_p(0), 0, _p(d_rows), n, h, w, _p(field), stream)
        assert torch.count_nonzero(field) == 0


# ---- 3. elastic image and mask --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("band", BANDS)
def test_elastic_image_and_mask_parity_with_the_restatement(band, store):
    """The restatement is evaluated from the DEVICE field read back (the field itself is pinned by the test above): image within
    the warp test's per-sample tolerance with S over the displaced coordinates, mask exact outside the pixels whose coordinate lies
    within 1e-3 of a k + 1/2 (at most 2 % per case: tests/test_cube_deform_cpu.py)."""
    C = band[2] - band[1]
    cs = (C + 7) // 8 * 8
    for ci, case in enumerate(R.ELASTIC_CASES):
        (Hs, Ws, h, w), pitch, _, _ = case
        cache, stored, masks = _setup(Hs, Ws, band, store, classes=4 if ci == 0 else 2)
        nodes = R.case_nodes(case)
        deform = _deform_rows(3, h, w, pitch)
        cache.batch([0, 1, 2], patch=(h, w))                    # a first tenant of the buffers, then poison
        for fh, fw in ((0, 0), (1, 1)):
            _poison(cache)
            out = cache.batch([0, 1, 2], elastic=(nodes, pitch), **_case_kw(case, fh, fw))
            fields = cache._fout[0][:3].double().cpu().numpy()
            assert np.isfinite(fields).all() and np.abs(fields).max() > 0.3
            want, want_m, tols, sure = R.restate_deform(R.case_warp_entries(case, fh, fw), deform, fields, stored, masks, C, cs, h, w)
            got = _underlying(out["image"], cs).double().cpu().numpy()
            assert got.shape == want.shape and not np.isnan(got).any()
            key = f"{_name(band, store)}/{Hs}x{Ws}:{h}x{w}/flip{fh}{fw}"
            for i, tol in enumerate(tols):
                err = float(np.abs(got[i] - want[i]).max())
                print(f"elastic {key} sample {i}: max error {err:.3e}, tolerance {tol:.3e}")
                record_margin(f"cube_deform/elastic/{key}", err, tol)
                assert err <= tol, (key, i, err, tol)
                assert not got[i][..., C:].any()
            gm = out["mask"].double().cpu().numpy()
            assert sure.mean() >= 0.98 and not np.isnan(gm).any() and np.array_equal(gm[sure], want_m[sure]), key
            # the field did change the picture
            plain = cache.batch([0, 1, 2], **_case_kw(case, fh, fw))
            assert not np.array_equal(_underlying(plain["image"], cs).double().cpu().numpy(), got)


# ---- 4. noise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("band", BANDS)
def test_noise_is_the_documented_stream(band, store):
    """out(sigma) - out(0) from the same kernel against sigma * z of the restatement within
    sigma * 2^-17 + 2^-23 * (|out(0)| + 5.77 sigma): 2 ulp each for logf, sqrtf, cospif and sinpif plus one product rounding at
    |z| <= 5.77 give |dz| <= 2.4e-6 (2^-17 is three times that); the second term is the rounding of the final fma and of the
    difference.  A wrong stream is wrong by about sigma."""
    C = band[2] - band[1]
    cs = (C + 7) // 8 * 8
    drop = (1, 2) if C >= 3 else (0, 0)                   # (the one-band cube keeps its band)
    for case in (R.ELASTIC_CASES[0], R.ELASTIC_CASES[2]):
        (Hs, Ws, h, w), pitch, _, _ = case
        cache, _, _ = _setup(Hs, Ws, band, store)
        geo = dict(_case_kw(case), elastic=(R.case_nodes(case), pitch), band_drop=drop)
        noise = [(0.05, 0xDEADBEEF, 17), (0.0, 1, 2), (0.3, 2 ** 32 - 1, 2 ** 31)]
        mixes = [None, [(2, 1, 3, 2, 30), (-1, 0, 0, 0, 0), (0, 0, 2, 0, 4)]]                 # the owner changes, the noise must not
        for cutmix in mixes:
            base = cache.batch([0, 1, 2], _force_deform=True, cutmix=cutmix, **geo)
            b_under, b_mask = _underlying(base["image"], cs).clone(), base["mask"].clone()
            _poison(cache)
            out = cache.batch([0, 1, 2], noise=noise, cutmix=cutmix, **geo)
            under = _underlying(out["image"], cs)
            assert not torch.isnan(under).any() and torch.equal(out["mask"], b_mask)           # the mask is never touched
            assert torch.count_nonzero(under[..., C:]) == 0 and torch.count_nonzero(under[..., drop[0]:drop[0] + drop[1]]) == 0
            assert torch.equal(under[1], b_under[1])                                           # sigma 0: the same bits
            for s, (sigma, k0, k1) in enumerate(noise):
                if sigma == 0:
                    continue
                sg = float(np.float32(sigma))
                z = R.noise64(k0, k1, h, w, cs)
                z[..., C:] = 0.0
                z[..., drop[0]:drop[0] + drop[1]] = 0.0
                b = b_under[s].double().cpu().numpy()
                diff = under[s].double().cpu().numpy() - b
                tol = sg * 2.0 ** -17 + 2.0 ** -23 * (np.abs(b) + R.ZMAX * sg)
                ratio = float((np.abs(diff - sg * z) / tol).max())
                print(f"noise {_name(band, store)} {h}x{w} sample {s} cutmix {cutmix is not None}: worst error / tolerance {ratio:.3f}")
                record_margin(f"cube_deform/noise/{_name(band, store)}/{h}x{w}", ratio, 1.0)
                assert ratio <= 1.0, (s, ratio)
                assert float(np.abs(diff).max()) > sg                                          # (there is noise)
        # two samples that differ in nothing but the key differ; with the same key they carry the same bits
        same = dict(patch=(h, w), angle=10.0, elastic=(np.repeat(R.case_nodes(case)[:1], 2, 0), pitch))
        a = _underlying(cache.batch([1, 1], noise=[(0.1, 7, 8), (0.1, 7, 8)], **same)["image"], cs).clone()
        assert torch.equal(a[0], a[1])
        for other in ((7, 9), (8, 8)):
            b = _underlying(cache.batch([1, 1], noise=[(0.1, 7, 8), (0.1,) + other], **same)["image"], cs)
            assert torch.equal(b[0], a[0]) and not torch.equal(b[1], a[1])
            assert float((b[1] - a[1])[..., :C].abs().mean()) > 0.05                            # by about sigma, everywhere


# ---- 5. CutMix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("band", BANDS)
def test_cutmix_is_a_bit_exact_where_of_unmixed_outputs(band, store):
    C = band[2] - band[1]
    cs = (C + 7) // 8 * 8
    for case in R.ELASTIC_CASES:
        (Hs, Ws, h, w), pitch, _, _ = case
        cache, _, _ = _setup(Hs, Ws, band, store, classes=4 if case is R.ELASTIC_CASES[0] else 2)
        geo = dict(_case_kw(case, 0, 1), elastic=(R.case_nodes(case), pitch), band_drop=[(0, 0), (1, 2) if C >= 3 else (0, 0), (0, 1)])
        _, m, under = _clone(cache.batch([0, 1, 2], **geo), cs)
        # an edge inside a work item (60 or 2 quads per pixel, 512 per item) | empty | reaching past the window on every side;
        # then: out of range (3, 7, a large one), the sample's own index, -1
        rects = [[(2, 1, h - 1, 2, w - 2), (0, 2, 2, 0, w), (1, -3, h + 100, w // 2, w + 100)],
                 [(3, 0, h, 0, w), (1, 0, h, 0, w), (-1, 0, h, 0, w)],
                 [(7, 0, h, 0, w), (2 ** 31 - 1, 0, h, 0, w), (0, 0, h, 0, w)],
                 [(1, 0, h, 0, 1), (2, h - 1, h, 0, w), (0, 0, 1, w - 1, w)]]
        for cm in rects:
            _poison(cache)
            out, calls = _spy(lambda: cache.batch([0, 1, 2], cutmix=cm, **geo))
            assert calls == ["hpri_elastic_field", "hpri_cube_deform", "hpri_mask_deform"]
            own = torch.from_numpy(R.owners(_deform_rows(3, h, w, pitch, cutmix=cm), h, w)).to(DEV)       # (3, h, w)
            want_u = under.clone()
            for s in range(3):
                for o in range(3):
                    sel = own[s] == o
                    want_u[s][sel] = under[o][sel]
            want_m = torch.gather(m, 0, own[:, None])
            got_u = _underlying(out["image"], cs)
            assert not torch.isnan(got_u).any()
            assert torch.equal(got_u, want_u) and torch.equal(out["mask"], want_m), (case[0], cm)
        assert (own != torch.arange(3, device=DEV)[:, None, None]).any()                        # the last set does mix


# ---- 6. epochs --------------------------------------------------------------------------------------------------------------------
EPOCH_KW = dict(patch=(20, 31), shuffle=True, random_crop=True, flips=True)


def _epoch(cache, seed, **kw):
    return _spy(lambda: [(_underlying(b["image"], 8).clone(), b["mask"].clone(), b["index"]) for b in cache.epoch(2, generator=_gen(seed), **EPOCH_KW, **kw)])


def test_deformed_epoch_reproduces_batch_called_with_the_plans_values():
    """Identity geometry with gain / offset / band drop (values ``batch()`` turns into the very same entries), every deformation:
    each served batch equals ``cache.batch(...)`` called with what ``last_plan`` holds, bit for bit; unflagged batches are served by
    the old kernels."""
    from hyperpri_amd.cache import CubeAugment, CubeDeform, elastic_lattice, plan_epoch_deformed
    cache, _, _ = _tiny_cache(5)
    aug = CubeAugment(gain=(0.9, 1.1), offset=(-0.05, 0.05), band_drop=(0.5, 2))
    h, w = EPOCH_KW["patch"]
    pitch = 8.0
    gy, gx = elastic_lattice(h, w, pitch)
    seen = set()
    for dfm, seed in ((CubeDeform(elastic=(0.5, 1.5, pitch), noise=(0.01, 0.05), cutmix=(0.5, 0.2, 0.6)), 5),
                      (CubeDeform(elastic=(0.3, 1.5, pitch), cutmix=(0.3, 0.2, 0.6)), 6), (CubeDeform(noise=(0.02, 0.02)), 7)):
        want_plan = plan_epoch_deformed(5, 2, (36, 50), 6, aug, dfm, generator=_gen(seed), **EPOCH_KW)
        got, calls = _epoch(cache, seed, augment=aug, deform=dfm)
        plan = cache.last_plan
        assert torch.equal(plan.deform, want_plan.deform) and torch.equal(plan.entries, want_plan.entries) and plan.deformed == want_plan.deformed
        assert (plan.nodes is None) == (want_plan.nodes is None) and (plan.nodes is None or torch.equal(plan.nodes, want_plan.nodes))
        want_calls = []
        for b, (s, e) in enumerate(plan.batches):
            d = plan.deform[s:e].numpy()
            lat = bool((d[:, 5] >= 0).any())
            want_calls += ((["hpri_elastic_field"] if lat else []) + ["hpri_cube_deform", "hpri_mask_deform"] if plan.deformed[b] else
                           ["hpri_cube_warp", "hpri_mask_warp"] if plan.warped[b] else ["hpri_cube_gather", "hpri_mask_gather"])
            seen.add((plan.deformed[b], lat))
            t = plan.table[s:e].numpy()
            f = plan.entries[s:e].numpy()[:, 4:12].copy().view(np.float32).astype(np.float64)
            nodes = np.zeros((e - s, gy, gx, 2), dtype=np.float32)                    # (a zero lattice is no lattice: exact +0)
            for i in range(e - s):
                if d[i, 5] >= 0:
                    nodes[i] = plan.nodes.numpy()[d[i, 5]:d[i, 5] + 2 * gy * gx].reshape(gy, gx, 2)
            ref = cache.batch(t[:, 0], top=t[:, 1], left=t[:, 2], flip_h=t[:, 3] & 1, flip_w=(t[:, 3] >> 1) & 1, patch=(h, w), gain=f[:, 6],
                              offset=f[:, 7], band_drop=plan.entries[s:e, 1:3].numpy(), elastic=(nodes, pitch) if lat else None,
                              noise=[(float(r[9:10].view(np.float32)[0]), int(np.uint32(r[10])), int(np.uint32(r[11]))) for r in d],
                              cutmix=d[:, :5])
            under, m, names = got[b]
            assert torch.equal(_underlying(ref["image"], 8), under) and torch.equal(ref["mask"], m) and ref["index"] == names, (seed, b)
            assert not torch.isnan(under).any() and torch.count_nonzero(under[..., 6:]) == 0
        assert calls == want_calls, (seed, calls)
    assert (True, True) in seen and (True, False) in seen and (False, False) in seen


def test_deformed_epoch_with_rotations_matches_the_restatement():
    from hyperpri_amd.cache import CubeAugment, CubeDeform
    cache, stored, masks = _tiny_cache(5)
    aug = CubeAugment(p=0.7, rotate=20.0, zoom=(0.8, 1.25), shift=2.0, gain=(0.9, 1.1), offset=(-0.05, 0.05), band_drop=(0.5, 2))
    dfm = CubeDeform(elastic=(0.7, 1.5, 8.0), noise=(0.01, 0.05), cutmix=(0.6, 0.2, 0.6))
    h, w = EPOCH_KW["patch"]
    got = []
    for b in cache.epoch(2, generator=_gen(9), augment=aug, deform=dfm, **EPOCH_KW):
        k = b["image"]._hpri_slot
        got.append((_underlying(b["image"], 8).clone(), b["mask"].clone(), None if cache._fout[k] is None else cache._fout[k].clone()))
    plan = cache.last_plan
    assert all(plan.deformed) and (plan.deform[:, 0] >= 0).any() and (plan.deform[:, 5] >= 0).any()
    order = plan.order.tolist()
    for (under, m, fld), (s, e) in zip(got, plan.batches):
        d = plan.deform[s:e].numpy()
        fields = fld[:e - s].double().cpu().numpy() if (d[:, 5] >= 0).any() else None
        want, want_m, tols, sure = R.restate_deform(plan.entries[s:e].numpy(), d, fields, stored, masks, 6, 8, h, w)
        if fields is not None:                                                          # the field the kernels read is the planner's
            assert np.abs(fields - R.fields64(d, plan.nodes.numpy(), h, w)).max() <= 2.0 ** -18 * float(plan.nodes.abs().max())
        g = under.double().cpu().numpy()
        for i, tol in enumerate(tols):
            sg = R.sigma_of(d[i])
            bound = tol + sg * 2.0 ** -17 + 2.0 ** -23 * (float(np.abs(want[i]).max()) + R.ZMAX * sg)
            err = float(np.abs(g[i] - want[i]).max())
            record_margin("cube_deform/epoch", err, bound)
            assert err <= bound, (s, i, err, bound)
        assert sure.mean() > 0.98 and np.array_equal(m.double().cpu().numpy()[sure], want_m[sure])
    assert order == plan.table[:, 0].tolist()


def test_no_deform_is_todays_epoch_bit_for_bit():
    from hyperpri_amd.cache import CubeAugment, CubeDeform
    cache, _, _ = _tiny_cache(5)
    aug = CubeAugment(p=0.5, rotate=15.0, gain=(0.9, 1.1))
    for a in (None, aug):
        today, calls0 = _epoch(cache, 5, augment=a)
        assert not any(c.startswith(("hpri_cube_deform", "hpri_mask_deform", "hpri_elastic")) for c in calls0)
        for dfm in (None, CubeDeform(), CubeDeform(elastic=(1.0, 0.0, 8.0), cutmix=(0.0, 0.5, 0.5))):
            got, calls = _epoch(cache, 5, augment=a, deform=dfm)
            assert calls == calls0, (a, dfm)
            for (x, m, names), (x0, m0, names0) in zip(got, today):
                assert torch.equal(x, x0) and torch.equal(m, m0) and names == names0


def test_cubenet_consumes_a_deformed_batch_in_place():
    from hyperpri_amd.cache import elastic_lattice
    cache, _, _ = _tiny_cache()
    nodes = (np.random.default_rng(3).standard_normal((2,) + elastic_lattice(36, 50, 8.0) + (2,)) * 1.5).astype(np.float32)
    out = cache.batch([1, 0], angle=[12.0, -20.0], zoom=[1.1, 0.9], gain=[1.2, 0.9], band_drop=[(1, 2), (0, 0)], elastic=(nodes, 8.0),
                      noise=[(0.05, 1, 2), (0.02, 3, 4)], cutmix=[(1, 4, 20, 10, 40), (-1, 0, 0, 0, 0)])
    assert getattr(out["image"], "_hpri_zero_padded", False) and tuple(out["image"].shape) == (2, 1, 6, 36, 50)
    x_ref, m_ref = out["image"].contiguous().clone(), out["mask"].clone()
    assert torch.isfinite(x_ref).all() and float(x_ref.std()) > 0.1
    loss, logits, grads, _ = _step(_tiny_cubenet(), x_ref, m_ref)
    loss2, logits2, grads2, calls = _step(_tiny_cubenet(), out["image"], out["mask"], log_calls=True)
    assert calls and not any(c.startswith("hpri_nchw_to_nhwc") for c in calls)            # consumed in place
    assert torch.isfinite(loss2) and all(torch.isfinite(g).all() for g in grads2)
    assert torch.equal(loss2, loss) and torch.equal(logits2, logits) and all(torch.equal(a, b) for a, b in zip(grads2, grads))
