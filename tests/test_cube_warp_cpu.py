"""Augmenting gather of the cube cache (hyperpri_amd/cache.py: CubeAugment, plan_epoch_augmented; csrc/cache_warp.hip) -- CPU
half: the C-ABI entry points exist and reject bad arguments without a launch, the config validates, the planner keeps
``plan_epoch``'s draws and makes its own in the documented order whatever the knobs are, and the numpy fp64 restatement of the
kernels' semantics (used by tests/test_gpu_cube_warp.py) agrees with ``torch.nn.functional.grid_sample``.  No GPU needed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import hyperpri_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hpri_cube_warp", "hpri_mask_warp")

# (Hs, Ws, h, w)
GEOMETRIES = [(12, 20, 5, 7), (12, 20, 12, 20), (9, 14, 9, 14), (5, 40, 4, 37), (16, 24, 8, 8), (12, 20, 1, 20), (12, 20, 12, 1)]
# (angle in degrees, zoom, dx, dy): the source centre is ((Ws-1)/2 + dx, (Hs-1)/2 + dy)
PARAMS = [(17, 1.25, 0.54, 0.36), (17, 0.8, -0.20, 0.11), (-33, 1.25, 0.50, 0.23), (-33, 0.6, -1.86, -0.35), (90, 1.0, -2.25, 1.24),
          (45.5, 1.5, 0.27, -1.45), (-7.5, 0.6, -1.01, -0.73), (123, 1.25, -0.32, -0.29), (5, 1.25, -1.5, 0.5)]
FLIPS = [(0, 0), (1, 0), (0, 1), (1, 1)]


# ---- the restatement ---------------------------------------------------------------------------------------------------
def matrix64(angle, zoom, flip_h, flip_w):
    """A = (1/zoom) [[cos, -sin], [sin, cos]] in fp64; a column flip negates column 0, a row flip column 1; quarter turns exact."""
    if angle % 90 == 0:
        c, s = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][int(angle // 90) % 4]
    else:
        c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    a = np.array([[c, -s], [s, c]], dtype=np.float64) / zoom
    if flip_w:
        a[:, 0] = -a[:, 0]
    if flip_h:
        a[:, 1] = -a[:, 1]
    return a


def entry_fields(row):
    """One (16,) int32 entry -> (slot, drop_lo, drop_n, [a00, a01, cx, a10, a11, cy, gain, offset] as fp64 of the fp32 values)."""
    row = np.ascontiguousarray(np.asarray(row, dtype=np.int32))
    assert row.shape == (16,) and row[3] == 0 and not row[12:].any()
    f = row[4:12].view(np.float32).astype(np.float64)
    return int(row[0]), int(row[1]), int(row[2]), f


def coords64(f, h, w):
    """sx, sy (h, w) in fp64 from the fp32 table values, and S: the largest absolute partial sum of the two multiply-adds."""
    u = (np.arange(w, dtype=np.float64) - (w - 1) / 2)[None, :]
    v = (np.arange(h, dtype=np.float64) - (h - 1) / 2)[:, None]
    out, S = [], 0.0
    for au, av, c in ((f[0], f[1], f[2]), (f[3], f[4], f[5])):
        p, q = au * u + 0 * v, av * v + 0 * u
        for part in (p, q, p + q, p + c, q + c, p + q + c, np.array(c)):
            S = max(S, float(np.abs(part).max()))
        out.append(p + q + c)
    return out[0], out[1], S


def bilinear64(src, sy, sx):
    """src (Hs, Ws, C) fp64; neighbours (floor sy, floor sx), (+0,+1), (+1,+0), (+1,+1); outside the frame counts as 0."""
    Hs, Ws, C = src.shape
    y0, x0 = np.floor(sy), np.floor(sx)
    fy, fx = sy - y0, sx - x0
    out = np.zeros(sy.shape + (C,), dtype=np.float64)
    for dy, dx, wgt in ((0, 0, (1 - fy) * (1 - fx)), (0, 1, (1 - fy) * fx), (1, 0, fy * (1 - fx)), (1, 1, fy * fx)):
        yi, xi = (y0 + dy).astype(np.int64), (x0 + dx).astype(np.int64)
        ok = (yi >= 0) & (yi < Hs) & (xi >= 0) & (xi < Ws)
        val = src[np.clip(yi, 0, Hs - 1), np.clip(xi, 0, Ws - 1)]
        out += np.where(ok, wgt, 0.0)[..., None] * val
    return out


def nearest64(mask, sy, sx):
    Hs, Ws = mask.shape
    yi, xi = np.floor(sy + 0.5).astype(np.int64), np.floor(sx + 0.5).astype(np.int64)
    ok = (yi >= 0) & (yi < Hs) & (xi >= 0) & (xi < Ws)
    return np.where(ok, mask[np.clip(yi, 0, Hs - 1), np.clip(xi, 0, Ws - 1)], 0).astype(np.float64)


def half_margin(sy, sx):
    """Distance of the nearest coordinate to a k + 1/2 (where nearest-neighbour sampling switches pixels)."""
    return float(min(np.abs(s - np.floor(s) - 0.5).min() for s in (sy, sx)))


def restate(entries, cubes, masks, C, cs, h, w):
    """What the warp kernels must write for ``entries`` ((n, 16) int32): image (n, h, w, cs) fp64 with dropped and pad channels
    0, mask (n, 1, h, w), the per-sample tolerance of the issue and the smallest distance of a coordinate to a k + 1/2.
    ``cubes[slot]`` is the stored (Hs, Ws, C) slot content as fp64, ``masks[slot]`` (Hs, Ws)."""
    n = len(entries)
    img, msk, tols, margin = np.zeros((n, h, w, cs)), np.zeros((n, 1, h, w)), [], 1.0
    for i, row in enumerate(np.asarray(entries)):
        slot, dlo, dn, f = entry_fields(row)
        sx, sy, S = coords64(f, h, w)
        gain, offset = f[6], f[7]
        src = cubes[slot]
        img[i, :, :, :C] = gain * bilinear64(src, sy, sx) + offset
        img[i, :, :, dlo:dlo + dn] = 0.0
        msk[i, 0] = nearest64(masks[slot], sy, sx)
        R = max(float(src.max()), 0.0) - min(float(src.min()), 0.0)          # the zero fill is a neighbour too
        M = float(np.abs(src).max())
        tols.append(abs(gain) * (2 * 2.0 ** -21 * S * R + 2.0 ** -21 * M) + 2.0 ** -22 * (abs(gain) * M + abs(offset)))
        margin = min(margin, half_margin(sy, sx))
    return img, msk, tols, margin


def centre_shift(geom, dx, dy):
    """The ``shift`` that puts the centre of the CENTRED h x w window at ((Ws-1)/2 + dx, (Hs-1)/2 + dy)."""
    Hs, Ws, h, w = geom
    return ((Ws - 1) / 2 + dx - ((Ws - w) // 2 + (w - 1) / 2), (Hs - 1) / 2 + dy - ((Hs - h) // 2 + (h - 1) / 2))


def case_entries(geom, slots, params, flip_h, flip_w, gain=1.0, offset=0.0, drop=(0, 0)):
    """Entries for ``slots`` with one parameter set each, built by the package's ``warp_entries`` for the centred window."""
    from hyperpri_amd.cache import warp_entries
    Hs, Ws, h, w = geom
    n = len(slots)
    sh = [centre_shift(geom, p[2], p[3]) for p in params]
    return warp_entries(slots, [(Hs - h) // 2] * n, [(Ws - w) // 2] * n, [flip_h] * n, [flip_w] * n, (h, w), [p[0] for p in params],
                        [p[1] for p in params], [s[0] for s in sh], [s[1] for s in sh], [gain] * n, [offset] * n, [drop[0]] * n,
                        [drop[1]] * n).numpy()


def _u(seed, shape):
    return O._u(seed, int(np.prod(shape))).reshape(shape).copy()


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_warp_symbols_are_declared_and_exported():
    from hyperpri_amd import _lib
    header = open(os.path.join(ROOT, "include", "hyperpri_hip.h")).read()
    declared = set(re.findall(r"\b(hpri_\w+)\s*\(", header))
    decls = _lib.parse_header()
    lib = _lib.load()
    for n in NEW:
        assert n in declared and n in decls and hasattr(lib, n), n
        assert hasattr(_lib.load_f16(), n)
    assert len(decls["hpri_cube_warp"][1]) == 13 and len(decls["hpri_mask_warp"][1]) == 10


def test_warps_reject_bad_arguments_without_launch():
    from hyperpri_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(4096)                 # never dereferenced: every call below must fail its argument checks
    ok = dict(slots=3, Hs=12, Ws=20, cs=8, C=7, N=2, h=12, w=20)

    def cube(cache=one, dt=0, entries=one, dst=one, **kw):
        a = dict(ok, **kw)
        return lib.hpri_cube_warp(cache, dt, a["slots"], a["Hs"], a["Ws"], a["cs"], a["C"], entries, a["N"], a["h"], a["w"], dst, null)

    def mask(masks=one, entries=one, dst=one, **kw):
        a = dict(ok, **kw)
        return lib.hpri_mask_warp(masks, a["slots"], a["Hs"], a["Ws"], entries, a["N"], a["h"], a["w"], dst, null)
    for fn in (cube, mask):
        assert fn(null) == -1 and b"null" in lib.hpri_last_error()
        assert fn(entries=null) == -1 and b"null" in lib.hpri_last_error()
        assert fn(dst=null) == -1
        for bad in (dict(h=0), dict(w=0), dict(h=-3), dict(slots=0), dict(N=0), dict(Hs=0), dict(Ws=-1)):
            assert fn(**bad) == -1 and len(lib.hpri_last_error()) > 0, bad
        assert fn(h=4097) == -1 and b"4096" in lib.hpri_last_error()        # (a window larger than the frame is fine, up to here)
        assert fn(w=4097) == -1 and b"4096" in lib.hpri_last_error()
        assert fn(entries=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.hpri_last_error()
        assert fn(N=2 ** 20, h=4096) == -1 and b"too large" in lib.hpri_last_error()      # N * h >= 2^31
    assert cube(cs=12, C=12) == -1 and b"multiple of 8" in lib.hpri_last_error()
    assert cube(cs=4, C=4) == -1
    assert cube(cs=0) == -1
    assert cube(C=0) == -1 and b"band count" in lib.hpri_last_error()
    assert cube(C=9) == -1 and b"band count" in lib.hpri_last_error()
    assert cube(dt=2) == -1 and cube(dt=-1) == -1
    assert cube(cache=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.hpri_last_error()
    assert cube(dst=ctypes.c_void_p(4104)) == -1
    assert cube(cs=2 ** 21, C=8, w=4096) == -1 and b"too large" in lib.hpri_last_error()   # w * cs/4 >= 2^30
    with pytest.raises(RuntimeError, match="hpri_cube_warp"):
        _lib.call("hpri_cube_warp", null, 0, 3, 12, 20, 8, 7, null, 2, 12, 20, null, null)


# ---- config --------------------------------------------------------------------------------------------------------------
def test_cube_augment_rejects_bad_settings():
    import dataclasses
    import hyperpri_amd as H
    a = H.CubeAugment(p=0.5, rotate=20, zoom=(0.8, 1.25), shift=3, gain=(0.9, 1.1), offset=(-0.05, 0.05), band_drop=(0.3, 8))
    assert a.zoom == (0.8, 1.25) and a.band_drop == (0.3, 8) and H.CubeAugment().p == 0.0
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.p = 1.0
    nan, inf = float("nan"), float("inf")
    for bad in (dict(p=-0.1), dict(p=1.5), dict(p=nan), dict(rotate=inf), dict(rotate=nan), dict(shift=nan), dict(shift=inf),
                dict(zoom=(0.0, 1.0)), dict(zoom=(-1.0, 1.0)), dict(zoom=(0.05, 1.0)), dict(zoom=(1.0, 17.0)), dict(zoom=(1.0, nan)),
                dict(zoom=(1.0, inf)), dict(zoom=(1.2, 0.9)), dict(gain=(1.0, inf)), dict(gain=(nan, 1.0)), dict(offset=(0.0, nan)),
                dict(offset=(-inf, 0.0)), dict(band_drop=(1.5, 3)), dict(band_drop=(-0.1, 3)), dict(band_drop=(nan, 3)),
                dict(band_drop=(0.5, 0)), dict(band_drop=(0.5, -2))):
        with pytest.raises(ValueError, match="CubeAugment"):
            H.CubeAugment(**bad)
    H.CubeAugment(zoom=(1 / 16, 16.0))                                         # the bounds themselves are allowed


# ---- planner ---------------------------------------------------------------------------------------------------------------
AUG_KW = dict(p=0.7, rotate=25.0, zoom=(0.7, 1.4), shift=4.0, gain=(0.8, 1.3), offset=(-0.1, 0.2), band_drop=(0.4, 9))
PLAN_KW = dict(patch=(32, 48), shuffle=True, random_crop=True, flips=True)


def test_augmented_plan_keeps_the_plain_plans_order_windows_and_flips():
    from hyperpri_amd.cache import CubeAugment, plan_epoch, plan_epoch_augmented
    for n, bs, drop_last in [(45, 2, False), (7, 3, True), (1, 1, False)]:
        a = plan_epoch_augmented(n, bs, (608, 968), 238, CubeAugment(**AUG_KW), generator=_gen(7), drop_last=drop_last, **PLAN_KW)
        b = plan_epoch(n, bs, (608, 968), generator=_gen(7), drop_last=drop_last, **PLAN_KW)
        assert torch.equal(a.order, b.order) and torch.equal(a.table, b.table) and a.batches == b.batches and a.window == b.window
        assert a.entries.dtype == torch.int32 and tuple(a.entries.shape) == (b.table.shape[0], 16) and len(a.warped) == len(b.batches)
        assert torch.equal(a.entries[:, 0], b.table[:, 0])
    with pytest.raises(ValueError):
        plan_epoch_augmented(4, 2, (36, 50), 0)


def _restated_draws(n, C, aug, g, frame=(608, 968), hw=(32, 48)):
    """The documented draw order from a fresh generator: plan_epoch's five, then ten float64 vectors."""
    order = torch.randperm(n, generator=g)
    top = torch.randint(0, frame[0] - hw[0] + 1, (n,), generator=g)
    left = torch.randint(0, frame[1] - hw[1] + 1, (n,), generator=g)
    fh = torch.randint(0, 2, (n,), generator=g)
    fw = torch.randint(0, 2, (n,), generator=g)
    r = [torch.rand(n, dtype=torch.float64, generator=g).numpy() for _ in range(10)]
    rows = np.zeros((n, 16), dtype=np.int32)
    for j in range(n):
        warped = r[0][j] < aug["p"]
        angle = (2 * r[1][j] - 1) * aug["rotate"] if warped else 0.0
        zoom = math.exp(math.log(aug["zoom"][0]) + r[2][j] * (math.log(aug["zoom"][1]) - math.log(aug["zoom"][0]))) if warped else 1.0
        shx = (2 * r[3][j] - 1) * aug["shift"] if warped else 0.0
        shy = (2 * r[4][j] - 1) * aug["shift"] if warped else 0.0
        gain = aug["gain"][0] + r[5][j] * (aug["gain"][1] - aug["gain"][0])
        offset = aug["offset"][0] + r[6][j] * (aug["offset"][1] - aug["offset"][0])
        run = min(1 + int(math.floor(r[8][j] * aug["band_drop"][1])), aug["band_drop"][1], C)
        dn = run if r[7][j] < aug["band_drop"][0] else 0
        dlo = min(int(math.floor(r[9][j] * (C - run + 1))), C - run) if dn else 0
        a = matrix64(angle, zoom, int(fh[j]), int(fw[j]))
        f = np.array([a[0, 0], a[0, 1], int(left[j]) + (hw[1] - 1) / 2 + shx, a[1, 0], a[1, 1], int(top[j]) + (hw[0] - 1) / 2 + shy,
                      gain, offset], dtype=np.float64).astype(np.float32)
        rows[j, 0], rows[j, 1], rows[j, 2] = int(order[j]), dlo, dn
        rows[j, 4:12] = f.view(np.int32)
    return order, rows, r


def test_augmentation_draws_follow_the_documented_order():
    from hyperpri_amd.cache import CubeAugment, plan_epoch_augmented
    n, C = 45, 238
    plan = plan_epoch_augmented(n, 2, (608, 968), C, CubeAugment(**AUG_KW), generator=_gen(11), **PLAN_KW)
    order, rows, r = _restated_draws(n, C, AUG_KW, _gen(11))
    assert torch.equal(plan.order, order)
    got = plan.entries.numpy()
    assert np.array_equal(got[:, :4], rows[:, :4])                                       # slot, drop_lo, drop_n, reserved
    gf, wf = got[:, 4:12].copy().view(np.float32), rows[:, 4:12].copy().view(np.float32)
    assert np.array_equal(gf[:, [2, 5, 6, 7]], wf[:, [2, 5, 6, 7]])                      # cx, cy, gain, offset: the same fp64 expression
    assert np.abs(gf - wf).max() <= 2.0 ** -22                                           # the matrix: cos / sin, 1 ulp of freedom
    assert not got[:, 12:].any()
    # the draws do what they say: some samples warped and some not, runs inside the bands, values inside their ranges
    warped = r[0] < AUG_KW["p"]
    assert 0 < warped.sum() < n
    ident = gf[~warped][:, [0, 1, 3, 4]]
    assert set(np.abs(ident).ravel().tolist()) == {0.0, 1.0}
    assert (got[:, 2] > 0).any() and (got[:, 2] == 0).any() and (got[:, 1] + got[:, 2] <= C).all() and (got[:, 2] <= 9).all()
    assert (gf[:, 6] >= 0.8).all() and (gf[:, 6] <= 1.3).all() and (gf[:, 7] >= -0.1).all() and (gf[:, 7] <= 0.2).all()
    scale = np.hypot(gf[:, 0], gf[:, 3])                                                 # |column 0| = 1 / zoom
    assert (scale >= 1 / 1.4 - 1e-6).all() and (scale <= 1 / 0.7 + 1e-6).all()
    # the generator has moved by exactly these draws: the next epoch continues behind them
    g1, g2 = _gen(11), _gen(11)
    plan_epoch_augmented(n, 2, (608, 968), C, CubeAugment(**AUG_KW), generator=g1, **PLAN_KW)
    _restated_draws(n, C, AUG_KW, g2)
    assert torch.equal(torch.rand(4, generator=g1), torch.rand(4, generator=g2))


def test_augmentation_draws_do_not_depend_on_the_knobs():
    from hyperpri_amd.cache import CubeAugment, plan_epoch_augmented
    n, C = 44, 238
    full = plan_epoch_augmented(n, 2, (608, 968), C, CubeAugment(**AUG_KW), generator=_gen(3), **PLAN_KW).entries.numpy()
    ff = full[:, 4:12].copy().view(np.float32)
    for off in ("rotate", "zoom", "shift", "gain", "offset", "band_drop"):
        kw = dict(AUG_KW)
        kw[off] = dict(rotate=0.0, zoom=(1.0, 1.0), shift=0.0, gain=(1.0, 1.0), offset=(0.0, 0.0), band_drop=(0.0, 1))[off]
        g = _gen(3)
        e = plan_epoch_augmented(n, 2, (608, 968), C, CubeAugment(**kw), generator=g, **PLAN_KW).entries.numpy()
        f = e[:, 4:12].copy().view(np.float32)
        assert np.array_equal(e[:, 0], full[:, 0])
        if off != "band_drop":
            assert np.array_equal(e[:, 1:3], full[:, 1:3])
        if off != "gain":
            assert np.array_equal(f[:, 6], ff[:, 6])
        if off != "offset":
            assert np.array_equal(f[:, 7], ff[:, 7])
        if off not in ("rotate", "zoom"):
            assert np.array_equal(f[:, [0, 1, 3, 4]], ff[:, [0, 1, 3, 4]])
        if off != "shift":
            assert np.array_equal(f[:, [2, 5]], ff[:, [2, 5]])
        if off == "rotate":                                                              # the zoom stream is where it was
            assert np.allclose(np.hypot(f[:, 0], f[:, 3]), np.hypot(ff[:, 0], ff[:, 3]), rtol=1e-6, atol=0)
        h = _gen(3)
        plan_epoch_augmented(n, 2, (608, 968), C, CubeAugment(**AUG_KW), generator=h, **PLAN_KW)
        assert torch.equal(torch.rand(4, generator=g), torch.rand(4, generator=h))       # and the generator ends in the same state


def test_neutral_settings_flag_every_batch_as_plain():
    from hyperpri_amd.cache import CubeAugment, plan_epoch_augmented
    for aug in (None, CubeAugment(), CubeAugment(p=0.0, rotate=30.0, zoom=(0.5, 2.0), shift=5.0),
                CubeAugment(p=1.0), CubeAugment(p=1.0, band_drop=(0.0, 5))):
        plan = plan_epoch_augmented(45, 2, (608, 968), 238, aug, generator=_gen(5), **PLAN_KW)
        assert len(plan.warped) == 23 and not any(plan.warped)
        f = plan.entries.numpy()[:, 4:12].copy().view(np.float32)
        assert set(np.abs(f[:, [0, 1, 3, 4]]).ravel().tolist()) == {0.0, 1.0} and (f[:, 6] == 1).all() and (f[:, 7] == 0).all()
        assert not plan.entries[:, 1:4].any()
    for aug in (CubeAugment(p=1.0, rotate=10.0), CubeAugment(gain=(1.1, 1.2)), CubeAugment(offset=(0.1, 0.1)),
                CubeAugment(band_drop=(1.0, 3)), CubeAugment(p=1.0, shift=0.5), CubeAugment(p=1.0, zoom=(1.1, 1.1))):
        plan = plan_epoch_augmented(45, 2, (608, 968), 238, aug, generator=_gen(5), **PLAN_KW)
        assert all(plan.warped), aug
    some = plan_epoch_augmented(45, 2, (608, 968), 238, CubeAugment(p=0.3, rotate=10.0), generator=_gen(5), **PLAN_KW)
    assert any(some.warped) and not all(some.warped)                                     # the flag is per batch


def test_quarter_turn_matrices_are_exact():
    from hyperpri_amd.cache import warp_entries, warp_matrix
    want = {0: (1, 0, 0, 1), 90: (0, -1, 1, 0), 180: (-1, 0, 0, -1), 270: (0, 1, -1, 0), -90: (0, 1, -1, 0), 360: (1, 0, 0, 1),
            -180: (-1, 0, 0, -1)}
    for angle, m in want.items():
        for fh, fw in FLIPS:
            got = warp_matrix(float(angle), 1.0, fh, fw)
            exp = (m[0] * (-1 if fw else 1), m[1] * (-1 if fh else 1), m[2] * (-1 if fw else 1), m[3] * (-1 if fh else 1))
            assert got == tuple(float(e) for e in exp), (angle, fh, fw, got)
            assert not any(math.copysign(1.0, g) < 0 and g == 0 for g in got)            # no negative zeros in the table
            assert np.array_equal(np.array(got).reshape(2, 2), matrix64(angle, 1.0, fh, fw) + 0.0)
    e = warp_entries([2], [3], [4], [0], [1], (8, 8), [90.0], [0.5], [0.0], [0.0], [1.0], [0.0], [0], [0]).numpy()
    _, _, _, f = entry_fields(e[0])
    assert f.tolist() == [0.0, -2.0, 7.5, -2.0, 0.0, 6.5, 1.0, 0.0]                       # zoom 1/2: exact steps of 2 pixels
    for angle, zoom, _, _ in PARAMS:                                                      # and the general convention
        for fh, fw in FLIPS:
            assert np.allclose(np.array(warp_matrix(float(angle), zoom, fh, fw)).reshape(2, 2), matrix64(angle, zoom, fh, fw),
                               rtol=1e-15, atol=1e-16)


# ---- the restatement against grid_sample ---------------------------------------------------------------------------------
def test_restatement_agrees_with_grid_sample():
    """``bilinear64`` / ``nearest64`` at the coordinates the entries give against ``grid_sample(padding_mode="zeros",
    align_corners=True)`` in fp64 with the grid built from the same sx, sy -- every parameter set, geometry and flip pair."""
    import torch.nn.functional as F
    C = 5
    worst, margin, outside = 0.0, 1.0, []
    for gi, geom in enumerate(GEOMETRIES):
        Hs, Ws, h, w = geom
        src = _u(900 + gi, (Hs, Ws, C)).astype(np.float64)
        mask = (_u(950 + gi, (Hs, Ws)) * 4).astype(np.int64)                              # class ids 0 .. 3
        timg = torch.from_numpy(src).permute(2, 0, 1)[None]
        tmsk = torch.from_numpy(mask.astype(np.float64))[None, None]
        for fh, fw in FLIPS:
            entries = case_entries(geom, [0] * len(PARAMS), PARAMS, fh, fw)
            for row in entries:
                _, _, _, f = entry_fields(row)
                sx, sy, _ = coords64(f, h, w)
                margin = min(margin, half_margin(sy, sx))
                outside.append(float(((sx < 0) | (sx > Ws - 1) | (sy < 0) | (sy > Hs - 1)).mean()))
                grid = torch.from_numpy(np.stack([2 * sx / (Ws - 1) - 1, 2 * sy / (Hs - 1) - 1], axis=-1))[None]
                want = F.grid_sample(timg, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0].permute(1, 2, 0).numpy()
                worst = max(worst, float(np.abs(bilinear64(src, sy, sx) - want).max()))
                wantm = F.grid_sample(tmsk, grid, mode="nearest", padding_mode="zeros", align_corners=True)[0, 0].numpy()
                assert np.array_equal(nearest64(mask, sy, sx), wantm), (geom, fh, fw)
    assert worst < 1e-12, worst                      # fp64 against fp64: un-normalising the grid costs a few ulps of the coordinate
    assert margin >= 1e-3, margin                    # no sample sits where nearest-neighbour sampling switches pixels
    assert max(outside) > 0.4 and np.mean(outside) > 0.05         # the zero fill is exercised
