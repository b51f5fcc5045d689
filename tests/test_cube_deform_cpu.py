"""Deforming gather of the cube cache (hyperpri_amd/cache.py: CubeDeform, plan_epoch_deformed; csrc/cache_warp.hip, csrc/cache_deform.hip) -- CPU half:
the C-ABI entry points exist and reject bad arguments without a launch, the noise generator is Philox4x32-10 bit for bit (through
the library's host entry), its normals have the moments they should, the planner keeps ``plan_epoch_augmented``'s draws and makes
its own in the documented order whatever the knobs are, the fp64 restatement (tests/_deform_ref.py) agrees with independent forms,
and the cases tests/test_gpu_cube_deform.py uses keep the share of mask pixels it must leave out below 2 %.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _deform_ref as R
from test_cube_warp_cpu import AUG_KW, PLAN_KW, _gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hpri_elastic_field", "hpri_cube_deform", "hpri_mask_deform", "hpri_deform_noise_host")
DEF_KW = dict(elastic=(0.6, 6.0, 16.0), noise=(0.01, 0.05), cutmix=(0.5, 0.2, 0.6))


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_deform_symbols_are_declared_and_exported():
    from hyperpri_amd import _lib
    header = open(os.path.join(ROOT, "include", "hyperpri_hip.h")).read()
    declared = set(re.findall(r"\b(hpri_\w+)\s*\(", header))
    decls = _lib.parse_header()
    lib = _lib.load()
    for n in NEW:
        assert n in declared and n in decls and hasattr(lib, n), n
        assert hasattr(_lib.load_f16(), n)
    assert [len(decls[n][1]) for n in NEW] == [8, 15, 12, 5]
    src = open(os.path.join(ROOT, "hyperpri_amd", "build.py")).read()
    assert '"cache_deform.hip"' in src


def test_deform_launchers_reject_bad_arguments_without_launch():
    from hyperpri_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(4096)                 # never dereferenced: every call below must fail its argument checks
    ok = dict(slots=3, Hs=12, Ws=20, cs=8, C=7, N=2, h=12, w=20)

    def cube(cache=one, dt=0, entries=one, deform=one, field=null, dst=one, **kw):
        a = dict(ok, **kw)
        return lib.hpri_cube_deform(cache, dt, a["slots"], a["Hs"], a["Ws"], a["cs"], a["C"], entries, deform, field, a["N"], a["h"],
                                    a["w"], dst, null)

    def mask(masks=one, entries=one, deform=one, field=null, dst=one, **kw):
        a = dict(ok, **kw)
        return lib.hpri_mask_deform(masks, a["slots"], a["Hs"], a["Ws"], entries, deform, field, a["N"], a["h"], a["w"], dst, null)

    def field(nodes=one, nodes_len=64, deform=one, dst=one, **kw):
        a = dict(ok, **kw)
        return lib.hpri_elastic_field(nodes, nodes_len, deform, a["N"], a["h"], a["w"], dst, null)
    for fn in (cube, mask):
        assert fn(null) == -1 and b"null" in lib.hpri_last_error()
        assert fn(entries=null) == -1 and b"null" in lib.hpri_last_error()
        assert fn(deform=null) == -1 and b"null" in lib.hpri_last_error()
        assert fn(dst=null) == -1
        for bad in (dict(h=0), dict(w=0), dict(h=-3), dict(slots=0), dict(N=0), dict(Hs=0), dict(Ws=-1)):
            assert fn(**bad) == -1 and len(lib.hpri_last_error()) > 0, bad
        assert fn(h=4097) == -1 and b"4096" in lib.hpri_last_error()
        assert fn(w=4097) == -1 and b"4096" in lib.hpri_last_error()
        assert fn(entries=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.hpri_last_error()
        assert fn(deform=ctypes.c_void_p(4104)) == -1 and b"aligned" in lib.hpri_last_error()
        assert fn(field=ctypes.c_void_p(4104)) == -1 and b"aligned" in lib.hpri_last_error()      # a field, where given, is checked
        assert fn(N=2 ** 20, h=4096) == -1 and b"too large" in lib.hpri_last_error()               # N * h >= 2^31
    assert cube(cs=12, C=12) == -1 and b"multiple of 8" in lib.hpri_last_error()
    assert cube(cs=4, C=4) == -1
    assert cube(cs=0) == -1
    assert cube(C=0) == -1 and b"band count" in lib.hpri_last_error()
    assert cube(C=9) == -1 and b"band count" in lib.hpri_last_error()
    assert cube(dt=2) == -1 and cube(dt=-1) == -1
    assert cube(cache=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.hpri_last_error()
    assert cube(dst=ctypes.c_void_p(4104)) == -1
    assert cube(cs=2 ** 21, C=8, w=4096) == -1 and b"too large" in lib.hpri_last_error()          # w * cs/4 >= 2^30
    # the field launcher
    assert field(deform=null) == -1 and b"null" in lib.hpri_last_error()
    assert field(dst=null) == -1 and b"null" in lib.hpri_last_error()
    assert field(nodes=null) == -1 and b"null" in lib.hpri_last_error()                           # (null nodes only with nodes_len 0)
    assert field(nodes_len=-1) == -1 and b"nodes_len" in lib.hpri_last_error()
    for bad in (dict(h=0), dict(w=-1), dict(N=0)):
        assert field(**bad) == -1, bad
    assert field(h=4097) == -1 and b"4096" in lib.hpri_last_error()
    assert field(w=4097) == -1 and b"4096" in lib.hpri_last_error()
    assert field(N=2 ** 20, h=4096) == -1 and b"too large" in lib.hpri_last_error()
    assert field(deform=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.hpri_last_error()
    assert field(dst=ctypes.c_void_p(4104)) == -1 and b"aligned" in lib.hpri_last_error()
    assert lib.hpri_deform_noise_host(0, 0, 0, null, null) == -1
    with pytest.raises(RuntimeError, match="hpri_cube_deform"):
        _lib.call("hpri_cube_deform", null, 0, 3, 12, 20, 8, 7, null, null, null, 2, 12, 20, null, null)


# ---- Philox ------------------------------------------------------------------------------------------------------------------
def _host(k0, k1, e):
    from hyperpri_amd import _lib
    bits, z = (ctypes.c_uint * 4)(), (ctypes.c_float * 4)()
    assert _lib.load().hpri_deform_noise_host(int(k0), int(k1), int(e), bits, z) == 0
    return list(bits), list(z)


def test_philox_known_answers():
    """The Random123 known-answer vectors of philox4x32-10: the first through the library (counter words 2, 3 are 0 in the ABI), all
    three on the test's restatement, and the restatement against the library on 10^4 random (k0, k1, e), e >= 2^32 included."""
    assert [f"{b:08x}" for b in _host(0, 0, 0)[0]] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        got = R.philox(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert " ".join(f"{int(b):08x}" for b in got) == want, (ctr, key)
    rng = np.random.default_rng(5)
    k = rng.integers(0, 2 ** 32, (10000, 2), dtype=np.uint64)
    e = rng.integers(0, 2 ** 63, 10000, dtype=np.uint64) >> rng.integers(0, 63, 10000, dtype=np.uint64)     # every magnitude
    e[:4] = [0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1]
    assert (e >= 2 ** 32).sum() > 3000 and (e < 2 ** 32).sum() > 3000
    ctr = np.stack([e & R.MASK32, e >> np.uint64(32), np.zeros_like(e), np.zeros_like(e)], axis=-1)
    want = R.philox(ctr, k)
    for i in range(len(e)):
        assert _host(k[i, 0], k[i, 1], e[i])[0] == want[i].tolist(), (k[i], e[i])


def test_host_normals_match_fp64_box_muller_and_have_unit_moments():
    n = 2 ** 16                                                          # counters: 2^18 values from one key
    k = (0x1234ABCD, 0x9E3779B9)
    bits = R.bits_at(k[0], k[1], np.arange(n, dtype=np.uint64))
    want = R.normals64(bits)
    got = np.array([_host(k[0], k[1], e)[1] for e in range(0, n, 16)], dtype=np.float64)      # every 16th through the library
    assert np.abs(got - want[::16]).max() <= 2.0 ** -17
    z = want.ravel()
    N = z.size
    assert N == 2 ** 18
    assert abs(z.mean()) <= 5 / 512 and abs(z.var() - 1) <= 0.015 and np.abs(z).max() <= R.ZMAX
    bound = 5 / np.sqrt(N)
    other = R.normals64(R.bits_at(k[0] ^ 1, k[1], np.arange(n, dtype=np.uint64))).ravel()
    assert abs(np.mean(z * other)) <= bound                              # two keys
    assert abs(np.mean(want[:-1].ravel() * want[1:].ravel())) <= bound   # neighbouring counters
    assert abs(np.mean(z[:-1] * z[1:])) <= bound                         # neighbouring channels
    # the extreme words: the largest |z| the transform can give, and no NaN / inf at either end
    for r in (0, 0xFFFFFFFF, 0x1FF, 0xFFFFFE00):
        zz = R.normals64(np.array([r, 0, 0xFFFFFFFF, r], dtype=np.uint32))
        assert np.isfinite(zz).all() and np.abs(zz).max() <= R.ZMAX


# ---- config --------------------------------------------------------------------------------------------------------------
def test_cube_deform_rejects_bad_settings():
    import dataclasses
    import hyperpri_amd as H
    d = H.CubeDeform(**DEF_KW)
    assert d.elastic == (0.6, 6.0, 16.0) and d.noise == (0.01, 0.05) and d.cutmix == (0.5, 0.2, 0.6)
    assert H.CubeDeform() == H.CubeDeform(elastic=(0.0, 0.0, 32.0), noise=(0.0, 0.0), cutmix=(0.0, 0.1, 0.5))
    with pytest.raises(dataclasses.FrozenInstanceError):
        d.noise = (0.0, 1.0)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(elastic=(-0.1, 1.0, 8.0)), dict(elastic=(1.5, 1.0, 8.0)), dict(elastic=(nan, 1.0, 8.0)), dict(elastic=(0.5, -1.0, 8.0)),
                dict(elastic=(0.5, inf, 8.0)), dict(elastic=(0.5, 1.0, 3.9)), dict(elastic=(0.5, 1.0, nan)), dict(elastic=(0.5, 1.0)),
                dict(noise=(-0.1, 0.1)), dict(noise=(0.2, 0.1)), dict(noise=(0.0, inf)), dict(noise=(nan, 0.1)), dict(noise=0.1),
                dict(cutmix=(1.5, 0.1, 0.5)), dict(cutmix=(-0.5, 0.1, 0.5)), dict(cutmix=(0.5, 0.0, 0.5)), dict(cutmix=(0.5, 0.6, 0.5)),
                dict(cutmix=(0.5, 0.1, 1.1)), dict(cutmix=(0.5, nan, 0.5)), dict(cutmix=(nan, 0.1, 0.5))):
        with pytest.raises(ValueError, match="CubeDeform"):
            H.CubeDeform(**bad)
    H.CubeDeform(elastic=(1.0, 0.0, 4.0), cutmix=(1.0, 1.0, 1.0))            # the bounds themselves are allowed
    assert H.elastic_lattice(608, 968, 64.0) == (13, 19) and H.elastic_lattice(5, 7, 4.0) == (5, 5) and H.elastic_lattice(1, 1, 4.0) == (4, 4)
    for case in R.ELASTIC_CASES:
        assert H.elastic_lattice(case[0][2], case[0][3], case[1]) == R.lattice(case[0][2], case[0][3], case[1])


# ---- planner ---------------------------------------------------------------------------------------------------------------
def _plan(n, bs, deform, seed, augment=None, **kw):
    from hyperpri_amd.cache import CubeAugment, plan_epoch_deformed
    g = _gen(seed)
    aug = CubeAugment(**AUG_KW) if augment is None else augment
    return plan_epoch_deformed(n, bs, (608, 968), 238, aug, deform, generator=g, **dict(PLAN_KW, **kw)), g


def test_deformed_plan_keeps_the_augmented_plan():
    from hyperpri_amd.cache import CubeAugment, CubeDeform, plan_epoch_augmented
    for n, bs, drop_last in [(45, 2, False), (7, 3, True), (1, 1, False)]:
        a, _ = _plan(n, bs, CubeDeform(**DEF_KW), 7, drop_last=drop_last)
        b = plan_epoch_augmented(n, bs, (608, 968), 238, CubeAugment(**AUG_KW), generator=_gen(7), drop_last=drop_last, **PLAN_KW)
        assert torch.equal(a.order, b.order) and torch.equal(a.table, b.table) and torch.equal(a.entries, b.entries)
        assert a.batches == b.batches and a.window == b.window and a.warped == b.warped
        assert a.deform.dtype == torch.int32 and tuple(a.deform.shape) == (b.table.shape[0], 16) and len(a.deformed) == len(b.batches)
        assert not a.deform[:, 12:].any()


def test_deformation_draws_follow_the_documented_order():
    from hyperpri_amd.cache import CubeDeform
    from test_cube_warp_cpu import _restated_draws
    n, bs, (h, w) = 45, 2, PLAN_KW["patch"]
    plan, g1 = _plan(n, bs, CubeDeform(**DEF_KW), 11)
    g2 = _gen(11)
    _restated_draws(n, 238, AUG_KW, g2)                                  # plan_epoch's five and the augmentation's ten
    r = [torch.rand(n, dtype=torch.float64, generator=g2).numpy() for _ in range(7)]
    keys = torch.randint(0, 2 ** 32, (n, 2), dtype=torch.int64, generator=g2).numpy()
    ep, es, pitch = DEF_KW["elastic"]
    gy, gx = R.lattice(h, w, pitch)
    nodes = (torch.randn(n, gy, gx, 2, dtype=torch.float64, generator=g2) * es).to(torch.float32).numpy()
    assert torch.equal(torch.rand(4, generator=g1), torch.rand(4, generator=g2))          # the generator moved by exactly these draws
    d = plan.deform.numpy()
    fmin, fmax = DEF_KW["cutmix"][1:]
    some_cut = some_el = 0
    for j in range(n):
        bstart = j - j % bs
        bsize = min(bs, n - bstart)
        cut = r[2][j] < DEF_KW["cutmix"][0] and bsize > 1
        if cut:
            rh = int(min(max(round((fmin + r[3][j] * (fmax - fmin)) * h), 1), h))
            rw = int(min(max(round((fmin + r[4][j] * (fmax - fmin)) * w), 1), w))
            y0 = min(int(np.floor(r[5][j] * (h - rh + 1))), h - rh)
            x0 = min(int(np.floor(r[6][j] * (w - rw + 1))), w - rw)
            assert d[j, :5].tolist() == [(j - bstart - 1) % bsize, y0, y0 + rh, x0, x0 + rw], j
            some_cut += 1
        else:
            assert d[j, :5].tolist() == [-1, 0, 0, 0, 0], j
        if r[0][j] < ep:
            assert d[j, 5:8].tolist() == [j * 2 * gy * gx, gy, gx] and d[j, 8:9].view(np.float32)[0] == np.float32(1 / pitch)
            assert np.array_equal(plan.nodes.numpy()[d[j, 5]:d[j, 5] + 2 * gy * gx], nodes[j].ravel())
            some_el += 1
        else:
            assert d[j, 5] == -1
        assert d[j, 9:10].view(np.float32)[0] == np.float32(DEF_KW["noise"][0] + r[1][j] * (DEF_KW["noise"][1] - DEF_KW["noise"][0]))
        assert (int(np.uint32(d[j, 10])), int(np.uint32(d[j, 11]))) == (int(keys[j, 0]), int(keys[j, 1]))
    assert 0 < some_cut < n and 0 < some_el < n and plan.nodes.numel() == n * gy * gx * 2
    assert (keys >= 2 ** 31).any()                                        # keys use all 32 bits
    # what the issue asks of every plan: rectangles inside the window, partners inside the batch
    on = d[:, 0] >= 0
    assert (d[on, 1] >= 0).all() and (d[on, 2] <= h).all() and (d[on, 1] < d[on, 2]).all()
    assert (d[on, 3] >= 0).all() and (d[on, 4] <= w).all() and (d[on, 3] < d[on, 4]).all()
    for (s, e) in plan.batches:
        assert (d[s:e, 0] < e - s).all() and (d[s:e, 0] != np.arange(e - s)).all()
    assert all(plan.deformed)                                             # (noise lo > 0: every sample is noisy)


def test_deformation_draws_do_not_depend_on_the_knobs():
    from hyperpri_amd.cache import CubeDeform
    n = 44
    full, gfull = _plan(n, 4, CubeDeform(**DEF_KW), 3)
    end_full = torch.rand(4, generator=gfull)
    f = full.deform.numpy()
    neutral = dict(elastic=(0.0, 6.0, 16.0), noise=(0.0, 0.0), cutmix=(0.0, 0.2, 0.6))
    for off in ("elastic", "noise", "cutmix"):
        plan, g = _plan(n, 4, CubeDeform(**dict(DEF_KW, **{off: neutral[off]})), 3)
        d = plan.deform.numpy()
        assert torch.equal(plan.entries, full.entries) and torch.equal(plan.table, full.table)
        if off != "cutmix":
            assert np.array_equal(d[:, :5], f[:, :5])
        if off != "elastic":
            assert np.array_equal(d[:, 5:9], f[:, 5:9]) and torch.equal(plan.nodes, full.nodes)
            assert torch.equal(torch.rand(4, generator=g), end_full)      # the lattice draw has the same size: the same end state
        if off != "noise":
            assert np.array_equal(d[:, 9], f[:, 9])
        assert np.array_equal(d[:, 10:12], f[:, 10:12])                   # the keys never move
    # elastic switched off by its probability or by sigma 0: no lattice draw, no table, and the other streams where they were
    for el in ((0.0, 6.0, 16.0), (0.6, 0.0, 16.0)):
        plan, _ = _plan(n, 4, CubeDeform(**dict(DEF_KW, elastic=el)), 3)
        assert plan.nodes is None and (plan.deform[:, 5] == -1).all() and np.array_equal(plan.deform.numpy()[:, 9:12], f[:, 9:12])
    # another pitch changes the lattice's size and nothing before it
    plan, _ = _plan(n, 4, CubeDeform(**dict(DEF_KW, elastic=(0.6, 6.0, 8.0))), 3)
    assert np.array_equal(plan.deform.numpy()[:, [0, 1, 2, 3, 4, 9, 10, 11]], f[:, [0, 1, 2, 3, 4, 9, 10, 11]])
    assert plan.nodes.numel() != full.nodes.numel()


def test_neutral_deform_flags_no_batch():
    from hyperpri_amd.cache import CubeAugment, CubeDeform
    for dfm in (None, CubeDeform(), CubeDeform(elastic=(0.0, 8.0, 16.0), cutmix=(0.0, 0.3, 0.3)), CubeDeform(elastic=(1.0, 0.0, 16.0))):
        plan, _ = _plan(45, 2, dfm, 5)
        assert len(plan.deformed) == 23 and not any(plan.deformed) and plan.nodes is None
        d = plan.deform.numpy()
        assert (d[:, 0] == -1).all() and (d[:, 5] == -1).all() and not d[:, 1:5].any() and (d[:, 9] == 0).all()
    for dfm in (CubeDeform(elastic=(1.0, 2.0, 16.0)), CubeDeform(noise=(0.1, 0.1)), CubeDeform(cutmix=(1.0, 0.2, 0.4))):
        plan, _ = _plan(44, 2, dfm, 5)
        assert all(plan.deformed), dfm
    one, _ = _plan(5, 1, CubeDeform(cutmix=(1.0, 0.2, 0.4)), 5)          # a batch of one has no CutMix
    assert not any(one.deformed) and (one.deform[:, 0] == -1).all()
    some, _ = _plan(45, 2, CubeDeform(cutmix=(0.2, 0.2, 0.4)), 5, augment=CubeAugment())
    assert any(some.deformed) and not all(some.deformed) and not any(some.warped)        # the flag is per batch


# ---- the restatement against independent forms -----------------------------------------------------------------------------
def test_field_restatement_agrees_with_independent_forms():
    rng = np.random.default_rng(3)
    pitch, h, w = 4.0, 13, 17
    gy, gx = R.lattice(h, w, pitch)
    nodes = rng.standard_normal((gy, gx, 2))
    fld = R.field64(nodes, h, w, np.float32(1 / pitch))
    # at lattice-aligned pixels the B-spline is the (1, 4, 1) / 6 stencil, separably
    k = np.array([1.0, 4.0, 1.0]) / 6
    for y in range(0, h, 4):
        for x in range(0, w, 4):
            i, j = y // 4, x // 4
            want = np.einsum("a,b,abc->c", k, k, nodes[i:i + 3, j:j + 3])
            assert np.abs(fld[y, x] - want).max() < 1e-14, (y, x)
    assert np.abs(R.bspline64(np.linspace(0, 1, 33)).sum(0) - 1).max() < 1e-15              # the basis is a partition of unity
    const = np.broadcast_to(np.array([0.75, -1.5]), (gy, gx, 2))
    assert np.abs(R.field64(const, h, w, np.float32(1 / pitch)) - const[0, 0]).max() < 1e-14  # a constant lattice: a constant field
    assert not R.field64(np.zeros((gy, gx, 2)), h, w, np.float32(1 / pitch)).any()           # a zero lattice: zero
    # a lattice linear in the node index gives a field linear in the pixel (B-splines reproduce linear functions): slope / pitch
    lin = np.stack([np.arange(gx)[None, :] + 0.0 * np.arange(gy)[:, None], np.arange(gy)[:, None] + 0.0 * np.arange(gx)[None, :]], -1)
    fl = R.field64(lin, h, w, np.float32(1 / pitch))
    assert np.abs(fl[..., 0] - (np.arange(w)[None, :] / pitch + 1)).max() < 1e-13
    assert np.abs(fl[..., 1] - (np.arange(h)[:, None] / pitch + 1)).max() < 1e-13
    # descriptors the kernel answers with zeros
    from hyperpri_amd.cache import deform_entries
    flat = nodes.astype(np.float32).ravel()
    rows = deform_entries([-1] * 5, [0] * 5, [0] * 5, [0] * 5, [0] * 5, [0, -1, 2, 0, 0], [gy, gy, gy, 3, gy], [gx, gx, gx, gx, 3],
                          [1 / pitch] * 5, [0.0] * 5, [0] * 5, [0] * 5).numpy()
    f5 = R.fields64(rows, flat, h, w)
    assert f5[0].any() and not f5[1:].any()                               # no lattice, past the table's end, gy < 4, gx < 4
    assert np.abs(f5[0] - R.field64(flat.reshape(gy, gx, 2), h, w, np.float32(1 / pitch))).max() == 0


def test_owner_and_noise_restatement():
    from hyperpri_amd.cache import deform_entries
    h, w = 6, 9
    rows = deform_entries([2, 0, 1, 7, -1], [1, 0, 2, 0, 0], [4, 0, 9, 6, 6], [2, 0, -3, 0, 0], [20, 9, 4, 9, 9], [-1] * 5, [0] * 5, [0] * 5,
                          [0.0] * 5, [0.5, 0.0, -1.0, float("nan"), 2.0], [1, 2, 3, 4, 2 ** 32 - 1], [5, 6, 7, 8, 2 ** 31]).numpy()
    own = R.owners(rows, h, w)
    want0 = np.zeros((h, w), dtype=int)
    want0[1:4, 2:9] = 2                                                   # clamped at the window's right edge
    assert np.array_equal(own[0], want0)
    assert (own[1] == 1).all()                                            # an empty rectangle
    want2 = np.full((h, w), 2)
    want2[2:6, 0:4] = 1                                                   # clamped at the bottom and the left
    assert np.array_equal(own[2], want2)
    assert (own[3] == 3).all() and (own[4] == 4).all()                    # mix_from out of range, -1
    assert [R.sigma_of(r) for r in rows] == [0.5, 0.0, 0.0, 0.0, 2.0]     # negative and NaN: none
    assert (int(np.uint32(rows[4][10])), int(np.uint32(rows[4][11]))) == (2 ** 32 - 1, 2 ** 31)
    z = R.noise64(9, 10, 3, 5, 16)                                        # the counter layout: pixel-major, then quad, word = c % 4
    for (y, x, c) in [(0, 0, 0), (1, 2, 7), (2, 4, 15)]:
        bits = R.bits_at(9, 10, np.array((y * 5 + x) * 4 + c // 4, dtype=np.uint64))
        assert z[y, x, c] == R.normals64(bits)[c % 4]


# ---- the cap on what the GPU mask comparison leaves out ------------------------------------------------------------------------
def test_gpu_cases_leave_out_at_most_two_percent_of_the_mask_pixels():
    """tests/test_gpu_cube_deform.py compares masks outside the pixels whose restated sx or sy lies within 1e-3 of a k + 1/2 (an
    elastic field makes them unavoidable by choice of parameters).  For exactly its cases, both flip settings it uses: the share
    left out is at most 2 % per case (0.4 % is the expectation for uniformly spread fractional parts)."""
    from hyperpri_amd.cache import deform_entries
    worst = 0.0
    for case in R.ELASTIC_CASES:
        (Hs, Ws, h, w), pitch, _, _ = case
        nodes = R.case_nodes(case)
        gy, gx = nodes.shape[1:3]
        deform = deform_entries([-1] * 3, [0] * 3, [0] * 3, [0] * 3, [0] * 3, [i * 2 * gy * gx for i in range(3)], [gy] * 3, [gx] * 3,
                                [1 / pitch] * 3, [0.0] * 3, [0] * 3, [0] * 3).numpy()
        fields = R.fields64(deform, nodes.ravel(), h, w)
        assert np.abs(fields).max() > 0.3                                 # the field does move pixels
        for fh, fw in ((0, 0), (1, 1)):
            entries = R.case_warp_entries(case, fh, fw)
            cubes = [np.zeros((Hs, Ws, 1))] * 3
            masks = [np.zeros((Hs, Ws))] * 3
            _, _, _, sure = R.restate_deform(entries, deform, fields, cubes, masks, 1, 8, h, w)
            share = 1.0 - float(sure.mean())
            print(f"{case[0]} flips {fh}{fw}: {share:.4f} of the mask pixels left out")
            assert share <= 0.02, (case, fh, fw, share)
            worst = max(worst, share)
    print("worst share:", worst)
