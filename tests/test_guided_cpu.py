"""The guided filter without a GPU (hyperpri_amd/guided.py): the restated contract against a ridge regression per window and against
the published moment form, the bound against an fp32 emulation of the device on every case the GPU tests use (and against the
classical fp32 form, which must break it on an offset guide), the filter's properties, the argument errors, the module's state, the
ABI and the code objects of the new kernels."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import _guided_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.bounded_cases()


# ---- the restated contract against independent forms -----------------------------------------------------------------
@pytest.mark.parametrize("frame", [(1, 1), (3, 5), (11, 13)])
@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("Kg", [1, 2, 3])
def test_the_reference_equals_a_ridge_regression_per_window(Kg, r, frame):
    from hyperpri_amd import guided as G
    h, w = frame
    I, p = K.real_guide(2, Kg, h, w, seed=r), K.real_maps(2, 2, h, w, "linear", seed=Kg)
    ref = G.guided_reference(I, p, r, 1e-2)
    q, a, b = G.guided_bruteforce(I, p, r, 1e-2)
    planes = ref["planes"]
    ar, mI, mp = planes[:, :, :Kg], planes[:, :, Kg:2 * Kg], planes[:, :, 2 * Kg]
    assert np.abs(ar.transpose(0, 3, 4, 1, 2) - a).max() <= 1e-10
    assert np.abs((mp - (ar * mI).sum(axis=2)).transpose(0, 2, 3, 1) - b).max() <= 1e-10         # b = mp - a . mI
    assert np.abs(ref["q"] - q).max() <= 1e-10
    assert ref["q"] is ref["value"] or np.array_equal(ref["q"], ref["value"])
    assert ref["count"][0, 0] == min(r + 1, h) * min(r + 1, w) and ref["count"].max() == min(2 * r + 1, h) * min(2 * r + 1, w)
    # a map without T comes back without T
    one = G.guided_reference(I, p[:, 1], r, 1e-2)
    assert one["q"].shape == (2, h, w) and np.array_equal(one["q"], ref["q"][:, 1])


@pytest.mark.parametrize("Kg,r", [(1, 1), (2, 2), (3, 4), (3, 8)])
def test_the_reference_equals_the_classical_moment_form_in_fp64(Kg, r):
    from hyperpri_amd import guided as G
    I, p = K.real_guide(2, Kg, 19, 23, seed=r), K.real_maps(2, 3, 19, 23, "linear", seed=Kg)
    eps = float(np.float32(1e-2))
    assert np.abs(G.guided_reference(I, p, r, eps)["q"] - K.classical(I, p, r, eps)).max() <= 1e-12


# ---- the bound is not vacuous ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_an_fp32_emulation_of_the_device_stays_inside_the_bound(case):
    """Every window sum in fp32, everything else in fp64 (``guided_reference(dtype=float32)``): inside ``guided_bound`` on every
    real-valued case of the GPU tests, planes and q."""
    from hyperpri_amd import guided as G
    name, Kg, r, T, gs, domain, frame, eps, offset = case
    I, p = K.case_data(case)
    assert I.shape == (frame[0], Kg) + frame[1:] and p.shape == (frame[0], T) + frame[1:]
    ref, emu, bound = G.guided_reference(I, p, r, eps, domain), G.guided_reference(I, p, r, eps, domain, dtype=np.float32), G.guided_bound(I, p, r, eps, domain)
    assert np.isfinite(bound["planes"]).all() and np.isfinite(bound["value"]).all()
    assert (np.abs(emu["planes"].astype(np.float32) - ref["planes"]) <= bound["planes"]).all()
    assert (np.abs(emu["value"] - ref["value"]) <= bound["value"]).all()
    # and it is a bound worth having: a fiftieth of the spread of the values it guards at the most (the offset guides come closest:
    # their fp32 mI planes alone are off by 2^-24 * 1000 = 6e-5 where the guide varies by 1e-2)
    assert bound["value"].max() <= 2e-2 * max(np.ptp(ref["value"]), 1e-3 if frame[1:] == (1, 1) else 0.0)
    if offset:
        # the usual route in fp32 breaks it: E[I I^T] - E[I] E[I]^T cancels
        lin = p if domain == "linear" else 1.0 / (1.0 + np.exp(-p.astype(np.float64)))
        broken = np.abs(K.classical(I, lin, r, np.float32(eps), np.float32) - ref["value"])
        assert broken.max() > 10 * bound["value"].max(), (broken.max(), bound["value"].max())


def test_the_bounded_cases_cover_every_combination_stride_domain_and_frame():
    from hyperpri_amd import guided as G
    assert G.tile_shape() == (K.TILE_H, K.TILE_W) and G.max_radius() == G.MAX_RADIUS == 8 and G.max_guides() == G.MAX_GUIDES == 3
    combos = {(c[1], c[2], c[3]) for c in CASES if not c[8]}
    assert combos == {(k, r, t) for k in K.KS for r in K.RADII for t in K.TS}
    assert {c[4] for c in CASES} == set(K.STRIDES) and {c[5] for c in CASES} == set(K.DOMAINS) and {c[6] for c in CASES} == set(K.FRAMES)
    assert all(c[4] >= c[1] for c in CASES) and any(c[8] for c in CASES)
    th, tw = G.tile_shape()
    assert {(1, 1), (3, 5), (th - 1, tw - 1), (th + 1, tw + 1), (37, 130)} <= {f[1:] for f in K.FRAMES} and any(f[0] == 3 for f in K.FRAMES)


# ---- properties ------------------------------------------------------------------------------------------------------
def test_constants_and_partitions_of_unity_are_preserved():
    from hyperpri_amd import guided as G
    I = K.real_guide(2, 3, 13, 17)
    const = np.full((2, 2, 13, 17), 0.375, dtype=np.float32)
    assert np.abs(G.guided_reference(I, const, 2, 1e-3)["q"] - 0.375).max() <= 1e-15
    # a partition of unity that fp32 holds exactly (multiples of 1/256): by linearity the filtered planes sum to the filtered one
    cuts = np.sort(np.random.RandomState(1).randint(0, 257, size=(2, 4, 13, 17)), axis=1)
    edges = np.concatenate([np.zeros((2, 1, 13, 17), int), cuts, np.full((2, 1, 13, 17), 256)], axis=1)
    soft = (np.diff(edges, axis=1) / 256.0).astype(np.float32)
    assert soft.shape == (2, 5, 13, 17) and np.array_equal(soft.astype(np.float64).sum(axis=1), np.ones((2, 13, 17)))
    q = G.guided_reference(I, soft, 2, 1e-3)["q"]
    assert np.abs(q.sum(axis=1) - 1).max() <= 1e-12 and np.ptp(q) > 0.1


def test_a_map_that_is_linear_in_the_guide_is_reproduced_as_eps_vanishes():
    from hyperpri_amd import guided as G
    I = K.real_guide(1, 3, 13, 17).astype(np.float64)
    p = (0.5 * I[:, 0] - 0.25 * I[:, 1] + 2.0 * I[:, 2] + 0.125).astype(np.float32)[:, None]
    err = [np.abs(G.guided_reference(I, p, 2, eps)["q"] - p).max() for eps in (1e-2, 1e-4, 1e-6)]
    assert err[0] > err[1] > err[2] and err[2] <= 1e-4
    a = G.guided_reference(I, p, 2, 1e-6)["planes"][:, 0, :3]
    assert np.abs(a - np.array([0.5, -0.25, 2.0])[None, :, None, None]).max() <= 1e-3


def test_a_constant_guide_gives_the_twice_clipped_box_mean():
    from hyperpri_amd import guided as G
    p = K.real_maps(2, 2, 13, 17, "linear")
    I = np.full((2, 2, 13, 17), 3.0, dtype=np.float32)
    for r in (1, 3):
        want = K.box_mean(K.box_mean(p.astype(np.float64), r), r)
        ref = G.guided_reference(I, p, r, 0.5)
        assert np.abs(ref["q"] - want).max() <= 1e-13
        assert not ref["planes"][:, :, :2].any()


def test_with_the_guide_as_the_map_a_is_var_over_var_plus_eps():
    from hyperpri_amd import guided as G
    I = K.real_guide(1, 1, 13, 17)
    I64 = I.astype(np.float64)
    for r, eps in ((1, 0.25), (3, 1e-2)):
        var = K.box_mean(I64 * I64, r) - K.box_mean(I64, r) ** 2
        a = G.guided_reference(I, I[:, 0], r, eps)["planes"][:, 0, 0]
        assert np.abs(a - (var / (var + float(np.float32(eps))))[:, 0]).max() <= 1e-12


def test_a_step_edge_of_the_guide_is_kept_and_the_flats_are_smoothed():
    from hyperpri_amd import guided as G
    I, p = K.step_scene()
    q = G.guided_reference(I, p, 3, 1e-3)["q"][0, 0]
    w = I.shape[-1]
    left, right = q[:, :w // 2], q[:, w // 2:]
    assert right.mean() - left.mean() >= 0.9 and q[:, w // 2].mean() - q[:, w // 2 - 1].mean() >= 0.8         # the step survives, one pixel wide
    flats = np.concatenate([left[:, :w // 2 - 4].ravel() - left.mean(), right[:, 4:].ravel() - right.mean()])
    raw = p[0, 0].astype(np.float64)
    raw_flats = np.concatenate([raw[:, :w // 2 - 4].ravel(), raw[:, w // 2 + 4:].ravel() - 1.0])
    assert flats.var() <= 0.5 * raw_flats.var()
    # a box mean of the same radius would have smeared the step over the window
    smeared = K.box_mean(raw, 3)
    assert abs(smeared[:, w // 2].mean() - smeared[:, w // 2 - 1].mean()) <= 0.3


def test_the_scene_of_the_end_to_end_test_has_a_noisy_map_that_the_guide_repairs():
    """On the reference alone: an ACE map of ``blob_scene`` is noisy (best Dice below 0.9), its first principal component carries a
    quarter more variance than the noise, and the filtered map's best Dice is higher."""
    from hyperpri_amd import guided as G
    cubes, masks = K.blob_scene()
    n, H, W, C = cubes.shape
    X, m = cubes.reshape(-1, C).astype(np.float64), masks.reshape(-1) != 0
    lam, V = np.linalg.eigh(np.cov(X.T))
    assert lam[-1] > 1.25 * lam[-2]
    guide = ((X - X.mean(axis=0)) @ V[:, ::-1][:, :3]).reshape(n, H, W, 3).transpose(0, 3, 1, 2).astype(np.float32)
    mub, Sb = X[~m].mean(axis=0), np.cov(X[~m].T)
    Si = np.linalg.inv(Sb + 1e-4 * np.trace(Sb) / C * np.eye(C))
    t, z = X[m].mean(axis=0) - mub, X - mub
    ace = np.clip((z @ Si @ t) / np.sqrt((t @ Si @ t) * np.einsum("pi,ij,pj->p", z, Si, z)), G.P_LO, G.P_HI)
    raw = K.best_dice(ace, masks)
    logit = (np.log(ace) - np.log1p(-ace)).reshape(n, H, W).astype(np.float32)
    refined = K.best_dice(G.guided_reference(guide, logit, 2, 0.1, "prob")["value"], masks)
    assert 0.7 <= raw <= 0.9 and refined >= raw + 0.05, (raw, refined)


# ---- arguments and state ---------------------------------------------------------------------------------------------
def test_argument_errors():
    from hyperpri_amd import GuidedFilter, guided_filter
    from hyperpri_amd import guided as G
    I, p = torch.zeros(2, 3, 4, 5), torch.zeros(2, 2, 4, 5)
    for radius in (0, 9, 1.5, True):
        with pytest.raises(ValueError, match="radius"):
            guided_filter(I, p, radius, 1e-2)
    for eps in (0.0, -1.0, float("nan"), float("inf"), 1e-50):
        with pytest.raises(ValueError, match="eps"):
            guided_filter(I, p, 2, eps)
    with pytest.raises(ValueError, match="domain"):
        guided_filter(I, p, 2, 1e-2, domain="logit")
    with pytest.raises(ValueError, match="float32 guide"):
        guided_filter(I.double(), p, 2, 1e-2)
    with pytest.raises(ValueError, match="float32 maps"):
        guided_filter(I, p.double(), 2, 1e-2)
    with pytest.raises(ValueError, match="K in"):
        guided_filter(torch.zeros(2, 4, 4, 5), p, 2, 1e-2)
    with pytest.raises(ValueError, match="5-d guide"):
        guided_filter(torch.zeros(2, 2, 3, 4, 5), p, 2, 1e-2)
    for bad in (torch.zeros(2, 2, 4, 6), torch.zeros(3, 2, 4, 5), torch.zeros(2, 4, 5, 1, 1), torch.zeros(4, 5)):
        with pytest.raises(ValueError, match="frame"):
            guided_filter(I, bad, 2, 1e-2)
    with pytest.raises(ValueError, match="empty"):
        guided_filter(torch.zeros(2, 3, 0, 5), torch.zeros(2, 0, 5), 2, 1e-2)
    with pytest.raises(ValueError, match="tensor"):
        guided_filter(I.numpy(), p, 2, 1e-2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        guided_filter(I, p, 2, 1e-2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GuidedFilter(2, 1e-2)(I, p)
    with pytest.raises(ValueError, match="radius"):
        GuidedFilter(0, 1e-2)
    with pytest.raises(ValueError, match="radius"):
        G.guided_reference(I.numpy(), p.numpy(), 9, 1e-2)
    with pytest.raises(ValueError, match="eps"):
        G.guided_bound(I.numpy(), p.numpy(), 2, 0.0)
    with pytest.raises(ValueError, match="frame"):
        G.guided_reference(I.numpy(), np.zeros((2, 2, 4, 6)), 2, 1e-2)
    with pytest.raises(ValueError, match="K in"):
        G.guided_reference(np.zeros((2, 4, 4, 5)), p.numpy(), 2, 1e-2)


def test_refine_split_checks_its_arguments_before_any_launch():
    import hyperpri_amd as H
    pred = H.SplitPrediction(torch.zeros(40), torch.zeros(40), [0, 20, 40], [(4, 5), (4, 5)], ["a", "b"], None)
    wide = H.SpectralProjection(np.eye(4, 6), np.zeros(4))
    with pytest.raises(ValueError, match="at most 3"):
        H.refine_split(pred, [], wide, 2, 1e-2)
    guide = lambda image: image[:, :1]                                                   # noqa: E731
    with pytest.raises(ValueError, match="held 0 of the 2"):
        H.refine_split(pred, [], guide, 2, 1e-2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.refine_split(pred, [{"image": torch.zeros(2, 6, 4, 5), "index": ["a", "b"]}], guide, 2, 1e-2)


def test_the_module_carries_its_parameters_in_the_state_dict():
    from hyperpri_amd import GuidedFilter
    src = GuidedFilter(3, 1e-3, "prob")
    sd = src.state_dict()
    assert set(sd) == {"_extra_state"} and sd["_extra_state"] == {"radius": 3, "eps": float(np.float32(1e-3)), "domain": "prob"}
    dst = GuidedFilter(1, 1.0)
    dst.load_state_dict(sd)
    assert (dst.radius, dst.eps, dst.domain) == (3, float(np.float32(1e-3)), "prob") and "radius=3" in repr(dst)
    with pytest.raises(ValueError, match="radius"):
        dst.load_state_dict({"_extra_state": {"radius": 12, "eps": 1.0, "domain": "linear"}})
    assert not list(src.parameters()) and not list(src.buffers())


# ---- the ABI and the code objects ------------------------------------------------------------------------------------
ENTRIES = ("hpri_guided_coeffs", "hpri_guided_apply", "hpri_guided_workspace_bytes", "hpri_guided_max_radius", "hpri_guided_max_guides",
           "hpri_guided_tile_h", "hpri_guided_tile_w")


def test_the_header_declares_and_the_library_exports_the_entry_points():
    from hyperpri_amd import _lib
    decls = _lib.parse_header()
    src = open(os.path.join(ROOT, "include", "hyperpri_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in decls and re.search(r"\b" + name + r"\s*\(", src) and hasattr(lib, name), name
    assert len(decls["hpri_guided_coeffs"][1]) == 14 and len(decls["hpri_guided_apply"][1]) == 13
    assert (lib.hpri_guided_max_radius(), lib.hpri_guided_max_guides(), lib.hpri_guided_tile_h(), lib.hpri_guided_tile_w()) == (8, 3, 16, 32)
    assert lib.hpri_guided_workspace_bytes(2, 5, 37, 130, 3) == 4 * 2 * 5 * 7 * 37 * 130
    for bad in ((0, 1, 4, 4, 1), (1, 0, 4, 4, 1), (1, 1, 0, 4, 1), (1, 1, 4, 0, 1), (1, 1, 4, 4, 0), (1, 1, 4, 4, 4), (1, 1, 1 << 16, 1 << 16, 1)):
        assert lib.hpri_guided_workspace_bytes(*bad) == 0, bad
    assert "guided.hip" in __import__("hyperpri_amd.build", fromlist=["SOURCES"]).SOURCES
    # bad arguments return before any launch
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    big = 1 << 20
    assert lib.hpri_guided_coeffs(null, 1, 1, p, 1, 1, 4, 4, 2, 0.1, 0, p, big, null) == -1
    assert b"guided_coeffs" in lib.hpri_last_error()
    for args in ((p, 1, 1, null, 1, 1, 4, 4, 2, 0.1, 0, p, big, null), (p, 1, 1, p, 1, 1, 4, 4, 2, 0.1, 0, null, big, null),
                 (p, 1, 0, p, 1, 1, 4, 4, 2, 0.1, 0, p, big, null),          # K
                 (p, 4, 4, p, 1, 1, 4, 4, 2, 0.1, 0, p, big, null),
                 (p, 2, 3, p, 1, 1, 4, 4, 2, 0.1, 0, p, big, null),          # gs < K
                 (p, 1, 1, p, 0, 1, 4, 4, 2, 0.1, 0, p, big, null),          # sizes
                 (p, 1, 1, p, 1, 0, 4, 4, 2, 0.1, 0, p, big, null), (p, 1, 1, p, 1, 1, 0, 4, 2, 0.1, 0, p, big, null),
                 (p, 1, 1, p, 1, 1, 4, 0, 2, 0.1, 0, p, big, null),
                 (p, 1, 1, p, 1, 1, 4, 4, 0, 0.1, 0, p, big, null),          # radius
                 (p, 1, 1, p, 1, 1, 4, 4, 9, 0.1, 0, p, big, null),
                 (p, 1, 1, p, 1, 1, 4, 4, 2, 0.0, 0, p, big, null),          # eps
                 (p, 1, 1, p, 1, 1, 4, 4, 2, -1.0, 0, p, big, null), (p, 1, 1, p, 1, 1, 4, 4, 2, float("nan"), 0, p, big, null),
                 (p, 1, 1, p, 1, 1, 4, 4, 2, float("inf"), 0, p, big, null),
                 (p, 1, 1, p, 1, 1, 4, 4, 2, 0.1, 2, p, big, null),          # domain
                 (p, 1, 1, p, 1, 1, 4, 4, 2, 0.1, 0, p, 4 * 3 * 16 - 1, null),           # workspace too small
                 (odd, 1, 1, p, 1, 1, 4, 4, 2, 0.1, 0, p, big, null)):       # misaligned
        assert lib.hpri_guided_coeffs(*args) == -1, args
        assert b"guided_coeffs" in lib.hpri_last_error()
    assert lib.hpri_guided_apply(null, 1, 1, 1, 1, 4, 4, 2, 0, p, big, p, null) == -1
    assert b"guided_apply" in lib.hpri_last_error()
    for args in ((p, 1, 1, 1, 1, 4, 4, 2, 0, null, big, p, null), (p, 1, 1, 1, 1, 4, 4, 2, 0, p, big, null, null),
                 (p, 1, 4, 1, 1, 4, 4, 2, 0, p, big, p, null), (p, 1, 2, 1, 1, 4, 4, 2, 0, p, big, p, null),
                 (p, 1, 1, 1, 1, 4, 4, 9, 0, p, big, p, null), (p, 1, 1, 1, 1, 4, 4, 2, -1, p, big, p, null),
                 (p, 1, 1, 1, 1, 4, 4, 2, 0, p, 8, p, null), (p, 1, 1, 1, 1, 4, 4, 2, 0, p, big, odd, null)):
        assert lib.hpri_guided_apply(*args) == -1, args
        assert b"guided_apply" in lib.hpri_last_error()


def test_the_guided_kernels_hold_everything_in_registers():
    """tools/check_codeobj.py's report: all six instantiations are there, gated, with zero scratch and no spilled vector register."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_codeobj as C
    rep = C.run()
    rows = {k["demangled"].split("(")[0].replace("void ", ""): k for k in rep["kernels"] if k["file"] == "guided.hip"}
    want = [f"guided_{stage}_kernel<{k}>" for stage in ("coeff", "apply") for k in (1, 2, 3)]
    assert sorted(rows) == sorted(want), sorted(rows)
    for name in want:
        k = rows[name]
        assert k["hot"] and k["clean"] and k["scratch"] == 0 and k["vgpr_spill"] == 0, k
        assert k["vgprs"] + k.get("agprs", 0) <= 128 and k["max_flat_wg"] == 512, k     # 512 lanes a workgroup: two fit a CU's registers
