"""Spectral unmixing without a GPU (hyperpri_amd/unmix.py): the restated active-set rule against the enumeration of every support,
the conditions the case data must meet so that the GPU tests exercise every branch, the fit's conventions, the ATGP restatement,
the argument errors, the checkpoint round trip, the ABI and the code objects of the new kernels."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import _unmix_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND_CASES = [(37, 2), (37, 5), (37, 8), (238, 2), (238, 5), (238, 8)]     # the (C, M) of the GPU bound test


def _fit(C, M):
    from hyperpri_amd import unmix as Um
    E = K.endmembers(C, M)
    return (E,) + Um.unmix_operands(E)[1:]


# ---- the rule against the enumeration --------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 37])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 6])
def test_the_active_set_rule_equals_the_enumeration_of_every_support(M, C):
    from hyperpri_amd import unmix as Um
    E, Q32, R, G = _fit(C, M)
    x = K.mixed_pixels(E, 400, pure=False)
    for mode in K.MODES:
        a, its, rem, capped = Um.unmix_reference(x, Q32, R, mode)
        want = Um.unmix_bruteforce(x, Q32, R, mode)
        assert np.isfinite(want).all() and not capped.any()
        assert np.abs(a - want).max() <= 1e-10, (mode, np.abs(a - want).max())
    with pytest.raises(ValueError, match="exceeds 6"):
        Um.unmix_bruteforce(np.zeros((1, 8)), np.eye(7, 8), np.eye(7), "fcls")


@pytest.mark.parametrize("C,M", BOUND_CASES)
def test_the_case_data_exercise_every_branch_of_the_rule(C, M):
    """Conditions on the inputs of the GPU tests, checked on the reference: nothing is capped, every support size occurs, and from
    three members on some pixel needs a removal step."""
    from hyperpri_amd import unmix as Um
    E, Q32, R, G = _fit(C, M)
    x = K.mixed_pixels(E, 2000)
    for mode in K.MODES:
        a, its, rem, capped = Um.unmix_reference(x, Q32, R, mode)
        assert capped.sum() == 0 and its.max() <= 3 * M and its.min() >= 1
        if mode in ("ncls", "fcls"):
            sizes = set((a > 0).sum(axis=1).tolist())
            assert set(range(1, M + 1)) <= sizes, (mode, sorted(sizes))
            assert (a >= 0).all()
            if M >= 3:
                assert (rem > 0).any(), mode
        else:
            assert (its == 1).all() and not rem.any()
    # a cap of one sub-solve stops the constrained modes early, on a feasible point
    a, its, rem, capped = Um.unmix_reference(x, Q32, R, "fcls", cap=1)
    assert capped.any() and (its <= 1).all() and np.abs(a.sum(axis=1) - 1).max() <= 1e-12 and (a >= 0).all()
    assert Um.unmix_reference(x, Q32, R, "ncls", cap=1)[3].any()


# ---- properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,M", [(37, 5), (238, 8)])
def test_properties_of_the_solutions(C, M):
    from hyperpri_amd import unmix as Um
    E, Q32, R, G = _fit(C, M)
    x = K.mixed_pixels(E, 500)
    a = Um.unmix_reference(x, Q32, R, "fcls")[0]
    assert np.abs(a.sum(axis=1) - 1).max() <= 1e-12 and (a >= 0).all()
    assert np.abs(Um.unmix_reference(x, Q32, R, "scls")[0].sum(axis=1) - 1).max() <= 1e-10
    assert (Um.unmix_reference(x, Q32, R, "ncls")[0] >= 0).all()
    # ucls is the least-squares solution: of R a = y exactly, and of E a = x up to the rounding of Q to fp32
    u = Um.unmix_reference(x, Q32, R, "ucls")[0]
    y = x.astype(np.float64) @ Q32.astype(np.float64).T
    assert np.abs(u - np.linalg.lstsq(R, y.T, rcond=None)[0].T).max() <= 1e-10
    assert np.abs(u - np.linalg.lstsq(E.astype(np.float64).T, x.astype(np.float64).T, rcond=None)[0].T).max() <= 1e-4
    # a pure pixel: one member carries it
    for mode in ("ncls", "fcls"):
        p = Um.unmix_reference(E, Q32, R, mode)[0]
        assert np.array_equal(np.argmax(p, axis=1), np.arange(M))
        assert np.abs(p - np.eye(M)).max() <= 1e-5, mode


def test_a_pure_pixel_of_exact_endmembers_is_exactly_one_hot():
    from hyperpri_amd import unmix as Um
    E = K.indicator_endmembers(37, 5)
    E32, Q32, R, G = Um.unmix_operands(E)
    assert np.array_equal(R, np.diag(np.diag(R))) and set(np.diag(R).tolist()) <= {1.0, 2.0, 4.0}
    for mode in K.MODES:
        assert np.array_equal(Um.unmix_reference(3.0 * E if mode in ("ucls", "ncls") else E, Q32, R, mode)[0],
                              (3.0 if mode in ("ucls", "ncls") else 1.0) * np.eye(5)), mode


# ---- the fit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,M", [(8, 3), (37, 5), (238, 8)])
def test_qr_conventions(C, M):
    from hyperpri_amd import unmix as Um
    E = K.endmembers(C, M)
    E32, Q32, R, G = Um.unmix_operands(E.astype(np.float64))
    assert E32.dtype == np.float32 and Q32.dtype == np.float32 and R.dtype == np.float64 and G.dtype == np.float64
    assert E32.shape == (M, C) and Q32.shape == (M, C) and R.shape == (M, M)
    assert (np.diag(R) > 0).all() and np.array_equal(R, np.triu(R)) and np.array_equal(G, R.T @ R)
    assert np.array_equal(E32, E)                                      # rounded once: fp32 values come back as they are
    Q64 = np.linalg.solve(R.T, E.astype(np.float64))                   # the rows of Q^T = R^-T E^T
    assert np.abs(Q64 @ Q64.T - np.eye(M)).max() <= 1e-12
    assert (np.abs(Q32.astype(np.float64) - Q64) <= 2.0 ** -24 * np.abs(Q64) + 1e-13).all()      # one rounding, of the fp64 factor
    # the module carries exactly these
    from hyperpri_amd import SpectralUnmixer
    m = SpectralUnmixer(E, foreground=[True] + [False] * (M - 1))
    assert np.array_equal(m.basis.numpy(), Q32) and np.array_equal(m.tri.numpy(), R) and np.array_equal(m.gram.numpy(), G)
    assert m.endmembers.dtype == torch.float32 and m.tri.dtype == torch.float64 and m.foreground.dtype == torch.bool
    assert m.num_members == M and m.in_channels == C and m.capped == 0


def test_argument_errors():
    from hyperpri_amd import SpectralUnmixer
    from hyperpri_amd import unmix as Um
    assert Um.max_members() == Um.MAX_MEMBERS == 8
    with pytest.raises(ValueError, match="exceeds the 8"):
        SpectralUnmixer(K.endmembers(37, 9))
    with pytest.raises(ValueError, match="cannot be independent"):
        SpectralUnmixer(np.eye(4)[:, :3])
    bad = K.endmembers(37, 3).astype(np.float64)
    bad[1, 5] = np.inf
    with pytest.raises(ValueError, match="finite"):
        SpectralUnmixer(bad)
    dep = K.endmembers(37, 4).astype(np.float64)
    dep[2] = 0.25 * dep[0] + 0.75 * dep[1]
    with pytest.raises(ValueError, match="rank-deficient.*column 2"):
        SpectralUnmixer(dep)
    with pytest.raises(ValueError, match="foreground"):
        SpectralUnmixer(K.endmembers(37, 3), foreground=[True])
    E, Q32, R, G = _fit(37, 3)
    with pytest.raises(ValueError, match="bands"):
        Um.unmix_reference(np.zeros((4, 36)), Q32, R, "fcls")
    with pytest.raises(ValueError, match="mode"):
        Um.unmix_reference(np.zeros((4, 37)), Q32, R, "nnls")
    m = SpectralUnmixer(E)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 37, 2, 2))
    with pytest.raises(ValueError, match="mode"):
        m(torch.zeros(1, 37, 2, 2), mode="nnls")


def test_state_dict_round_trip_through_blank():
    from hyperpri_amd import SpectralUnmixer
    src = SpectralUnmixer(K.endmembers(37, 5), foreground=[False, True, False, False, True], positions=np.arange(10).reshape(5, 2))
    sd = src.state_dict()
    assert set(sd) == {"endmembers", "basis", "tri", "gram", "foreground", "meta"}
    dst = SpectralUnmixer.blank(37, 5)
    assert not torch.equal(dst.basis, src.basis)
    dst.load_state_dict(sd)
    for name, v in sd.items():
        assert torch.equal(getattr(dst, name), v) and getattr(dst, name).dtype == v.dtype, name


# ---- ATGP ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,M", [(37, 4), (238, 6), (238, 8)])
def test_atgp_reference_finds_the_planted_pixels(C, M):
    from hyperpri_amd import unmix as Um
    cubes, masks, planted = K.planted_scene(C, M)
    for select in ("all", "foreground"):
        picks, values, gaps = Um.atgp_reference(cubes, M, masks, select)
        assert sorted(map(tuple, picks)) == sorted(map(tuple, planted))
        assert (gaps > 0).all() and (gaps / values).min() > 1e-3        # far above the fp32 bound, about 1e-5 of the value
    # background only: none of the planted pixels is seen
    picks, _, _ = Um.atgp_reference(cubes, M, masks, "background")
    assert not set(map(tuple, picks)) & set(map(tuple, planted))


def test_atgp_ties_go_to_the_lowest_position():
    from hyperpri_amd import unmix as Um
    cubes, masks, planted = K.planted_scene(37, 4)
    picks, _, _ = Um.atgp_reference(cubes, 1)
    (e, p), (n, H, W, C) = picks[0], cubes.shape
    flat = cubes.reshape(n, H * W, C).copy()
    later = (n - 1, H * W - 1)
    assert later != (e, p)
    flat[later] = flat[e, p]
    assert tuple(Um.atgp_reference(flat.reshape(cubes.shape), 1)[0][0]) == (e, p)
    assert (e, p) != (0, 0)
    flat[0, 0] = flat[e, p]
    got, _, gaps = Um.atgp_reference(flat.reshape(cubes.shape), 1)
    assert tuple(got[0]) == (0, 0) and gaps[0] <= 0                     # a tie has no gap


# ---- the ABI and the code objects ------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_entry_points():
    from hyperpri_amd import _lib
    decls = _lib.parse_header()
    src = open(os.path.join(ROOT, "include", "hyperpri_hip.h")).read()
    lib = _lib.load()
    for name in ("hpri_band_unmix", "hpri_band_unmix_max_members", "hpri_band_extreme", "hpri_band_extreme_workspace_bytes"):
        assert name in decls and re.search(r"\b" + name + r"\s*\(", src) and hasattr(lib, name), name
    assert len(decls["hpri_band_unmix"][1]) == 16 and len(decls["hpri_band_extreme"][1]) == 17
    assert lib.hpri_band_unmix_max_members() == 8 and lib.hpri_band_extreme_workspace_bytes() >= 1024 * 16
    assert "unmix.hip" in __import__("hyperpri_amd.build", fromlist=["SOURCES"]).SOURCES
    # bad arguments return before any launch
    null = ctypes.c_void_p(0)
    assert lib.hpri_band_unmix(null, 64, 8, 3, null, null, null, 3, 3, 0, 0, null, null, null, null, null) == -1
    assert b"band_unmix" in lib.hpri_last_error()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for args in ((p, 64, 12, 3, p, p, p, 3, 3, 0, 0, p, null, null, p, null),       # cs % 8
                 (p, 64, 8, 3, p, p, p, 9, 3, 0, 0, p, null, null, p, null),        # M beyond the maximum
                 (p, 64, 8, 2, p, p, p, 3, 3, 0, 0, p, null, null, p, null),        # C < M
                 (p, 64, 8, 3, p, p, p, 3, 4, 0, 0, p, null, null, p, null),        # mode
                 (p, 64, 8, 3, p, p, p, 3, 3, -1, 0, p, null, null, p, null),       # cap
                 (p, 64, 8, 3, p, p, p, 3, 3, 0, 8, p, null, null, p, null),        # a foreground bit beyond M
                 (p, 0, 8, 3, p, p, p, 3, 3, 0, 0, p, null, null, p, null)):        # no pixels
        assert lib.hpri_band_unmix(*args) == -1, args
    assert lib.hpri_band_extreme(null, 0, 1, 4, 4, 8, null, null, 1, 0, null, 0, null, 0, null, null, null) == -1
    assert b"band_extreme" in lib.hpri_last_error()
    assert lib.hpri_band_extreme(p, 0, 1, 4, 4, 8, null, p, 1, 0, null, 9, p, 1 << 20, p, p, null) == -1        # K beyond the maximum
    assert lib.hpri_band_extreme(p, 0, 1, 4, 4, 8, null, p, 1, 0, null, 0, p, 16, p, p, null) == -1             # workspace too small
    assert lib.hpri_band_extreme(p, 0, 1, 4, 4, 8, null, p, 1, 1, null, 0, p, 1 << 20, p, p, null) == -1        # a selection without masks


def test_the_unmixing_kernels_hold_everything_in_registers():
    """tools/check_codeobj.py's report: every instantiation of the two kernels is there, gated, with zero scratch and no spilled
    vector register."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_codeobj as C
    rep = C.run()
    # (a c++filt that does not know _Float16 leaves that instantiation's name mangled: IDF16_E is <_Float16>)
    rows = {k["demangled"].split("(")[0].replace("void ", "").replace("_Z19band_extreme_kernelIDF16_E", "band_extreme_kernel<_Float16>@"): k
            for k in rep["kernels"] if k["file"] == "unmix.hip"}
    rows = {n.split("@")[0]: k for n, k in rows.items()}
    want = [f"band_unmix_kernel<{m}>" for m in range(1, 9)] + ["band_extreme_kernel<float>", "band_extreme_kernel<_Float16>"]
    for name in want:
        assert name in rows, (name, sorted(rows))
        k = rows[name]
        assert k["clean"] and k["scratch"] == 0 and k["vgpr_spill"] == 0, k
        assert k["hot"] or k["demangled"].startswith("_Z"), k            # gated by the tool wherever the name could be demangled
        assert k["vgprs"] + k.get("agprs", 0) <= 256, k                  # two waves a SIMD: two workgroups share a CU
    assert all(n.startswith(("band_unmix", "band_extreme")) for n in rows)
