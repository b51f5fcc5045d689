"""The dense CRF without a GPU (hyperpri_amd/crf.py): the restated contract against an explicit pairwise matrix, the bound against an
fp32 emulation of the device on every case the GPU tests use (and against single mutations of the contract, which must break it), the
properties of mean field on the reference, the scene of the end-to-end test, the argument errors, the module's state, the ABI and the
code objects of the new kernels."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import _crf_cases as K
import _guided_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.bounded_cases()
INF = float("inf")


def _frac(err, bound):
    """The largest used fraction of a bound; a zero error under a zero bound (the binary L_0 = 0) uses nothing."""
    err, bound = np.asarray(err), np.asarray(bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bound).max())


def _worst(got, ref, bound):
    """The largest used fraction over Q^1, the last Q and the last L."""
    return max(_frac(np.abs(got["steps"][0] - ref["steps"][0]), bound["steps"][0]), _frac(np.abs(got["Q"] - ref["Q"]), bound["Q"]),
               _frac(np.abs(got["L"] - ref["L"]), bound["L"]))


# ---- the restated contract against the independent oracle ------------------------------------------------------------
@pytest.mark.parametrize("frame", [(1, 1), (3, 5), (11, 13)])
@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("Kg", [0, 1, 3])
def test_the_reference_equals_mean_field_on_an_explicit_pairwise_matrix(Kg, C, r, frame):
    from hyperpri_amd import crf
    h, w = frame
    T, wa, ws = 3, (1.5 if Kg else 0.0), 0.5
    U = (2.0 * np.random.RandomState(10 * Kg + C + r).randn(2, C, h, w)).astype(np.float32)
    I = G.real_guide(2, Kg, h, w, seed=r) if Kg else None
    for mu in (None, K.compat(C)):
        kw = dict(radius=r, iterations=T, theta_alpha=2.0, theta_beta=0.7, theta_gamma=1.5, w_appearance=wa, w_smooth=ws, compat=mu)
        ref, brute = crf.crf_reference(U, I, **kw), crf.crf_bruteforce(U, I, **kw)
        tol = K.fp64_tolerance((2 * r + 1) ** 2, C, T, wa + ws, 1.0, float(np.abs(U).max()))
        assert tol <= 1e-9
        assert len(ref["steps"]) == len(brute["steps"]) == T and ref["L"].shape == (2, C, h, w)
        for key in ("L", "Q", "logit", "prob"):
            assert np.abs(ref[key] - brute[key]).max() <= tol, (key, mu is None)
        for a, b in zip(ref["steps"], brute["steps"]):
            assert np.abs(a - b).max() <= tol
        assert np.array_equal(ref["steps"][-1], ref["Q"])
    # Potts is the matrix -Id, bit for bit in the reference as on the device
    kw["compat"] = None
    explicit = crf.crf_reference(U, I, **{**kw, "compat": -np.eye(C, dtype=np.float32)})
    assert np.array_equal(explicit["L"], crf.crf_reference(U, I, **kw)["L"])
    # binary logits are the two-class problem (0, z)
    if C == 2:
        z = U[:, 1]
        two = crf.crf_reference(np.stack([np.zeros_like(z), z], axis=1), I, **kw)
        one = crf.crf_reference(z, I, **kw)
        assert one["logit"].shape == (2, h, w) and np.array_equal(one["L"], two["L"])
        assert np.array_equal(one["logit"], two["L"][:, 1] - two["L"][:, 0]) and np.array_equal(one["prob"], two["Q"][:, 1])


# ---- the bound is not vacuous ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_an_fp32_emulation_of_the_device_stays_inside_the_bound(case):
    from hyperpri_amd import crf
    unary, guide, kw = K.case_inputs(case)
    ref, bound = K.reference(case[0]), K.bound(case[0])
    emu = crf.crf_reference(unary, guide, dtype=np.float32, **kw)
    for key in ("L", "Q", "logit", "prob"):
        assert np.isfinite(bound[key]).all() and bound[key].shape == ref[key].shape, key
    assert _worst(emu, ref, bound) <= 1.0
    assert _frac(np.abs(emu["logit"] - ref["logit"]), bound["logit"]) <= 1.0 and _frac(np.abs(emu["prob"] - ref["prob"]), bound["prob"]) <= 1.0
    # and it is a bound worth having: a hundredth of a probability at the very most
    assert bound["Q"].max() <= 1e-2 and max(b.max() for b in bound["steps"]) <= 1e-2


MUTATIONS = ("centre included", "division by n", "theta_beta not squared", "one iteration fewer", "mu transposed")


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_a_single_mutation_of_the_contract_breaks_the_bound(mutation):
    """On the bounded cases with small frames (the cheap ones): the mutated reference leaves the bound on at least one of them."""
    from hyperpri_amd import crf
    broken = []
    for case in CASES:
        name, Kg, r, C, gs, T, (N, h, w), binary, potts, kw0 = case
        if h * w > 20 * 40 or h * w == 1:
            continue
        unary, guide, kw = K.case_inputs(case)
        if mutation == "centre included":
            got = crf.crf_reference(unary, guide, _variant="centre", **kw)
        elif mutation == "division by n":
            got = crf.crf_reference(unary, guide, _variant="n", **kw)
        elif mutation == "theta_beta not squared":
            if Kg == 0:
                continue
            got = crf.crf_reference(unary, guide, **{**kw, "theta_beta": float(np.sqrt(kw["theta_beta"]))})      # 1 / (2 theta_beta)
        elif mutation == "one iteration fewer":
            if T == 1:
                continue
            got = crf.crf_reference(unary, guide, **{**kw, "iterations": T - 1})
            got["steps"] = [got["steps"][0]]                                            # (Q^1 is the same; the last Q and L are not)
        else:
            if potts:
                continue
            got = crf.crf_reference(unary, guide, **{**kw, "compat": kw["compat"].T.copy()})
        ref, bound = K.reference(name), K.bound(name)
        worst = max(_frac(np.abs(got["Q"] - ref["Q"]), bound["Q"]), _frac(np.abs(got["L"] - ref["L"]), bound["L"]))
        if worst > 1.0:
            broken.append((name, worst))
    assert broken, mutation
    assert max(v for _, v in broken) > 100.0, broken                                    # not by a hair: by orders of magnitude


def test_the_bounded_cases_cover_every_combination_stride_frame_and_iteration_count():
    from hyperpri_amd import crf
    assert crf.tile_shape() == (K.TILE_H, K.TILE_W) and crf.max_radius() == crf.MAX_RADIUS == 8 and crf.max_guides() == crf.MAX_GUIDES == 3
    assert crf.max_classes() == crf.MAX_CLASSES == 8 and crf.max_iterations() == crf.MAX_ITERATIONS == 16
    assert {(c[1], c[2], c[3]) for c in CASES} == {(k, r, C) for k in K.KS for r in K.RADII for C in K.CS} and len(CASES) == 48
    for k in K.KS[1:]:
        assert {c[4] for c in CASES if c[1] == k} == {g for g in (k, 3, 8) if g >= k}, k          # every stride in {K, 3, 8}
    assert all(c[4] == 0 for c in CASES if c[1] == 0)
    assert {c[6] for c in CASES} == set(K.FRAMES) and {c[5] for c in CASES} == {1, 2, 5}
    th, tw = crf.tile_shape()
    assert set(K.FRAMES) == {(1, 1, 1), (1, 3, 5), (1, th - 1, tw - 1), (1, th + 1, tw + 1), (1, 37, 130), (3, th + 1, tw + 1)}
    assert {c[7] for c in CASES if c[3] == 2} == {True, False} and {c[8] for c in CASES} == {True, False}
    assert any(c[9]["theta_alpha"] == INF for c in CASES) and any(c[9]["theta_gamma"] == INF for c in CASES)
    mu = K.compat(3)
    assert not np.array_equal(mu, mu.T)


# ---- properties on the reference -------------------------------------------------------------------------------------
def test_q_sums_to_one_and_zero_weights_leave_the_logits_alone():
    from hyperpri_amd import crf
    U, I = (2.0 * np.random.RandomState(3).randn(2, 5, 9, 11)).astype(np.float32), G.real_guide(2, 2, 9, 11)
    ref = crf.crf_reference(U, I, 2, 4, 2.0, 0.5, 1.0, 2.0, 1.0, compat=K.compat(5))
    for q in ref["steps"] + [ref["Q"]]:
        assert np.abs(q.sum(axis=1) - 1).max() <= 1e-15 and q.min() > 0
    assert np.abs(ref["L"] - U).max() > 0.1
    for dtype in (np.float64, np.float32):
        zero = crf.crf_reference(U, I, 2, 4, 2.0, 0.5, 1.0, 0.0, 0.0, compat=K.compat(5), dtype=dtype)
        assert np.array_equal(zero["L"], U.astype(np.float64))
        z = crf.crf_reference(U[:, 1], I, 2, 4, 2.0, 0.5, 1.0, 0.0, 0.0, dtype=dtype)
        assert np.array_equal(z["logit"], U[:, 1].astype(np.float64))


def test_under_a_constant_guide_the_appearance_kernel_is_a_smoothness_kernel_of_scale_theta_alpha():
    from hyperpri_amd import crf
    U = (2.0 * np.random.RandomState(4).randn(1, 3, 9, 11)).astype(np.float32)
    I = np.full((1, 2, 9, 11), 3.0, dtype=np.float32)
    a = crf.crf_reference(U, I, 3, 3, 1.5, 0.5, INF, 2.0, 0.0)
    s = crf.crf_reference(U, None, 3, 3, INF, 1.0, 1.5, 0.0, 2.0)
    assert np.array_equal(a["L"], s["L"]) and np.array_equal(a["Q"], s["Q"])


def test_a_step_edge_of_the_guide_keeps_a_label_step_that_smoothness_alone_blurs():
    from hyperpri_amd import crf
    I, p = G.step_scene()
    z = (p[:, 0] - 0.5).astype(np.float32)                                              # weak, noisy binary logits of the step: +-0.5
    w = I.shape[-1]
    edge = crf.crf_reference(z, I, 3, 5, 3.0, 0.1, 1.0, 4.0, 0.0)["prob"][0]            # listens to its own side of the edge only
    blur = crf.crf_reference(z, None, 3, 5, 3.0, 1.0, 3.0, 0.0, 4.0)["prob"][0]         # the same spatial kernel, no appearance
    step_e, step_b = (q[:, w // 2].mean() - q[:, w // 2 - 1].mean() for q in (edge, blur))
    assert step_e >= 0.6 and step_e >= 1.5 * step_b, (step_e, step_b)                   # one pixel wide
    # smoothness alone decides the flats as firmly, and spreads the transition over the window
    assert blur[:, -5:].mean() - blur[:, :5].mean() >= 0.8 and step_b <= 0.45, step_b
    raw = 1.0 / (1.0 + np.exp(-z[0].astype(np.float64)))
    assert edge[:, :w // 2 - 1].var() <= 0.25 * raw[:, :w // 2 - 1].var()              # and the flats are cleaned


def test_the_scene_of_the_end_to_end_test_has_a_noisy_map_that_the_crf_repairs():
    from hyperpri_amd import crf
    ace, logit, guide, masks = K.scene()
    raw = G.best_dice(ace, masks)
    refined = G.best_dice(crf.crf_reference(logit, guide, **K.SCENE)["prob"], masks)
    assert 0.7 <= raw <= 0.9 and refined >= raw + 0.05, (raw, refined)


def test_the_multiclass_case_leaves_fewer_than_one_percent_of_its_pixels_undecided():
    from hyperpri_amd import crf
    unary, guide, kw, lab = K.multiclass_case()
    ref, bound = crf.crf_reference(unary, guide, **kw), crf.crf_bound(unary, guide, **kw)
    top = np.sort(ref["L"], axis=1)
    decided = top[:, -1] - top[:, -2] > 2 * bound["L"].max(axis=1)
    assert decided.mean() > 0.99
    before, after = (unary.argmax(axis=1) == lab).mean(), (ref["L"].argmax(axis=1) == lab).mean()
    assert after >= before + 0.1, (before, after)


# ---- arguments and state ---------------------------------------------------------------------------------------------
ARGS = (2, 3, 2.0, 1.0, 1.0, 1.0, 1.0)


def test_argument_errors():
    from hyperpri_amd import DenseCRF, dense_crf
    from hyperpri_amd import crf
    U, I = torch.zeros(2, 3, 4, 5), torch.zeros(2, 2, 4, 5)
    for radius in (0, 9, 1.5, True):
        with pytest.raises(ValueError, match="radius"):
            dense_crf(U, I, radius, *ARGS[1:])
    for iters in (0, 17, 2.5, False):
        with pytest.raises(ValueError, match="iterations"):
            dense_crf(U, I, 2, iters, *ARGS[2:])
    for pos, name in ((2, "theta_alpha"), (3, "theta_beta"), (4, "theta_gamma")):
        for bad in (0.0, -1.0, float("nan")) + ((INF,) if name == "theta_beta" else ()):
            with pytest.raises(ValueError, match=name):
                dense_crf(U, I, *ARGS[:pos], bad, *ARGS[pos + 1:])
    with pytest.raises(ValueError, match="theta_beta"):
        dense_crf(U, I, 2, 3, 2.0, 1e-30, 1.0, 1.0, 1.0)                                # 1 / (2 theta_beta^2) overflows fp32
    for pos, name in ((5, "w_appearance"), (6, "w_smooth")):
        for bad in (-1.0, float("nan"), INF):
            with pytest.raises(ValueError, match=name):
                dense_crf(U, I, *ARGS[:pos], bad, *ARGS[pos + 1:])
    with pytest.raises(ValueError, match="output"):
        dense_crf(U, I, *ARGS, output="label")
    with pytest.raises(ValueError, match="float32 unary"):
        dense_crf(U.double(), I, *ARGS)
    with pytest.raises(ValueError, match="float32 guide"):
        dense_crf(U, I.double(), *ARGS)
    with pytest.raises(ValueError, match="tensor"):
        dense_crf(U.numpy(), I, *ARGS)
    for bad in (torch.zeros(2, 1, 4, 5), torch.zeros(2, 9, 4, 5), torch.zeros(4, 5), torch.zeros(2, 1, 3, 4, 5)):
        with pytest.raises(ValueError, match="unaries"):
            dense_crf(bad, I, *ARGS)
    with pytest.raises(ValueError, match="K in"):
        dense_crf(U, torch.zeros(2, 4, 4, 5), *ARGS)
    with pytest.raises(ValueError, match="5-d guide"):
        dense_crf(U, torch.zeros(2, 2, 3, 4, 5), *ARGS)
    for bad in (torch.zeros(2, 2, 4, 6), torch.zeros(3, 2, 4, 5)):
        with pytest.raises(ValueError, match="frame"):
            dense_crf(U, bad, *ARGS)
    with pytest.raises(ValueError, match="without a guide"):
        dense_crf(U, None, *ARGS)
    for bad in (np.zeros((2, 2)), np.zeros((3, 4)), np.full((3, 3), np.nan), np.zeros(3)):
        with pytest.raises(ValueError, match="compat"):
            dense_crf(U, I, *ARGS, compat=bad)
    with pytest.raises(ValueError, match="empty"):
        dense_crf(torch.zeros(2, 3, 0, 5), torch.zeros(2, 2, 0, 5), *ARGS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dense_crf(U, I, *ARGS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dense_crf(U[:, 0], None, 2, 3, 2.0, 1.0, 1.0, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DenseCRF(*ARGS)(U, I)
    with pytest.raises(ValueError, match="radius"):
        DenseCRF(0, *ARGS[1:])
    with pytest.raises(ValueError, match="radius"):
        crf.crf_reference(U.numpy(), I.numpy(), 9, *ARGS[1:])
    with pytest.raises(ValueError, match="w_smooth"):
        crf.crf_bound(U.numpy(), I.numpy(), *ARGS[:6], -1.0)
    with pytest.raises(ValueError, match="frame"):
        crf.crf_reference(U.numpy(), np.zeros((2, 2, 4, 6)), *ARGS)
    with pytest.raises(ValueError, match="without a guide"):
        crf.crf_reference(U.numpy(), None, *ARGS)
    ta, tg, b = crf.crf_tables(3, INF, 0.5, 1.0)
    assert ta.dtype == tg.dtype == np.float32 and np.array_equal(ta, np.ones(4, np.float32)) and b == 2.0
    assert np.array_equal(tg, np.exp(-np.arange(4.0) ** 2 / 2).astype(np.float32))


def test_crf_split_checks_its_arguments_before_any_launch():
    import hyperpri_amd as H
    pred = H.SplitPrediction(torch.zeros(40), torch.zeros(40), [0, 20, 40], [(4, 5), (4, 5)], ["a", "b"], None)
    kw = dict(radius=2, iterations=3, theta_alpha=2.0, theta_beta=1.0, theta_gamma=1.0, w_appearance=1.0, w_smooth=1.0)
    wide = H.SpectralProjection(np.eye(4, 6), np.zeros(4))
    with pytest.raises(ValueError, match="at most 3"):
        H.crf_split(pred, [], wide, **kw)
    guide = lambda image: image[:, :1]                                                   # noqa: E731
    with pytest.raises(ValueError, match="output"):
        H.crf_split(pred, [], guide, output="prob", **kw)
    with pytest.raises(ValueError, match="held 0 of the 2"):
        H.crf_split(pred, [], guide, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.crf_split(pred, [{"image": torch.zeros(2, 6, 4, 5), "index": ["a", "b"]}], guide, **kw)


def test_the_module_carries_its_parameters_in_the_state_dict():
    from hyperpri_amd import DenseCRF
    mu = K.compat(3)
    src = DenseCRF(3, 5, INF, 0.5, 2.0, 4.0, 1.0, compat=mu, output="prob")
    sd = src.state_dict()
    assert set(sd) == {"_extra_state"}
    assert sd["_extra_state"] == {"radius": 3, "iterations": 5, "theta_alpha": INF, "theta_beta": 0.5, "theta_gamma": 2.0, "w_appearance": 4.0,
                                  "w_smooth": 1.0, "compat": mu.tolist(), "output": "prob"}
    dst = DenseCRF(1, 1, 1.0, 1.0, 1.0, 0.0, 0.0)
    assert dst.compat is None and "potts" in repr(dst)
    dst.load_state_dict(sd)
    assert dst.get_extra_state() == src.get_extra_state() and "radius=3" in repr(dst) and "matrix" in repr(dst)
    with pytest.raises(ValueError, match="iterations"):
        dst.load_state_dict({"_extra_state": {**sd["_extra_state"], "iterations": 40}})
    assert not list(src.parameters()) and not list(src.buffers())


# ---- the ABI and the code objects ------------------------------------------------------------------------------------
ENTRIES = ("hpri_dense_crf", "hpri_crf_workspace_bytes", "hpri_crf_max_radius", "hpri_crf_max_classes", "hpri_crf_max_guides",
           "hpri_crf_max_iterations", "hpri_crf_tile_h", "hpri_crf_tile_w")


def test_the_header_declares_and_the_library_exports_the_entry_points():
    from hyperpri_amd import _lib
    decls = _lib.parse_header()
    src = open(os.path.join(ROOT, "include", "hyperpri_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in decls and re.search(r"\b" + name + r"\s*\(", src) and hasattr(lib, name), name
        assert hasattr(_lib.load_f16(), name), name                                      # both libraries compile the source
    assert len(decls["hpri_dense_crf"][1]) == 22
    assert (lib.hpri_crf_max_radius(), lib.hpri_crf_max_classes(), lib.hpri_crf_max_guides(), lib.hpri_crf_max_iterations(), lib.hpri_crf_tile_h(),
            lib.hpri_crf_tile_w()) == (8, 8, 3, 16, 16, 32)
    assert lib.hpri_crf_workspace_bytes(2, 5, 37, 130) == 8 * 2 * 5 * 37 * 130
    for bad in ((0, 2, 4, 4), (1, 1, 4, 4), (1, 9, 4, 4), (1, 2, 0, 4), (1, 2, 4, 0), (1, 2, 1 << 16, 1 << 16)):
        assert lib.hpri_crf_workspace_bytes(*bad) == 0, bad
    assert "crf.hip" in __import__("hyperpri_amd.build", fromlist=["SOURCES"]).SOURCES
    # bad arguments return before any launch
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    one = (ctypes.c_float * 9)(*([1.0] * 9))
    t = ctypes.cast(one, ctypes.c_void_p)

    def table(*v):
        return ctypes.cast((ctypes.c_float * 9)(*(list(v) + [0.0] * (9 - len(v)))), ctypes.c_void_p)
    mu = ctypes.cast((ctypes.c_float * 4)(-1.0, 0.5, float("inf"), -1.0), ctypes.c_void_p)
    big = 1 << 20
    ok = [p, 0, p, 1, 1, 1, 2, 4, 4, 2, 2, t, t, 0.5, 1.0, 1.0, null, 0, p, big, p, null]
    bad_calls = {0: null, 11: null, 12: null, 20: null,                                 # null pointers
                 1: 2, 4: 4, 5: 0, 6: 9, 7: 0, 8: 0, 9: 0, 10: 17, 13: 0.0, 14: -1.0, 15: float("inf"), 16: mu, 17: 2, 19: 8, 18: odd}
    for pos, v in bad_calls.items():
        args = list(ok)
        args[pos] = v
        assert lib.hpri_dense_crf(*args) == -1, (pos, v)
        assert b"dense_crf" in lib.hpri_last_error()
    for args in (ok[:1] + [1] + ok[2:6] + [3] + ok[7:],                                   # binary with C = 3
                 ok[:2] + [null] + ok[3:],                                                # K = 1 without a guide
                 ok[:3] + [0] + ok[4:],                                                   # gs < K
                 ok[:2] + [null, 0, 0] + ok[5:],                                          # K = 0 with w_a != 0
                 ok[:9] + [9] + ok[10:], ok[:10] + [0] + ok[11:],                         # radius, iterations
                 ok[:11] + [table(0.5, 0.25, 0.1)] + ok[12:],                             # a table that does not start at 1
                 ok[:12] + [table(1.0, 0.5, 0.75)] + ok[13:],                             # a table that rises
                 ok[:12] + [table(1.0, float("nan"), 0.0)] + ok[13:]):
        assert lib.hpri_dense_crf(*args) == -1, args
        assert b"dense_crf" in lib.hpri_last_error()


def test_the_crf_kernels_hold_everything_in_registers():
    """tools/check_codeobj.py's report: all 28 instantiations are there, gated, with zero scratch and no spilled register, and two
    workgroups of 512 lanes fit a CU's registers."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_codeobj as C
    rep = C.run()
    rows = {k["demangled"].split("(")[0].replace("void ", ""): k for k in rep["kernels"] if k["file"] == "crf.hip"}
    want = [f"crf_iter_kernel<{k}, {c}>" for k in range(4) for c in range(2, 9)]
    assert sorted(rows) == sorted(want), sorted(rows)
    for name in want:
        k = rows[name]
        assert k["hot"] and k["clean"] and k["scratch"] == 0 and k["vgpr_spill"] == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["vgprs"] + k.get("agprs", 0) <= 128 and k["max_flat_wg"] == 512, k
