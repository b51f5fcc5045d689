"""The ridge filter without a GPU (hyperpri_amd/ridge.py): the taps, the restated contract against ``scipy.ndimage.correlate1d`` and a
textbook eigen-decomposition, exactness on polynomials, the exact zeros, the bound against an fp32 emulation of the device on every case
the GPU tests use (and against the plain uncentred fp32 form, which must break it on an offset plane), the measures' properties, the
scene of the end-to-end test, the argument errors, the module's state, the ABI and the code objects of the new kernels."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import _ridge_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.bounded_cases()
U = 2.0 ** -24


# ---- taps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.5, 4.0])
def test_the_taps_are_normalised(sigma):
    from hyperpri_amd import ridge as R
    Rr, g0, g1, g2 = R.ridge_taps(sigma, dtype=np.float64)
    assert Rr == int(np.ceil(3 * sigma)) == len(g0) == len(g1) == len(g2) and g0.dtype == np.float64
    x = np.arange(1, Rr + 1, dtype=np.float64)
    w = np.exp(-x * x / (2 * sigma * sigma))
    assert abs((1.0 - 2.0 * g0.sum()) - 1.0 / (1.0 + 2.0 * w.sum())) <= 1e-12         # g0 with its implied centre tap: the unit-sum Gaussian
    assert abs(2.0 * (x * g1).sum() - 1.0) <= 1e-12                                   # the derivative of x is 1
    assert abs(2.0 * (x * x * g2).sum() - 2.0) <= 1e-12                               # the second derivative of x^2 is 2
    R32 = R.ridge_taps(sigma)
    assert R32[0] == Rr and all(a.dtype == np.float32 and np.array_equal(a, b.astype(np.float32)) for a, b in zip(R32[1:], (g0, g1, g2)))
    assert (g0 > 0).all() and (g1 > 0).all() and g2[-1] > 0


def test_the_radius_is_the_ceiling_of_three_sigma():
    from hyperpri_amd import ridge as R
    for sigma, want in ((0.5, 2), (0.75, 3), (1.0, 3), (1.1, 4), (2.0, 6), (3.9, 12), (4.0, 12)):
        assert R.ridge_taps(sigma)[0] == want
    taps, radii, s2 = R._host_taps([0.5, 4.0])
    assert taps.shape == (2, 3, 12) and list(radii) == [2, 12] and not taps[0, :, 2:].any() and s2.dtype == np.float32 and list(s2) == [0.25, 16.0]


def test_argument_errors():
    from hyperpri_amd import RidgeFilter, ridge_filter
    from hyperpri_amd import ridge as R
    I = torch.zeros(2, 2, 4, 5)
    for sig in ((), (1.0,) * 9, (0.49,), (4.01,), (float("nan"),), (1.0, float("inf"))):
        with pytest.raises(ValueError, match="scales|sigma"):
            ridge_filter(I, sig)
        with pytest.raises(ValueError, match="scales|sigma"):
            R.ridge_reference(I.numpy(), sig)
    for beta in (0.0, -1.0, float("nan"), float("inf"), 1e-50):
        with pytest.raises(ValueError, match="beta"):
            ridge_filter(I, (1.0,), beta=beta)
    for c in (0.0, -1.0, float("nan"), float("inf"), 1e-50):
        with pytest.raises(ValueError, match="c must"):
            ridge_filter(I, (1.0,), c=c)
    for kw, what in ((dict(measure="hessian"), "measure"), (dict(polarity="white"), "polarity"), (dict(domain="logit"), "domain"),
                     (dict(output="prob"), "output")):
        with pytest.raises(ValueError, match=what):
            ridge_filter(I, (1.0,), **kw)
    with pytest.raises(ValueError, match="sigma"):
        R.ridge_taps(0.25)
    with pytest.raises(ValueError, match="float32 maps"):
        ridge_filter(I.double(), (1.0,))
    with pytest.raises(ValueError, match="tensor"):
        ridge_filter(I.numpy(), (1.0,))
    for bad in (torch.zeros(4, 5), torch.zeros(2, 2, 3, 4, 5), torch.zeros(1, 1, 1, 1, 4, 5)):
        with pytest.raises(ValueError, match="need maps|5-d maps"):
            ridge_filter(bad, (1.0,))
    with pytest.raises(ValueError, match="empty"):
        ridge_filter(torch.zeros(2, 0, 5), (1.0,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ridge_filter(I, (1.0,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RidgeFilter((1.0, 2.0))(I)
    with pytest.raises(ValueError, match="scales"):
        RidgeFilter(())
    with pytest.raises(ValueError, match="polarity"):
        R.ridge_bound(I.numpy(), (1.0,), polarity="white")
    with pytest.raises(ValueError, match="need non-empty"):
        R.ridge_reference(np.zeros((4, 5)), (1.0,))


def test_the_split_functions_check_their_arguments_before_any_launch():
    import hyperpri_amd as H
    pred = H.SplitPrediction(torch.zeros(40), torch.zeros(40), [0, 20, 40], [(4, 5), (4, 5)], ["a", "b"], None)
    with pytest.raises(ValueError, match="no batches"):
        H.ridge_split([], lambda im: im, (1.0,))
    with pytest.raises(ValueError, match="not its to take"):
        H.ridge_split([], lambda im: im, (1.0,), return_scale=True)
    with pytest.raises(RuntimeError, match="ROCm|no CPU fallback"):
        H.ridge_split([{"image": torch.zeros(2, 6, 4, 5), "mask": torch.zeros(2, 4, 5), "index": ["a", "b"]}], lambda im: im[:, :1], (1.0,))
    with pytest.raises(ValueError, match="not its to take"):
        H.enhance_split(pred, (1.0,), output="value")
    with pytest.raises(ValueError, match="empty split"):
        H.enhance_split(H.SplitPrediction(torch.zeros(0), torch.zeros(0), [0], [], [], None), (1.0,))
    with pytest.raises(RuntimeError, match="ROCm|no CPU fallback"):
        H.enhance_split(pred, (1.0,))


# ---- the restated contract against independent forms -----------------------------------------------------------------
@pytest.mark.parametrize("frame", [(1, 1), (1, 7), (3, 5), (2, 30), (37, 45)])
def test_the_reference_equals_scipy_and_a_textbook_eigen_decomposition(frame):
    from hyperpri_amd import ridge as R
    I = (np.random.RandomState(sum(frame)).rand(2, 2, *frame) * 200 - 100).astype(np.float32)             # |I| <= 100
    sig = (0.5, 1.0, 2.5, 4.0)
    for measure in K.MEASURES:
        for polarity in K.POLARITIES:
            ref, brute = R.ridge_reference(I, sig, measure, polarity, 0.5, 20.0), R.ridge_bruteforce(I, sig, measure, polarity, 0.5, 20.0)
            bound = R.ridge_bound(I, sig, measure, polarity, 0.5, 20.0)
            assert np.abs(ref["hessian"] - brute["hessian"]).max() <= 1e-10
            keep = ~bound["undecided"]
            assert keep.mean() >= 0.99 or frame == (1, 1)
            assert np.abs(ref["response"] - brute["response"])[keep].max(initial=0.0) <= 1e-9
            assert np.abs(ref["scales"] - brute["scales"])[~bound["gate"]].max(initial=0.0) <= 1e-9
            sure = ~bound["undecided_index"]
            assert np.array_equal(ref["index"][sure], brute["index"][sure])
    one = R.ridge_reference(I[:, 1], sig)                                                                 # a map without T comes back without T
    assert one["response"].shape == (2,) + frame and np.array_equal(one["response"], R.ridge_reference(I, sig)["response"][:, 1])
    five = R.ridge_reference(I[:, None], sig)
    assert five["response"].shape == (2, 1, 2) + frame and np.array_equal(five["index"][:, 0], R.ridge_reference(I, sig)["index"])


@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.5])
def test_derivatives_are_exact_on_a_quadratic(sigma):
    """I = 3x^2 - 2xy + y^2 + 5x - 7y + 1000 (integers that fp32 holds): farther than R from the borders H / sigma^2 = (6, -2, 2) up to
    what the rounding of the taps does, 2^-24 sum |tap| |difference| chained through both passes."""
    from hyperpri_amd import ridge as R
    y, x = np.mgrid[0:40, 0:50].astype(np.float64)
    I = (3 * x * x - 2 * x * y + y * y + 5 * x - 7 * y + 1000).astype(np.float32)[None, None]
    assert np.array_equal(I[0, 0], 3 * x * x - 2 * x * y + y * y + 5 * x - 7 * y + 1000)
    Rr = R.ridge_taps(sigma)[0]
    H = R.ridge_reference(I, (sigma,))["hessian"][0, 0, 0] / float(np.float32(sigma * sigma))
    tol = R._hessian_bound(I.astype(np.float64), None, sigma, unit=U)[0, 0] / float(np.float32(sigma * sigma)) + 1e-9
    inner = (slice(None), slice(Rr, 40 - Rr), slice(Rr, 50 - Rr))
    err = np.abs(H - np.array([6.0, -2.0, 2.0])[:, None, None])
    print("quadratic", sigma, err[inner].max(), tol[inner].max())
    assert (err[inner] <= tol[inner]).all() and err[inner].max() <= 1e-5
    assert err[:, 0, 0].max() > 1.0                                                                    # the reflected border is no quadratic


def _plus_zero(a):
    a = np.asarray(a, dtype=np.float64)
    return not a.any() and not np.signbit(a).any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_exact_zeros_bit_for_bit(dtype):
    from hyperpri_amd import ridge as R
    h, w, sig = 40, 70, (1.0, 2.0, 4.0)
    y, x = np.mgrid[0:h, 0:w]
    for measure in K.MEASURES:
        ref = R.ridge_reference(np.full((2, 2, 17, 33), 1e6, dtype=np.float32), sig, measure, "both", dtype=dtype)
        assert _plus_zero(ref["hessian"]) and _plus_zero(ref["response"]) and not ref["index"].any()   # a constant plane of any magnitude
    H = R.ridge_reference((np.sin(0.7 * y) * 100).astype(np.float32)[None, None], sig, dtype=dtype)["hessian"]
    assert _plus_zero(H[:, :, :, 0]) and _plus_zero(H[:, :, :, 1]) and H[:, :, :, 2].any()             # constant along x
    H = R.ridge_reference((3 * x - 2 * y).astype(np.float32)[None, None], sig, dtype=dtype)["hessian"]
    assert _plus_zero(H[:, :, :, 1])                                                                   # an integer ramp: Hxy everywhere
    for s, sigma in enumerate(sig):
        Rr = int(np.ceil(3 * sigma))
        assert _plus_zero(H[:, :, s, 0, :, Rr:w - Rr]) and _plus_zero(H[:, :, s, 2, Rr:h - Rr, :])
    assert H[:, :, 0, 0, :, 0].any() and H[:, :, 0, 2, 0, :].any()                                     # the reflected borders bend the ramp
    H = R.ridge_reference((3 * x + 0 * y).astype(np.float32)[None, None], sig, dtype=dtype)["hessian"]
    assert _plus_zero(H[:, :, :, 2]) and _plus_zero(H[:, :, :, 1])                                     # b = 0: Hyy everywhere


def test_negation_is_exact():
    from hyperpri_amd import ridge as R
    I = K.real_maps(1, 2, 17, 33, seed=5)
    for dtype in (np.float64, np.float32):
        a, b = R.ridge_reference(I, (0.75, 3.0), dtype=dtype)["hessian"], R.ridge_reference(-I, (0.75, 3.0), dtype=dtype)["hessian"]
        assert np.array_equal(a, -b)


# ---- the bound is not vacuous ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_an_fp32_emulation_of_the_device_stays_inside_the_bound(case):
    """Every operation of the two passes in fp32 (``ridge_reference(dtype=float32)``): inside ``ridge_bound`` on every bounded case of
    the GPU tests -- planes, responses outside the undecided mask, one branch's value inside it, the index -- with at most 1 % of the
    pixels undecided, in the reference alone."""
    from hyperpri_amd import ridge as R
    name, sig, T, stride, domain, measure, polarity, output, frame, c, offset = case
    I, args = K.case_data(case), K.case_args(case)
    assert I.shape == (frame[0], T) + frame[1:]
    ref, emu, bound = R.ridge_reference(I, **args), R.ridge_reference(I, dtype=np.float32, **args), R.ridge_bound(I, **args)
    assert all(np.isfinite(bound[k]).all() for k in ("hessian", "scales", "value", "prob"))
    f = K.fractions(ref, bound, emu["hessian"].astype(np.float32), emu["response"].astype(np.float32), emu["index"])
    print(name, f)
    assert f["hessian"] <= 1.0 and f["value"] <= 1.0 and f["inside_ok"] and f["index_ok"], (name, f)
    assert f["share"] <= 0.01, (name, f)                                                               # the cap on what a GPU test may leave out
    # and it is a bound worth having: a thousandth of the largest response at the most
    if frame[1:] != (1, 1):
        assert bound["value"].max() <= 1e-3 * ref["response"].max()
    if offset:
        # the usual route in fp32 breaks it: zero-sum taps applied to 1000 + 0.01 U cancel
        plain = K.plain_fp32(I[0, 0], sig[0])
        over = (np.abs(plain - ref["hessian"][0, 0, 0]) / bound["hessian"][0, 0, 0]).max()
        print(name, "plain fp32 over the bound", over, "error", np.abs(plain - ref["hessian"][0, 0, 0]).max(), "centred",
              np.abs(emu["hessian"] - ref["hessian"]).max())
        assert over > 10.0


def test_the_bounded_cases_cover_every_scale_set_stride_domain_measure_polarity_and_frame():
    from hyperpri_amd import ridge as R
    assert R.tile_shape() == (K.TILE_H, K.TILE_W) and R.max_scales() == R.MAX_SCALES == 8 and R.max_radius() == R.MAX_RADIUS == 12
    assert {(c[1], c[2]) for c in CASES if not c[10]} == {(s, t) for s in K.SCALE_SETS for t in K.TS}
    assert {c[3] for c in CASES} == set(K.STRIDES) and {c[4] for c in CASES} == set(K.DOMAINS) and {c[8] for c in CASES} == set(K.FRAMES)
    assert {(c[5], c[6]) for c in CASES} == {(m, p) for m in K.MEASURES for p in K.POLARITIES} and {c[7] for c in CASES} == set(K.OUTPUTS)
    assert all(c[3] == 1 or c[3] >= c[2] for c in CASES) and sum(c[10] for c in CASES) == 2
    th, tw = R.tile_shape()
    assert {(1, 1), (3, 5), (th - 1, tw - 1), (th + 1, tw + 1), (37, 130)} <= {f[1:] for f in K.FRAMES} and any(f[0] == 3 for f in K.FRAMES)
    assert K.SCALE_SETS[0] == (0.5,) and K.SCALE_SETS[1] == (4.0,) and len(K.SCALE_SETS[-1]) == 8 and K.SCENE_SIGMAS in K.SCALE_SETS


# ---- the measures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", K.MEASURES)
@pytest.mark.parametrize("sigma0", [1.0, 2.0])
def test_a_gaussian_line_selects_its_scale(sigma0, measure):
    """Under Lindeberg's normalisation with gamma = 1 the response at the centre of a Gaussian line of width sigma0 is proportional to
    sigma^2 sigma0 / (sigma0^2 + sigma^2)^(3/2), largest at sigma = sqrt(2) sigma0.  On the octave set (0.6, 1.2, 2.4) the scale nearest
    sigma0 and the scale nearest sqrt(2) sigma0 are the same one, and it wins along the whole centre line; on the scene's set the
    winner is the scale nearest sqrt(2) sigma0."""
    from hyperpri_amd import ridge as R
    line = K.gaussian_line(41, 41, sigma0)[None]
    for sig in ((0.6, 1.2, 2.4), K.SCENE_SIGMAS):
        want = int(np.argmin(np.abs(np.array(sig) - np.sqrt(2.0) * sigma0)))
        if len(sig) == 3:
            assert want == int(np.argmin(np.abs(np.array(sig) - sigma0)))
        for vertical in (True, False):
            img = line if vertical else line.transpose(0, 2, 1).copy()
            ref = R.ridge_reference(img, sig, measure, "bright", 0.5, 0.5)
            centre = ref["index"][0, :, 20] if vertical else ref["index"][0, 20, :]
            assert (centre == want).all(), (sig, centre)
            dark = R.ridge_reference(img, sig, measure, "dark", 0.5, 0.5)["response"][0]
            assert not (dark[:, 20] if vertical else dark[20, :]).any()                                  # no dark line along a bright one


@pytest.mark.parametrize("sigma0", [1.0, 2.0])
def test_frangi_scores_a_blob_below_a_line(sigma0):
    from hyperpri_amd import ridge as R
    beta = 0.5
    line, blob = K.gaussian_line(41, 41, sigma0)[None], K.gaussian_blob(41, 41, sigma0)[None]
    vl = R.ridge_reference(line, K.SCENE_SIGMAS, "frangi", "bright", beta, 0.5)["response"][0, 20, 20]
    vb = R.ridge_reference(blob, K.SCENE_SIGMAS, "frangi", "bright", beta, 0.5)["response"][0, 20, 20]
    assert 0 < vb <= np.exp(-1.0 / (2 * beta * beta)) * vl, (vb, vl)
    sl = R.ridge_reference(line, K.SCENE_SIGMAS, "sato", "bright")["response"][0, 20, 20]
    sb = R.ridge_reference(blob, K.SCENE_SIGMAS, "sato", "bright")["response"][0, 20, 20]
    assert sb > 0.5 * sl                                                                               # sato has no blob term


def test_polarities():
    from hyperpri_amd import ridge as R
    I = K.real_maps(2, 2, 23, 31, seed=9)
    for measure in K.MEASURES:
        for dtype in (np.float64, np.float32):
            b = R.ridge_reference(I, K.SCENE_SIGMAS, measure, "bright", dtype=dtype)
            d = R.ridge_reference(-I, K.SCENE_SIGMAS, measure, "dark", dtype=dtype)
            assert b["response"].tobytes() == d["response"].tobytes() and b["index"].tobytes() == d["index"].tobytes()   # bit for bit
            assert b["scales"].tobytes() == d["scales"].tobytes() and b["logit"].tobytes() == d["logit"].tobytes()
        bright, dark, both = (R.ridge_reference(I, K.SCENE_SIGMAS, measure, p) for p in K.POLARITIES)
        ok = both["mu"] != 0
        assert ok.all() and np.array_equal(both["scales"][ok], np.maximum(bright["scales"], dark["scales"])[ok])
        assert (np.minimum(bright["scales"], dark["scales"]) == 0).all() or measure == "sato"


@pytest.mark.parametrize("measure", K.MEASURES)
def test_the_response_of_the_transposed_plane_is_the_transposed_response(measure):
    from hyperpri_amd import ridge as R
    I = K.real_maps(1, 2, 19, 37, seed=4)
    It = np.ascontiguousarray(I.transpose(0, 1, 3, 2))
    ref, bound = R.ridge_reference(I, K.SCENE_SIGMAS, measure, "both"), R.ridge_bound(I, K.SCENE_SIGMAS, measure, "both")
    for dtype in (np.float64, np.float32):
        t = R.ridge_reference(It, K.SCENE_SIGMAS, measure, "both", dtype=dtype)
        err = np.abs(t["response"].transpose(0, 1, 3, 2) - ref["response"])
        assert (err <= bound["value"]).all() and (dtype is np.float32 or err.max() <= 1e-12)
        assert (np.abs(t["hessian"][:, :, :, ::-1].transpose(0, 1, 2, 3, 5, 4) - ref["hessian"]) <= bound["hessian"]).all()   # Hxx <-> Hyy
    assert not bound["undecided"].any()


# ---- end to end on the reference -------------------------------------------------------------------------------------
def test_the_scene_of_the_end_to_end_test_has_lines_that_a_threshold_misses_and_the_ridge_measure_finds():
    from hyperpri_amd import ridge as R
    for seed in range(3):
        plane, mask = K.root_scene(seed)
        assert plane.shape == (48, 64) and 0.1 < mask.mean() < 0.25
        raw = K.best_dice((plane - plane.min()) / (plane.max() - plane.min()), mask)
        ridge = K.best_dice(R.ridge_reference(plane[None], K.SCENE_SIGMAS, "frangi", "bright", 0.5, 0.5)["response"], mask)
        print("scene", seed, "raw", raw, "ridge", ridge)
        assert raw < 0.6 and ridge >= raw + 0.1, (seed, raw, ridge)
    # embedded in cubes the first principal component carries the scene: the GPU test filters that component
    cubes, masks, planes = K.scene_cubes()
    X = cubes.reshape(-1, cubes.shape[-1]).astype(np.float64)
    lam, V = np.linalg.eigh(np.cov(X.T))
    pc = ((X - X.mean(axis=0)) @ V[:, -1]).reshape(planes.shape)
    assert lam[-1] > 100 * lam[-2] and abs(np.corrcoef(pc.ravel(), planes.ravel())[0, 1]) > 0.999
    pc = pc * np.sign(np.corrcoef(pc.ravel(), planes.ravel())[0, 1])
    raw = K.best_dice((pc - pc.min()) / (pc.max() - pc.min()), masks)
    ridge = K.best_dice(R.ridge_reference(pc.astype(np.float32), K.SCENE_SIGMAS, "frangi", "bright", 0.5, 0.5)["response"], masks)
    print("cubes: raw", raw, "ridge", ridge)
    assert raw < 0.6 and ridge >= raw + 0.1, (raw, ridge)


# ---- the module's state ----------------------------------------------------------------------------------------------
def test_the_module_carries_its_parameters_in_the_state_dict():
    from hyperpri_amd import RidgeFilter
    src = RidgeFilter((0.75, 1.5), "sato", "dark", 0.25, 1e-3, "prob", "logit")
    sd = src.state_dict()
    want = {"sigmas": [0.75, 1.5], "measure": "sato", "polarity": "dark", "beta": 0.25, "c": float(np.float32(1e-3)), "domain": "prob",
            "output": "logit"}
    assert set(sd) == {"_extra_state"} and sd["_extra_state"] == want
    dst = RidgeFilter((1.0,))
    assert (dst.measure, dst.polarity, dst.beta, dst.c, dst.domain, dst.output) == ("frangi", "bright", 0.5, 0.5, "linear", "value")
    dst.load_state_dict(sd)
    assert dst.get_extra_state() == want and "sigmas=(0.75, 1.5)" in repr(dst) and "'sato'" in repr(dst)
    with pytest.raises(ValueError, match="sigma"):
        dst.load_state_dict({"_extra_state": dict(want, sigmas=[5.0])})
    assert not list(src.parameters()) and not list(src.buffers())


# ---- the ABI and the code objects ------------------------------------------------------------------------------------
ENTRIES = ("hpri_ridge_filter", "hpri_ridge_max_scales", "hpri_ridge_max_radius", "hpri_ridge_tile_h", "hpri_ridge_tile_w")


def test_the_header_declares_and_the_library_exports_the_entry_points():
    from hyperpri_amd import _lib
    from hyperpri_amd import ridge as R
    decls = _lib.parse_header()
    src = open(os.path.join(ROOT, "include", "hyperpri_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in decls and re.search(r"\b" + name + r"\s*\(", src) and hasattr(lib, name), name
    assert len(decls["hpri_ridge_filter"][1]) == 22
    assert (lib.hpri_ridge_max_scales(), lib.hpri_ridge_max_radius(), lib.hpri_ridge_tile_h(), lib.hpri_ridge_tile_w()) == (8, 12, 16, 32)
    assert "ridge.hip" in __import__("hyperpri_amd.build", fromlist=["SOURCES"]).SOURCES
    # bad arguments return before any launch
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    taps, radii, s2 = R._host_taps([1.0, 2.0])
    t, r, s = taps.ctypes.data, radii.ctypes.data, s2.ctypes.data

    def call(**kw):
        a = dict(maps=p, si=20, st=20, sp=1, N=1, T=1, H=4, W=5, taps=t, radii=r, s2=s, S=2, beta=0.5, c=0.5, pol=0, meas=0, dom=0, out_code=0,
                 out=p, scale=null, hess=null)
        a.update(kw)
        rc = lib.hpri_ridge_filter(a["maps"], a["si"], a["st"], a["sp"], a["N"], a["T"], a["H"], a["W"], a["taps"], a["radii"], a["s2"], a["S"],
                                   a["beta"], a["c"], a["pol"], a["meas"], a["dom"], a["out_code"], a["out"], a["scale"], a["hess"], null)
        assert rc == -1 and b"ridge_filter" in lib.hpri_last_error(), kw
    for kw in (dict(maps=null), dict(taps=null), dict(radii=null), dict(s2=null), dict(out=null),
               dict(N=0), dict(T=0), dict(H=0), dict(W=0), dict(N=1 << 10, T=1 << 10, H=1 << 10, W=2),           # N T H W >= 2^31
               dict(S=0), dict(S=9), dict(sp=0), dict(si=-1), dict(st=-1),
               dict(beta=0.0), dict(beta=-1.0), dict(beta=float("nan")), dict(beta=float("inf")),
               dict(c=0.0), dict(c=float("nan")), dict(c=float("inf")),
               dict(pol=3), dict(pol=-1), dict(meas=2), dict(dom=2), dict(out_code=2), dict(maps=odd), dict(out=odd), dict(hess=odd)):
        call(**kw)
    for bad_r in (0, 13):
        rr = radii.copy()
        rr[1] = bad_r
        call(radii=rr.ctypes.data)
    for bad in (float("nan"), float("inf")):
        tt = taps.copy()
        tt[1, 2, 3] = bad
        call(taps=tt.ctypes.data)
        ss = s2.copy()
        ss[0] = bad
        call(s2=ss.ctypes.data)


def test_the_ridge_kernels_hold_everything_in_registers():
    """tools/check_codeobj.py's report: all 24 instantiations (polarity x measure x domain x with or without the Hessian planes) are
    there, gated, with zero scratch and no spilled vector register, about 24 KB of LDS each."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_codeobj as C
    rep = C.run()
    rows = {k["demangled"].split("(")[0].replace("void ", ""): k for k in rep["kernels"] if k["file"] == "ridge.hip"}
    want = [f"ridge_filter_kernel<{p}, {m}, {d}, {h}>" for p in range(3) for m in range(2) for d in range(2) for h in range(2)]
    assert sorted(rows) == sorted(want), sorted(rows)
    for name in want:
        k = rows[name]
        assert k["hot"] and k["clean"] and k["scratch"] == 0 and k["vgpr_spill"] == 0, k
        assert k["vgprs"] + k.get("agprs", 0) <= 128 and k["max_flat_wg"] == 512, k     # 512 lanes a workgroup: two fit a CU's registers
        assert k["lds"] == 4 * (40 * 56 + 3 * 40 * 32), k                               # 24320 bytes: six workgroups fit a CU's LDS
