"""Distances without a GPU (hyperpri_amd/distance.py, csrc/distance.hip): the numpy restatements of the contract against
scipy.ndimage and the MedPy recipe written out with scipy, the thinning and link rules on hand-drawn maps, and the argument checks of
the hpri_edt / hpri_select_* / hpri_thin / hpri_skeleton_links launchers, which return before any launch."""
import ctypes

import numpy as np
import pytest

from hyperpri_amd import distance as D

try:
    from scipy import ndimage
except ImportError:                             # (the scipy comparisons need scipy; the rules on drawn maps do not)
    ndimage = None
needs_scipy = pytest.mark.skipif(ndimage is None, reason="scipy is not installed")


def _maps():
    rng = np.random.RandomState(3)
    out = []
    for h, w in ((1, 1), (1, 9), (9, 1), (9, 13), (31, 47)):
        for density in (0.05, 0.5, 0.95):
            out.append(rng.rand(h, w) < density)
    blob = np.zeros((40, 52), dtype=bool)
    blob[5:22, 7:30] = True
    blob[18:36, 25:33] = True
    blob[0:3, 40:52] = True         # touches two edges of the image
    out.append(blob)
    return out


def _scipy_boundary(a):
    return a & ~ndimage.binary_erosion(a, ndimage.generate_binary_structure(2, 1), border_value=0)


def _scipy_d2(sites):
    """Squared distance to the nearest True pixel of ``sites`` (which has one)."""
    return np.rint(ndimage.distance_transform_edt(~sites) ** 2).astype(np.int64)


@needs_scipy
def test_boundary_reference_is_scipys_erosion_surface():
    for a in _maps():
        assert np.array_equal(D.boundary_reference(a), _scipy_boundary(a))


@needs_scipy
@pytest.mark.parametrize("sites", ["background", "foreground", "boundary"])
def test_edt_reference_matches_scipy(sites):
    for a in _maps():
        s = {"background": ~a, "foreground": a, "boundary": _scipy_boundary(a)}[sites]
        got = D.edt_reference(a, sites)
        assert got.dtype == np.int32 and got.shape == a.shape
        if s.any():
            assert np.array_equal(got, _scipy_d2(s)), (sites, a.shape)
            assert not got[s].any()                                      # a site itself holds 0
        else:
            assert (got == a.shape[0] ** 2 + a.shape[1] ** 2).all()      # no site: FAR everywhere
    stack = np.stack([np.zeros((5, 7), bool), np.ones((5, 7), bool)])
    got = D.edt_reference(stack, "background")
    assert not got[0].any() and (got[1] == 25 + 49).all()                # images never influence each other
    with pytest.raises(ValueError):
        D.edt_reference(stack, "edges")


def _medpy_recipe(a, b, tolerances):
    """hd, hd95, assd as MedPy computes them (surface distances of both directions from the erosion surfaces and
    distance_transform_edt), and surface Dice at a tolerance as the DeepMind surface-distance code defines it for unit pixels."""
    sa, sb = _scipy_boundary(a), _scipy_boundary(b)
    ab = ndimage.distance_transform_edt(~sb)[sa]
    ba = ndimage.distance_transform_edt(~sa)[sb]
    both = np.concatenate([ab, ba])
    out = {"hd": max(ab.max(), ba.max()), "hd95": np.percentile(both, 95), "assd": np.mean([ab.mean(), ba.mean()])}
    out["surface_dice"] = {t: ((ab <= t).sum() + (ba <= t).sum()) / len(both) for t in tolerances}
    return out


@needs_scipy
def test_surface_metrics_match_the_medpy_recipe():
    rng = np.random.RandomState(11)
    tol = (1.0, 2.0, 3.5)
    pairs = []
    for a in _maps():
        if a.any():
            b = np.roll(a, (1, -2), axis=(0, 1)) ^ (rng.rand(*a.shape) < 0.03)
            if b.any():
                pairs.append((a, b))
    assert len(pairs) >= 10
    for a, b in pairs:
        ref = D.surface_hist_reference(a, b)
        assert ref["hist"].shape[:2] == (1, 2) and ref["hist"].sum(axis=2).tolist() == ref["counts"].tolist()
        got = D.surface_metrics_from_hist(ref["hist"], tol)
        want = _medpy_recipe(a, b, tol)
        assert got["images_undefined"] == 0
        for key in ("hd", "hd95", "assd"):
            assert got[key][0] == pytest.approx(want[key], rel=1e-9, abs=0), key
        for t in tol:
            assert got["surface_dice"][t][0] == pytest.approx(want["surface_dice"][t], rel=1e-9, abs=0), t


def test_surface_metrics_of_an_empty_map_are_undefined():
    a = np.zeros((3, 8, 9), dtype=bool)
    a[0, 2:5, 2:6] = True
    a[2, 1:4, 3:8] = True
    b = np.zeros_like(a)
    b[0, 3:6, 2:6] = True
    b[1, 1:3, 1:3] = True           # image 1: no prediction; image 2: no truth
    ref = D.surface_hist_reference(a, b)
    assert ref["counts"][1].tolist() == [0, 4] and ref["counts"][2, 1] == 0 and not ref["hist"][1:].any()
    assert ref["max_d2"][2, 0] == 64 + 81                                # the prediction's boundary is FAR from a truth that has none
    got = D.surface_metrics_from_hist(ref["hist"])
    assert got["images_undefined"] == 2
    for key in ("hd", "hd95", "assd"):
        assert np.isfinite(got[key][0]) and np.isnan(got[key][1:]).all()
    assert np.isnan(got["surface_dice"][1.0][1:]).all() and got["surface_dice"][2.0][0] == 1.0


def _draw(h, w, *boxes):
    a = np.zeros((h, w), dtype=bool)
    for y0, y1, x0, x1 in boxes:
        a[y0:y1, x0:x1] = True
    return a


def test_thin_reference_properties():
    rng = np.random.RandomState(5)
    for a in _maps() + [rng.rand(3, 20, 33) < 0.7]:
        t = D.thin_reference(a)
        assert t.dtype == np.uint8 and t.shape == a.shape
        assert not (t.astype(bool) & ~a).any()                           # a subset of the input
        assert np.array_equal(D.thin_reference(t), t)                    # idempotent
    line = _draw(9, 20, (4, 5, 2, 18))
    ell = _draw(12, 12, (2, 10, 3, 4), (9, 10, 3, 10))
    plus = _draw(11, 11, (5, 6, 1, 10), (1, 10, 5, 6))
    for a in (line, line.T, ell, plus):
        assert np.array_equal(D.thin_reference(a), a.astype(np.uint8))   # one pixel wide: unchanged
    assert not D.thin_reference(_draw(6, 6, (2, 4, 2, 4))).any()         # a solid 2x2 block vanishes
    bar, pairs = D.thin_reference(_draw(11, 50, (3, 8, 5, 45)), return_pairs=True)
    ys, xs = np.nonzero(bar)
    assert len(set(ys.tolist())) == 1 and ys[0] == 5 and np.array_equal(xs, np.arange(xs[0], xs[-1] + 1)) and len(xs) >= 30
    assert pairs == 2


def test_links_reference_on_drawn_lines():
    n = 9
    line = _draw(5, 14, (2, 3, 2, 2 + n))
    assert D.links_reference(line).tolist() == [n, n - 1, 0]
    assert D.links_reference(line.T).tolist() == [n, n - 1, 0]
    diag = np.eye(n, dtype=bool)
    assert D.links_reference(diag).tolist() == [n, 0, n - 1]
    assert D.links_reference(diag[::-1]).tolist() == [n, 0, n - 1]
    stairs = np.zeros((n + 1, n + 1), dtype=bool)
    for k in range(n):
        stairs[k, k] = stairs[k, k + 1] = True                           # right, down, right, down, ...
    assert D.links_reference(stairs).tolist() == [2 * n, 2 * n - 1, 0]   # only straight links: no corner is counted twice
    stack = np.stack([diag, np.zeros_like(diag), np.ones_like(diag)])
    assert D.links_reference(stack).tolist() == [[n, 0, n - 1], [0, 0, 0], [n * n, 2 * n * (n - 1), 0]]


def test_traits_of_a_solid_bar():
    for r in (1, 2, 4):
        a = _draw(30, 80, (10, 10 + 2 * r + 1, 8, 70))
        t = D.traits_reference(a)
        assert t["area"] == [(2 * r + 1) * 62] and t["diameter_median_px"] == [2 * r + 1.0]
        assert t["links_diagonal"] == [0] and t["length_px"] == [t["skeleton_pixels"][0] - 1.0]
    empty = D.traits_reference(np.zeros((4, 4), dtype=bool))
    assert empty["skeleton_pixels"] == [0] and np.isnan(empty["diameter_mean_px"][0]) and np.isnan(empty["diameter_median_px"][0])
    k, c = D.traits_from_counts(7, (4, 3, 0), np.array([0, 3, 0, 0, 1]))["diameter_hist"]
    assert k.tolist() == [1, 4] and c.tolist() == [3, 1]
    assert D.traits_from_counts(7, (4, 3, 0), np.array([0, 2, 0, 0, 2]))["diameter_median_px"] == 2.0     # the mean of 1 and 3


def test_limits_and_tile_constants_are_pure_host_functions():
    from hyperpri_amd import _lib
    import hyperpri_amd as H
    lib = _lib.load()
    assert lib.hpri_edt_max_width() == D.edt_max_width() >= 4096
    assert (lib.hpri_edt_col_threads(), lib.hpri_edt_row_threads()) == (D.COL_THREADS, D.ROW_THREADS)
    assert lib.hpri_select_hist_lds_bins() == D.HIST_LDS_BINS
    assert lib.hpri_edt_far(608, 968) == 608 * 608 + 968 * 968
    assert lib.hpri_edt_far(1, 1) == 2
    assert lib.hpri_edt_far(46340, 1000) == -1 and lib.hpri_edt_far(46000, 4000) == 46000 ** 2 + 4000 ** 2      # FAR >= 2^31
    assert lib.hpri_edt_far(8, lib.hpri_edt_max_width() + 1) == -1 and lib.hpri_edt_far(8, lib.hpri_edt_max_width()) > 0
    assert lib.hpri_edt_far(0, 5) == -1
    assert H.distance_transform is D.distance_transform and H.surface_metrics is not None and H.root_traits is not None


def test_bad_arguments_are_rejected_without_launch():
    from hyperpri_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    p = ctypes.c_void_p(0x1000)                 # never dereferenced: every call below must return before a launch
    q = ctypes.c_void_p(0x2000)

    def rejected(rc, word):
        assert rc == -1 and word.encode() in lib.hpri_last_error(), (rc, lib.hpri_last_error())
    wide = lib.hpri_edt_max_width() + 1
    # hpri_edt(pred, kind, thr, is_logits, sites, N, h, w, d2, stream)
    rejected(lib.hpri_edt(null, 0, 0.5, 1, 0, 1, 2, 2, p, null), "null")
    rejected(lib.hpri_edt(p, 0, 0.5, 1, 0, 1, 2, 2, null, null), "null")
    rejected(lib.hpri_edt(p, 3, 0.5, 1, 0, 1, 2, 2, p, null), "pred_kind")
    rejected(lib.hpri_edt(p, 0, 0.5, 1, 3, 1, 2, 2, p, null), "sites")
    rejected(lib.hpri_edt(p, 0, 0.5, 1, -1, 1, 2, 2, p, null), "sites")
    for N, h, w in ((0, 2, 2), (1, 0, 2), (1, 2, -1)):
        rejected(lib.hpri_edt(p, 0, 0.5, 1, 0, N, h, w, p, null), "sizes")
    rejected(lib.hpri_edt(p, 0, 0.5, 1, 0, 4, 32768, 16384, p, null), "2^31")
    rejected(lib.hpri_edt(p, 0, 0.5, 1, 0, 1, 2, wide, p, null), "row")
    rejected(lib.hpri_edt(p, 0, 0.5, 1, 0, 1, 46340, 1000, p, null), "h*h + w*w")
    # hpri_select_stats(values, selector, sel_kind, N, per_image, stats, stride, stream)
    rejected(lib.hpri_select_stats(null, p, 0, 1, 4, p, 2, null), "null")
    rejected(lib.hpri_select_stats(p, null, 0, 1, 4, p, 2, null), "null")
    rejected(lib.hpri_select_stats(p, p, 0, 1, 4, null, 2, null), "null")
    rejected(lib.hpri_select_stats(p, p, 2, 1, 4, p, 2, null), "sel_kind")
    rejected(lib.hpri_select_stats(p, p, 0, 0, 4, p, 2, null), "sizes")
    rejected(lib.hpri_select_stats(p, p, 0, 65536, 32768, p, 2, null), "sizes")
    rejected(lib.hpri_select_stats(p, p, 0, 1, 4, p, 1, null), "stride")
    # hpri_select_hist(values, selector, sel_kind, N, per_image, bins, hist, hist_stride, stream)
    rejected(lib.hpri_select_hist(p, p, 0, 1, 4, 8, null, 8, null), "null")
    rejected(lib.hpri_select_hist(p, p, -1, 1, 4, 8, p, 8, null), "sel_kind")
    rejected(lib.hpri_select_hist(p, p, 0, 1, 0, 8, p, 8, null), "sizes")
    rejected(lib.hpri_select_hist(p, p, 0, 1, 4, 0, p, 8, null), "bins")
    rejected(lib.hpri_select_hist(p, p, 0, 1, 4, 8, p, 7, null), "bins")
    # hpri_thin(pred, kind, thr, is_logits, N, h, w, decide, pairs, map, other, deleted, stream)
    rejected(lib.hpri_thin(p, 0, 0.5, 1, 1, 2, 2, 1, 1, null, q, p, null), "maps")
    rejected(lib.hpri_thin(p, 0, 0.5, 1, 1, 2, 2, 1, 1, q, q, p, null), "maps")
    rejected(lib.hpri_thin(p, 0, 0.5, 1, 1, 2, 2, 1, 1, p, q, null, null), "pairs")
    rejected(lib.hpri_thin(p, 0, 0.5, 1, 1, 2, 2, 1, -1, p, q, p, null), "pairs")
    rejected(lib.hpri_thin(p, 0, 0.5, 1, 1, 2, 2, 0, 0, p, q, p, null), "nothing")
    rejected(lib.hpri_thin(null, 0, 0.5, 1, 1, 2, 2, 1, 0, p, q, null, null), "null")
    rejected(lib.hpri_thin(p, 5, 0.5, 1, 1, 2, 2, 1, 0, p, q, null, null), "pred_kind")
    rejected(lib.hpri_thin(p, 0, 0.5, 1, 1, 0, 2, 1, 0, p, q, null, null), "sizes")
    # hpri_skeleton_links(skeleton, N, h, w, links, stream)
    rejected(lib.hpri_skeleton_links(null, 1, 2, 2, p, null), "null")
    rejected(lib.hpri_skeleton_links(p, 1, 2, 2, null, null), "null")
    rejected(lib.hpri_skeleton_links(p, 1, 2, 0, p, null), "sizes")
    with pytest.raises(RuntimeError, match="sites"):
        _lib.call("hpri_edt", p, 0, 0.5, 1, 7, 1, 2, 2, p, null)


def test_python_checks_come_before_any_launch():
    import torch
    cpu = torch.zeros(2, 4, 5)
    for fn in (D.distance_transform, D.skeletonize, D.root_traits):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(cpu, 0.5)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(cpu.to(torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.surface_distances(cpu, 0.5, cpu)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.skeleton_links(cpu.to(torch.uint8))
    with pytest.raises(ValueError, match="sites"):
        D.distance_transform(cpu, 0.5, sites="edges")
