"""Distances on the device (hyperpri_amd/distance.py, csrc/distance.hip) against the numpy restatements of the contract
(``edt_reference``, ``surface_hist_reference``, ``thin_reference``, ``links_reference``, ``traits_reference``;
tests/test_distance_cpu.py holds those against scipy).  Squared distances, histograms, skeletons and link counts are integers: every
comparison is EXACT.  The fp64 figures derived from them are compared with ``==`` too: both sides apply the same host formulas to
the same integers.

Wherever logits are thresholded they are built so that every fp32 sigmoid stays at least 1e-5 away from the threshold.
Needs a real MI355X."""
import numpy as np
import pytest
import torch

import _components_patterns as P
from hyperpri_amd import distance as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 3
# (1, 1) ... (9, 13): degenerate rows and columns; 63 / 64 / 65: a wave's width; 257 = COL_THREADS + 1 = ROW_THREADS + 1 columns and
# ROWS_PER_GROUP + 1 rows: one more than a workgroup's share in either pass
SHAPES = [(1, 1), (1, 70), (70, 1), (9, 13), (20, 63), (20, 64), (20, 65), (D.ROWS_PER_GROUP + 1, D.COL_THREADS + 1), (12, D.ROW_THREADS + 1)]
WIDE = (40, 1100)               # a row of more than 1024 pixels: four and a bit pixels per thread of the row pass
SITES = ("background", "foreground", "boundary")


def _roots(h, w, widths):
    """Thick drawn "roots": a horizontal, a vertical and a diagonal bar of the given widths, crossing, touching the image edges."""
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.zeros((h, w), dtype=bool)
    a[(yy >= h // 3) & (yy < h // 3 + widths[0])] = True
    a[(xx >= w // 4) & (xx < w // 4 + widths[1])] = True
    a |= np.abs(2 * (yy * max(w, 2) - xx * max(h, 2))) < widths[2] * max(h, w)
    return a


def _own_patterns(shape):
    h, w = shape
    rng = np.random.RandomState(7 * h + w)
    out = []
    out.append(("mixed", np.stack([np.zeros(shape, bool), np.ones(shape, bool), rng.rand(h, w) < 0.4])))
    hole = np.ones((4, h, w), dtype=bool)       # one background pixel in a corner: the longest outward scans, the largest values
    dot = np.zeros((4, h, w), dtype=bool)       # one foreground pixel in a corner: the same for the other two forms
    for k, (y, x) in enumerate(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1))):
        hole[k, y, x] = False
        dot[k, y, x] = True
    out += [("hole_corners_a", hole[:3]), ("hole_corners_b", np.stack([hole[3], dot[0], dot[3]])), ("dot_corners", dot[1:])]
    tiles = np.zeros(shape, dtype=bool)         # isolated pixels where the shares of two workgroups or two waves meet
    for x in (0, 63, 64, D.COL_THREADS - 1, D.COL_THREADS, w - 1):
        if x < w:
            tiles[::5, x] = True
    out.append(("tile_corners", np.stack([tiles, tiles[::-1], ~tiles])))
    out.append(("roots", np.stack([_roots(h, w, (1, 2, 3)), _roots(h, w, (4, 5, 6))[:, ::-1], _roots(h, w, (7, 8, 9))[::-1]])))
    return out


_patterns_cache, _ref_cache = {}, {}


def _patterns(shape):
    if shape not in _patterns_cache:
        pats = _own_patterns(shape)
        if shape == WIDE:                       # the whole list on the small shapes, a selection on the wide one
            pats += [(n, P.pattern(n, shape)) for n in ("checkerboard", "noise_0.3", "noise_0.8")]
        else:
            pats += P.all_patterns(shape)
        for _, a in pats:
            a.setflags(write=False)
        _patterns_cache[shape] = pats
    return _patterns_cache[shape]


def _ref(kind, name, shape, a, *extra):
    """A restatement's answer for a pattern, computed once per session and never changed."""
    key = (kind, name, shape) + extra
    if key not in _ref_cache:
        fn = {"edt": D.edt_reference, "thin": lambda m: D.thin_reference(m, return_pairs=True), "traits": D.traits_reference}[kind]
        _ref_cache[key] = fn(a, *extra)
    return _ref_cache[key]


def _logits_for(a, seed, thr):
    """Logits whose decision ``sigmoid(x) > thr`` is the boolean map ``a``, every sigmoid at least 1e-5 away from ``thr``."""
    u = torch.from_numpy(np.random.RandomState(seed).rand(*a.shape).astype(np.float32))
    centre = float(np.log(thr / (1 - thr)))
    x = centre + torch.where(torch.from_numpy(np.array(a)), 0.1 + 3 * u, -(0.1 + 3 * u))
    s = torch.sigmoid(x)
    assert not bool(((s - thr).abs() < 1e-5).any()) and np.array_equal((s > thr).numpy(), a)
    return x


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint8)).to(DEV)


@pytest.mark.parametrize("shape", SHAPES + [WIDE])
def test_distance_transform_matches_the_reference(shape):
    import hyperpri_amd as H
    h, w = shape
    far = h * h + w * w
    side = torch.cuda.Stream(device=DEV)
    for k, (name, a) in enumerate(_patterns(shape)):
        dev = _u8(a)
        got = {}
        for sites in SITES:
            d2 = H.distance_transform(dev, sites=sites)
            assert d2.dtype == torch.int32 and d2.is_cuda and tuple(d2.shape) == (N, h, w)
            got[sites] = d2
            assert np.array_equal(d2.cpu().numpy(), _ref("edt", name, shape, a, sites)), (name, sites)
        if name == "mixed":                     # an image without a site is FAR everywhere, beside images that have sites
            assert bool((got["background"][1] == far).all()) and bool((got["foreground"][0] == far).all())
            assert bool((got["boundary"][0] == far).all()) and not bool((got["boundary"][1] == far).any())
        if name == "hole_corners_a" and min(shape) > 1:
            assert int(got["background"][0, h - 1, w - 1]) == (h - 1) ** 2 + (w - 1) ** 2      # the largest attainable value
        sites = SITES[k % 3]
        assert torch.equal(H.distance_transform(dev, sites=sites), got[sites]), name           # a second run: bit-identical
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                                                          # a side stream: bit-identical
            other = H.distance_transform(dev, sites=sites)
        side.synchronize()
        assert torch.equal(other, got[sites]), name
        thr = (0.5, 0.3, 0.77)[k % 3]           # the fp32 / threshold forms and the bool form of the same decision
        x = _logits_for(a, 17 + k, thr).to(DEV)
        for form in (H.distance_transform(x, thr, sites=sites), H.distance_transform(torch.sigmoid(x), thr, is_logits=False, sites=sites),
                     H.distance_transform(torch.from_numpy(np.array(a)).to(DEV), sites=sites),
                     H.distance_transform(x.reshape(N, 1, h, w), thr, sites=sites)):
            assert torch.equal(form, got[sites]), (name, sites)


def test_images_never_influence_each_other():
    import hyperpri_amd as H
    shape = (20, 65)
    a, b = P.pattern("noise_0.8", shape)[2], _own_patterns(shape)[-1][1][0]
    for sites in SITES:
        both = H.distance_transform(_u8(np.stack([a, b])), sites=sites)
        alone_a, alone_b = H.distance_transform(_u8(a), sites=sites), H.distance_transform(_u8(b), sites=sites)
        assert tuple(alone_a.shape) == (1, 20, 65)                                             # a (h, w) map is one image
        assert torch.equal(both[0], alone_a[0]) and torch.equal(both[1], alone_b[0]), sites
    skel = H.skeletonize(_u8(np.stack([a, b])))
    assert torch.equal(skel[0], H.skeletonize(_u8(a))[0]) and torch.equal(skel[1], H.skeletonize(_u8(b))[0])


def _assert_surface(pred, truth, **how):
    import hyperpri_amd as H
    want = D.surface_hist_reference(pred, truth)
    got = H.surface_distances(how.get("pred_dev", _u8(pred)), how.get("threshold"), how.get("truth_dev", _u8(truth)))
    for key in ("hist", "counts", "max_d2"):
        assert got[key].dtype == np.int64 and np.array_equal(got[key], want[key]), key
    m, mw = H.surface_metrics_from_hist(got["hist"], (1.0, 2.0, 3.0)), D.surface_metrics_from_hist(want["hist"], (1.0, 2.0, 3.0))
    assert m["images_undefined"] == mw["images_undefined"]
    for key in ("hd", "hd95", "assd"):
        assert np.array_equal(m[key], mw[key], equal_nan=True), key
    for t in (1.0, 2.0, 3.0):
        assert np.array_equal(m["surface_dice"][t], mw["surface_dice"][t], equal_nan=True), t
    return got, m


@pytest.mark.parametrize("shape", [(9, 13), (20, 65), (12, D.ROW_THREADS + 1), WIDE])
def test_surface_histograms_match_the_reference(shape):
    pats = _patterns(shape)
    bins = []
    for k, (name, a) in enumerate(pats):
        truth = pats[(k + 1) % len(pats)][1]
        got, _ = _assert_surface(a, truth)
        bins.append(got["hist"].shape[2])
    if shape == WIDE:                           # both ways to the histogram were taken: reduced in LDS, straight into global memory
        assert min(bins) <= D.HIST_LDS_BINS < max(bins), bins
    # the fp32 / threshold prediction against a fp32 truth read as int(mask) != 0 (0.5 is background), and a bool truth
    name, a = pats[-1]
    truth = pats[0][1]
    x = _logits_for(a, 3, 0.4).to(DEV)
    mask = torch.from_numpy(np.where(truth, 2.0, 0.5).astype(np.float32)).to(DEV)
    _assert_surface(a, truth, pred_dev=x, threshold=0.4, truth_dev=mask)
    _assert_surface(a, truth, truth_dev=torch.from_numpy(np.array(truth)).to(DEV))


def test_surface_metrics_of_an_empty_map_are_undefined():
    a = np.zeros((3, 30, 41), dtype=bool)
    a[0, 5:15, 6:30] = True
    a[2, 3:9, 3:9] = True
    b = np.zeros_like(a)
    b[0, 8:20, 4:28] = True
    b[1, 10:12, 10:12] = True                   # image 1: an empty prediction; image 2: an empty truth
    got, m = _assert_surface(a, b)
    assert m["images_undefined"] == 2 and got["counts"][1, 0] == 0 and got["counts"][2, 1] == 0 and not got["hist"][1:].any()
    for key in ("hd", "hd95", "assd"):
        assert np.isfinite(m[key][0]) and np.isnan(m[key][1:]).all()
    assert np.isnan(m["surface_dice"][1.0][1:]).all()
    _, m = _assert_surface(np.zeros_like(a), b)                                                # nothing predicted anywhere
    assert m["images_undefined"] == 3 and np.isnan(m["hd"]).all()


def test_surface_known_answers():
    shape = (40, 70)
    for name, a in _patterns(shape)[:6]:
        if not a.any(axis=(1, 2)).all():
            continue
        _, m = _assert_surface(a, a)            # a map against itself
        for key in ("hd", "hd95", "assd"):
            assert (m[key] == 0).all(), (name, key)
        assert (m["surface_dice"][1.0] == 1).all()
    line = np.zeros((3, 40, 70), dtype=bool)
    line[:, 12, 20:50] = True                   # one pixel wide, well inside the image
    shifted = np.roll(line, 3, axis=1)
    _, m = _assert_surface(line, shifted)
    for key in ("hd", "hd95", "assd"):
        assert (m[key] == 3).all(), key
    assert (m["surface_dice"][2.0] == 0).all() and (m["surface_dice"][3.0] == 1).all()


@pytest.mark.parametrize("shape", SHAPES + [WIDE])
def test_skeleton_links_and_traits_match_the_reference(shape):
    import hyperpri_amd as H
    for k, (name, a) in enumerate(_patterns(shape)):
        want, _ = _ref("thin", name, shape, a)
        dev = _u8(a)
        skel = H.skeletonize(dev)
        assert skel.dtype == torch.uint8 and skel.is_cuda
        assert np.array_equal(skel.cpu().numpy(), want), name
        assert np.array_equal(H.skeleton_links(skel), D.links_reference(want)), name
        assert np.array_equal(H.skeleton_links(dev), D.links_reference(a)), name               # any map has links, not only a skeleton
        if k % 3 == 0:
            thr = 0.35
            x = _logits_for(a, 40 + k, thr).to(DEV)
            assert torch.equal(H.skeletonize(x, thr), skel) and torch.equal(H.skeletonize(torch.sigmoid(x), thr, is_logits=False), skel)
            got, ref = H.root_traits(x, thr, truth=dev), _ref("traits", name, shape, a)
            for side in (got, got["truth"]):
                for key in D.TRAIT_NAMES[:-1]:
                    assert np.array_equal(np.asarray(side[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64), equal_nan=True), (name, key)
                for (gk, gc), (rk, rc) in zip(side["diameter_hist"], ref["diameter_hist"]):
                    assert np.array_equal(gk, rk) and np.array_equal(gc, rc), name


def test_thinning_checks_the_counters_more_than_twice():
    """A solid block thick enough to need more than 2 * THIN_CHECK_PAIRS pairs: the host looks at the counters at least three times,
    and the number of pairs the device reports is the reference's."""
    import hyperpri_amd as H
    a = np.zeros((3, 60, 70), dtype=bool)
    a[0, 5:55, 8:62] = True
    a[1, 20:24, 10:60] = True                   # converges long before image 0: the pairs after that are no-ops for it
    want, pairs = D.thin_reference(a, return_pairs=True)
    assert pairs > 2 * D.THIN_CHECK_PAIRS
    skel, got_pairs = H.skeletonize(_u8(a), return_pairs=True)
    assert np.array_equal(skel.cpu().numpy(), want) and got_pairs == pairs
    assert not skel[2].any() and int(skel[1].sum()) > 30
    assert torch.equal(H.skeletonize(skel), skel)                                              # idempotent


def test_bar_diameter_is_its_width():
    import hyperpri_amd as H
    for r in (0, 1, 3, 4):
        a = np.zeros((1, 40, 120), dtype=bool)
        a[0, 15:15 + 2 * r + 1, 10:110] = True
        t = H.root_traits(_u8(a))
        assert t["diameter_median_px"] == [2 * r + 1.0] and t["area"] == [(2 * r + 1) * 100] and t["links_diagonal"] == [0]
        assert t["length_px"] == [t["skeleton_pixels"][0] - 1.0]


def _split(thr):
    """A synthetic stored split of two sizes, the way tests/test_gpu_evaluate.py and test_gpu_components.py build one: no network.
    Prediction and truth are blobs (3 x 3 and 2 x 2 blocks), so both have boundaries, skeletons and small components."""
    import hyperpri_amd as H
    sizes = [(37, 70)] * 3 + [(20, 33)] * 2
    names = [f"img{i}" for i in range(len(sizes))]
    offsets = [0]
    for h, w in sizes:
        offsets.append(offsets[-1] + h * w)
    logits = torch.empty(offsets[-1])
    masks = torch.empty(offsets[-1])
    for i, (h, w) in enumerate(sizes):
        m = np.kron(np.random.RandomState(60 + i).rand((h + 2) // 3, (w + 2) // 3) < 0.3, np.ones((3, 3)))[:h, :w]
        s = np.kron(np.random.RandomState(80 + i).rand((h + 1) // 2, (w + 1) // 2) < 0.3, np.ones((2, 2)))[:h, :w] > 0
        masks[offsets[i]:offsets[i + 1]] = torch.from_numpy(m.astype(np.float32).reshape(-1))
        logits[offsets[i]:offsets[i + 1]] = _logits_for(s, 70 + i, thr).reshape(-1)
    return H.SplitPrediction(logits.to(DEV), masks.to(DEV), offsets, sizes, names)


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and a and isinstance(a[0], (list, tuple, np.ndarray)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


@pytest.mark.parametrize("min_area", [0, 6])
def test_evaluate_entry_points_equal_the_per_image_calls(min_area):
    import hyperpri_amd as H
    from hyperpri_amd import evaluate as E
    thr, tol = 0.6, (1.0, 2.0)
    pred = _split(thr)
    src, t = (H.clean_prediction(pred, thr, min_area)[0], 0.5) if min_area else (pred, thr)
    if min_area:
        assert not torch.equal(src.logits > 0, torch.sigmoid(pred.logits) > thr)               # the cleaning removed something
    per = {"hd": [], "hd95": [], "assd": [], "surface_dice": {x: [] for x in tol}}
    traits = {name: [] for name in D.TRAIT_NAMES}
    truth = {name: [] for name in D.TRAIT_NAMES}
    for i in range(len(src)):
        x, m = src.image(i)
        one = H.surface_metrics_from_hist(H.surface_distances(x, t, m)["hist"], tol)
        for key in ("hd", "hd95", "assd"):
            per[key].append(float(one[key][0]))
        for x_ in tol:
            per["surface_dice"][x_].append(float(one["surface_dice"][x_][0]))
        tr = H.root_traits(x, t, truth=m)
        for name in D.TRAIT_NAMES:
            traits[name] += tr[name]
            truth[name] += tr["truth"][name]
    got = H.surface_metrics(pred, thr, tolerances=tol, min_area=min_area)
    assert _same(got["per_image"], per) and got["images_undefined"] == 0 and got["names"] == pred.names
    for key in ("hd", "hd95", "assd"):
        assert got[key] == float(np.mean(per[key])) and got[key] > 0
    assert all(got["surface_dice"][x_] == float(np.mean(per["surface_dice"][x_])) for x_ in tol)
    rt = E.root_traits(pred, thr, min_area=min_area)
    assert H.split_root_traits is E.root_traits and rt["names"] == pred.names
    assert _same({k: rt[k] for k in D.TRAIT_NAMES}, traits) and _same(rt["truth"], truth)
    assert sum(rt["skeleton_pixels"]) > 0 and sum(rt["truth"]["links_straight"]) > 0
    # an image nobody predicted anything in: undefined, and left out of the means
    blank = H.SplitPrediction(pred.logits.clone(), pred.masks, pred.offsets, pred.sizes, pred.names)
    blank.logits[pred.offsets[1]:pred.offsets[2]] = -9.0
    got2 = H.surface_metrics(blank, thr, tolerances=tol, min_area=min_area)
    assert got2["images_undefined"] == 1 and np.isnan(got2["per_image"]["hd"][1])
    assert got2["hd"] == float(np.mean(per["hd"][:1] + per["hd"][2:]))


def test_bad_arguments_raise_before_any_launch():
    import hyperpri_amd as H
    good = torch.zeros(2, 4, 5, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.distance_transform(torch.zeros(2, 4, 5), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.surface_distances(good, 0.5, torch.zeros(2, 4, 5))
    with pytest.raises(RuntimeError, match="float32"):
        H.distance_transform(good.to(torch.float64), 0.5)
    with pytest.raises(ValueError, match="uint8 or bool"):
        H.distance_transform(good)                                                             # fp32 without a threshold
    with pytest.raises(ValueError, match="uint8 or bool"):
        H.skeletonize(good.to(torch.int32))
    with pytest.raises(ValueError, match="truth must be"):
        H.surface_distances(good, 0.5, good.to(torch.int32))
    with pytest.raises(ValueError, match="does not match"):
        H.surface_distances(good, 0.5, torch.zeros(2, 5, 4, device=DEV))
    with pytest.raises(ValueError, match="sites"):
        H.distance_transform(good, 0.5, sites="edges")
    with pytest.raises(ValueError, match="exceeds"):
        H.distance_transform(torch.zeros(1, 2, D.edt_max_width() + 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="exceeds"):
        H.root_traits(torch.zeros(1, 2, D.edt_max_width() + 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="non-empty"):
        H.distance_transform(torch.zeros(2, 3, 4, 5, device=DEV), 0.5)
    with pytest.raises(ValueError, match="int32 values"):
        D.select_hist([(good, good.to(torch.uint8))])
    assert D.edt_max_width() >= 4096
