"""The guided filter on the device (hyperpri_amd/guided.py, csrc/guided.hip) against the numpy restatement of its contract: coefficient
planes bit for bit on integer data, planes and q within the rounding-model bound on real-valued data for every K, radius and group
size, results that do not depend on the batch, the number of maps, the tile or the run, the same bits from every guide layout, and end
to end from a filled cache through ``detect_split`` and ``refine_split`` to the evaluation of a split.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest
import torch

import _guided_cases as K
from conftest import record_margin
from test_gpu_detect import _check_logit
from test_gpu_spectral import DEV, U, _cache, _real_cubes

pytestmark = pytest.mark.gpu
CASES = K.bounded_cases()


def _launch(guide, maps, r, eps, domain="linear", gs=None):
    """``hpri_guided_coeffs`` and ``hpri_guided_apply`` themselves on an (N, K, h, w) guide laid out channels-last with stride ``gs``
    (NaN in the channels past K: they must never count) and (N, T, h, w) maps: ``(planes (N, T, 2K+1, h, w), out (N, T, h, w))``."""
    from hyperpri_amd import _lib
    from hyperpri_amd._args import _p, _stream
    N, Kg, h, w = guide.shape
    T = maps.shape[1]
    gs = Kg if gs is None else gs
    buf = np.full((N, h, w, gs), np.nan, dtype=np.float32)
    buf[..., :Kg] = guide.transpose(0, 2, 3, 1)
    g, p = torch.from_numpy(buf).to(DEV), torch.from_numpy(np.ascontiguousarray(maps, dtype=np.float32)).to(DEV)
    nbytes = int(_lib.load().hpri_guided_workspace_bytes(N, T, h, w, Kg))
    assert nbytes == 4 * N * T * (2 * Kg + 1) * h * w
    work = torch.full((N, T, 2 * Kg + 1, h, w), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full((N, T, h, w), float("nan"), dtype=torch.float32, device=DEV)
    code = K.DOMAINS.index(domain)
    _lib.call("hpri_guided_coeffs", _p(g), gs, Kg, _p(p), N, T, h, w, r, float(eps), code, _p(work), nbytes, _stream())
    _lib.call("hpri_guided_apply", _p(g), gs, Kg, N, T, h, w, r, code, _p(work), nbytes, _p(out), _stream())
    torch.cuda.synchronize()
    return work.cpu().numpy(), out.cpu().numpy()


def _ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def _bits(t):
    return t.contiguous().cpu().numpy().tobytes()


# ---- exact on integers -----------------------------------------------------------------------------------------------
EXACT_FRAMES = ((1, 3, 5), (1, K.TILE_H + 1, K.TILE_W + 1), (3, K.TILE_H - 1, K.TILE_W - 1), (1, 37, 130))


def _covered(r, most):
    """Frames (N, h, w) that every window of radius r covers whole, with a power of two of pixels up to ``most``: n is that power of
    two for every pixel."""
    return [(2, h, w) for h in (1, 2, 4, 8) for w in (2, 4, 8) if max(h, w) <= r + 1 and h * w <= most]


@pytest.mark.parametrize("r", [1, 2, 8])
@pytest.mark.parametrize("Kg", [1, 2, 3])
def test_a_constant_guide_is_exact_on_integers(Kg, r):
    """Integer maps in [-4, 4] under a constant guide: dI = 0, the sums of dp are integers below 2^24 in any order, a = 0, mI = I and
    mp = p_k + s / n is one fp64 division and one addition: the planes equal the reference's, rounded once, bit for bit.  q is a
    chain of n fp32 additions of non-integers and is held to 2 ulp where that can be derived: on frames every window covers whole,
    with 2^k pixels, mp = (the image's sum) / 2^k and every partial sum of the chain are exact, so q is."""
    from hyperpri_amd import guided as G
    const = np.array([3.0, -2.0, 4.0], dtype=np.float32)[:Kg]
    for frame in EXACT_FRAMES + tuple(_covered(r, 64)):
        N, h, w = frame
        I = np.broadcast_to(const[None, :, None, None], (N, Kg, h, w)).copy()
        p = K.int_frame(N, 2, h, w, seed=r)
        ref = G.guided_reference(I, p, r, 0.5)
        planes, out = _launch(I, p, r, 0.5, gs=(1, 3, 8)[Kg - 1])
        assert np.array_equal(planes, ref["planes"].astype(np.float32)), frame
        assert not planes[:, :, :Kg].any() and np.array_equal(planes[:, 0, Kg:2 * Kg], I)
        assert np.isfinite(out).all()
        if frame not in EXACT_FRAMES:
            assert (np.abs(out - ref["q"]) <= 2 * _ulp32(ref["q"])).all(), frame
            assert np.array_equal(out, ref["q"]), frame                         # (in fact exact, as derived)


@pytest.mark.parametrize("r", [1, 3, 8])
@pytest.mark.parametrize("eps", [0.25, 2.0])
def test_the_guide_as_its_own_map_is_exact_on_integers(eps, r):
    """K = 1, p = I, integers in [-4, 4], eps a power of two: S1, S2 = Sp and s = S1 are integers, m, C and c are dyadic and exact in
    fp64, a = c / (C + eps) is one division, mI = mp = I_k + m: the planes equal the reference's, rounded once, bit for bit.  q within
    2 ulp of the fp64 evaluation of stage 2 on those planes, on the covered frames of at most four pixels: there every term of the
    chain is the same t (one rounding, of the fmaf), t + t is exact, the third and the fourth addition round once each and the
    division by 2 or 4 is exact -- 1/2 + 1/4 + 1/2 ulp at the most."""
    from hyperpri_amd import guided as G
    for frame in EXACT_FRAMES + tuple(_covered(r, 4)):
        N, h, w = frame
        I = K.int_frame(N, 1, h, w, seed=10 + r)
        ref = G.guided_reference(I, I, r, eps)
        planes, out = _launch(I, I, r, eps)
        assert np.array_equal(planes, ref["planes"].astype(np.float32)), frame
        assert np.array_equal(planes[:, :, 1], planes[:, :, 2])
        if frame not in EXACT_FRAMES:
            want = G.guided_apply_reference(I, planes, r)
            assert (np.abs(out - want) <= 2 * _ulp32(want)).all(), (frame, np.abs(out - want).max())


# ---- real-valued data inside the rounding-model bound ------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_planes_and_q_within_the_bound(case):
    from hyperpri_amd import guided as G
    name, Kg, r, T, gs, domain, frame, eps, offset = case
    I, p = K.case_data(case)
    ref, bound = G.guided_reference(I, p, r, eps, domain), G.guided_bound(I, p, r, eps, domain)
    planes, out = _launch(I, p, r, eps, domain, gs)
    assert np.isfinite(planes).all() and np.isfinite(out).all()
    frac = (np.abs(planes - ref["planes"]) / bound["planes"]).max()
    print(name, "planes", frac)
    record_margin(f"guided/planes/K{Kg}/{domain}" + ("/offset" if offset else ""), frac, 1.0)
    assert frac <= 1.0, (name, frac)
    if domain == "linear":
        frac = (np.abs(out - ref["q"]) / bound["value"]).max()
        print(name, "q", frac)
        record_margin(f"guided/q/K{Kg}/linear" + ("/offset" if offset else ""), frac, 1.0)
        assert frac <= 1.0, (name, frac)
    else:
        _check_logit(f"guided/q/K{Kg}/prob" + ("/offset" if offset else ""), out.astype(np.float64).ravel(), ref["value"].ravel(),
                     bound["value"].ravel())


# ---- independence, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("domain", K.DOMAINS)
@pytest.mark.parametrize("Kg,r", [(1, 2), (3, 1), (3, 8)])
def test_a_result_depends_neither_on_the_batch_nor_on_the_other_maps_nor_on_the_run(Kg, r, domain):
    from hyperpri_amd import guided_filter
    N, T, h, w = 3, 5, K.TILE_H + 1, 2 * K.TILE_W + 3
    I = torch.from_numpy(K.real_guide(N, Kg, h, w, seed=r)).to(DEV)
    p = torch.from_numpy(K.real_maps(N, T, h, w, domain, seed=Kg)).to(DEV)
    q, planes = guided_filter(I, p, r, 1e-2, domain, return_coefficients=True)
    q2, planes2 = guided_filter(I, p, r, 1e-2, domain, return_coefficients=True)
    assert _bits(q) == _bits(q2) and _bits(planes) == _bits(planes2)                     # two runs
    assert tuple(q.shape) == (N, T, h, w) and tuple(planes.shape) == (N, T, 2 * Kg + 1, h, w) and bool(torch.isfinite(q).all())
    qa, pa = guided_filter(I[2:].contiguous(), p[2:].contiguous(), r, 1e-2, domain, return_coefficients=True)
    assert _bits(qa) == _bits(q[2:]) and _bits(pa) == _bits(planes[2:])                  # alone, and third of three
    for t in (2, 4):                                                                     # inside a group of four, and a group of its own
        qt, pt = guided_filter(I, p[:, t].contiguous(), r, 1e-2, domain, return_coefficients=True)
        assert tuple(qt.shape) == (N, h, w)
        assert _bits(qt) == _bits(q[:, t]) and _bits(pt[:, 0]) == _bits(planes[:, t])    # one map, and that map among five


@pytest.mark.parametrize("Kg,r", [(1, 1), (2, 2), (3, 4)])
def test_in_phase_pixels_of_a_periodic_image_are_equal(Kg, r):
    """Periods of 5 rows and 7 columns against tiles of 16 x 32: pixels of one phase sit at every place of a tile.  Farther than 2r
    from every border their neighbourhoods are the same, so their results must be -- whatever tile or lane computed them."""
    from hyperpri_amd import guided_filter
    h, w = 37 + 4 * r, 130
    I = torch.from_numpy(K.periodic(2, Kg, h, w, seed=r)).to(DEV)
    p = torch.from_numpy(K.periodic(2, 2, h, w, seed=50 + r)).to(DEV)
    q, planes = guided_filter(I, p, r, 1e-3, return_coefficients=True)
    m = 2 * r
    for name, v in (("q", q[:, :, m:h - m, m:w - m].cpu().numpy()), ("planes", planes[:, :, :, r:h - r, r:w - r].cpu().numpy())):
        assert v.shape[-2] > 2 * K.TILE_H and v.shape[-1] > 3 * K.TILE_W
        assert np.array_equal(v[..., 5:, :], v[..., :-5, :]) and np.array_equal(v[..., :, 7:], v[..., :, :-7]), name
    assert float(q.std()) > 0.01


# ---- layouts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unsqueeze", [True, False])
def test_every_guide_layout_gives_the_same_bits(unsqueeze):
    import hyperpri_amd as H
    from hyperpri_amd import guided as G
    cubes, masks = _real_cubes(31, 3, 19, 45, 37)
    cache = _cache(cubes, masks, unsqueeze=unsqueeze)
    proj = H.SpectralProjection.pca(H.band_statistics(cache), 3).to(DEV)
    batch = cache.batch([2, 0])
    guide = proj(batch["image"])                                                        # (N, 1, 3, h, w) from the 5-d cache image
    assert tuple(guide.shape) == ((2, 1, 3, 19, 45) if unsqueeze else (2, 3, 19, 45))
    g4 = guide[:, 0] if unsqueeze else guide
    src, gs = G._guide_input(g4)
    assert gs == 8 and src.data_ptr() == g4.data_ptr()                                   # zero-copy: the projection's own buffer
    maps = torch.from_numpy(K.real_maps(2, 3, 19, 45, "prob", seed=3)).to(DEV)
    want = G.guided_filter(guide, maps, 2, 1e-2, "prob")
    assert tuple(want.shape) == (2, 3, 19, 45) and want.dtype == torch.float32
    plain = g4.contiguous()                                                             # plain NCHW: one layout pass
    src, gs = G._guide_input(plain)
    assert gs == 3 and src.data_ptr() != plain.data_ptr()
    assert _bits(G.guided_filter(plain, maps, 2, 1e-2, "prob")) == _bits(want)
    last = plain.contiguous(memory_format=torch.channels_last)                          # channels-last with a stride of 3: zero-copy
    src, gs = G._guide_input(last)
    assert gs == 3 and src.data_ptr() == last.data_ptr()
    assert _bits(G.guided_filter(last, maps, 2, 1e-2, "prob")) == _bits(want)
    # one channel: the projection's first output in place (stride 8), and a plain plane (stride 1)
    one = G.guided_filter(g4[:, :1], maps, 2, 1e-2, "prob")
    assert G._guide_input(g4[:, :1])[1] == 8 and G._guide_input(plain[:, :1].contiguous())[1] == 1
    assert _bits(G.guided_filter(plain[:, :1].contiguous(), maps, 2, 1e-2, "prob")) == _bits(one)
    assert _bits(H.GuidedFilter(2, 1e-2, "prob")(guide, maps)) == _bits(want)
    # against the reference, from the device's own guide
    ref, bound = G.guided_reference(g4.cpu().numpy(), maps.cpu().numpy(), 2, 1e-2, "prob"), G.guided_bound(g4.cpu().numpy(), maps.cpu().numpy(), 2, 1e-2, "prob")
    _check_logit("guided/layouts", want.cpu().numpy().astype(np.float64).ravel(), ref["value"].ravel(), bound["value"].ravel())
    with pytest.raises(RuntimeError, match="autograd"):
        G.guided_filter(plain.clone().requires_grad_(True), maps, 2, 1e-2)
    with pytest.raises(ValueError, match="frame"):
        G.guided_filter(guide, maps[:, :, :-1], 2, 1e-2)


# ---- end to end ------------------------------------------------------------------------------------------------------
def _best_dice(val):
    """(the best Dice 2 tp / (2 tp + fp + fn) over the thresholds of ``validate_net``'s curve, its threshold), from the integer counts:
    defined at every threshold, also at those above the largest score, where the curve's precision is not."""
    tp, fp, fn = (val["curve_counts"][k].cpu().numpy().astype(np.float64) for k in ("tp", "fp", "fn"))
    thr = val["thresholds"].cpu().numpy()
    dice = (2 * tp / (2 * tp + fp + fn))[:len(thr)]
    return float(dice.max()), float(thr[int(dice.argmax())])


def test_statistics_guide_detect_refine_and_evaluate():
    import hyperpri_amd as H
    cubes, masks = K.blob_scene()
    n = cubes.shape[0]
    cache = _cache(cubes, masks)

    def epoch():
        return cache.epoch(batch_size=2, shuffle=False)
    proj = H.SpectralProjection.pca(H.band_statistics(cache), 3).to(DEV)
    det = H.SpectralDetector.fit(cache)
    pred = H.detect_split(det, epoch(), score="ace")
    refined = H.refine_split(pred, epoch(), proj, 2, 0.1)
    assert refined is not pred and len(refined) == n and refined.spread is None
    assert refined.masks is pred.masks and refined.offsets == pred.offsets and refined.sizes == pred.sizes and refined.names == pred.names
    by_batch = torch.cat([H.guided_filter(proj(bt["image"]), det(bt, score="ace", logit=True)[:, 0].contiguous(), 2, 0.1, "prob").reshape(-1).clone()
                          for bt in epoch()])
    assert _bits(refined.logits) == _bits(by_batch) and _bits(refined.logits) != _bits(pred.logits)
    raw, val = H.validate_net(pred), H.validate_net(refined)
    (raw_dice, _), (dice, threshold) = _best_dice(raw), _best_dice(val)
    print("best Dice raw", raw_dice, "refined", dice)
    assert 0.5 < raw_dice < 0.95                                     # the detector's map is noisy (the CPU test says so of the scene)
    assert dice >= raw_dice and np.isfinite(val["avg_prec"]) and np.isfinite(val["bce_loss"])
    test = H.test_net(refined, threshold)
    assert sum(test["counts"][k] for k in ("tp", "fp", "fn", "tn")) == masks.size and abs(test["dice"] - dice) <= 1e-6
    # any callable is a guide: here the first component alone; the stored spread is carried over
    pred.spread = torch.zeros_like(pred.logits)
    one = H.refine_split(pred, epoch(), lambda image: proj(image)[:, 0, :1], 2, 0.1)
    assert one.spread is pred.spread and _best_dice(H.validate_net(one))[0] >= raw_dice
    with pytest.raises(ValueError, match="same order"):
        H.refine_split(pred, reversed(list(epoch())), proj, 2, 0.1)
    with pytest.raises(ValueError, match="held 2 of the 3"):
        H.refine_split(pred, list(epoch())[:1], proj, 2, 0.1)
    with pytest.raises(ValueError, match="at most 3"):
        H.refine_split(pred, epoch(), H.SpectralProjection.pca(H.band_statistics(cache), 4), 2, 0.1)


def test_filtered_softmax_planes_still_sum_to_one():
    import hyperpri_amd as H
    from hyperpri_amd import guided as G
    N, C, h, w, r = 2, 5, 21, 50, 2
    I = K.real_guide(N, 3, h, w, seed=9)
    soft = torch.softmax(torch.from_numpy(K.real_maps(N, C, h, w, "prob", seed=9)).to(DEV), dim=1)
    q = H.guided_filter(torch.from_numpy(I).to(DEV), soft, r, 1e-2)
    ref, bound = G.guided_reference(I, soft.cpu().numpy(), r, 1e-2), G.guided_bound(I, soft.cpu().numpy(), r, 1e-2)
    got = q.cpu().numpy().astype(np.float64)
    # the device's sum against the reference's, and the reference's against one: the fp32 planes sum to one within 5 u, and the
    # filter's gain on that residue is at most 1 + K sqrt(n) (Cauchy-Schwarz on its kernel)
    frac = (np.abs(got.sum(axis=1) - ref["q"].sum(axis=1)) / bound["value"].sum(axis=1)).max()
    record_margin("guided/softmax_sum", frac, 1.0)
    assert frac <= 1.0
    assert np.abs(ref["q"].sum(axis=1) - 1).max() <= 5 * U * (1 + 3 * (2 * r + 1))
    assert np.abs(got.sum(axis=1) - 1).max() <= bound["value"].sum(axis=1).max() + 5 * U * (1 + 3 * (2 * r + 1))
    classes = H.argmax_classes(q)
    assert classes.dtype == torch.uint8 and np.array_equal(classes.cpu().numpy(), got.argmax(axis=1).astype(np.uint8))
