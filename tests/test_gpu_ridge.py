"""The ridge filter on the device (hyperpri_amd/ridge.py, csrc/ridge.hip) against the numpy restatement of its contract: Hessian planes,
responses, scale indices and logits within the rounding-model bound for every scale set, T, pixel stride, domain, measure and polarity,
exact zeros bit for bit, results that do not depend on the batch, the other maps, the other scales, the tile or the run, the same bits
from every layout, and end to end from a filled cache through ``ridge_split`` and ``enhance_split`` to the evaluation of a split.
Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest
import torch

import _ridge_cases as K
from conftest import record_margin
from test_gpu_detect import _check_logit
from test_gpu_guided import _best_dice, _bits
from test_gpu_spectral import DEV, _cache

pytestmark = pytest.mark.gpu
CASES = K.bounded_cases()


def _launch(maps, sigmas, measure="frangi", polarity="bright", beta=0.5, c=0.5, domain="linear", output="value", stride=1):
    """``hpri_ridge_filter`` itself on (N, T, h, w) maps laid out plain (stride 1) or channels-last with ``stride`` channels (NaN in the
    channels past T: they must never count): ``(out (N, T, h, w), scale, hessian (N, T, S, 3, h, w))``, every output pre-filled."""
    from hyperpri_amd import _lib
    from hyperpri_amd import ridge as R
    from hyperpri_amd._args import _p, _stream
    N, T, h, w = maps.shape
    if stride == 1:
        buf, strides = np.ascontiguousarray(maps, dtype=np.float32), (T * h * w, h * w, 1)
    else:
        buf = np.full((N, h, w, stride), np.nan, dtype=np.float32)
        buf[..., :T] = maps.transpose(0, 2, 3, 1)
        strides = (h * w * stride, 1, stride)
    src = torch.from_numpy(buf).to(DEV)
    sig = R._check_sigmas(sigmas, "test")
    taps, radii, sigma2 = R._host_taps(sig)
    S = len(sig)
    out = torch.full((N, T, h, w), float("nan"), dtype=torch.float32, device=DEV)
    scale = torch.full((N, T, h, w), 255, dtype=torch.uint8, device=DEV)
    hess = torch.full((N, T, S, 3, h, w), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("hpri_ridge_filter", _p(src), *strides, N, T, h, w, taps.ctypes.data, radii.ctypes.data, sigma2.ctypes.data, S,
              float(np.float32(beta)), float(np.float32(c)), K.POLARITIES.index(polarity), K.MEASURES.index(measure),
              K.DOMAINS.index(domain), K.OUTPUTS.index(output), _p(out), _p(scale), _p(hess), _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), scale.cpu().numpy(), hess.cpu().numpy()


# ---- real-valued data inside the rounding-model bound ------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_planes_responses_and_indices_within_the_bound(case):
    from hyperpri_amd import ridge as R
    name, sig, T, stride, domain, measure, polarity, output, frame, c, offset = case
    I, args = K.case_data(case), K.case_args(case)
    ref, bound = R.ridge_reference(I, **args), R.ridge_bound(I, **args)
    out, scale, hess = _launch(I, sig, measure, polarity, 0.5, c, domain, output, stride)
    assert np.isfinite(hess).all() and np.isfinite(out).all() and scale.max() < len(sig)
    tag = f"{measure}/{polarity}/{domain}" + ("/offset" if offset else "")
    if output == "value":
        f = K.fractions(ref, bound, hess, out, scale)
        print(name, f)
        record_margin(f"ridge/value/{tag}", f["value"], 1.0)
        assert f["value"] <= 1.0 and f["inside_ok"], (name, f)
    else:
        f = K.fractions(ref, bound, hess, ref["response"], scale)          # (the response itself is not written: the logit is)
        print(name, f)
        keep = ~bound["undecided"].ravel()
        assert keep.mean() >= 0.99
        if frame[1:] == (1, 1):                                            # one pixel: H = 0, V = 0, the logit of the clamp
            floor = np.log(R.P_LO) - np.log1p(-R.P_LO)
            assert not ref["prob"].any() and (np.abs(out - floor) <= 8 * 2.0 ** -24 * abs(floor)).all(), (name, out)
        else:
            _check_logit(f"ridge/logit/{tag}", out.astype(np.float64).ravel()[keep], ref["prob"].ravel()[keep], bound["prob"].ravel()[keep])
    record_margin(f"ridge/hessian/{tag}", f["hessian"], 1.0)
    assert f["hessian"] <= 1.0 and f["index_ok"], (name, f)
    assert f["share"] <= 0.01, (name, f)


# ---- exact zeros and the exact negation --------------------------------------------------------------------------------
def _plus_zero(a):
    return not np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).any()


@pytest.mark.parametrize("measure", K.MEASURES)
def test_exact_zeros_bit_for_bit(measure):
    h, w, sig = 40, 70, (1.0, 2.0, 4.0)
    y, x = np.mgrid[0:h, 0:w]
    out, scale, hess = _launch(np.full((2, 2, 17, 33), 1e6, dtype=np.float32), sig, measure, "both", c=0.5)
    assert _plus_zero(hess) and _plus_zero(out) and not scale.any()                # a constant plane of any magnitude
    rows = (np.sin(0.7 * y) * 100).astype(np.float32)[None, None]
    out, scale, hess = _launch(rows, sig, measure)
    assert _plus_zero(hess[:, :, :, 0]) and _plus_zero(hess[:, :, :, 1]) and hess[:, :, :, 2].any()    # constant along x
    ramp = (3 * x - 2 * y).astype(np.float32)[None, None]
    out, scale, hess = _launch(ramp, sig, measure)
    assert _plus_zero(hess[:, :, :, 1])                                             # Hxy everywhere
    for s, sigma in enumerate(sig):
        R = int(np.ceil(3 * sigma))
        assert _plus_zero(hess[:, :, s, 0, :, R:w - R]) and _plus_zero(hess[:, :, s, 2, R:h - R, :])
    assert hess[:, :, 0, 0, :, 0].any() and hess[:, :, 0, 2, 0, :].any()            # the reflected borders bend the ramp


@pytest.mark.parametrize("measure", K.MEASURES)
def test_dark_on_the_negated_plane_equals_bright_bit_for_bit(measure):
    I = K.real_maps(2, 2, K.TILE_H + 1, K.TILE_W + 1, seed=5)
    sig = (0.75, 1.5, 3.0)
    a, sa, ha = _launch(I, sig, measure, "bright")
    b, sb, hb = _launch(-I, sig, measure, "dark")
    assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes() and np.array_equal(ha, -hb) and a.max() > 0.01


# ---- independence, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure,polarity,domain", [("frangi", "bright", "linear"), ("sato", "both", "prob")])
def test_a_result_depends_neither_on_the_batch_nor_on_the_other_maps_or_scales_nor_on_the_run(measure, polarity, domain):
    from hyperpri_amd import ridge_filter
    N, T, h, w = 3, 5, K.TILE_H + 1, 2 * K.TILE_W + 3
    I = torch.from_numpy(K.real_maps(N, T, h, w, domain, seed=11)).to(DEV)
    kw = dict(measure=measure, polarity=polarity, domain=domain, return_scale=True, return_hessian=True)
    v, s, H = ridge_filter(I, K.SCENE_SIGMAS, **kw)
    v2, s2, H2 = ridge_filter(I, K.SCENE_SIGMAS, **kw)
    assert _bits(v) == _bits(v2) and _bits(s) == _bits(s2) and _bits(H) == _bits(H2)                  # two runs
    assert tuple(v.shape) == (N, T, h, w) and s.dtype == torch.uint8 and tuple(H.shape) == (N, T, 5, 3, h, w)
    assert bool(torch.isfinite(v).all()) and int(s.max()) <= 4 and len(torch.unique(s)) > 1
    va, sa, Ha = ridge_filter(I[2:].contiguous(), K.SCENE_SIGMAS, **kw)
    assert _bits(va) == _bits(v[2:]) and _bits(sa) == _bits(s[2:]) and _bits(Ha) == _bits(H[2:])       # alone, and third of three
    vt, st, Ht = ridge_filter(I[:, 3].contiguous(), K.SCENE_SIGMAS, **kw)
    assert tuple(vt.shape) == (N, h, w)
    assert _bits(vt) == _bits(v[:, 3]) and _bits(st) == _bits(s[:, 3]) and _bits(Ht[:, 0]) == _bits(H[:, 3])   # one map, and among five
    for k in (0, 2, 4):                                                                                # a scale alone, and among five
        _, _, H1 = ridge_filter(I, (K.SCENE_SIGMAS[k],), **kw)
        assert _bits(H1[:, :, 0]) == _bits(H[:, :, k]), k


def test_in_phase_pixels_of_a_periodic_image_are_equal():
    """Periods of 5 rows and 7 columns against tiles of 16 x 32: pixels of one phase sit at every place of a tile.  Farther than the
    largest R from every border their neighbourhoods are the same, so their results must be -- whatever tile or lane computed them."""
    from hyperpri_amd import ridge_filter
    m = 9                                                                               # R of sigma = 3
    h, w = 37 + 2 * m, 130
    I = torch.from_numpy(K.periodic(2, 2, h, w, seed=3)).to(DEV)
    v, s, H = ridge_filter(I, K.SCENE_SIGMAS, c=0.2, return_scale=True, return_hessian=True)
    for name, a in (("value", v), ("scale", s), ("hessian", H)):
        a = a[..., m:h - m, m:w - m].cpu().numpy()
        assert a.shape[-2] > 2 * K.TILE_H and a.shape[-1] > 3 * K.TILE_W
        assert np.array_equal(a[..., 5:, :], a[..., :-5, :]) and np.array_equal(a[..., :, 7:], a[..., :, :-7]), name
    assert float(v.std()) > 1e-3


# ---- layouts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unsqueeze", [True, False])
def test_every_layout_gives_the_same_bits(unsqueeze):
    import hyperpri_amd as H
    from hyperpri_amd import ridge as R
    from test_gpu_spectral import _real_cubes
    cubes, masks = _real_cubes(31, 3, 19, 45, 37)
    cache = _cache(cubes, masks, unsqueeze=unsqueeze)
    proj = H.SpectralProjection.pca(H.band_statistics(cache), 3).to(DEV)
    planes = proj(cache.batch([2, 0])["image"])                                         # (N, 1, 3, h, w) from the 5-d cache image
    assert tuple(planes.shape) == ((2, 1, 3, 19, 45) if unsqueeze else (2, 3, 19, 45))
    g4 = planes[:, 0] if unsqueeze else planes
    two = g4[:, :2]
    src, si, st, sp = R._plane_input(two)
    assert (si, st, sp) == (19 * 45 * 8, 1, 8) and src.data_ptr() == g4.data_ptr()        # zero-copy: the projection's own buffer
    kw = dict(sigmas=(1.0, 2.0), c=0.05, return_scale=True, return_hessian=True)
    want = R.ridge_filter(two, **kw)
    assert tuple(want[0].shape) == (2, 2, 19, 45) and float(want[0].max()) > 0.01
    plain = two.contiguous()                                                            # plain NCHW: read in place
    src, si, st, sp = R._plane_input(plain)
    assert (si, st, sp) == (2 * 19 * 45, 19 * 45, 1) and src.data_ptr() == plain.data_ptr()
    last = plain.contiguous(memory_format=torch.channels_last)                          # channels-last with a stride of 2: in place
    src, si, st, sp = R._plane_input(last)
    assert (st, sp) == (1, 2) and src.data_ptr() == last.data_ptr()
    turned = plain.transpose(2, 3).contiguous().transpose(2, 3)                         # columns first: one layout pass
    assert R._plane_input(turned)[0].data_ptr() != turned.data_ptr()
    for other in (plain, last, turned):
        got = R.ridge_filter(other, **kw)
        assert all(_bits(a) == _bits(b) for a, b in zip(got, want))
    if unsqueeze:                                                                       # (N, 1, T, h, w): the output has the input's shape
        got = R.ridge_filter(planes[:, :, :2], **kw)
        assert tuple(got[0].shape) == (2, 1, 2, 19, 45) and _bits(got[0]) == _bits(want[0])
    one = R.ridge_filter(g4[:, 0], **kw)                                                # a single plane at stride 8, and a plain one
    assert R._plane_input(g4[:, :1])[3] == 8 and tuple(one[0].shape) == (2, 19, 45)
    assert all(_bits(a) == _bits(b) for a, b in zip(R.ridge_filter(g4[:, 0].contiguous(), **kw), one))
    assert _bits(one[0]) == _bits(want[0][:, 0]) and _bits(one[2][:, 0]) == _bits(want[2][:, 0])
    assert _bits(H.RidgeFilter((1.0, 2.0), c=0.05)(two)) == _bits(want[0])
    # against the reference, from the device's own planes
    ref, bound = R.ridge_reference(two, (1.0, 2.0), c=0.05), R.ridge_bound(two, (1.0, 2.0), c=0.05)
    f = K.fractions(ref, bound, want[2].cpu().numpy(), want[0].cpu().numpy(), want[1].cpu().numpy())
    record_margin("ridge/layouts", max(f["hessian"], f["value"]), 1.0)
    assert f["hessian"] <= 1.0 and f["value"] <= 1.0 and f["inside_ok"] and f["index_ok"] and f["share"] <= 0.01, f
    with pytest.raises(RuntimeError, match="autograd"):
        R.ridge_filter(plain.clone().requires_grad_(True), (1.0,))
    with pytest.raises(ValueError, match="5-d maps"):
        R.ridge_filter(torch.zeros(2, 2, 3, 4, 5, device=DEV), (1.0,))


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_statistics_projection_ridge_split_and_evaluate():
    import hyperpri_amd as H
    cubes, masks, _ = K.scene_cubes()
    n = cubes.shape[0]
    cache = _cache(cubes, masks)

    def epoch():
        return cache.epoch(batch_size=2, shuffle=False)
    proj = H.SpectralProjection.pca(H.band_statistics(cache), 3).to(DEV)
    first = torch.cat([proj(bt["image"])[:, 0, 0].reshape(-1).clone() for bt in epoch()])
    m = torch.from_numpy(masks.reshape(-1) != 0).to(DEV)
    bright = bool(first[m].mean() > first[~m].mean())                                   # the sign of a principal axis is arbitrary
    kw = dict(polarity="bright" if bright else "dark", beta=0.5, c=0.5)
    pred = H.ridge_split(epoch(), proj, K.SCENE_SIGMAS, **kw)
    assert len(pred) == n and pred.spread is None and pred.sizes == [(48, 64)] * n and pred.offsets == [0, 3072, 6144, 9216]
    assert np.array_equal(pred.masks.cpu().numpy(), masks.reshape(-1).astype(np.float32))
    by_batch = torch.cat([H.ridge_filter(proj(bt["image"])[:, 0, :1], K.SCENE_SIGMAS, output="logit", **kw).reshape(-1).clone() for bt in epoch()])
    assert _bits(pred.logits) == _bits(by_batch)
    same = H.ridge_split(epoch(), lambda im: proj(im)[:, 0, :1], K.SCENE_SIGMAS, **kw)      # any callable is a plane
    assert _bits(same.logits) == _bits(pred.logits) and same.names == pred.names
    # the raw plane as a split of its own: a threshold on it is what the ridge measure has to beat
    p = (first if bright else -first)
    p = ((p - p.min()) / (p.max() - p.min())).clamp(2.0 ** -24, 1 - 2.0 ** -24)
    raw_pred = H.SplitPrediction(torch.log(p) - torch.log1p(-p), pred.masks, list(pred.offsets), list(pred.sizes), list(pred.names), None)
    (raw_dice, _), val = _best_dice(H.validate_net(raw_pred)), H.validate_net(pred)
    dice, threshold = _best_dice(val)
    print("best Dice raw", raw_dice, "ridge", dice)
    assert raw_dice < 0.6 and dice >= raw_dice + 0.1
    assert np.isfinite(val["avg_prec"]) and np.isfinite(val["bce_loss"])
    test = H.test_net(pred, threshold)
    assert sum(test["counts"][k] for k in ("tp", "fp", "fn", "tn")) == masks.size and abs(test["dice"] - dice) <= 1e-6
    with pytest.raises(ValueError, match="no batches"):
        H.ridge_split([], proj, K.SCENE_SIGMAS)
    with pytest.raises(ValueError, match="not its to take"):
        H.ridge_split(epoch(), proj, K.SCENE_SIGMAS, output="value")
    with pytest.raises(ValueError, match="must be"):
        H.ridge_split(epoch(), lambda im: proj(im)[:, 0, 0], K.SCENE_SIGMAS)


def test_enhance_split_carries_the_split_over():
    import hyperpri_amd as H
    from _guided_cases import blob_scene
    cubes, masks = blob_scene()
    cache = _cache(cubes, masks)
    det = H.SpectralDetector.fit(cache)
    pred = H.detect_split(det, cache.epoch(batch_size=2, shuffle=False), score="ace")
    pred.spread = torch.zeros_like(pred.logits)
    out = H.enhance_split(pred, (1.0, 2.0), measure="sato", polarity="bright", c=0.1)
    assert out is not pred and len(out) == len(pred) and out.spread is pred.spread
    assert out.masks is pred.masks and out.offsets == pred.offsets and out.sizes == pred.sizes and out.names == pred.names
    n, (h, w) = len(pred), pred.sizes[0]
    want = H.ridge_filter(pred.logits.view(n, h, w), (1.0, 2.0), measure="sato", polarity="bright", c=0.1, domain="prob", output="logit")
    assert _bits(out.logits) == _bits(want) and _bits(out.logits) != _bits(pred.logits)
    # images of two sizes: runs of one size go through one launch each, with the same bits
    a, b = pred.offsets[1], pred.offsets[2]
    mixed = H.SplitPrediction(torch.cat([pred.logits[:a], pred.logits[a:b].view(h, w)[:, :-3].reshape(-1), pred.logits[b:]]),
                              torch.cat([pred.masks[:a], pred.masks[a:b].view(h, w)[:, :-3].reshape(-1), pred.masks[b:]]),
                              [0, a, a + h * (w - 3), a + h * (w - 3) + h * w], [(h, w), (h, w - 3), (h, w)], list(pred.names), None)
    got = H.enhance_split(mixed, (1.0, 2.0), measure="sato", polarity="bright", c=0.1)
    assert _bits(got.image(0)[0]) == _bits(out.image(0)[0]) and _bits(got.image(2)[0]) == _bits(out.image(2)[0])
    assert tuple(got.image(1)[0].shape) == (h, w - 3) and np.isfinite(H.validate_net(got)["avg_prec"])
    with pytest.raises(ValueError, match="empty split"):
        H.enhance_split(H.SplitPrediction(pred.logits[:0], pred.masks[:0], [0], [], [], None), (1.0,))
    with pytest.raises(ValueError, match="not its to take"):
        H.enhance_split(pred, (1.0,), domain="linear")
    with pytest.raises(ValueError, match="their sizes say"):
        H.enhance_split(H.SplitPrediction(pred.logits, pred.masks, list(pred.offsets), [(h, w - 1)] * n, list(pred.names), None), (1.0,))
