"""Spectral unmixing on the device (hyperpri_amd/unmix.py, csrc/unmix.hip) against the numpy restatement of its contract: exact on
integer data with endmembers whose factors are powers of two, within the derived bound on mixed pixels, bit-reproducible, the same
bits from every input layout, ATGP picks equal to the restatement's, and end to end from a filled cache through ``unmix_split`` to
the evaluation of a split.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest
import torch

import _unmix_cases as K
from conftest import record_margin
from test_gpu_detect import SIZES, _check_logit, _padded
from test_gpu_spectral import DEV, U, _cache, _stored

pytestmark = pytest.mark.gpu


def _launch(x, E32, Q32, R, mode, cap=0, fg=0, C=None):
    """``hpri_band_unmix`` itself on a (P, cs) fp32 device buffer: ``(a (M, P), rmse (P,), value (P,) or None, capped)``."""
    from hyperpri_amd import _lib
    from hyperpri_amd._args import _p, _stream
    P, cs = int(x.shape[0]), int(x.shape[1])
    M, bands = E32.shape
    basis = np.zeros((16, cs), dtype=np.float32)
    basis[:M, :bands] = Q32
    memb = np.zeros((M, cs), dtype=np.float32)
    memb[:, :bands] = E32
    tri = np.concatenate([R.reshape(-1), (R.T @ R).reshape(-1)])
    bd, md, td = (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in (basis, memb, tri))
    a = torch.full((M, P), float("nan"), dtype=torch.float32, device=DEV)
    rmse = torch.full((P,), float("nan"), dtype=torch.float32, device=DEV)
    value = torch.full((P,), float("nan"), dtype=torch.float32, device=DEV) if fg else None
    capped = torch.zeros(4, dtype=torch.int64, device=DEV)
    _lib.call("hpri_band_unmix", _p(x), P, cs, bands if C is None else C, _p(bd), _p(md), _p(td), M, K.MODES.index(mode), cap, fg, _p(a),
              _p(rmse), _p(value), _p(capped), _stream())
    torch.cuda.synchronize()
    assert not capped[1:].any()
    return a.cpu().numpy(), rmse.cpu().numpy(), (None if value is None else value.cpu().numpy()), int(capped[0])


def _rmse_reference(x, E32, a32, cs):
    """The reconstruction error from the abundances THE DEVICE returned, in fp64, and the bound of its fp32 chains: per band M
    roundings, ``e_r = (M + 1) u (|x| + |E32|^T |a32|)``; the sum of squares, ``e_s = sum (2 |r| e_r + e_r^2) + (cs + 1) u sum (|r|
    + e_r)^2``; then a division and a square root, one rounding each: ``|sqrt(s~ / C) - sqrt(s / C)| <= min(e_s / (2 sqrt(C (s -
    e_s))), sqrt(e_s / C))`` plus 3 u of the value."""
    X, E, A = x.astype(np.float64), E32.astype(np.float64), a32.astype(np.float64).T       # (P, C), (M, C), (P, M)
    M, C = E.shape
    r = X - A @ E
    er = (M + 1) * U * (np.abs(X) + np.abs(A) @ np.abs(E))
    s = (r * r).sum(axis=1)
    es = (2 * np.abs(r) * er + er * er).sum(axis=1) + (cs + 1) * U * ((np.abs(r) + er) ** 2).sum(axis=1)
    ref = np.sqrt(s / C)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = np.where(s > es, es / (2 * np.sqrt(C * np.maximum(s - es, 1e-300))), np.inf)
    return ref, np.minimum(slope, np.sqrt(es / C)) + 3 * U * ref


def _ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


# ---- exact on integers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 5, 8])
@pytest.mark.parametrize("C", [3, 37, 238])
def test_abundances_are_exact_on_integers(C, M):
    """Indicator endmembers of disjoint band groups of 1, 4 and 16 bands: Q32 holds 1, 1/2, 1/4 and R, G are diagonal powers of
    two, so for integer pixels y, b and the ucls / ncls abundances are exact in fp32 and must come back bit for bit; scls and fcls
    divide by sum v and are held to one fp32 ulp (plus 2^-45 of the pixel's scale: u - lambda v cancels in fp64).  M is cut to C."""
    from hyperpri_amd import unmix as Um
    M = min(M, C)
    cs = K.rup(C, 8)
    E = K.indicator_endmembers(C, M)
    E32, Q32, R, G = Um.unmix_operands(E)
    rng = np.random.RandomState(100 * C + M)
    for (n, h, w) in SIZES:
        pixels = rng.randint(-4, 5, size=(n * h * w, C)).astype(np.float32)
        x = _padded(pixels, cs)
        for mode in K.MODES:
            if n == 2 and mode in ("scls", "ncls") and (h, M) != (130, 8):       # the large frames: ucls and fcls, all four once
                continue
            ref, its, rem, capped, trace = Um.unmix_reference(pixels, Q32, R, mode, return_trace=True)
            # what makes "exact" mean something: the reference's intermediates are fp32 numbers
            for v in (trace["y"], trace["b"]) + ((ref,) if mode in ("ucls", "ncls") else ()):
                assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
            assert not capped.any()
            a, rmse, _, ncap = _launch(x, E32, Q32, R, mode)
            assert ncap == 0 and np.isfinite(a).all()
            if mode in ("ucls", "ncls"):
                assert np.array_equal(a.T, ref.astype(np.float32)), mode
                want = np.sqrt(((pixels.astype(np.float64) - ref @ E.astype(np.float64)) ** 2).sum(axis=1) / C)
                assert (np.abs(rmse - want) <= 2 * _ulp32(want)).all(), mode     # s is exact: the division and the root round
            else:
                tol = _ulp32(ref) + 2.0 ** -45 * np.maximum(1.0, np.abs(ref).max(axis=1))[:, None]
                assert (np.abs(a.T - ref) <= tol).all(), (mode, np.abs(a.T - ref).max())
                want, bound = _rmse_reference(pixels, E32, a, cs)
                assert (np.abs(rmse - want) <= bound).all(), mode
            if mode == "fcls":
                assert (a >= 0).all() and np.abs(a.sum(axis=0) - 1).max() <= 4 * U * M


# ---- mixed pixels inside the derived bound ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("M", [2, 5, 8])
@pytest.mark.parametrize("C", [37, 238])
def test_abundances_within_the_derived_bound(C, M, size):
    from hyperpri_amd import unmix as Um
    n, h, w = size
    cs = K.rup(C, 8)
    E = K.endmembers(C, M)
    E32, Q32, R, G = Um.unmix_operands(E)
    pixels = K.mixed_pixels(E, n * h * w, seed=h)
    x = _padded(pixels, cs)
    fg = 0b101 & ((1 << M) - 1)
    for mode in K.MODES:
        ref, its, rem, capped = Um.unmix_reference(pixels, Q32, R, mode)
        assert not capped.any()
        bound = Um.unmix_bound(pixels, Q32, R, ref, cs)
        a, rmse, value, ncap = _launch(x, E32, Q32, R, mode, fg=fg)
        name = f"unmix/{mode}/C{C}/M{M}"
        err = np.sqrt(((a.T - ref) ** 2).sum(axis=1))
        print(name, size, "abundance", (err / bound).max())
        record_margin(name + "/abundance", (err / bound).max(), 1.0)
        assert ncap == 0
        assert (err <= bound).all(), (name, (err / bound).max())
        want, rb = _rmse_reference(pixels, E32, a, cs)
        print(name, size, "rmse", (np.abs(rmse - want) / rb).max())
        record_margin(name + "/rmse", (np.abs(rmse - want) / rb).max(), 1.0)
        assert (np.abs(rmse - want) <= rb).all(), name
        # the logit of the fp32 sum of the flagged planes, ascending: one rounding per addition
        members = [m for m in range(M) if fg >> m & 1]
        s = a[members].astype(np.float64).sum(axis=0)
        es = len(members) * U * np.abs(a[members].astype(np.float64)).sum(axis=0)
        _check_logit(name + "/logit", value.astype(np.float64), s, es)
        if mode == "fcls":
            assert (a >= 0).all() and np.abs(a.sum(axis=0) - 1).max() <= 4 * U * M


def test_the_counter_counts_capped_pixels():
    from hyperpri_amd import unmix as Um
    C, M = 37, 5
    E = K.endmembers(C, M)
    E32, Q32, R, G = Um.unmix_operands(E)
    pixels = K.mixed_pixels(E, 1000)
    x = _padded(pixels, K.rup(C, 8))
    for mode in ("ncls", "fcls"):
        assert _launch(x, E32, Q32, R, mode)[3] == 0
        want = Um.unmix_reference(pixels, Q32, R, mode, cap=1)
        a, _, _, ncap = _launch(x, E32, Q32, R, mode, cap=1)
        assert 0 < ncap <= 1000 and want[3].sum() > 0
        # (the M noise-free pixels sit at the threshold after one sub-solve -- their w is the rounding of y -- and may go either way)
        assert abs(ncap - int(want[3].sum())) <= M
        assert (a >= 0).all()                                       # a capped pixel keeps a feasible point
    for mode in ("ucls", "scls"):
        assert _launch(x, E32, Q32, R, mode, cap=1)[3] == 0
    # through the module: the counter of the last call
    m = Um.SpectralUnmixer(E).to(DEV)
    img = torch.from_numpy(np.ascontiguousarray(pixels.reshape(1, 25, 40, C).transpose(0, 3, 1, 2))).to(DEV)
    m(img, mode="fcls", cap=1)
    first = m.capped
    m(img, mode="fcls")
    assert first > 0 and m.capped == 0


# ---- reproducibility and layouts -------------------------------------------------------------------------------------
def _scene_cache(C, M, **kw):
    cubes, masks, planted = K.planted_scene(C, M)
    return cubes, masks, planted, _cache(cubes, masks, **kw)


def test_maps_are_bit_reproducible_and_independent_of_the_batch():
    from hyperpri_amd import unmix as Um
    C, M = 37, 5
    cubes, masks, _, cache = _scene_cache(C, M, out_slots=4)
    m = Um.SpectralUnmixer(K.endmembers(C, M), foreground=[True, False, True, False, False]).to(DEV)
    for mode in K.MODES:
        for output in Um.OUTPUTS:
            both = cache.batch([0, 2])
            a = m(both, mode=mode, output=output).clone()
            b = m(both, mode=mode, output=output).clone()
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
            alone = m(cache.batch([0]), mode=mode, output=output)
            assert alone.cpu().numpy().tobytes() == a[:1].contiguous().cpu().numpy().tobytes()


@pytest.mark.parametrize("C,M", [(3, 3), (37, 5), (238, 8)])
def test_every_input_layout_gives_the_same_bits(C, M):
    from hyperpri_amd import unmix as Um
    rng = np.random.RandomState(C)
    E = K.endmembers(C, M)
    cubes = K.mixed_pixels(E, 3 * 13 * 11).reshape(3, 13, 11, C)
    masks = (rng.rand(3, 13, 11) < 0.5).astype(np.uint8)
    m = Um.SpectralUnmixer(E, foreground=[True] + [False] * (M - 1)).to(DEV)
    plain = torch.from_numpy(np.ascontiguousarray(cubes[[2, 0]].transpose(0, 3, 1, 2))).to(DEV)       # plain NCHW: the slow path
    for output in Um.OUTPUTS:
        want = m(plain, output=output)
        assert tuple(want.shape) == (2, M if output == "abundance" else 1, 13, 11) and want.dtype == torch.float32
        want = want.contiguous().cpu().numpy().tobytes()
        for unsqueeze in (True, False):
            cache = _cache(cubes, masks, unsqueeze=unsqueeze)
            batch = cache.batch([2, 0])
            for arg in (batch, batch["image"]):
                assert m(arg, output=output).contiguous().cpu().numpy().tobytes() == want, (output, unsqueeze)
    picked = m(plain, members=[M - 1, 0])
    full = m(plain)
    assert tuple(picked.shape) == (2, 2, 13, 11) and torch.equal(picked, full[:, [M - 1, 0]])
    with pytest.raises(RuntimeError, match="autograd"):
        m(plain.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="bands"):
        m(torch.zeros((1, C + 1, 4, 4), device=DEV))
    with pytest.raises(ValueError, match="members"):
        m(plain, members=[M])


# ---- ATGP ------------------------------------------------------------------------------------------------------------
def _check_atgp(cache, stored, masks, M, select="all", slots=None):
    """The device's picks equal the restatement's, every gap is positive and the values lie within the chain bound."""
    from hyperpri_amd import unmix as Um
    order = list(range(stored.shape[0])) if slots is None else list(slots)
    picks, values, gaps = Um.atgp_reference(stored[order], M, None if masks is None else masks[order], select)
    assert (gaps > 0).all()
    spectra, positions, got = Um.extract_endmembers(cache, M, slots, select, return_values=True)
    assert np.array_equal(positions, picks), (positions, picks)
    n, H, W, C = stored.shape
    X = stored[order].reshape(-1, C).astype(np.float64)
    rows, rows32 = [], np.zeros((0, C), dtype=np.float32)
    for k, (e, p) in enumerate(picks):
        assert np.array_equal(spectra[k], X[e * H * W + p])
        v, ev = Um.extreme_reference(X[[e * H * W + p]], rows32, cache.cs)
        record_margin(f"atgp/C{C}/M{M}", abs(got[k] - v[0]) / ev[0], 1.0)
        assert abs(got[k] - v[0]) <= ev[0], (k, got[k], v[0], ev[0])
        rows.append(Um._atgp_row(X[e * H * W + p], rows))
        rows32 = np.stack(rows).astype(np.float32)
    return picks


@pytest.mark.parametrize("store_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("C,M", [(37, 4), (238, 8)])
def test_atgp_finds_the_planted_pixels(C, M, store_dtype):
    cubes, masks, planted, cache = _scene_cache(C, M, capacity=4, store_dtype=store_dtype)
    stored = _stored(cubes, store_dtype)
    picks = _check_atgp(cache, stored, masks, M)
    assert sorted(map(tuple, picks)) == sorted(map(tuple, planted))
    # a slot list in another order: positions count list entries
    _check_atgp(cache, stored, masks, M, slots=[2, 0])
    # foreground only, with the first pick masked out: it is not seen, and every pick is a masked pixel
    e, p = picks[0]
    masks2 = masks.copy()
    masks2.reshape(masks.shape[0], -1)[e, p] = 0
    cache2 = _cache(cubes, masks2, store_dtype=store_dtype)
    fg = _check_atgp(cache2, stored, masks2, M, select="foreground")
    assert (e, p) not in set(map(tuple, fg)) and all(masks2.reshape(masks.shape[0], -1)[a, b] for a, b in fg)
    # the winner duplicated at a later position loses to the earlier one; duplicated earlier, the duplicate wins
    n, H, W, _ = cubes.shape
    flat = cubes.reshape(n, H * W, C).copy()
    assert (e, p) not in ((n - 1, H * W - 1), (0, 0))
    flat[n - 1, H * W - 1] = flat[e, p]
    from hyperpri_amd import unmix as Um
    assert tuple(Um.extract_endmembers(_cache(flat.reshape(cubes.shape), masks, store_dtype=store_dtype), 1)[1][0]) == (e, p)
    flat[0, 0] = flat[e, p]
    assert tuple(Um.extract_endmembers(_cache(flat.reshape(cubes.shape), masks, store_dtype=store_dtype), 1)[1][0]) == (0, 0)


def test_atgp_on_a_grid_that_wraps():
    """2 cubes of 130 x 200: 814 tiles, more than two workgroups per CU."""
    C, M = 37, 4
    cubes, masks, planted = K.planted_scene(C, M, n=2, H=130, W=200)
    picks = _check_atgp(_cache(cubes, masks), cubes, masks, M)
    assert sorted(map(tuple, picks)) == sorted(map(tuple, planted))


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_fit_unmix_split_and_evaluate():
    import hyperpri_amd as H
    cubes, masks = K.root_scene()
    n = cubes.shape[0]
    cache = _cache(cubes, masks)
    model = H.SpectralUnmixer.fit(cache, 4, reference=H.class_spectra(cache))
    assert model.num_members == 4 and model.endmembers.device.type == "cuda" and bool(model.foreground.any())
    picks, _, gaps = H.atgp_reference(cubes, 4)
    assert (gaps > 0).all() and np.array_equal(model.meta.cpu().numpy().astype(np.int64), picks)
    pred = H.unmix_split(model, cache.epoch(batch_size=2, shuffle=False))
    assert len(pred) == n and pred.spread is None
    by_batch = torch.cat([model(bt, output="logit")[:, 0].reshape(-1).clone() for bt in cache.epoch(batch_size=2, shuffle=False)])
    assert pred.logits.cpu().numpy().tobytes() == by_batch.cpu().numpy().tobytes()
    assert torch.equal(pred.masks.cpu(), torch.from_numpy(masks.reshape(-1).astype(np.float32)))
    val = H.validate_net(pred)
    assert np.isfinite(val["avg_prec"]) and np.isfinite(val["dice_at_threshold"]) and np.isfinite(val["best_threshold"])
    test = H.test_net(pred, val["best_threshold"])
    assert sum(test["counts"][k] for k in ("tp", "fp", "fn", "tn")) == masks.size
    # the other constructors build and run
    two = H.SpectralUnmixer.from_class_spectra(cache)
    assert two.num_members == 2 and two.foreground.tolist() == [True, False]
    a = two(cache.batch([0, 1]))
    assert tuple(a.shape) == (2, 2) + masks.shape[1:] and bool(torch.isfinite(a).all())
    assert np.abs(a.sum(dim=1).cpu().numpy() - 1).max() <= 8 * U
    assert bool(torch.isfinite(two(cache.batch([0, 1]), output="logit")).all())
    km = H.SpectralKMeans.fit(cache, 3, seed=0)
    with pytest.raises(ValueError, match="calibrate"):
        H.SpectralUnmixer.from_kmeans(km)
    km.calibrate(cache)
    three = H.SpectralUnmixer.from_kmeans(km)
    assert three.num_members == 3 and three.foreground.tolist() == (km.foreground_share.cpu().numpy() > 0.5).tolist()
    r = three(cache.batch([2]), mode="ncls", output="rmse")
    assert tuple(r.shape) == (1, 1) + masks.shape[1:] and bool(torch.isfinite(r).all()) and float(r.min()) >= 0
    with pytest.raises(ValueError, match="no batches"):
        H.unmix_split(model, [])
