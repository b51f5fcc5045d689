"""Spectral statistics and projection on the device (hyperpri_amd/spectral.py, csrc/spectral.hip) against the numpy restatements of
their contract: exact on integer data (every fp32 partial sum stays below 2^24), within derived rounding bounds on real-valued
data, bit-reproducible, and end to end from a filled cache to a network that consumes the projected batch in place.
Needs a real MI355X: ``-m gpu``."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import record_margin
from oracle import hyperpri_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24                      # the unit roundoff of fp32
SELECTS = ("all", "foreground", "background")


def _int_cubes(seed, n, H, W, C):
    """n cubes of integers in [-4, 4] (exact in fp16 as well) and masks; slot 1 has no foreground pixel at all."""
    rng = np.random.RandomState(seed)
    cubes = rng.randint(-4, 5, size=(n, H, W, C)).astype(np.float32)
    masks = (rng.rand(n, H, W) < 0.45).astype(np.uint8)
    if n > 1:
        masks[1] = 0
    return cubes, masks


def _real_cubes(seed, n, H, W, C, rank=5):
    """Low-rank-plus-noise "reflectance": mean about 0.3, ``rank`` smooth components plus white noise."""
    rng = np.random.RandomState(seed)
    band = np.linspace(0.0, 1.0, C)
    comps = np.stack([np.cos(np.pi * (k + 1) * band) for k in range(rank)])
    amp = 0.08 * 0.6 ** np.arange(rank)
    x = 0.3 + 0.05 * np.sin(2 * np.pi * band) + (rng.randn(n, H, W, rank) * amp) @ comps + 0.004 * rng.randn(n, H, W, C)
    masks = (rng.rand(n, H, W) < 0.45).astype(np.uint8)
    return x.astype(np.float32), masks


def _cache(cubes, masks, capacity=None, store_dtype=torch.float32, unsqueeze=True, out_slots=2):
    from hyperpri_amd.cache import CubeCache
    n, H, W, C = cubes.shape
    cache = CubeCache(capacity or n, H, W, C, device=DEV, store_dtype=store_dtype, unsqueeze_hsi=unsqueeze, out_slots=out_slots)
    cache._cubes.fill_(float("nan"))                        # an unfilled slot must never be read
    for k in range(n):
        cache.put(k, cubes[k], masks[k], name=f"cube{k}")
    return cache


def _stored(cubes, store_dtype):
    return cubes.astype(np.float16) if store_dtype == torch.float16 else cubes


def _underlying(x, cs):
    x4 = x.squeeze(1) if x.dim() == 5 else x
    N, _, h, w = x4.shape
    return torch.as_strided(x4, (N, h, w, cs), (h * w * cs, w * cs, cs, 1))


# ---- exact-integer parity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [[2, 0], [0, 1, 2]])
@pytest.mark.parametrize("store_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("C", [3, 37, 238])
def test_moments_and_gram_are_exact_on_integers(C, store_dtype, order):
    from hyperpri_amd import spectral as S
    cubes, masks = _int_cubes(10 + C, 3, 13, 11, C)
    cache = _cache(cubes, masks, capacity=4, store_dtype=store_dtype)
    cs = cache.cs
    pivot = np.random.RandomState(C).randint(-2, 3, size=C).astype(np.float64)
    xs, ms = cubes[order].astype(np.int64), masks[order]
    for select in SELECTS:
        sel = np.ones(ms.shape, bool) if select == "all" else (ms != 0) if select == "foreground" else (ms == 0)
        rows = xs[sel]                                       # (P, C) int64
        n, sums = S.band_moments(cache, order, select)
        assert n == rows.shape[0] and sums.dtype == np.float64 and sums.shape == (cs,)
        assert np.array_equal(sums[:C], rows.sum(axis=0).astype(np.float64)) and not sums[C:].any()
        G = S.band_gram(cache, pivot, order, select)
        d = rows - pivot.astype(np.int64)
        assert G.dtype == np.float64 and G.shape == (cs, cs)
        assert np.array_equal(G[:C, :C], (d.T @ d).astype(np.float64))
        assert np.array_equal(G, G.T)                        # exactly symmetric
        assert not G[C:].any() and not G[:, C:].any()        # pad rows and columns are exactly zero
        # the references agree with the integer arithmetic, too
        assert np.array_equal(S.gram_reference(_stored(cubes, store_dtype)[order], pivot, ms, select), (d.T @ d).astype(np.float64))


def test_the_promotion_path_is_exact():
    """One slot of 2 * FP32_RUN + 37 pixels in one row: three runs, the last one short, each promoted from fp32 to fp64."""
    from hyperpri_amd import spectral as S
    assert S.fp32_run() == S.FP32_RUN
    W = 2 * S.FP32_RUN + 37
    cubes, masks = _int_cubes(5, 1, 1, W, 5)
    cache = _cache(cubes, masks)
    pivot = np.array([1, -2, 0, 2, -1], dtype=np.float64)
    for select in SELECTS:
        sel = np.ones(masks.shape, bool) if select == "all" else (masks != 0) if select == "foreground" else (masks == 0)
        rows = cubes.astype(np.int64)[sel]
        n, sums = S.band_moments(cache, None, select)
        assert n == rows.shape[0] and np.array_equal(sums[:5], rows.sum(axis=0).astype(np.float64))
        d = rows - pivot.astype(np.int64)
        G = S.band_gram(cache, pivot, None, select)
        assert np.array_equal(G[:5, :5], (d.T @ d).astype(np.float64)) and np.array_equal(G, G.T) and not G[5:].any()


def test_runs_wrap_around_the_partial_accumulators():
    """More runs than either pass has partial accumulators (2048 and 256): a partial then adds several runs, in run order."""
    from hyperpri_amd import spectral as S
    W = 2049 * S.FP32_RUN + 37
    cubes, masks = _int_cubes(6, 1, 1, W, 5)
    cache = _cache(cubes, masks)
    pivot = np.array([0, 1, -1, 2, -2], dtype=np.float64)
    rows = cubes.astype(np.int64)[masks != 0]
    n, sums = S.band_moments(cache, None, "foreground")
    assert n == rows.shape[0] and np.array_equal(sums[:5], rows.sum(axis=0).astype(np.float64))
    d = rows - pivot.astype(np.int64)
    G = S.band_gram(cache, pivot, None, "foreground")
    assert np.array_equal(G[:5, :5], (d.T @ d).astype(np.float64)) and np.array_equal(G, G.T) and not G[5:].any()


@pytest.mark.parametrize("K", [1, 8, 33, 64])
@pytest.mark.parametrize("C", [3, 37, 238])
def test_projection_is_exact_on_integers(C, K):
    from hyperpri_amd import spectral as S
    cubes, masks = _int_cubes(20 + C, 3, 13, 11, C)
    rng = np.random.RandomState(100 * C + K)
    Wt = rng.randint(-3, 4, size=(K, C)).astype(np.float32)
    b = rng.randint(-5, 6, size=K).astype(np.float32)
    proj = S.SpectralProjection(Wt, b).to(DEV)
    ks = (K + 7) // 8 * 8
    want = S.project_reference(cubes[[2, 0]], Wt, b)         # (2, 13, 11, K) fp64, every |y| < 2^24
    assert np.abs(want).max() < 2 ** 24
    for unsqueeze in (True, False):
        cache = _cache(cubes, masks, unsqueeze=unsqueeze)
        batch = cache.batch([2, 0])
        y = proj(batch["image"])
        assert tuple(y.shape) == ((2, 1, K, 13, 11) if unsqueeze else (2, K, 13, 11)) and y.dtype == torch.float32
        assert getattr(y, "_hpri_zero_padded", False)
        under = _underlying(y, ks).cpu().numpy()
        assert np.array_equal(under[..., :K].astype(np.float64), want)
        assert not under[..., K:].any() and not np.signbit(under[..., K:]).any()        # pad channels are exactly +0.0
    # the slow path: a plain NCHW tensor goes through one layout pass and the pad
    x = torch.from_numpy(np.ascontiguousarray(cubes[[2, 0]].transpose(0, 3, 1, 2))).to(DEV)
    y = proj(x)
    assert tuple(y.shape) == (2, K, 13, 11)
    assert np.array_equal(y.permute(0, 2, 3, 1).cpu().numpy().astype(np.float64), want)


@pytest.mark.parametrize("C", [3, 37, 238])
def test_affine_is_exact_on_integers(C):
    from hyperpri_amd import spectral as S
    cubes, masks = _int_cubes(30 + C, 3, 13, 11, C)
    rng = np.random.RandomState(C)
    s = rng.randint(-3, 4, size=C).astype(np.float32)
    t = rng.randint(-5, 6, size=C).astype(np.float32)
    proj = S.SpectralProjection(s, t).to(DEV)
    cache = _cache(cubes, masks)
    y = proj(cache.batch([1, 2]))["image"]
    assert tuple(y.shape) == (2, 1, C, 13, 11) and getattr(y, "_hpri_zero_padded", False)
    under = _underlying(y, cache.cs).cpu().numpy()
    assert np.array_equal(under[..., :C].astype(np.float64), S.project_reference(cubes[[1, 2]], s, t))
    assert not under[..., C:].any()


# ---- real-valued parity against fp64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("store_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("C", [37, 238])
def test_moments_and_gram_within_the_derived_bound(C, store_dtype):
    """|G_dev - G_64| <= ((FP32_RUN + 4) u + 1e-12) |D|^T |D| elementwise, D = X - pivot in fp64: one rounding for the subtraction,
    one per product, gamma_n for an fp32 sum of FP32_RUN terms in any order; sums: (FP32_RUN u + 1e-12) sum |x|."""
    from hyperpri_amd import spectral as S
    cubes, masks = _real_cubes(C, 3, 13, 11, C)
    cache = _cache(cubes, masks, capacity=4, store_dtype=store_dtype)
    q = _stored(cubes, store_dtype)
    name = "f16" if store_dtype == torch.float16 else "f32"
    for select in SELECTS:
        n, sums = S.band_moments(cache, [0, 1, 2], select)
        n_ref, sums_ref = S.moments_reference(q, masks, select)
        assert n == n_ref
        rows = S._selected_pixels(q, masks, select)
        tol = (S.FP32_RUN * U + 1e-12) * np.abs(rows).sum(axis=0)
        err = np.abs(sums[:C] - sums_ref)
        record_margin(f"spectral/sums/{name}/C{C}/{select}", (err / tol).max(), 1.0)
        assert (err <= tol).all() and not sums[C:].any()
        pivot = (sums_ref / n).astype(np.float32)
        G = S.band_gram(cache, pivot, [0, 1, 2], select)
        G_ref = S.gram_reference(q, pivot, masks, select)
        D = np.abs(rows - pivot.astype(np.float64))
        tol = ((S.FP32_RUN + 4) * U + 1e-12) * (D.T @ D)
        err = np.abs(G[:C, :C] - G_ref)
        record_margin(f"spectral/gram/{name}/C{C}/{select}", (err / tol).max(), 1.0)
        assert (err <= tol).all()
        assert np.array_equal(G, G.T) and not G[C:].any() and not G[:, C:].any()


@pytest.mark.parametrize("C,K", [(37, 6), (37, 33), (238, 32), (238, 64)])
def test_projection_and_affine_within_the_derived_bound(C, K):
    """|y - y_64| <= (cs + 1) u (|b| + |W| |x|): a chain of cs fused multiply-adds, one rounding each; affine: one fmaf, 2 u."""
    from hyperpri_amd import spectral as S
    cubes, masks = _real_cubes(7 * C + K, 2, 13, 11, C)
    cache = _cache(cubes, masks)
    rng = np.random.RandomState(K)
    Wt = (rng.randn(K, C) / np.sqrt(C)).astype(np.float32)
    b = rng.randn(K).astype(np.float32)
    x = cache.batch([1, 0])["image"]
    y = S.SpectralProjection(Wt, b).to(DEV)(x)
    got = _underlying(y, (K + 7) // 8 * 8).cpu().numpy()[..., :K].astype(np.float64)
    want = S.project_reference(cubes[[1, 0]], Wt, b)
    tol = (cache.cs + 1) * U * (np.abs(b.astype(np.float64)) + np.abs(cubes[[1, 0]].astype(np.float64)) @ np.abs(Wt.astype(np.float64)).T)
    err = np.abs(got - want)
    record_margin(f"spectral/project/C{C}/K{K}", (err / tol).max(), 1.0)
    assert (err <= tol).all()
    s = (1.0 + rng.rand(C)).astype(np.float32)
    t = rng.randn(C).astype(np.float32)
    ya = S.SpectralProjection(s, t).to(DEV)(x)
    got = _underlying(ya, cache.cs).cpu().numpy()[..., :C].astype(np.float64)
    xs = cubes[[1, 0]].astype(np.float64)
    tol = 2 * U * (np.abs(xs * s) + np.abs(t.astype(np.float64)))
    err = np.abs(got - S.project_reference(xs, s, t))
    record_margin(f"spectral/affine/C{C}", (err / tol).max(), 1.0)
    assert (err <= tol).all()


# ---- determinism -----------------------------------------------------------------------------------------------------
def test_band_statistics_is_bit_reproducible():
    from hyperpri_amd import spectral as S
    cubes, masks = _real_cubes(3, 3, 13, 11, 238)
    cache = _cache(cubes, masks)
    for select in ("all", "foreground"):
        a, b = S.band_statistics(cache, select=select), S.band_statistics(cache, select=select)
        assert a.count == b.count and a.mean.tobytes() == b.mean.tobytes() and a.cov.tobytes() == b.cov.tobytes()
    ref = S.statistics_reference(cubes, masks, "all")
    st = S.band_statistics(cache)
    assert st.count == ref.count and np.allclose(st.mean, ref.mean, rtol=1e-5) and np.allclose(st.cov, ref.cov, rtol=1e-3, atol=1e-9)
    spectra = S.class_spectra(cache)
    for name in ("foreground", "background"):
        r = S.statistics_reference(cubes, masks, name)
        assert spectra[name]["count"] == r.count
        assert np.allclose(spectra[name]["mean"], r.mean, rtol=1e-5) and np.allclose(spectra[name]["std"], r.std(), rtol=1e-3)


# ---- end to end ------------------------------------------------------------------------------------------------------
def _tiny_cubenet():
    import hyperpri_amd as H
    net = H.CubeNET(6, 1, first_depth=64, bilinear=False)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())
    net.load_state_dict(O.synth_state_dict(shapes))
    return net.to(DEV).train()


def _perturbed_cov_tolerance(E_cov, Wa, e_hat, yc, n):
    """How far the covariance of device outputs y = W x + b may lie from W cov_dev W^T, elementwise: ``|W| E |W|^T`` for the error E of
    the device covariance itself (W cov_true W^T = W cov_dev W^T - W E W^T) plus what per-pixel output errors |e_p| <= e_hat do to
    a covariance, sum_p (e_i |yc_j| + |yc_i| e_j + 2 e_i e_j) / (n - 1) (the centring of e only lowers the cross terms; the factor
    2 covers its own mean)."""
    return Wa @ E_cov @ Wa.T + (e_hat.T @ np.abs(yc) + np.abs(yc).T @ e_hat + 2 * e_hat.T @ e_hat) / (n - 1)


def test_fit_project_and_feed_a_network():
    import hyperpri_amd as H
    from hyperpri_amd import spectral as S
    C, k = 19, 6
    cubes, masks = _real_cubes(42, 3, 36, 50, C)
    cache = _cache(cubes, masks, capacity=4)
    with pytest.raises(IndexError):
        S.band_statistics(cache, slots=[0, 3])               # an unfilled slot
    stats = S.band_statistics(cache)
    proj = S.SpectralProjection.pca(stats, k).to(DEV)
    batch = cache.batch([2, 0])
    mask_before, image_before = batch["mask"].clone(), batch["image"].clone()
    out = proj(batch)
    y = out["image"]
    assert getattr(y, "_hpri_zero_padded", False) and tuple(y.shape) == (2, 1, k, 36, 50)
    assert out["mask"] is batch["mask"] and out["index"] == ["cube2", "cube0"] and torch.equal(out["mask"], mask_before)
    assert torch.equal(batch["image"], image_before)         # the input batch is left alone
    net = _tiny_cubenet()
    a = net(y).detach().clone()
    b = net(y.contiguous()).detach().clone()
    assert torch.equal(a, b)                                 # consumed in place: the same bits as from a contiguous copy
    # an input that requires grad raises, and so does a basis beyond the kernel's K
    with pytest.raises(RuntimeError, match="autograd"):
        proj(batch["image"].clone().requires_grad_(True))
    with pytest.raises(ValueError, match="exceeds"):
        S.SpectralProjection(np.zeros((S.project_max_k() + 1, C), np.float32), np.zeros(S.project_max_k() + 1, np.float32))
    # the state dict carries the basis
    again = S.SpectralProjection(np.zeros((k, C)), np.zeros(k)).to(DEV)
    again.load_state_dict(proj.state_dict())
    assert torch.equal(again(batch)["image"], y)

    # the projected training pixels have the covariance diag(explained variance), up to the derived bound
    X = cubes.reshape(-1, C).astype(np.float64)
    n = X.shape[0]
    ys = np.concatenate([_underlying(proj(cache.batch([i]))["image"], 8).cpu().numpy()[..., :k].reshape(-1, k) for i in range(3)]).astype(np.float64)
    got = S.statistics_reference(ys[None, None])
    gamma = (S.FP32_RUN + 4) * U + 1e-12
    D = np.abs(X - stats.mean.astype(np.float32).astype(np.float64))
    E_cov = gamma * (D.T @ D) / (n - 1)
    # (the device mean enters through n d d^T: its error bound dm, against |d| <= u |mean|)
    dm = S.FP32_RUN * U * np.abs(X).sum(axis=0) / n
    da = U * np.abs(stats.mean)
    E_cov = E_cov + (np.outer(da, dm) + np.outer(dm, da) + np.outer(dm, dm)) * n / (n - 1)
    W64, b64 = proj.weight.cpu().numpy().astype(np.float64), proj.bias.cpu().numpy().astype(np.float64)
    Wa = np.abs(W64)
    e_hat = (cache.cs + 2) * U * (np.abs(b64) + np.abs(X) @ Wa.T)       # the chain, plus the basis' own rounding to fp32
    yc = ys - ys.mean(axis=0)
    tol = _perturbed_cov_tolerance(E_cov, Wa, e_hat, yc, n) + 1e-12 * np.abs(stats.cov).max()
    err = np.abs(got.cov - np.diag(proj.explained_variance))
    record_margin("spectral/e2e/pca_cov", (err / tol).max(), 1.0)
    assert (err <= tol).all()
    mean_tol = e_hat.mean(axis=0) + Wa @ (S.FP32_RUN * U * np.abs(X).sum(axis=0) / n)
    record_margin("spectral/e2e/pca_mean", (np.abs(got.mean) / mean_tol).max(), 1.0)
    assert (np.abs(got.mean) <= mean_tol).all()

    # standardised bands: mean 0 and variance 1 under the same bound
    eps = 1e-6
    z = S.SpectralProjection.standardize(stats, eps=eps).to(DEV)
    zs = np.concatenate([_underlying(z(cache.batch([i]))["image"], cache.cs).cpu().numpy()[..., :C].reshape(-1, C) for i in range(3)]).astype(np.float64)
    gz = S.statistics_reference(zs[None, None])
    s64, t64 = z.weight.cpu().numpy().astype(np.float64), z.bias.cpu().numpy().astype(np.float64)
    e_hat = 3 * U * (np.abs(X * s64) + np.abs(t64))          # one fmaf (2 u as above), plus s and t rounded to fp32
    zc = zs - zs.mean(axis=0)
    var_tol = (np.diag(E_cov) + eps) * s64 ** 2 + (2 * (e_hat * np.abs(zc)).sum(axis=0) + 2 * (e_hat ** 2).sum(axis=0)) / (n - 1)
    err = np.abs(np.diag(gz.cov) - 1.0)
    record_margin("spectral/e2e/standardize_var", (err / var_tol).max(), 1.0)
    assert (err <= var_tol).all()
    mean_tol = e_hat.mean(axis=0) + s64 * (S.FP32_RUN * U * np.abs(X).sum(axis=0) / n)
    record_margin("spectral/e2e/standardize_mean", (np.abs(gz.mean) / mean_tol).max(), 1.0)
    assert (np.abs(gz.mean) <= mean_tol).all()
