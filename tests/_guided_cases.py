"""The data of the guided-filter tests (tests/test_guided_cpu.py and tests/test_gpu_guided.py): seeded and small.  The CPU tests assert
on the reference what the GPU tests rely on -- that the bound covers an fp32 emulation of the device on every bounded case (so it is
not vacuous before a GPU sees it), that the scene of the end-to-end test has a noisy map and a guide that shows the objects."""
import numpy as np

TILE_H, TILE_W = 16, 32                 # hpri_guided_tile_h / _w (test_guided_cpu.py asserts that the library says the same)
# 1x1; smaller than any window; one less and one more than the tile in each direction; several tiles; a batch
FRAMES = ((1, 1, 1), (1, 3, 5), (1, TILE_H - 1, TILE_W - 1), (1, TILE_H + 1, TILE_W + 1), (1, 37, 130), (3, TILE_H + 1, TILE_W + 1))
KS, RADII, TS, STRIDES, DOMAINS = (1, 2, 3), (1, 2, 4, 8), (1, 2, 5), (1, 3, 8), ("linear", "prob")


def bounded_cases():
    """Every combination of K, r and T, each with a channel stride, a domain and a frame drawn so that all of them occur, then the
    offset guide (1000 + 0.01 U, r = 2, eps = 1e-6: the trial that motivated the centring) with one and with three channels:
    ``(name, K, r, T, gs, domain, (N, h, w), eps, offset)``."""
    out = []
    for ki, K in enumerate(KS):
        for ri, r in enumerate(RADII):
            for ti, T in enumerate(TS):
                strides = [g for g in STRIDES if g >= K]
                gs = strides[(ri + ti) % len(strides)]
                domain = DOMAINS[(ki + ri + ti) % 2]
                frame = FRAMES[(ki + 2 * ri + 3 * ti) % len(FRAMES)]
                eps = (1e-2, 1e-3, 1e-1)[(ki + ti) % 3]
                out.append((f"K{K}-r{r}-T{T}-gs{gs}-{domain}-{'x'.join(map(str, frame))}", K, r, T, gs, domain, frame, eps, False))
    out.append(("offset-K1", 1, 2, 1, 1, "linear", (1, 37, 130), 1e-6, True))
    out.append(("offset-K3", 3, 2, 2, 8, "prob", (1, TILE_H + 1, TILE_W + 1), 1e-6, True))
    return out


def real_guide(N, K, h, w, seed=0, offset=False):
    """(N, K, h, w) fp32: smooth structure of order one plus noise; ``offset``: 1000 + 0.01 U(0, 1), a mean 1e5 times the variation."""
    rng = np.random.RandomState(100 + seed)
    if offset:
        return (1000.0 + 0.01 * rng.rand(N, K, h, w)).astype(np.float32)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([np.sin(0.3 * y + 0.2 * (k + 1) * x + k) + (x > w // 2) * (0.5 + k) for k in range(K)])
    return (base[None] + 0.3 * rng.randn(N, K, h, w)).astype(np.float32)


def real_maps(N, T, h, w, domain, seed=0):
    """(N, T, h, w) fp32: noisy probabilities in (0, 1) (linear), or logits N(0, 2^2) (prob)."""
    rng = np.random.RandomState(200 + seed)
    if domain == "prob":
        return (2.0 * rng.randn(N, T, h, w)).astype(np.float32)
    return rng.rand(N, T, h, w).astype(np.float32)


def case_data(case):
    name, K, r, T, gs, domain, (N, h, w), eps, offset = case
    seed = sum(map(ord, name))
    return real_guide(N, K, h, w, seed, offset), real_maps(N, T, h, w, domain, seed)


def int_frame(N, C, h, w, seed=0):
    """(N, C, h, w) fp32 integers in [-4, 4]: every centred window sum is an integer below 2^24, in any order."""
    return np.random.RandomState(300 + seed).randint(-4, 5, size=(N, C, h, w)).astype(np.float32)


def box_mean(X, r):
    """The mean over the clipped (2r+1)^2 window of an (N, ..., h, w) array, by summed-area differences in X's dtype."""
    h, w = X.shape[-2:]
    c = np.zeros(X.shape[:-2] + (h + 1, w + 1), dtype=X.dtype)
    c[..., 1:, 1:] = X.cumsum(axis=-2, dtype=X.dtype).cumsum(axis=-1, dtype=X.dtype)
    y0, y1 = np.maximum(np.arange(h) - r, 0), np.minimum(np.arange(h) + r + 1, h)
    x0, x1 = np.maximum(np.arange(w) - r, 0), np.minimum(np.arange(w) + r + 1, w)
    s = c[..., y1[:, None], x1[None, :]] - c[..., y0[:, None], x1[None, :]] - c[..., y1[:, None], x0[None, :]] + c[..., y0[:, None], x0[None, :]]
    n = ((y1 - y0)[:, None] * (x1 - x0)[None, :]).astype(X.dtype)
    return s / n


def classical(guide, maps, r, eps, dtype=np.float64):
    """The published algorithm in its moment form, uncentred: ``cov = E[I p] - E[I] E[p]``, ``var = E[I I^T] - E[I] E[I]^T``,
    ``a = (var + eps)^-1 cov``, ``b = E[p] - a . E[I]``, ``q = E[a] . I + E[b]``, every mean a clipped box mean, all of it in
    ``dtype``.  (N, K, h, w) and (N, T, h, w) -> q (N, T, h, w)."""
    I, p = np.asarray(guide).astype(dtype), np.asarray(maps).astype(dtype)
    K = I.shape[1]
    mI, mp = box_mean(I, r), box_mean(p, r)
    var = box_mean(I[:, :, None] * I[:, None, :], r) - mI[:, :, None] * mI[:, None, :]                  # (N, K, K, h, w)
    cov = box_mean(I[:, None, :] * p[:, :, None], r) - mI[:, None, :] * mp[:, :, None]                  # (N, T, K, h, w)
    A = var.transpose(0, 3, 4, 1, 2) + dtype(eps) * np.eye(K, dtype=dtype)
    a = np.linalg.solve(A[:, None], cov.transpose(0, 1, 3, 4, 2)[..., None])[..., 0].astype(dtype)      # (N, T, h, w, K)
    a = a.transpose(0, 1, 4, 2, 3)
    b = mp - (a * mI[:, None]).sum(axis=2)
    return ((box_mean(a, r) * I[:, None]).sum(axis=2) + box_mean(b, r)).astype(np.float64)


def step_scene(h=24, w=40, seed=0):
    """A guide that is 0 left and 1 right of the middle column, and a map that is the same step plus N(0, 0.2^2) noise."""
    rng = np.random.RandomState(400 + seed)
    step = (np.arange(w) >= w // 2).astype(np.float32)[None, :].repeat(h, axis=0)
    return step[None, None].copy(), (step + 0.2 * rng.randn(h, w)).astype(np.float32)[None, None]


def periodic(N, C, h, w, period=(5, 7), seed=0):
    """(N, C, h, w) fp32 with ``X[y, x] = X[y % 5, x % 7]``: periods coprime to the tile's 16 and 32."""
    base = np.random.RandomState(500 + seed).rand(N, C, period[0], period[1]).astype(np.float32)
    y, x = np.arange(h) % period[0], np.arange(w) % period[1]
    return np.ascontiguousarray(base[:, :, y[:, None], x[None, :]])


def blob_scene(C=19, n=3, H=36, W=50, noise=0.1, seed=0):
    """n cubes (n, H, W, C) of a smooth soil spectrum, brighter rectangles and 3-pixel stripes of a second spectrum (the mask) and white
    noise strong enough that a per-pixel detector errs: ``(cubes fp32, masks uint8)``."""
    rng = np.random.RandomState(600 + seed)
    band = np.linspace(0.0, 1.0, C)
    soil = 0.3 + 0.1 * np.sin(2 * np.pi * band)
    root = soil + 0.06 * (1.0 + np.cos(3.0 * band))
    masks = np.zeros((n, H, W), dtype=np.uint8)
    for k in range(n):
        for _ in range(3):
            y, x = rng.randint(0, H - 10), rng.randint(0, W - 12)
            masks[k, y:y + rng.randint(6, 10), x:x + rng.randint(6, 12)] = 1
        c = rng.randint(5, W - 8)
        masks[k, :, c:c + 3] = 1
    cubes = np.where(masks[..., None] != 0, root, soil) + noise * rng.randn(n, H, W, C)
    return cubes.astype(np.float32), masks


def best_dice(prob, masks, thresholds=500):
    """The best Dice over ``thresholds`` equally spaced thresholds of a probability map, as ``validate_net`` searches."""
    p, m = np.asarray(prob).reshape(-1), np.asarray(masks).reshape(-1) != 0
    best = 0.0
    for t in np.linspace(0.0, 1.0, thresholds + 1)[:-1]:
        d = p > t
        tp = (d & m).sum()
        best = max(best, 2.0 * tp / max(d.sum() + m.sum(), 1))
    return best
