"""Inputs of the spectral k-means tests, shared by the CPU tests (which check the conditions the GPU tests rely on) and the GPU tests.

``uniform``: pixels U[0, 1) fp32, centroids ``base + 0.15 N(0, 1)`` with ``base`` ~ U[0.2, 0.8] per band, ``pivot = fp32(mean of the
pixels)``.  No structure: every pixel has many centroids at similar distances, so a few are closer than the rounding bound.
``mixture``: a centroid plus ``noise * N(0, 1)``: well separated, the reference flags no pixel."""
import numpy as np

SLOT = (47, 53)             # 2491 pixels: two runs of 2048, a tail that is neither a multiple of 16 nor of the run
# (C, K) of the real-valued GPU tests on ``uniform`` data, three slots each
UNIFORM_CASES = ((20, 3), (238, 8), (238, 64), (300, 33))
# the end-to-end fit: C, K, slots, noise, seed (test_cluster_cpu holds that kmeans_reference meets no ambiguous pixel on it)
E2E = {"C": 37, "K": 5, "n": 3, "H": 36, "W": 50, "noise": 0.05, "seed": 11}
# the fitting pass on real values (test 5): C, K, noise, seed
SUMS = {"C": 238, "K": 8, "n": 3, "noise": 0.05, "seed": 5}


def _centroids(rng, C, K):
    return rng.uniform(0.2, 0.8, size=C)[None, :] + 0.15 * rng.randn(K, C)


def _finish(x, masks, centroids):
    pivot = x.reshape(-1, x.shape[-1]).astype(np.float64).mean(axis=0).astype(np.float32)
    centers = (centroids - pivot.astype(np.float64)).astype(np.float32)
    return {"cubes": x, "masks": masks, "centroids": centroids, "pivot": pivot, "centers": centers}


def uniform(seed, n, H, W, C, K):
    rng = np.random.RandomState(seed)
    x = rng.rand(n, H, W, C).astype(np.float32)
    centroids = _centroids(rng, C, K)
    masks = (rng.rand(n, H, W) < 0.45).astype(np.uint8)
    return _finish(x, masks, centroids)


def mixture(seed, n, H, W, C, K, noise=0.05):
    """Also ``truth`` (n, H, W): the component of every pixel; the mask is ``truth == 0``."""
    rng = np.random.RandomState(seed)
    centroids = _centroids(rng, C, K)
    truth = rng.randint(0, K, size=(n, H, W))
    x = (centroids[truth] + noise * rng.randn(n, H, W, C)).astype(np.float32)
    out = _finish(x, (truth == 0).astype(np.uint8), centroids)
    out["truth"] = truth
    return out


def uniform_case(C, K):
    return uniform(1000 * C + K, 3, SLOT[0], SLOT[1], C, K)


def e2e_case():
    e = E2E
    case = mixture(e["seed"], e["n"], e["H"], e["W"], e["C"], e["K"], e["noise"])
    # the explicit init: the planted centroids, displaced by about half the noise radius
    case["init"] = case["centroids"] + 0.03 * np.random.RandomState(e["seed"] + 1).randn(e["K"], e["C"])
    return case


def sums_case():
    s = SUMS
    return mixture(s["seed"], s["n"], SLOT[0], SLOT[1], s["C"], s["K"], s["noise"])
