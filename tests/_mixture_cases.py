"""Inputs of the spectral Gaussian mixture tests, shared by the CPU tests (which check the conditions the GPU tests rely on) and the
GPU tests.

``ladder_scene``: the masks of ``blob_scene`` with five materials on one spectral line -- soils at 0, 2 and 4 steps, roots at 1 and 3 --
so that no single Gaussian per class separates roots from soil and no single target spectrum does, while a mixture per class does.
``model_case``: a random model (projection, components, classes) with pixels drawn around its components, for the real-valued parity
tests.  ``int_case``: integer operands on which every intermediate of the contract is an integer or a half below 2^23."""
import numpy as np

import _guided_cases as G

SLOT = (47, 53)             # as _cluster_cases.SLOT: 2491 pixels, two runs of 2048 and a ragged tail
LADDER = {"C": 19, "noise": 0.07, "step": 0.06, "q": 4, "fit": (0, 1), "held_out": 2, "seed": 7}
# (C, q, K, classes) of the real-valued score test
SCORE_CASES = ((20, 1, 1, 1), (37, 5, 3, 2), (238, 16, 8, 2), (238, 32, 8, 8), (313, 32, 8, 2))
# the real-valued sums test
SUMS = {"C": 238, "q": 16, "K": 8, "n": 3}


def _rup(a, m):
    return (a + m - 1) // m * m


# ---- the ladder ------------------------------------------------------------------------------------------------------
def ladder_scene():
    """``(cubes (3, 36, 50, 19) fp32, masks uint8, material (3, 36, 50) in 0..4)``: material j has the spectrum ``soil + j step v``
    with ``v = 1 + cos(3 band)``, the offset of ``blob_scene``'s root; background pixels draw a soil (0, 2, 4), foreground pixels a root (1, 3); white noise on top."""
    L = LADDER
    _, masks = G.blob_scene(C=L["C"])
    rng = np.random.RandomState(L["seed"])
    material = np.where(masks != 0, 1 + 2 * rng.randint(0, 2, size=masks.shape), 2 * rng.randint(0, 3, size=masks.shape))
    spectra = ladder_spectra()
    cubes = spectra[material] + L["noise"] * rng.randn(*masks.shape, L["C"])
    return cubes.astype(np.float32), masks, material


def ladder_spectra():
    band = np.linspace(0.0, 1.0, LADDER["C"])
    return (0.3 + 0.1 * np.sin(2 * np.pi * band))[None, :] + LADDER["step"] * np.arange(5)[:, None] * (1.0 + np.cos(3.0 * band))[None, :]


def ladder_inits(cubes, masks, pivot, weight, components):
    """The planted init of ``fit_classes(components)``: per class the planted spectra, displaced by 0.03 N(0, 1) per band (about half
    the noise radius), projected; covariances and weights from the nearest-mean assignment of the class's fitting pixels.  With one
    component the start is the class's first spectrum (one pass gives the moments whatever the start)."""
    from hyperpri_amd.mixture import hard_init
    L = LADDER
    rng = np.random.RandomState(L["seed"] + 1)
    spectra = ladder_spectra() + 0.03 * rng.randn(5, L["C"])
    W, pv = np.asarray(weight, np.float64), np.asarray(pivot, np.float64)
    x = cubes[list(L["fit"])].reshape(-1, L["C"]).astype(np.float64)
    m = masks[list(L["fit"])].reshape(-1) != 0
    out = []
    for cls, (members, sel) in enumerate((((0, 2, 4), ~m), ((1, 3), m))):
        k = components[cls]
        assert k in (1, len(members))
        means = (spectra[list(members[:k])] - pv) @ W.T
        out.append(hard_init((x[sel] - pv) @ W.T, means))
    return out


def best_dice(logit, mask):
    """The largest Dice of ``logit > t`` over every threshold t."""
    order = np.argsort(-np.asarray(logit, np.float64).reshape(-1), kind="stable")
    m = (np.asarray(mask).reshape(-1) != 0)[order]
    tp = np.cumsum(m)
    return float((2.0 * tp / (np.arange(1, len(m) + 1) + m.sum())).max())


# ---- random models ---------------------------------------------------------------------------------------------------
def model_case(C, q, K, classes, n=1, H=SLOT[0], W=SLOT[1], seed=None):
    """A projection with rows of norm about 3, K components with means N(0, 1.5^2) and random covariances with eigenvalues in
    [0.3, 1.5], classes dealt round-robin, pixels ``pivot + pinv(W) (m_k + L_k N(0, 1)) + 0.01 N(0, 1)`` of a random component, and
    masks: ``(cubes (n, H, W, C) fp32, masks, dict(pivot, weight, means, covariances, weights, classes))``."""
    rng = np.random.RandomState(1000 * C + 10 * q + K if seed is None else seed)
    weight = (3.0 * rng.randn(q, C) / np.sqrt(C)).astype(np.float32)
    pivot = rng.uniform(0.2, 0.8, size=C).astype(np.float32)
    means = 1.5 * rng.randn(K, q)
    cov = np.zeros((K, q, q))
    for k in range(K):
        R = np.linalg.qr(rng.randn(q, q))[0]
        cov[k] = (R * rng.uniform(0.3, 1.5, size=q)) @ R.T
    pi = rng.uniform(0.5, 1.5, size=K)
    pi /= pi.sum()
    cls = np.arange(K) % classes
    comp = rng.randint(0, K, size=(n, H, W))
    L = np.linalg.cholesky(cov)
    zz = means[comp] + np.einsum("...ij,...j->...i", L[comp], rng.randn(n, H, W, q))
    x = pivot + zz @ np.linalg.pinv(weight.astype(np.float64)).T + 0.01 * rng.randn(n, H, W, C)
    masks = (rng.rand(n, H, W) < 0.45).astype(np.uint8)
    return x.astype(np.float32), masks, {"pivot": pivot, "weight": weight, "means": means, "covariances": cov, "weights": pi, "classes": cls}


# ---- integers --------------------------------------------------------------------------------------------------------
def int_case(C, K=4, q=5, seed=0):
    """Integer operands: ``weight`` rows of 0 / +-1 with at most 8 non-zeros, integer lower-triangular ``A_k`` with entries in [-2, 2]
    and a unit diagonal, integer ``a_k``, ``c = 0``, every component its own class.  Component 1 mirrors component 0 in u[0] (the row
    and its offset negated: the same m for every pixel), the last repeats component 0: ties that must go to the lowest class.  With
    |d| <= 5: |z| <= 40, |u| <= 2 * 40 * 5 + 3 < 2^9, m < 5 * 2^18 < 2^23, l = -m / 2 a multiple of 1/2."""
    rng = np.random.RandomState(100 * C + seed)
    weight = np.zeros((q, C), dtype=np.float32)
    for i in range(q):
        cols = rng.choice(C, size=min(C, 8), replace=False)
        weight[i, cols] = rng.choice([-1.0, 1.0], size=len(cols))
    A = np.tril(rng.randint(-2, 3, size=(K, q, q))).astype(np.float32)
    A[:, np.arange(q), np.arange(q)] = 1.0
    a = rng.randint(-3, 4, size=(K, q)).astype(np.float32)
    A[1], a[1] = A[0], a[0]
    A[1, 0], a[1, 0] = -A[0, 0], -a[0, 0]
    A[K - 1], a[K - 1] = A[0], a[0]
    pivot = rng.randint(0, 2, size=C).astype(np.float32)
    return {"pivot": pivot, "weight": weight, "A": A, "a": a, "c": np.zeros(K, np.float32), "classes": np.arange(K)}


def int_reference(pixels, case):
    """int64: ``(z (P, q), m (P, K), labels (P,))`` -- the lowest component at the least m."""
    d = pixels.astype(np.int64) - case["pivot"].astype(np.int64)
    z = d @ case["weight"].astype(np.int64).T
    u = np.einsum("kij,pj->pki", case["A"].astype(np.int64), z) + case["a"].astype(np.int64)[None]
    m = (u * u).sum(axis=2)
    return z, m, np.argmin(m, axis=1)
