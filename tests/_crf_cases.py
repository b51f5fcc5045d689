"""The data of the dense-CRF tests (tests/test_crf_cpu.py and tests/test_gpu_crf.py): seeded and small.  The CPU tests assert on the
reference what the GPU tests rely on -- that the bound covers an fp32 emulation of the device on every bounded case and that single
mutations of the contract break it, that the scene of the end-to-end test is repaired by the CRF, that the multi-class case leaves
fewer than 1 % of its pixels undecided.  A case's reference and bound are computed once and shared (``reference``, ``bound``)."""
import functools

import numpy as np

import _guided_cases as G

TILE_H, TILE_W = 16, 32                 # hpri_crf_tile_h / _w (test_crf_cpu.py asserts that the library says the same)
FRAMES = G.FRAMES                       # 1x1; smaller than any window; around the tile; several tiles; a batch
KS, RADII, CS, STRIDES, ITERS = (0, 1, 2, 3), (1, 2, 4, 8), (2, 3, 8), (3, 8), (1, 2, 5)
SCENE = dict(radius=3, iterations=5, theta_alpha=2.0, theta_beta=1.0, theta_gamma=1.0, w_appearance=4.0, w_smooth=1.0)
INF = float("inf")


def compat(C):
    """A non-symmetric compatibility matrix: -1 on the diagonal, 0.1, 0.2 or 0.3 off it, mu(l, l') != mu(l', l) somewhere."""
    l, k = np.mgrid[0:C, 0:C]
    return np.where(l == k, -1.0, 0.1 * (1 + (l + 2 * k) % 3)).astype(np.float32)


def bounded_cases():
    """Every combination of K, r and C, each with a guide stride out of {K, 3, 8}, a number of iterations, a frame, Potts or the
    non-symmetric mu, binary or two-plane input (C = 2) and a set of scales drawn so that all of them occur:
    ``(name, K, r, C, gs, T, (N, h, w), binary, potts, kw)`` with ``kw`` the thetas and weights."""
    out = []
    for ki, K in enumerate(KS):
        for ri, r in enumerate(RADII):
            for ci, C in enumerate(CS):
                strides = sorted({g for g in (K,) + STRIDES if g >= K})
                gs = strides[(ri + ci) % len(strides)] if K else 0
                T = ITERS[(ki + ri + ci) % len(ITERS)]
                frame = FRAMES[(ki + 2 * ri + 3 * ci) % len(FRAMES)]
                binary = C == 2 and (ki + ri) % 2 == 0
                potts = (ki + ri + ci) % 2 == 0
                kw = dict(theta_alpha=(2.0, 3.0, INF)[(ki + ci) % 3], theta_beta=(0.5, 1.0, 0.7)[(ri + ci) % 3],
                          theta_gamma=(1.0, INF, 2.0)[(ki + ri) % 3], w_appearance=(1.0, 2.0)[ri % 2] if K else 0.0, w_smooth=(0.5, 1.0)[ci % 2])
                name = f"K{K}-r{r}-C{C}{'b' if binary else ''}-gs{gs}-T{T}-{'potts' if potts else 'mu'}-{'x'.join(map(str, frame))}"
                out.append((name, K, r, C, gs, T, frame, binary, potts, kw))
    return out


def case_inputs(case):
    """``(unary (N, C, h, w) or binary (N, h, w), guide (N, K, h, w) or None, the keyword arguments of crf_reference)``."""
    name, K, r, C, gs, T, (N, h, w), binary, potts, kw = case
    seed = sum(map(ord, name))
    rng = np.random.RandomState(700 + seed)
    unary = (2.0 * rng.randn(*((N, h, w) if binary else (N, C, h, w)))).astype(np.float32)
    guide = G.real_guide(N, K, h, w, seed) if K else None
    return unary, guide, dict(radius=r, iterations=T, compat=None if potts else compat(C), **kw)


@functools.lru_cache(maxsize=None)
def _by_name(name):
    return next(c for c in bounded_cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    from hyperpri_amd import crf
    unary, guide, kw = case_inputs(_by_name(name))
    return crf.crf_reference(unary, guide, **kw)


@functools.lru_cache(maxsize=None)
def bound(name):
    from hyperpri_amd import crf
    unary, guide, kw = case_inputs(_by_name(name))
    return crf.crf_bound(unary, guide, **kw)


def fp64_tolerance(n, C, T, w_total, mu_max, u_max):
    """What two fp64 evaluations of the contract may differ by in L and Q after T iterations, with u = 2^-53: each forms sums of at
    most n - 1 non-negative terms with a handful of roundings per term (``(n + 8) u`` relative, and m <= w_total), so
    ``dm <= 2 (n + 8) u w_total + w_total dQ``; ``dL <= C mu_max dm + 4 u max|L|`` with ``max|L| <= u_max + C mu_max w_total``;
    the softmax is 2-Lipschitz in the maximum norm and rounds C + 4 times: ``dQ <= 2 dL + (C + 4) u``."""
    u = 2.0 ** -53
    l_max = u_max + C * mu_max * w_total
    dQ = (C + 4) * u
    dL = 0.0
    for _ in range(T):
        dm = 2 * (n + 8) * u * w_total + w_total * dQ
        dL = C * mu_max * dm + 4 * u * l_max
        dQ = 2 * dL + (C + 4) * u
    return max(dL, dQ)


def one_hot_logits(N, C, h, w, seed=0):
    """(N, C, h, w) fp32 logits in {-128, +128} with exactly one +128 per pixel: softmax gives exactly one-hot planes in fp32
    (expf(-256) underflows to +0.0, the sum is 1.0, the divisions are exact)."""
    lab = np.random.RandomState(800 + seed).randint(0, C, size=(N, h, w))
    return np.where(np.arange(C)[None, :, None, None] == lab[:, None], 128.0, -128.0).astype(np.float32)


def multiclass_case():
    """The multi-class use: four classes in blocks of a label map with noise of the blocks' own size, a one-channel guide that shows
    the blocks: ``(unary (2, 4, 37, 70), guide (2, 1, 37, 70), kw)``."""
    rng = np.random.RandomState(900)
    N, C, h, w = 2, 4, 37, 70
    y, x = np.mgrid[0:h, 0:w]
    lab = ((y // 9) + 2 * (x // 14)) % C
    unary = (1.5 * (np.arange(C)[None, :, None, None] == lab[None, None]) + 1.5 * rng.randn(N, C, h, w)).astype(np.float32)
    guide = (lab[None, None] + 0.2 * rng.randn(N, 1, h, w)).astype(np.float32)
    return unary, guide, dict(radius=3, iterations=5, theta_alpha=2.0, theta_beta=0.3, theta_gamma=1.0, w_appearance=6.0, w_smooth=1.0), lab


def scene():
    """The scene of the end-to-end test as the CPU sees it: ``blob_scene`` with its ACE map (as tests/test_guided_cpu.py forms it) and
    the first principal component, standardised: ``(ace probabilities (n, H, W), binary logits fp32, guide (n, 1, H, W) fp32, masks)``."""
    cubes, masks = G.blob_scene()
    n, H, W, C = cubes.shape
    X, m = cubes.reshape(-1, C).astype(np.float64), masks.reshape(-1) != 0
    lam, V = np.linalg.eigh(np.cov(X.T))
    pc1 = (X - X.mean(axis=0)) @ V[:, -1]
    guide = (pc1 / pc1.std()).reshape(n, 1, H, W).astype(np.float32)
    mub, Sb = X[~m].mean(axis=0), np.cov(X[~m].T)
    Si = np.linalg.inv(Sb + 1e-4 * np.trace(Sb) / C * np.eye(C))
    t, z = X[m].mean(axis=0) - mub, X - mub
    ace = np.clip((z @ Si @ t) / np.sqrt((t @ Si @ t) * np.einsum("pi,ij,pj->p", z, Si, z)), 2.0 ** -24, 1 - 2.0 ** -24)
    logit = (np.log(ace) - np.log1p(-ace)).reshape(n, H, W).astype(np.float32)
    return ace.reshape(n, H, W), logit, guide, masks
