"""The data of the unmixing tests (tests/test_unmix_cpu.py and tests/test_gpu_unmix.py): seeded, small, and hard enough that the
active set has work to do -- the CPU tests assert that on the reference, so the GPU tests cannot pass on easy pixels alone."""
import numpy as np

MODES = ("ucls", "scls", "ncls", "fcls")


def rup(a, m):
    return (a + m - 1) // m * m


def endmembers(C, M, seed=0):
    """(M, C) fp32 smooth positive spectra: 0.3 + 0.25 sin(2 pi (0.5 + 0.3 m) t + m) + 0.1 m t over t in [0, 1], plus a small seeded
    perturbation.  Strongly correlated, as root and soil are: cond(E) is about 93 at C = 238, M = 8."""
    rng = np.random.RandomState(1000 + 17 * C + M + seed)
    t = np.linspace(0.0, 1.0, C)
    m = np.arange(M)[:, None]
    E = 0.3 + 0.25 * np.sin(2 * np.pi * (0.5 + 0.3 * m) * t[None, :] + m) + 0.1 * m * t[None, :] + 0.002 * rng.randn(M, C)
    return E.astype(np.float32)


def mixed_pixels(E, P, seed=0, pure=True):
    """(P, C) fp32 pixels: Dirichlet(0.3) abundances times E plus N(0, 0.03^2) noise; every fifth pixel is noise only, and (where
    P allows) the pixels 1, 2, 3, 4, 6, ... are the M pure endmembers: a support of one.  (``pure=False`` leaves them out: the
    enumeration oracle ranks candidates by their objective, which tells abundances apart only down to sqrt(2^-53), and a
    noise-free pixel has two candidates that close.)"""
    M, C = E.shape
    rng = np.random.RandomState(2000 + 13 * C + M + seed)
    a = rng.dirichlet(np.full(M, 0.3), size=P)
    x = a @ E.astype(np.float64) + 0.03 * rng.randn(P, C)
    x[::5] = 0.03 * rng.randn(len(x[::5]), C)
    if pure:
        idx = [i for i in range(P) if i % 5][:M]
        x[idx] = E[:len(idx)]
    return x.astype(np.float32)


def planted_scene(C, M, n=3, H=20, W=24, seed=0):
    """n cubes (n, H, W, C) fp32 of mixtures 0.15 / M + 0.85 Dirichlet(0.6) of ``endmembers(C, M)`` with N(0, 0.002^2) noise, M pixels
    replaced by the pure endmembers; uint8 masks (about 45 % foreground) that cover every planted pixel; the planted positions as
    (M, 2) = (cube, pixel).  ATGP finds exactly the planted pixels, in an order of its own."""
    E = endmembers(C, M, seed).astype(np.float64)
    rng = np.random.RandomState(3000 + 11 * C + M + seed)
    P = n * H * W
    a = 0.15 / M + 0.85 * rng.dirichlet(np.full(M, 0.6), size=P)
    x = a @ E + 0.002 * rng.randn(P, C)
    where = np.sort(rng.choice(P, size=M, replace=False))
    x[where] = E
    masks = (rng.rand(P) < 0.45).astype(np.uint8)
    masks[where] = 1
    planted = np.stack([where // (H * W), where % (H * W)], axis=1).astype(np.int64)
    return x.reshape(n, H, W, C).astype(np.float32), masks.reshape(n, H, W), planted


def root_scene(C=19, M=4, n=3, H=36, W=50, seed=0):
    """A planted scene whose member 0 plays the root: the mask is where its abundance exceeds one half (the planted pure root pixel
    included).  ``(cubes, masks)``."""
    E = endmembers(C, M, seed).astype(np.float64)
    rng = np.random.RandomState(4000 + C + seed)
    P = n * H * W
    a = 0.15 / M + 0.85 * rng.dirichlet(np.full(M, 0.6), size=P)
    where = np.sort(rng.choice(P, size=M, replace=False))
    a[where] = np.eye(M)
    x = a @ E + 0.002 * rng.randn(P, C)
    x[where] = E
    masks = (a[:, 0] > 0.5).astype(np.uint8)
    return x.reshape(n, H, W, C).astype(np.float32), masks.reshape(n, H, W)


def indicator_endmembers(C, M):
    """(M, C) indicators of disjoint band groups of sizes 1, 4 and 16 (cycled, the largest shrunk until the groups fit C): Q32 holds
    1, 1/2 and 1/4, R and G are diagonal powers of two, so on integer pixels every step of the contract is exact in fp32."""
    sizes = [(1, 4, 16)[m % 3] for m in range(M)]
    while sum(sizes) > C:
        i = int(np.argmax(sizes))
        sizes[i] = {16: 4, 4: 1}[sizes[i]]
    E = np.zeros((M, C), dtype=np.float32)
    c = 0
    for m, s in enumerate(sizes):
        E[m, c:c + s] = 1.0
        c += s
    return E
