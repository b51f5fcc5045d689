"""The data of the ridge-filter tests (tests/test_ridge_cpu.py and tests/test_gpu_ridge.py): seeded and small.  The CPU tests assert on
the reference what the GPU tests rely on -- that the bound covers an fp32 emulation of the device on every bounded case (so it is not
vacuous before a GPU sees it), that at most 1 % of a case's pixels are undecided, that the scene of the end-to-end test has thin lines
a threshold misses and the ridge measure finds."""
import numpy as np

from _guided_cases import best_dice, periodic  # noqa: F401  (shared with the guided filter's tests)

TILE_H, TILE_W = 16, 32                 # hpri_ridge_tile_h / _w (test_ridge_cpu.py asserts that the library says the same)
# 1x1; smaller than any kernel; one less and one more than the tile in each direction; several tiles; a batch of three
FRAMES = ((1, 1, 1), (1, 3, 5), (1, TILE_H - 1, TILE_W - 1), (1, TILE_H + 1, TILE_W + 1), (1, 37, 130), (3, TILE_H + 1, TILE_W + 1))
SCALE_SETS = ((0.5,), (4.0,), (1.0, 2.0), (0.75, 1.0, 1.5, 2.0, 3.0), (0.5, 0.75, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0))
TS, STRIDES, DOMAINS = (1, 2, 5), (1, 3, 8), ("linear", "prob")
MEASURES, POLARITIES, OUTPUTS = ("frangi", "sato"), ("bright", "dark", "both"), ("value", "logit")
SCENE_SIGMAS = (0.75, 1.0, 1.5, 2.0, 3.0)


def bounded_cases():
    """Every combination of a scale set and T, each with a pixel stride, a domain, a measure, a polarity, an output and a frame drawn
    so that all of them occur (stride 1 is plain NCHW; strides 3 and 8 are channels-last buffers with NaN in the channels past T), then
    the offset plane (1000 + 0.01 U: the trial that motivated the centring) under both measures:
    ``(name, sigmas, T, stride, domain, measure, polarity, output, (N, h, w), c, offset)``."""
    out = []
    for si, sig in enumerate(SCALE_SETS):
        for ti, T in enumerate(TS):
            k = si * len(TS) + ti
            strides = [s for s in STRIDES if s == 1 or s >= T]
            stride = strides[(si + ti) % len(strides)]
            domain, measure, polarity = DOMAINS[(si + ti) % 2], MEASURES[(k // 3) % 2], POLARITIES[k % 3]
            output = OUTPUTS[(si + 2 * ti) % 2]
            frame = FRAMES[(si + 3 * ti) % len(FRAMES)]                     # (the 1 x 1 frames fall on the linear domain)
            name = f"S{len(sig)}a{si}-T{T}-ps{stride}-{domain}-{measure}-{polarity}-{output}-{'x'.join(map(str, frame))}"
            out.append((name, sig, T, stride, domain, measure, polarity, output, frame, 0.5, False))
    out.append(("offset-frangi", SCENE_SIGMAS, 1, 8, "linear", "frangi", "bright", "value", (1, 37, 130), 5e-3, True))
    out.append(("offset-sato", (1.0, 2.0), 2, 1, "linear", "sato", "both", "logit", (1, TILE_H + 1, TILE_W + 1), 5e-3, True))
    return out


def real_maps(N, T, h, w, domain="linear", seed=0, offset=False):
    """(N, T, h, w) fp32: smooth structure of order one plus noise (linear), logits N(0, 2^2) plus structure (prob); ``offset``:
    1000 + 0.01 U(0, 1), a mean 1e5 times the variation."""
    rng = np.random.RandomState(700 + seed)
    if offset:
        return (1000.0 + 0.01 * rng.rand(N, T, h, w)).astype(np.float32)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([np.sin(0.3 * y + 0.2 * (k + 1) * x + k) + (np.abs(x - w // 2) < 2) * (1.0 + k) for k in range(T)])
    amp = 2.0 if domain == "prob" else 0.3
    return (base[None] * (2.0 if domain == "prob" else 1.0) + amp * rng.randn(N, T, h, w)).astype(np.float32)


def case_data(case):
    name, sig, T, stride, domain, measure, polarity, output, (N, h, w), c, offset = case
    return real_maps(N, T, h, w, domain, sum(map(ord, name)), offset)


def case_args(case):
    """The keyword arguments of ``ridge_reference`` / ``ridge_bound`` for a case."""
    name, sig, T, stride, domain, measure, polarity, output, frame, c, offset = case
    return dict(sigmas=sig, measure=measure, polarity=polarity, beta=0.5, c=c, domain=domain)


def fractions(ref, bnd, hessian, response, index=None):
    """A device's (or an emulation's) planes against the reference, as fractions of ``ridge_bound``: ``{"hessian": the largest |error| /
    bound (0 where both vanish), "value": the same for the response outside the undecided mask, "inside_ok": whether every undecided
    pixel holds one branch's value within the bound, "index_ok": the scale index equals the reference's outside its mask and is a
    candidate inside, "share": the share of pixels left out of either comparison}``."""
    def frac(err, bound):
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        return float(f.max()) if f.size else 0.0
    shape = ref["scales"].shape                                   # (N, T, S, h, w)
    resp = np.asarray(response, dtype=np.float64).reshape(shape[:2] + shape[3:])
    want, bound = ref["response"].reshape(resp.shape), bnd["value"].reshape(resp.shape)
    und, undi = bnd["undecided"].reshape(resp.shape), bnd["undecided_index"].reshape(resp.shape)
    out = {"hessian": frac(np.abs(np.asarray(hessian, dtype=np.float64) - ref["hessian"]), bnd["hessian"]),
           "value": frac(np.abs(resp - want)[~und], bound[~und]), "share": float(max(und.mean(), undi.mean())), "inside_ok": True,
           "index_ok": True}
    if und.any():
        gate = bnd["gate"]
        decided = np.where(gate, 0.0, ref["scales"]).max(axis=2)                              # every undecided gate closed
        ok = np.abs(resp - decided) <= bound
        for s in range(shape[2]):                                                               # ... or scale s's gate open
            ok |= gate[:, :, s] & (np.abs(resp - np.maximum(decided, ref["open"][:, :, s])) <= bound)
        ok |= np.abs(resp - np.maximum(decided, np.where(gate, ref["open"], 0.0).max(axis=2))) <= bound   # ... or all of them
        out["inside_ok"] = bool(ok[und].all())
    if index is not None:
        idx = np.asarray(index).reshape(resp.shape).astype(np.int64)
        same = idx == ref["index"].reshape(resp.shape)
        cand = np.take_along_axis(bnd["candidates"], np.clip(idx, 0, shape[2] - 1)[:, :, None], axis=2)[:, :, 0]
        out["index_ok"] = bool(same[~undi].all() and cand[undi].all() and (idx < shape[2]).all())
    return out


def plain_fp32(I, sigma):
    """The usual route in fp32, uncentred: full kernels (the centre taps included) applied to the values themselves, row pass then
    column pass, every product and sum in fp32.  (h, w) fp32 -> (3, h, w) Hxx | Hxy | Hyy as fp64."""
    from hyperpri_amd.ridge import _rho, ridge_taps
    R, g0, g1, g2 = ridge_taps(sigma)
    k0 = np.concatenate([g0[::-1], [np.float32(1.0 - 2.0 * g0.astype(np.float64).sum())], g0]).astype(np.float32)
    k1 = np.concatenate([-g1[::-1], [np.float32(0.0)], g1]).astype(np.float32)
    k2 = np.concatenate([g2[::-1], [np.float32(-2.0 * g2.astype(np.float64).sum())], g2]).astype(np.float32)

    def conv(X, k, axis):
        n = X.shape[axis]
        acc = np.zeros(X.shape, np.float32)
        for j in range(-R, R + 1):
            acc = acc + k[j + R] * np.take(X, _rho(np.arange(n) + j, n), axis=axis)
        return acc
    I = np.asarray(I, dtype=np.float32)
    s2 = np.float32(np.float32(sigma) * np.float32(sigma))
    return np.stack([conv(conv(I, k2, 1), k0, 0) * s2, conv(conv(I, k1, 1), k1, 0) * s2, conv(conv(I, k0, 1), k2, 0) * s2]).astype(np.float64)


def gaussian_line(h, w, sigma0, vertical=True):
    """A bright line of Gaussian profile exp(-d^2 / 2 sigma0^2) through the middle of an (h, w) plane."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = x - w // 2 if vertical else y - h // 2
    return np.exp(-d * d / (2.0 * sigma0 * sigma0)).astype(np.float32)


def gaussian_blob(h, w, sigma0):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.exp(-((x - w // 2) ** 2 + (y - h // 2) ** 2) / (2.0 * sigma0 * sigma0)).astype(np.float32)


def root_scene(seed=0, h=48, w=64):
    """Curved lines of widths 0.6, 1.2 and 2.0 pixels (Gaussian profiles of height 0.8) and one vertical line, on a ramp of 3 across
    the frame plus blocky 8 x 8 soil of 0.4 plus Gaussian noise of 0.25: ``(plane fp32 (h, w), mask uint8 (h, w))``; the mask is each
    line's core, |d| <= max(0.75 width, 0.75)."""
    rng = np.random.RandomState(800 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    plane, mask = np.zeros((h, w)), np.zeros((h, w), dtype=bool)
    curves = ((lambda t: 9 + 5 * np.sin(t / 9.0 + seed), lambda t: 5 / 9.0 * np.cos(t / 9.0 + seed), 0.6),
              (lambda t: 24 + 6 * np.sin(t / 13.0 + 1 + seed), lambda t: 6 / 13.0 * np.cos(t / 13.0 + 1 + seed), 1.2),
              (lambda t: 39 + 4 * np.cos(t / 8.0 + seed), lambda t: -4 / 8.0 * np.sin(t / 8.0 + seed), 2.0))
    for f, df, width in curves:
        d = (y - f(x)) / np.sqrt(1.0 + df(x) ** 2)
        plane = np.maximum(plane, np.exp(-d * d / (2.0 * width * width)))
        mask |= np.abs(d) <= max(0.75 * width, 0.75)
    d = x - (w - 13)
    plane = np.maximum(plane, np.exp(-d * d / 2.0))
    mask |= np.abs(d) <= 1.0
    soil = 1.5 * (x / w + y / h) + 0.4 * np.kron(rng.rand(h // 8, w // 8), np.ones((8, 8)))
    return (0.8 * plane + soil + 0.25 * rng.randn(h, w)).astype(np.float32), mask.astype(np.uint8)


def scene_cubes(n=3, C=19):
    """``root_scene`` of seeds 0 .. n-1 embedded in small cubes, ``(cubes (n, h, w, C) fp32, masks (n, h, w) uint8, planes (n, h, w))``:
    cube = 0.3 + plane x spectrum + white noise of 0.01, so the first principal component carries the scene."""
    rng = np.random.RandomState(900)
    band = np.linspace(0.0, 1.0, C)
    spectrum = 0.2 * (1.0 + 0.5 * np.cos(3.0 * band))
    planes, masks = zip(*(root_scene(k) for k in range(n)))
    planes, masks = np.stack(planes), np.stack(masks)
    cubes = 0.3 + planes[..., None] * spectrum + 0.01 * rng.randn(*planes.shape, C)
    return cubes.astype(np.float32), masks, planes
