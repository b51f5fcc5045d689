"""The shapes and binary patterns of the connected-component tests (test_components_cpu.py, test_gpu_components.py): every
pattern is a (3, h, w) boolean stack; unless the pattern's point is its exact count, the last row of image 0 and the first row of
image 1 are fully set -- images must never merge."""
import numpy as np

from hyperpri_amd.components import TILE_H, TILE_W

N = 3
SHAPES = [(1, 1), (1, 2 * TILE_W + 3), (2 * TILE_H + 3, 1), (9, 13), (TILE_H + 5, 2 * TILE_W - 7), (76, 121)]
DENSITIES = (0.30, 0.41, 0.50, 0.593, 0.80)        # 0.41 and 0.593: the percolation thresholds of 8- and 4-connected sites
EXACT = ("empty", "full", "checkerboard")          # kept as they are: their counts are known in closed form


def spiral(h, w):
    """A one-pixel-wide spiral from the top-left corner inwards with a one-pixel gap between its arms."""
    a = np.zeros((h, w), dtype=bool)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = True
    while True:
        moved = False
        for _ in range(2):
            ny, nx = y + dy, x + dx
            ok = 0 <= ny < h and 0 <= nx < w and not a[ny, nx]
            if ok:
                ay, ax = ny + dy, nx + dx
                ok = not (0 <= ay < h and 0 <= ax < w and a[ay, ax])
            if ok:
                y, x = ny, nx
                a[y, x] = True
                moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            return a


def _single(name, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.zeros((h, w), dtype=bool)
    if name == "empty":
        pass
    elif name == "full":
        a[:] = True
    elif name == "checkerboard":
        a = (yy + xx) % 2 == 0
    elif name == "spiral":
        a = spiral(h, w)
    elif name in ("comb", "comb_mirror"):          # teeth that join only along one row: late merges, the root far from the join
        a[:, ::2] = True
        a[-1, :] = True
        if name == "comb_mirror":
            a = a[::-1].copy()
    elif name == "diagonal":
        a = (yy == xx) | (yy + 5 == xx)
    elif name == "antidiagonal":
        a = (yy + xx == min(h, w) - 1) | (yy + xx == w - 1)
    elif name == "stripes_last":                   # the last row / column of every tile
        a = (yy % TILE_H == TILE_H - 1) | (xx % TILE_W == TILE_W - 1)
    elif name == "stripes_first":                  # the first row / column of every tile but the first
        a = ((yy % TILE_H == 0) & (yy > 0)) | ((xx % TILE_W == 0) & (xx > 0))
    elif name == "stripes_both":                   # dashes two pixels thick astride every tile edge
        on = (yy % TILE_H >= TILE_H - 1) | ((yy % TILE_H == 0) & (yy > 0)) | (xx % TILE_W >= TILE_W - 1) | ((xx % TILE_W == 0) & (xx > 0))
        a = on & ((yy + xx) % 5 != 0)
    elif name == "corners":
        a[0, 0] = a[0, -1] = a[-1, 0] = a[-1, -1] = True
    else:
        raise KeyError(name)
    return a


NAMES = ("empty", "full", "checkerboard", "spiral", "comb", "comb_mirror", "diagonal", "antidiagonal", "stripes_last", "stripes_first",
         "stripes_both", "corners") + tuple(f"noise_{d}" for d in DENSITIES)
_cache = {}


def pattern(name, shape):
    """(3, h, w) bool; image 1 is the horizontal mirror of the single pattern, image 2 its vertical mirror."""
    key = (name, shape)
    if key not in _cache:
        h, w = shape
        if name.startswith("noise_"):
            seed = 1000 + int(float(name[6:]) * 1000) + 7 * h + w
            a = np.random.RandomState(seed).rand(N, h, w) < float(name[6:])
        else:
            s = _single(name, h, w)
            a = np.stack([s, s[:, ::-1], s[::-1]])
        if name not in EXACT:
            a[0, -1, :] = True
            a[1, 0, :] = True
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def all_patterns(shape):
    return [(name, pattern(name, shape)) for name in NAMES]


_refs = {}


def reference(name, shape, connectivity):
    """components_reference of a pattern, computed once per session."""
    from hyperpri_amd.components import components_reference
    key = (name, shape, connectivity)
    if key not in _refs:
        labels, counts = components_reference(pattern(name, shape), connectivity)
        labels.setflags(write=False)
        counts.setflags(write=False)
        _refs[key] = (labels, counts)
    return _refs[key]
