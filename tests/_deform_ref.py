"""fp64 / exact-integer restatement of the deforming gather (csrc/cache_warp.hip, csrc/cache_deform.hip): the B-spline field, the CutMix owner of a pixel,
the displaced coordinates, Philox4x32-10 and Box-Muller.  Builds on the warp restatement of tests/test_cube_warp_cpu.py
(``bilinear64`` / ``nearest64`` / ``entry_fields``); used by tests/test_cube_deform_cpu.py (which checks it against independent
forms) and tests/test_gpu_cube_deform.py.  Also the case list the two files share."""
import numpy as np

from test_cube_warp_cpu import PARAMS, bilinear64, case_entries, entry_fields, nearest64

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
ZMAX = 5.77                     # sqrt(-2 ln 2^-24) = 5.768

# (Hs, Ws, h, w): the 4 x 37 window spans several 512-quad work items at 60 quads per pixel
GEOMS = [(12, 20, 5, 7), (16, 24, 8, 8), (5, 40, 4, 37), (12, 20, 12, 20)]
# (geometry, node pitch, sigma of the node displacements in pixels, seed of the lattice): batches of three samples, each with its own
# affine map, gain / offset and lattice.  The seeds are picked so that at most 2 % of a case's pixels have a source coordinate
# within 1e-3 of a k + 1/2 (tests/test_cube_deform_cpu.py asserts it)
ELASTIC_CASES = [(GEOMS[0], 4.0, 0.8, 11), (GEOMS[1], 4.0, 1.2, 12), (GEOMS[2], 8.0, 1.5, 13), (GEOMS[3], 6.0, 1.5, 14)]
CASE_PARAMS = [PARAMS[0], PARAMS[5], PARAMS[7]]
CASE_GAINS, CASE_OFFSETS = [1.0, 1.3, 0.8], [0.0, -0.1, 0.2]


def lattice(h, w, pitch):
    return int(np.floor((h - 1) / pitch)) + 4, int(np.floor((w - 1) / pitch)) + 4


def case_nodes(case, n=3):
    """(n, gy, gx, 2) fp32 node displacements of one elastic case."""
    (_, _, h, w), pitch, sigma, seed = case
    gy, gx = lattice(h, w, pitch)
    return (np.random.default_rng(seed).standard_normal((n, gy, gx, 2)) * sigma).astype(np.float32)


def case_warp_entries(case, flip_h=0, flip_w=0):
    """The warp entries of a case's three samples (slots 0, 1, 2) with their gains and offsets."""
    rows = [case_entries(case[0], [i], [CASE_PARAMS[i]], flip_h, flip_w, gain=CASE_GAINS[i], offset=CASE_OFFSETS[i])[0] for i in range(3)]
    return np.stack(rows)


# ---- the field ------------------------------------------------------------------------------------------------------------------
def bspline64(f):
    f = np.asarray(f, dtype=np.float64)
    return np.stack([(1 - f) ** 3 / 6, (3 * f ** 3 - 6 * f ** 2 + 4) / 6, (-3 * f ** 3 + 3 * f ** 2 + 3 * f + 1) / 6, f ** 3 / 6])


def field64(nodes, h, w, inv_pitch):
    """(h, w, 2) fp64 field of one (gy, gx, 2) lattice; ``inv_pitch`` is the fp32 value of the entry, the products ``y * inv_pitch``
    are formed in fp32 as the kernel forms them (they decide the cell), everything after that in fp64."""
    nodes = np.asarray(nodes, dtype=np.float64)
    gy, gx = nodes.shape[:2]
    ip = np.float32(inv_pitch)
    ty = (np.arange(h, dtype=np.float32) * ip).astype(np.float64)
    tx = (np.arange(w, dtype=np.float32) * ip).astype(np.float64)
    iy = np.clip(np.floor(ty).astype(np.int64), 0, gy - 4)
    ix = np.clip(np.floor(tx).astype(np.int64), 0, gx - 4)
    By, Bx = bspline64(ty - iy), bspline64(tx - ix)                 # (4, h), (4, w)
    out = np.zeros((h, w, 2))
    for a in range(4):
        for b in range(4):
            out += (By[a][:, None] * Bx[b][None, :])[..., None] * nodes[(iy + a)[:, None], (ix + b)[None, :]]
    return out


def fields64(deform, nodes_flat, h, w):
    """(n, h, w, 2) fp64 from (n, 16) int32 deform entries and the flat node table: zeros where the kernel writes zeros."""
    deform = np.asarray(deform)
    out = np.zeros((len(deform), h, w, 2))
    L = 0 if nodes_flat is None else len(nodes_flat)
    for i, row in enumerate(deform):
        off, gy, gx = int(row[5]), int(row[6]), int(row[7])
        if off < 0 or gy < 4 or gx < 4 or off + 2 * gy * gx > L:
            continue
        ip = row[8:9].copy().view(np.float32)[0]
        out[i] = field64(np.asarray(nodes_flat[off:off + 2 * gy * gx]).reshape(gy, gx, 2), h, w, ip)
    return out


# ---- owner and coordinates ---------------------------------------------------------------------------------------------------------
def owners(deform, h, w):
    """(n, h, w) int: the batch sample every output pixel is taken from."""
    deform = np.asarray(deform)
    n = len(deform)
    own = np.repeat(np.arange(n)[:, None, None], h, 1).repeat(w, 2)
    for s, row in enumerate(deform):
        m, ry0, ry1, rx0, rx1 = (int(v) for v in row[:5])
        ry0, ry1, rx0, rx1 = max(ry0, 0), min(ry1, h), max(rx0, 0), min(rx1, w)
        if 0 <= m < n and m != s and ry0 < ry1 and rx0 < rx1:
            own[s, ry0:ry1, rx0:rx1] = m
    return own


def coords64_uv(f, u, v):
    """sx, sy from the fp32 table values ``f`` and displaced u, v (h, w) in fp64, and S: the largest absolute partial sum."""
    out, S = [], 0.0
    for au, av, c in ((f[0], f[1], f[2]), (f[3], f[4], f[5])):
        p, q = au * u, av * v
        for part in (p, q, p + q, p + c, q + c, p + q + c, np.array(c)):
            S = max(S, float(np.abs(part).max()))
        out.append(p + q + c)
    return out[0], out[1], S


def sigma_of(row):
    s = float(np.asarray(row[9:10], dtype=np.int32).copy().view(np.float32)[0])
    return s if s > 0 else 0.0


def restate_deform(entries, deform, fields, cubes, masks, C, cs, h, w, noise=True):
    """What the deforming kernels must write: image (n, h, w, cs) fp64 (dropped and pad channels 0), mask (n, 1, h, w), the
    per-sample tolerance of the warp restatement (S over the displaced u, v and over x + dx, y + dy, whose rounding is new; the
    largest over the owners a sample draws from; the noise term is NOT in it) and ``sure`` (n, 1, h, w): False where sx or sy
    lies within 1e-3 of a k + 1/2.  ``fields``: (n, h, w, 2) fp64 or None."""
    entries, deform = np.asarray(entries), np.asarray(deform)
    n = len(entries)
    own = owners(deform, h, w)
    img, msk, sure, tols = np.zeros((n, h, w, cs)), np.zeros((n, 1, h, w)), np.ones((n, 1, h, w), dtype=bool), []
    X, Y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    for s in range(n):
        tol = 0.0
        for o in np.unique(own[s]):
            sel = own[s] == o
            slot, dlo, dn, f = entry_fields(entries[o])
            dx, dy = (fields[o, ..., 0], fields[o, ..., 1]) if fields is not None else (0.0, 0.0)
            xd, yd = X + dx, Y + dy
            sx, sy, S = coords64_uv(f, xd - (w - 1) / 2, yd - (h - 1) / 2)
            S = max(S, float(np.abs(f[[0, 3]]).max() * np.abs(xd).max()), float(np.abs(f[[1, 4]]).max() * np.abs(yd).max()))
            sx, sy = np.clip(sx, -1, cubes[slot].shape[1]), np.clip(sy, -1, cubes[slot].shape[0])
            gain, offset = f[6], f[7]
            src = cubes[slot]
            val = np.zeros((h, w, cs))
            val[..., :C] = gain * bilinear64(src, sy, sx) + offset
            val[..., dlo:dlo + dn] = 0.0
            img[s][sel] = val[sel]
            msk[s, 0][sel] = nearest64(masks[slot], sy, sx)[sel]
            ok = (np.abs(sx - np.floor(sx) - 0.5) >= 1e-3) & (np.abs(sy - np.floor(sy) - 0.5) >= 1e-3)
            sure[s, 0][sel] = ok[sel]
            R = max(float(src.max()), 0.0) - min(float(src.min()), 0.0)
            M = float(np.abs(src).max())
            tol = max(tol, abs(gain) * (2 * 2.0 ** -21 * S * R + 2.0 ** -21 * M) + 2.0 ** -22 * (abs(gain) * M + abs(offset)))
        tols.append(tol)
        sg = sigma_of(deform[s])
        if noise and sg > 0:
            z = noise64(int(np.uint32(deform[s][10])), int(np.uint32(deform[s][11])), h, w, cs)
            live = np.zeros((h, w, cs), dtype=bool)
            live[..., :C] = True
            for o in np.unique(own[s]):
                _, dlo, dn, _ = entry_fields(entries[o])
                live[own[s] == o, dlo:dlo + dn] = False
            img[s] += np.where(live, sg * z, 0.0)
    return img, msk, tols, sure


# ---- Philox4x32-10 and Box-Muller ------------------------------------------------------------------------------------------------
def philox(ctr, key):
    """ctr (..., 4), key (..., 2) of integers -> (..., 4) uint32 words after ten rounds (uint64 arithmetic, masked)."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) & MASK32 for i in range(4)]
    k0, k1 = (np.asarray(key)[..., i].astype(np.uint64) & MASK32 for i in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return np.stack(c, axis=-1).astype(np.uint32)


def bits_at(k0, k1, e):
    """The four words of counters ``e`` (any shape, integers below 2^64) under one key."""
    e = np.asarray(e, dtype=np.uint64)
    ctr = np.stack([e & MASK32, e >> np.uint64(32), np.zeros_like(e), np.zeros_like(e)], axis=-1)
    key = np.stack([np.full(e.shape, k0, dtype=np.uint64), np.full(e.shape, k1, dtype=np.uint64)], axis=-1)
    return philox(ctr, key)


def normals64(bits):
    """(..., 4) uint32 -> (..., 4) fp64 normals: pairs (r0, r1), (r2, r3) through Box-Muller."""
    u = ((np.asarray(bits, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    out = np.empty(u.shape)
    for a in (0, 2):
        rad = np.sqrt(-2 * np.log(u[..., a]))
        out[..., a], out[..., a + 1] = rad * np.cos(2 * np.pi * u[..., a + 1]), rad * np.sin(2 * np.pi * u[..., a + 1])
    return out


def noise64(k0, k1, h, w, cs):
    """z (h, w, cs) fp64 of one sample: counter (y * w + x) * (cs / 4) + c / 4, word c % 4."""
    q = cs // 4
    e = (np.arange(h * w, dtype=np.uint64)[:, None] * np.uint64(q) + np.arange(q, dtype=np.uint64)[None, :])
    return normals64(bits_at(k0, k1, e)).reshape(h, w, cs)
