"""Spectral detectors on the device (hyperpri_amd/detect.py, csrc/detect.hip) against the numpy restatement of their contract:
exact on integer data (every fp32 partial sum stays below 2^24), within bounds derived from the fp32 rounding model on
real-valued data, bit-reproducible, and end to end from a filled cache through ``detect_split`` to the evaluation of a split.
Needs a real MI355X: ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import record_margin
from test_gpu_spectral import DEV, U, _cache, _int_cubes, _real_cubes

pytestmark = pytest.mark.gpu
# less than one tile of 64 pixels; one pixel past a tile; 390 tiles; 813 tiles: more than two workgroups per CU, the grid wraps
SIZES = ((1, 7, 9), (1, 5, 13), (2, 96, 130), (2, 130, 200))


def _rup(a, m):
    return (a + m - 1) // m * m


def _launch(x, W, b, Kq, T, cend, score, filters=None):
    """``hpri_band_detect`` itself on an (P, cs) fp32 device buffer: ``(q (P,), scores (T, P))`` as numpy arrays."""
    from hyperpri_amd import _lib
    from hyperpri_amd._args import _p, _stream
    P, cs = int(x.shape[0]), int(x.shape[1])
    q = torch.full((P,), float("nan"), dtype=torch.float32, device=DEV)
    s = torch.full((T, P), float("nan"), dtype=torch.float32, device=DEV) if T else None
    ce = None if cend is None else ctypes.cast((ctypes.c_int * len(cend))(*[int(c) for c in cend]), ctypes.c_void_p)
    if W is None:
        f = torch.from_numpy(np.ascontiguousarray(filters, dtype=np.float32)).to(DEV) if T else None
        bd = None if b is None else torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).to(DEV)
        _lib.call("hpri_band_detect", _p(x), P, cs, None, _p(bd), 0, 0, T, _p(f), None, score, _p(q), _p(s), _stream())
    else:
        wd = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)).to(DEV)
        bd = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).to(DEV)
        _lib.call("hpri_band_detect", _p(x), P, cs, _p(wd), _p(bd), int(W.shape[0]), Kq, T, None, ce, score, _p(q), _p(s), _stream())
    torch.cuda.synchronize()
    return q.cpu().numpy(), (s.cpu().numpy() if T else np.zeros((0, P), np.float32))


def _int_weight(rng, Kq, T, C, cs, triangular):
    """(ks, cs) weight with entries in {-1, 0, 1}, at most 8 non-zeros per row, an integer bias with |b| <= 4; ``triangular``: the
    quadratic row k has its non-zeros at columns <= k (the filter rows stay dense)."""
    ks = _rup(Kq + T, 8)
    W = np.zeros((ks, cs), dtype=np.float32)
    b = np.zeros(ks, dtype=np.float32)
    for k in range(Kq + T):
        hi = min(C, k + 1) if triangular and k < Kq else C
        cols = rng.choice(hi, size=min(8, hi), replace=False)
        W[k, cols] = rng.choice([-1.0, 1.0], size=len(cols))
        b[k] = rng.randint(-4, 5)
    return W, b


def _padded(pixels, cs):
    """(P, C) numpy -> the zero-padded (P, cs) fp32 device buffer."""
    P, C = pixels.shape
    buf = np.zeros((P, cs), dtype=np.float32)
    buf[:, :C] = pixels
    return torch.from_numpy(buf).to(DEV)


# ---- exact on integers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,Kq", [(3, 1), (3, 3), (3, 8), (37, 1), (37, 8), (37, 37), (238, 1), (238, 8), (238, 37), (238, 238)])
def test_q_and_t_are_exact_on_integers(C, Kq):
    """|z| <= 4 + 8 * 4 = 36 and q <= 256 * 1296 < 2^24: raw q and t equal int64 arithmetic, for T in {0, 1, 3, 8}, a dense and a
    lower-triangular weight (with the derived extents), 63, 65, 24960 and 52000 pixels."""
    from hyperpri_amd import detect as D
    cs = _rup(C, 8)
    rng = np.random.RandomState(1000 * C + Kq)
    for (n, h, w) in SIZES:
        pixels = rng.randint(-4, 5, size=(n * h * w, C))
        x = _padded(pixels, cs)
        for T in (0, 1, 3, 8):
            if (n, T) in ((2, 1), (2, 3)):                      # the large frames: T = 0 and T = 8 only
                continue
            for triangular in (False, True):
                W, b = _int_weight(rng, Kq, T, C, cs, triangular)
                cend = D.column_extents(W[:_rup(Kq + T, 16)], cs)[:(Kq + T + 15) // 16] if triangular else None
                if triangular and Kq >= 32:
                    assert cend[0] == 16 and cend[1] == 32       # the extents do cut the loop short
                q, t = _launch(x, W, b, Kq, T, cend, 0)
                # (the matrix product in fp64, where these integers are exact, then int64 arithmetic)
                z = (pixels.astype(np.float64) @ W[:, :C].astype(np.float64).T).astype(np.int64) + b.astype(np.int64)
                assert np.abs(z).max() <= 36
                assert np.array_equal(q.astype(np.int64), (z[:, :Kq] ** 2).sum(axis=1)) and np.array_equal(q, np.rint(q))
                assert np.array_equal(t.astype(np.int64), z[:, Kq:Kq + T].T) and np.array_equal(t, np.rint(t))


@pytest.mark.parametrize("C", [3, 37, 238])
def test_identity_metric_is_exact_on_integers(C):
    cs = _rup(C, 8)
    rng = np.random.RandomState(C)
    for (n, h, w) in SIZES:
        pixels = rng.randint(-4, 5, size=(n * h * w, C))
        x = _padded(pixels, cs)
        for T in (0, 1, 3, 8):
            F = np.zeros((T, cs), dtype=np.float32)
            F[:, :C] = rng.randint(-1, 2, size=(T, C))
            b = rng.randint(-4, 5, size=T).astype(np.float32) if T == 3 else None
            q, t = _launch(x, None, b, 0, T, None, 0, filters=F)
            px = pixels.astype(np.int64)
            assert np.array_equal(q.astype(np.int64), (px ** 2).sum(axis=1))
            want = (pixels.astype(np.float64) @ F[:, :C].astype(np.float64).T).astype(np.int64) + (0 if b is None else b.astype(np.int64))
            assert np.array_equal(t.astype(np.int64), want.T) and np.array_equal(t, np.rint(t))


@pytest.mark.parametrize("C", [3, 37, 238])
def test_module_shapes_and_layout_paths_are_exact_on_integers(C):
    """Both logical shapes the cache hands out, the batch dict and the slow layout path, through ``SpectralDetector``."""
    from hyperpri_amd import detect as D
    cubes, masks = _int_cubes(40 + C, 3, 13, 11, C)
    rng = np.random.RandomState(C)
    T, cs = 3, _rup(C, 8)
    W, b = _int_weight(rng, C, T, C, cs, True)
    tg = rng.randint(1, 4, size=(T, C)).astype(np.float64)
    filt = (W[C:C + T, :C], b[C:C + T])
    det = D.SpectralDetector(W[:C, :C], b[:C], tg, ace=filt, smf=filt).to(DEV)
    px = cubes[[2, 0]].astype(np.int64)
    z = px @ W[:C + T, :C].astype(np.int64).T + b[:C + T].astype(np.int64)
    want_t = np.moveaxis(z[..., C:], -1, 1)                     # (2, T, 13, 11)
    want_q = (z[..., :C] ** 2).sum(axis=-1)[:, None]
    sam = px @ np.round(tg).astype(np.int64).T
    for unsqueeze in (True, False):
        cache = _cache(cubes, masks, unsqueeze=unsqueeze)
        batch = cache.batch([2, 0])
        for arg in (batch, batch["image"]):
            y = det(arg, score="smf")
            assert tuple(y.shape) == (2, T, 13, 11) and y.dtype == torch.float32
            assert np.array_equal(y.cpu().numpy().astype(np.int64), want_t)
        r = det(batch, score="rx")
        assert tuple(r.shape) == (2, 1, 13, 11) and r.is_contiguous()
        assert np.array_equal(r.cpu().numpy().astype(np.int64), want_q)
    x = torch.from_numpy(np.ascontiguousarray(cubes[[2, 0]].transpose(0, 3, 1, 2))).to(DEV)       # plain NCHW: the slow path
    assert np.array_equal(det(x, score="smf").cpu().numpy().astype(np.int64), want_t)
    assert np.array_equal(det(x, score="rx").cpu().numpy().astype(np.int64), want_q)
    # the identity metric's raw filter output, through the module's unit targets: cos * |x| * |s| is the integer inner product
    c = det(x, score="sam").cpu().numpy().astype(np.float64)
    norm = np.sqrt((px ** 2).sum(axis=-1).astype(np.float64))[:, None] * np.sqrt((tg ** 2).sum(axis=1))[None, :, None, None]
    assert np.abs(c * norm - np.moveaxis(sam, -1, 1)).max() <= 1e-4 * norm.max()
    with pytest.raises(RuntimeError, match="autograd"):
        det(x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="bands"):
        det(x[:, :C - 1].contiguous())


# ---- real-valued data inside the derived bounds ----------------------------------------------------------------------
def _bounds(x, W, b, Kq, cs):
    """fp64 z, q and the bounds of the fp32 rounding model on them: a chain of cs fused multiply-adds, one rounding each, gives
    e_k = (cs + 1) u (|b| + |W| |x|)_k; q is a sum of Kq squares of perturbed z, each product and each addition rounded once:
    sum(2 |z_k| e_k + e_k^2) + (Kq + 2) u sum z_k^2."""
    z = x @ W.T + b
    e = (cs + 1) * U * (np.abs(b) + np.abs(x) @ np.abs(W).T)
    q = (z[:, :Kq] ** 2).sum(axis=1)
    eq = (2 * np.abs(z[:, :Kq]) * e[:, :Kq] + e[:, :Kq] ** 2).sum(axis=1) + (Kq + 2) * U * q
    return z, e, q, eq


def _cosine_bound(t, et, q, eq):
    """|t~ rsqrt(q~) (1 + 3u) - t / sqrt(q)| with |t~ - t| <= et, |q~ - q| <= eq < q: the quotient is largest at (|t| + et, q - eq);
    rsqrt (1 ulp) and the product (half an ulp) add 4 u of that."""
    lo = q - eq
    assert (lo > 0).all()
    worst = (np.abs(t) + et) / np.sqrt(lo)
    return worst - np.abs(t) / np.sqrt(q) + 4 * U * worst


def _check_logit(name, got, s, es):
    """The logit map against the fp64 score s with bound es.  logit(clamp(.)) is monotone with derivative 1 / (p (1 - p)) inside
    the clamp and 0 outside, so by the mean value theorem |got - ref| <= es * max over [s - es, s + es] of that derivative (convex:
    the larger end point, taken inside the clamp), plus the rounding of logf, log1pf (2 ulp each) and of the difference.  Where
    the reference lies outside the clamp by more than its bound the device must have clamped: one value, the logit of the clamp."""
    from hyperpri_amd import detect as D
    ref = D.logit_reference(s)
    a, c = np.clip(s - es, D.P_LO, D.P_HI), np.clip(s + es, D.P_LO, D.P_HI)
    slope = np.maximum(1 / (a * (1 - a)), 1 / (c * (1 - c)))
    p = np.clip(s, D.P_LO, D.P_HI)
    tol = es * slope + 4 * U * (np.abs(np.log(p)) + np.abs(np.log1p(-p))) + 2 * U * np.abs(ref) + 8 * U * es * slope
    err = np.abs(got - ref)
    record_margin(name, (err / tol).max(), 1.0)
    assert (err <= tol).all(), name
    inside = (s > D.P_LO) & (s < D.P_HI)
    assert inside.any()
    for out, clamp in ((s + es < D.P_LO, D.P_LO), (s - es > D.P_HI, D.P_HI)):
        if out.any():
            vals = np.unique(got[out])
            want = np.log(clamp) - np.log1p(-clamp)
            assert len(vals) == 1 and abs(vals[0] - want) <= 8 * U * abs(want), (name, vals, want)


@pytest.mark.parametrize("whitener", ["cholesky", "pca"])
@pytest.mark.parametrize("C", [37, 238])
def test_scores_within_the_derived_bound(C, whitener):
    from hyperpri_amd import detect as D
    cubes, masks = _real_cubes(11 * C, 3, 20, 24, C)
    cache = _cache(cubes, masks)
    det = D.SpectralDetector.fit(cache, whitener=whitener)
    assert det.rank == C and det.num_targets == 1 and det.weight.device.type == "cuda"
    cs = cache.cs
    x = np.zeros((2 * 20 * 24, cs))
    x[:, :C] = cubes[[1, 0]].reshape(-1, C)
    batch = cache.batch([1, 0])
    name = f"detect/{whitener}/C{C}"
    Kq = det.rank
    for kind in ("ace", "smf"):
        w, b, cend = det.host_weights(kind, cs)
        if whitener == "cholesky" and kind == "ace":
            assert list(cend[:-1]) == [min(cs, 16 * (i + 1)) for i in range(len(cend) - 1)]
        z, e, q, eq = _bounds(x, w.astype(np.float64), b.astype(np.float64), Kq, cs)
        t, et = z[:, Kq], e[:, Kq]
        got = det(batch, score=kind).cpu().numpy().astype(np.float64).reshape(-1)
        got_l = det(batch, score=kind, logit=True).cpu().numpy().astype(np.float64).reshape(-1)
        q_ref, ref = D.detect_reference(x, w[:Kq + 1], b[:Kq + 1], Kq, score=1 if kind == "ace" else 0)      # the oracle: the contract in fp64
        assert np.allclose(q_ref, q, rtol=1e-12, atol=0) and ref.shape == (1, x.shape[0])
        s, es = ref[0], (et if kind == "smf" else _cosine_bound(t, et, q, eq))
        err = np.abs(got - s)
        record_margin(f"{name}/{kind}", (err / es).max(), 1.0)
        assert (err <= es).all()
        _check_logit(f"{name}/{kind}_logit", got_l, s, es)
    rx = det(batch, score="rx").cpu().numpy().astype(np.float64).reshape(-1)
    err = np.abs(rx - q)
    record_margin(f"{name}/rx", (err / eq).max(), 1.0)
    assert (err <= eq).all()
    # p = q / (q + Kq): dp/dq = Kq / (q + Kq)^2, the division and the sum one rounding each
    pq = q / (q + Kq)
    epq = eq * Kq / (q - eq + Kq) ** 2 + 2 * U * pq
    _check_logit(f"{name}/rx_logit", det(batch, score="rx", logit=True).cpu().numpy().astype(np.float64).reshape(-1), pq, epq)
    # the identity metric: cs roundings in either chain
    f = np.zeros(cs)
    f[:C] = det.sam_weight.cpu().numpy().astype(np.float64)[0]
    t = x @ f
    et = (cs + 1) * U * (np.abs(x) @ np.abs(f))
    q = (x * x).sum(axis=1)
    eq = (cs + 1) * U * q
    got = det(batch, score="sam").cpu().numpy().astype(np.float64).reshape(-1)
    es = _cosine_bound(t, et, q, eq)
    err = np.abs(got - t / np.sqrt(q))
    record_margin(f"{name}/sam", (err / es).max(), 1.0)
    assert (err <= es).all()


# ---- reproducibility -------------------------------------------------------------------------------------------------
def test_scores_are_bit_reproducible_and_independent_of_the_batch():
    from hyperpri_amd import detect as D
    C = 37
    cubes, masks = _real_cubes(5, 3, 20, 24, C)
    cache = _cache(cubes, masks, out_slots=4)
    det = D.SpectralDetector.fit(cache)
    for score in ("ace", "smf", "rx", "sam"):
        both = cache.batch([0, 2])
        a = det(both, score=score, logit=True).clone()
        b = det(both, score=score, logit=True).clone()
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        alone = det(cache.batch([0]), score=score, logit=True)
        assert alone.cpu().numpy().tobytes() == a[:1].contiguous().cpu().numpy().tobytes()


# ---- end to end ------------------------------------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    def forward(self, x):
        t = x[:, 0] if x.dim() == 5 else x
        return torch.zeros((t.shape[0], 1, t.shape[2], t.shape[3]), dtype=torch.float32, device=x.device)


def test_fit_detect_split_and_evaluate(tmp_path):
    import hyperpri_amd as H
    from hyperpri_amd import detect as D
    C, n, Hh, Ww, amp = 19, 3, 36, 50, 0.5
    rng = np.random.RandomState(7)
    band = np.linspace(0.0, 1.0, C)
    signature = np.cos(3.0 * band) + 0.25
    masks = (rng.rand(n, Hh, Ww) < 0.3).astype(np.uint8)
    cubes = (0.3 + 0.02 * rng.randn(n, Hh, Ww, C) + amp * masks[..., None] * signature).astype(np.float32)
    cache = _cache(cubes, masks)
    det = H.SpectralDetector.fit(cache)
    cs = cache.cs
    # on the fp64 reference alone: the classes are separated by more than 100 times the derived bound
    w, b, _ = det.host_weights("ace", cs)
    x = np.zeros((n * Hh * Ww, cs))
    x[:, :C] = cubes.reshape(-1, C)
    z, e, q, eq = _bounds(x, w.astype(np.float64), b.astype(np.float64), C, cs)
    ace = z[:, C] / np.sqrt(q)
    bound = _cosine_bound(z[:, C], e[:, C], q, eq).max()
    fg = masks.reshape(-1) != 0
    assert ace[fg].min() - ace[~fg].max() > 100 * bound and ace[fg].min() - ace[~fg].max() > 0.05
    pred = H.detect_split(det, cache.epoch(batch_size=2, shuffle=False), score="ace")
    stub = H.predict_split(_Stub(), cache.epoch(batch_size=2, shuffle=False))
    assert pred.offsets == stub.offsets and pred.sizes == stub.sizes and pred.names == stub.names
    assert torch.equal(pred.masks, stub.masks) and pred.spread is None and len(pred) == n
    by_batch = torch.cat([det(bt, score="ace", logit=True)[:, 0].reshape(-1).clone() for bt in cache.epoch(batch_size=2, shuffle=False)])
    assert pred.logits.cpu().numpy().tobytes() == by_batch.cpu().numpy().tobytes()
    val = H.validate_net(pred)
    assert val["avg_prec"] == 1.0 and val["dice_at_threshold"] == 1.0
    test = H.test_net(pred, val["best_threshold"])
    assert test["counts"]["fp"] == 0 and test["counts"]["fn"] == 0
    files = H.write_segmaps(str(tmp_path), pred, cache.epoch(batch_size=2, shuffle=False), val["best_threshold"], bands=(0, 9, 18), gamma=1.0)
    assert len(files) == n
    with pytest.raises(ValueError, match="target"):
        H.detect_split(det, cache.epoch(batch_size=2, shuffle=False), target=1)
