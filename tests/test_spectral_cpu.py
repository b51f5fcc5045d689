"""Spectral statistics and projection, the parts that need no GPU: the numpy restatements of the contract against plain numpy
formulas, the host-side algebra (merge, PCA basis), the pure-host entry points of the C ABI with every argument error, and the
compiler's report on the new kernels."""
import ctypes
import os
import sys

import numpy as np
import pytest

from hyperpri_amd import spectral as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(seed=0, n=3, H=7, W=9, C=5, dtype=np.float32):
    rng = np.random.RandomState(seed)
    x = (0.3 + 0.1 * rng.randn(n, H, W, C)).astype(dtype)
    m = (rng.rand(n, H, W) < 0.4).astype(np.uint8)
    return x, m


def test_references_match_plain_numpy():
    x, m = _data()
    flat = x.reshape(-1, x.shape[-1]).astype(np.float64)
    fg = m.reshape(-1) != 0
    for select, rows in (("all", flat), ("foreground", flat[fg]), ("background", flat[~fg])):
        n, sums = S.moments_reference(x, m, select)
        assert n == rows.shape[0] and np.allclose(sums, rows.sum(axis=0), rtol=1e-13, atol=0)
        st = S.statistics_reference(x, m, select)
        assert st.count == n and st.select == select
        assert np.allclose(st.mean, rows.mean(axis=0), rtol=1e-13, atol=0)
        assert np.allclose(st.cov, np.cov(rows, rowvar=False), rtol=1e-11, atol=1e-18)
        assert np.allclose(st.std(), rows.std(axis=0, ddof=1), rtol=1e-11)
        assert np.allclose(st.correlation(), np.corrcoef(rows, rowvar=False), rtol=1e-9, atol=1e-12)
        pivot = rows.mean(axis=0).astype(np.float32)
        G = S.gram_reference(x, pivot, m, select)
        d = rows.mean(axis=0) - pivot.astype(np.float64)
        # the pivot identity band_statistics uses on the host
        assert np.allclose((G - n * np.outer(d, d)) / (n - 1), np.cov(rows, rowvar=False), rtol=1e-10, atol=1e-18)
    with pytest.raises(ValueError):
        S.moments_reference(x, None, "foreground")
    with pytest.raises(ValueError):
        S.moments_reference(x, m, "roots")
    # fp16 slots: the reference works on the quantised values
    xh = x.astype(np.float16)
    assert np.array_equal(S.moments_reference(xh)[1], xh.reshape(-1, 5).astype(np.float64).sum(axis=0))


def test_project_reference():
    rng = np.random.RandomState(1)
    x = rng.randn(4, 6, 5)
    W, b = rng.randn(3, 5), rng.randn(3)
    assert np.allclose(S.project_reference(x, W, b), np.einsum("kc,hwc->hwk", W, x) + b, rtol=1e-13)
    s, t = rng.randn(5), rng.randn(5)
    assert np.allclose(S.project_reference(x, s, t), x * s + t, rtol=1e-15)


def test_merge_equals_the_statistics_of_the_concatenation():
    xa, _ = _data(seed=2, n=2, C=11)
    xb, _ = _data(seed=3, n=5, C=11)
    xb = xb + 0.2                                         # different means: the delta term matters
    a, b = S.statistics_reference(xa), S.statistics_reference(xb)
    both = S.statistics_reference(np.concatenate([xa.reshape(-1, 11), xb.reshape(-1, 11)])[None, None])
    got = S.merge_statistics(a, b)
    assert got.count == both.count == a.count + b.count
    assert np.abs(got.mean - both.mean).max() <= 1e-12 * np.abs(both.mean).max()
    assert np.abs(got.cov - both.cov).max() <= 1e-12 * np.abs(both.cov).max()
    assert got.select == "all"
    with pytest.raises(ValueError):
        S.merge_statistics(a, S.statistics_reference(_data(C=4)[0]))


def _geometric_stats(C=12, seed=4):
    """A covariance with the spectrum 2^-i in a random orthonormal basis: well-separated eigenvalues."""
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.randn(C, C))
    lam = 2.0 ** -np.arange(C)
    return S.SpectralStats(1000, rng.randn(C), (Q * lam) @ Q.T, "all"), lam, Q


def test_pca_basis_on_a_geometric_spectrum():
    st, lam, Q = _geometric_stats()
    k = 5
    W, b, ev = S.pca_basis(st, k)
    assert W.dtype == np.float32 and W.shape == (k, 12) and b.dtype == np.float32 and b.shape == (k,) and ev.dtype == np.float64
    assert np.allclose(ev, lam[:k], rtol=1e-12) and (np.diff(ev) < 0).all()
    # fp64 rows before the fp32 rounding: repeat the host computation at k = C and compare after rounding
    W64 = np.linalg.eigh(st.cov)[1][:, ::-1].T[:k].copy()
    for i in range(k):
        j = int(np.argmax(np.abs(W64[i])))
        W64[i] *= 1.0 if W64[i, j] > 0 else -1.0
    assert np.array_equal(W, W64.astype(np.float32))
    D = W64 @ st.cov @ W64.T
    assert np.abs(D - np.diag(ev)).max() <= 1e-9 * lam[0]
    # the sign rule: the entry of largest magnitude of every row is positive
    for i in range(k):
        assert W[i, int(np.argmax(np.abs(W[i])))] > 0
    assert np.array_equal(b, (-(W64 @ st.mean)).astype(np.float32))
    # whitening gives the identity
    Ww, bw, evw = S.pca_basis(st, k, whiten=True)
    Ww64 = W64 / np.sqrt(ev)[:, None]
    assert np.array_equal(Ww, Ww64.astype(np.float32)) and np.array_equal(evw, ev)
    assert np.abs(Ww64 @ st.cov @ Ww64.T - np.eye(k)).max() <= 1e-9
    assert np.array_equal(bw, (-(Ww64 @ st.mean)).astype(np.float32))
    with pytest.raises(ValueError):
        S.pca_basis(st, 13)
    with pytest.raises(ValueError):
        S.pca_basis(st, 0)


def test_sign_rule_ties_go_to_the_lowest_index():
    # cov = diag(2, 2 - tiny) rotated by 45 degrees: the first eigenvector is (1, 1) / sqrt(2) up to sign, a tie of magnitudes
    cov = np.array([[2.0, 1.0], [1.0, 2.0]])
    W, _, ev = S.pca_basis(S.SpectralStats(10, np.zeros(2), cov), 2)
    assert np.allclose(ev, [3.0, 1.0])
    assert np.allclose(np.abs(W), np.sqrt(0.5), rtol=1e-6)
    assert W[0, 0] * W[0, 1] > 0 and W[1, 0] * W[1, 1] < 0
    for i in range(2):                                    # numpy's argmax is the lowest index among equal magnitudes
        assert W[i, int(np.argmax(np.abs(W[i])))] > 0


def test_pure_host_entry_points():
    from hyperpri_amd import _lib
    lib = _lib.load()
    run = lib.hpri_band_fp32_run()
    assert 1 <= run <= 4096 and run == S.FP32_RUN == S.fp32_run()
    assert lib.hpri_band_project_max_k() >= 64 and S.project_max_k() == lib.hpri_band_project_max_k()
    assert lib.hpri_band_max_cs() >= 304 and lib.hpri_band_max_cs() % 32 == 0
    # the workspace is a function of cs alone -- the signature takes nothing else -- and stays far below a slab per chunk
    restype, argtypes = _lib.parse_header()["hpri_band_workspace_bytes"]
    assert restype is ctypes.c_size_t and argtypes == [ctypes.c_int]
    sizes = [lib.hpri_band_workspace_bytes(cs) for cs in (8, 40, 240, 304)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] < 256 * 2 ** 20
    assert lib.hpri_band_workspace_bytes(0) == 0 and lib.hpri_band_workspace_bytes(12) == 0
    assert lib.hpri_band_workspace_bytes(lib.hpri_band_max_cs() + 8) == 0
    assert S.workspace_bytes(240) == sizes[2]


def test_argument_errors_return_minus_one_before_any_launch():
    from hyperpri_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    ok = ctypes.c_void_p(4096)                            # an aligned non-null address: never dereferenced on the host
    odd = ctypes.c_void_p(4100)                           # 4-byte aligned only
    ws = lib.hpri_band_workspace_bytes(40)

    def moments(cache=ok, dtype=0, slots=4, Hs=13, Ws=11, cs=40, masks=ok, table=ok, n=2, select=0, pivot=null, work=ok, nbytes=ws,
                count=ok, sums=ok, sumsq=null):
        return lib.hpri_band_moments(cache, dtype, slots, Hs, Ws, cs, masks, table, n, select, pivot, work, nbytes, count, sums, sumsq, null)

    def gram(cache=ok, dtype=0, slots=4, Hs=13, Ws=11, cs=40, masks=ok, table=ok, n=2, select=0, pivot=ok, work=ok, nbytes=ws, out=ok):
        return lib.hpri_band_gram(cache, dtype, slots, Hs, Ws, cs, masks, table, n, select, pivot, work, nbytes, out, null)

    def project(x=ok, pixels=100, cs=40, w=ok, b=ok, K=8, y=ok):
        return lib.hpri_band_project(x, pixels, cs, w, b, K, y, null)

    def affine(x=ok, pixels=100, cs=40, C=37, s=ok, t=ok, y=ok):
        return lib.hpri_band_affine(x, pixels, cs, C, s, t, y, null)

    def rejected(rc, word):
        msg = lib.hpri_last_error()
        assert rc == -1 and word.encode() in msg, (rc, msg)

    for fn in (moments, gram):
        rejected(fn(cache=null), "null")
        rejected(fn(table=null), "null")
        rejected(fn(work=null), "null")
        rejected(fn(dtype=2), "dtype")
        rejected(fn(dtype=-1), "dtype")
        for bad in ({"slots": 0}, {"Hs": 0}, {"Ws": -3}, {"n": 0}):
            rejected(fn(**bad), "sizes")
        rejected(fn(cs=36), "multiple of 8")
        rejected(fn(cs=0), "multiple of 8")
        rejected(fn(cs=lib.hpri_band_max_cs() + 8), "multiple of 8")
        rejected(fn(select=3), "select")
        rejected(fn(select=-1), "select")
        rejected(fn(select=1, masks=null), "masks")
        rejected(fn(nbytes=ws - 1), "workspace")
        rejected(fn(cache=odd), "aligned")
        rejected(fn(work=odd), "aligned")
    rejected(moments(count=null), "null")
    rejected(moments(sums=null), "null")
    rejected(moments(pivot=ok), "together")
    rejected(moments(pivot=odd, sumsq=ok), "misaligned")
    rejected(gram(pivot=null), "null")
    rejected(gram(out=null), "null")
    rejected(gram(pivot=odd), "misaligned")
    for bad in ({"x": null}, {"w": null}, {"b": null}, {"y": null}):
        rejected(project(**bad), "null")
    rejected(project(pixels=0), "sizes")
    rejected(project(K=0), "sizes")
    rejected(project(cs=36), "multiple of 8")
    rejected(project(cs=lib.hpri_band_max_cs() + 8), "multiple of 8")
    rejected(project(K=lib.hpri_band_project_max_k() + 1), "max_k")
    rejected(project(cs=lib.hpri_band_max_cs(), K=64), "LDS")
    rejected(project(x=odd), "aligned")
    rejected(project(y=odd), "aligned")
    for bad in ({"x": null}, {"s": null}, {"t": null}, {"y": null}):
        rejected(affine(**bad), "null")
    rejected(affine(pixels=-1), "sizes")
    rejected(affine(cs=12), "multiple of 8")
    rejected(affine(C=41), "multiple of 8")
    rejected(affine(C=0), "multiple of 8")
    rejected(affine(y=odd), "aligned")
    with pytest.raises(RuntimeError, match="band_project"):
        _lib.call("hpri_band_project", null, 1, 8, null, null, 1, null, null)


def test_projection_rejects_what_it_cannot_take_without_a_device():
    st, _, _ = _geometric_stats(C=80)
    with pytest.raises(ValueError, match="exceeds"):
        S.SpectralProjection(np.zeros((S.project_max_k() + 1, 80), dtype=np.float32), np.zeros(S.project_max_k() + 1, dtype=np.float32))
    with pytest.raises(ValueError):
        S.SpectralProjection(np.zeros((4, 8)), np.zeros(5))
    with pytest.raises(ValueError, match="finite"):
        S.SpectralProjection(np.full((4, 8), np.nan), np.zeros(4))
    import torch
    p = S.SpectralProjection.pca(st, 6)
    assert not p.diagonal and p.in_channels == 80 and p.out_channels == 6 and len(p.explained_variance) == 6
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        p(torch.zeros(1, 80, 4, 4))
    # the state dict carries the preprocessing
    sd = p.state_dict()
    assert sorted(sd) == ["bias", "weight"]
    q = S.SpectralProjection(np.zeros((6, 80)), np.zeros(6))
    q.load_state_dict(sd)
    assert torch.equal(q.weight, p.weight) and torch.equal(q.bias, p.bias)
    z = S.SpectralProjection.standardize(st, eps=1e-6)
    assert z.diagonal and z.in_channels == z.out_channels == 80
    s = 1.0 / np.sqrt(np.diag(st.cov) + 1e-6)
    assert np.array_equal(z.weight.numpy(), s.astype(np.float32)) and np.array_equal(z.bias.numpy(), (-st.mean * s).astype(np.float32))


def test_new_kernels_hold_everything_in_registers():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_codeobj
    rep = check_codeobj.run()
    rows = [k for k in rep["kernels"] if k["file"] == "spectral.hip"]
    names = " ".join(k["demangled"] + " " + k["name"] for k in rows)      # (the demangler at hand may leave the _Float16 instantiations mangled)
    for kernel in ("band_moments_kernel<float>", "band_moments_kernelIDF16_", "band_gram_kernel<float, 14>", "band_gram_kernelIDF16_Li14E",
                   "band_project_kernel", "band_affine_kernel", "band_moments_finish_kernel", "band_gram_finish_kernel"):
        assert kernel in names, kernel
    assert len(rows) >= 18                                 # six Gram instantiations per slot type
    for k in rows:
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
