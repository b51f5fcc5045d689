"""Spectral detectors, the parts that need no GPU: the numpy restatement of the contract against the textbook formulas, the
host-side fit (whiteners, filter rows, column extents), every argument error of the C ABI, the constructor's errors, the state
dict, and the compiler's report on the new kernels."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from hyperpri_amd import detect as D
from hyperpri_amd import spectral as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(C=12, seed=0, n=1000):
    """A well-conditioned synthetic covariance (eigenvalues in [0.5, 2.5]) and a mean."""
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.randn(C, C))
    lam = 0.5 + 2.0 * rng.rand(C)
    return S.SpectralStats(n, rng.randn(C), (Q * lam) @ Q.T, "background"), rng


def _scores64(stats, targets, x, whitener="cholesky", rank=None, shrink=0.0):
    """RX, ACE and SMF of pixels x (P, C) in fp64 through whitener_reference, filter_rows and detect_reference."""
    W, b = D.whitener_reference(stats.mean, stats.cov, whitener, shrink=shrink, rank=rank)
    Kq = W.shape[0]
    out = {}
    for kind in ("ace", "smf"):
        f, g = D.filter_rows(W, b, targets, kind)
        q, t = D.detect_reference(x, np.vstack([W, f]), np.concatenate([b, g]), Kq, score=1 if kind == "ace" else 0)
        out[kind] = t
    out["rx"] = q
    return out


def test_reference_agrees_with_the_textbook_formulas():
    st, rng = _stats()
    C = 12
    tg = st.mean + rng.randn(3, C)
    x = st.mean + rng.randn(40, C) @ np.linalg.cholesky(st.cov).T
    got = _scores64(st, tg, x)
    d = (x - st.mean).T                                       # (C, P)
    si = np.linalg.solve(st.cov, d)                           # S^-1 (x - mu)
    rx = (d * si).sum(axis=0)
    assert np.abs(got["rx"] - rx).max() <= 1e-10 * rx.max()
    s = (tg - st.mean).T                                      # (C, T)
    ss = (s * np.linalg.solve(st.cov, s)).sum(axis=0)         # s^T S^-1 s
    sx = s.T @ si                                             # (T, P)
    assert np.abs(got["ace"] - sx / np.sqrt(ss[:, None] * rx[None, :])).max() <= 1e-10
    assert np.abs(got["smf"] - sx / ss[:, None]).max() <= 1e-10
    # a target scores ACE = 1 and SMF = 1, the background mean SMF = 0
    own = _scores64(st, tg, tg)
    assert np.abs(np.diag(own["ace"]) - 1).max() <= 1e-12 and np.abs(np.diag(own["smf"]) - 1).max() <= 1e-12
    assert np.abs(_scores64(st, tg, st.mean[None])["smf"]).max() <= 1e-12
    # the logit form: the clamp and the rx map's p = q / (q + Kq)
    W, b = D.whitener_reference(st.mean, st.cov)
    f, g = D.filter_rows(W, b, tg[:1], "ace")
    q, t = D.detect_reference(x, np.vstack([W, f]), np.concatenate([b, g]), C, score=1, logit=True)
    p = np.clip(got["ace"][:1], 2.0 ** -24, 1 - 2.0 ** -24)
    assert np.allclose(t, np.log(p / (1 - p)), rtol=1e-9, atol=1e-9)
    assert np.allclose(q, np.log(rx / C), rtol=1e-9, atol=1e-9)          # logit(q / (q + Kq)) = log(q / Kq)
    assert t.min() == np.log(2.0 ** -24) - np.log1p(-2.0 ** -24)         # a negative cosine is clamped
    # the identity metric
    q, t = D.detect_reference(x, None, None, 0, filters=tg / np.linalg.norm(tg, axis=1)[:, None], score=1)
    cos = (x @ tg.T).T / (np.linalg.norm(x, axis=1)[None] * np.linalg.norm(tg, axis=1)[:, None])
    assert np.allclose(q, (x * x).sum(axis=1), rtol=1e-13) and np.abs(t - cos).max() <= 1e-12
    q, t = D.detect_reference(np.zeros((2, C)), None, None, 0, filters=tg, score=1)
    assert not t.any() and not q.any()                                   # q == 0: the cosine is 0


@pytest.mark.parametrize("whitener", ["cholesky", "pca"])
def test_scores_are_invariant_under_an_affine_map_of_the_bands(whitener):
    st, rng = _stats(C=10, seed=3)
    C = 10
    tg = st.mean + rng.randn(2, C)
    x = st.mean + 2.0 * rng.randn(30, C)
    A = np.eye(C) + 0.3 * rng.randn(C, C) / np.sqrt(C)
    assert np.linalg.cond(A) < 10
    a = rng.randn(C)
    st2 = S.SpectralStats(st.count, A @ st.mean + a, A @ st.cov @ A.T, st.select)
    one, two = _scores64(st, tg, x, whitener), _scores64(st2, tg @ A.T + a, x @ A.T + a, whitener)
    for k in ("rx", "ace", "smf"):
        assert np.abs(one[k] - two[k]).max() <= 1e-9 * max(1.0, np.abs(one[k]).max()), k


def test_the_fit_matches_its_restatement_and_pca_equals_cholesky_at_full_rank():
    st, rng = _stats(C=37, seed=5)
    C = 37
    tg = st.mean + rng.randn(2, C)
    x = st.mean + rng.randn(25, C)
    one, two = _scores64(st, tg, x, "cholesky"), _scores64(st, tg, x, "pca")
    assert np.abs(one["rx"] - two["rx"]).max() <= 1e-9 * one["rx"].max()
    for whitener, rank, shrink in (("cholesky", None, 0.0), ("cholesky", None, 1e-3), ("pca", None, 1e-3), ("pca", 9, 0.0)):
        det = D.SpectralDetector.from_statistics(st, tg, whitener=whitener, shrink=shrink, rank=rank)
        W, b = D.whitener_reference(st.mean, st.cov, whitener, shrink=shrink, rank=rank)
        assert det.rank == (rank or C) and det.num_targets == 2 and det.in_channels == C and det.whitener == whitener
        # rounded once: fp32 of the fp64 fit, which agrees with the library restatement far below an fp32 ulp
        assert np.abs(det.weight.numpy() - W).max() <= 1e-6 * np.abs(W).max() and np.abs(det.bias.numpy() - b).max() <= 1e-6 * np.abs(b).max()
        Sr = st.cov + shrink * np.trace(st.cov) / C * np.eye(C)
        assert np.abs(W @ Sr @ W.T - np.eye(W.shape[0])).max() <= 1e-9
        for kind in ("ace", "smf"):
            f, g = D.filter_rows(W, b, tg, kind)
            assert np.abs(getattr(det, kind + "_weight").numpy() - f).max() <= 1e-6 * np.abs(f).max()
            assert np.abs(getattr(det, kind + "_bias").numpy() - g).max() <= 1e-6 * max(1.0, np.abs(g).max())
        assert np.allclose(np.linalg.norm(det.sam_weight.numpy().astype(np.float64), axis=1), 1.0, rtol=1e-6)


def test_cholesky_is_lower_triangular_and_the_extents_follow_the_zero_pattern():
    C = 37
    st, rng = _stats(C=C, seed=7)
    det = D.SpectralDetector.from_statistics(st, st.mean + rng.randn(C), shrink=0.0)
    w = det.weight.numpy()
    assert not np.triu(w, 1).any() and (np.diag(w) > 0).all()
    cs = 40
    wp, bp, cend = det.host_weights("ace", cs)
    assert wp.shape == (40, cs) and bp.shape == (40,) and not wp[38:].any() and not wp[:, C:].any() and not bp[38:].any()
    assert np.array_equal(wp[:C, :C], w) and np.array_equal(wp[C, :C], det.ace_weight.numpy()[0])
    # rows 0..15 end at column 16, rows 16..31 at 32, the last block holds the dense filter row
    assert list(cend) == [16, 32, 40]
    for rb, ce in enumerate(cend):
        assert ce % 8 == 0 and not wp[16 * rb:16 * rb + 16, ce:].any()
        assert ce == 8 or wp[16 * rb:16 * rb + 16, ce - 8:ce].any()
    assert list(det.host_weights("rx", cs)[2]) == [16, 32, 40]              # the last block: rows 32..36 reach column 37
    assert list(D.column_extents(np.zeros((16, 24), np.float32), 24)) == [8]
    # the pca whitener is dense
    pca = D.SpectralDetector.from_statistics(st, st.mean + 1.0, whitener="pca", rank=20)
    assert list(pca.host_weights("smf", cs)[2]) == [40, 40]


def test_argument_errors_return_minus_one_before_any_launch():
    from hyperpri_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    ok = ctypes.c_void_p(4096)                            # an aligned non-null address: never dereferenced on the host
    odd = ctypes.c_void_p(4100)                           # 4-byte aligned only
    odder = ctypes.c_void_p(4098)
    assert lib.hpri_band_detect_max_targets() == 8 == D.max_targets()

    def extents(*v):
        return ctypes.cast((ctypes.c_int * len(v))(*v), ctypes.c_void_p)

    def detect(x=ok, pixels=100, cs=40, w=ok, b=ok, ks=40, Kq=37, T=1, filters=null, cend=null, score=0, q=ok, scores=ok):
        return lib.hpri_band_detect(x, pixels, cs, w, b, ks, Kq, T, filters, cend, score, q, scores, null)

    def identity(**kw):
        args = dict(w=null, b=null, ks=0, Kq=0, T=2, filters=ok, score=1)
        args.update(kw)
        return detect(**args)

    def rejected(rc, word):
        msg = lib.hpri_last_error()
        assert rc == -1 and word.encode() in msg, (rc, msg)

    rejected(detect(x=null), "null")
    rejected(detect(b=null), "bias")
    rejected(detect(filters=ok), "bias")
    rejected(detect(pixels=0), "sizes")
    rejected(detect(Kq=-1), "sizes")
    rejected(detect(cs=36), "multiple of 8")
    rejected(detect(cs=0), "multiple of 8")
    rejected(detect(cs=lib.hpri_band_max_cs() + 8), "multiple of 8")
    rejected(detect(T=9), "max_targets")
    rejected(detect(T=-1), "max_targets")
    rejected(detect(score=4), "score")
    rejected(detect(score=-1), "score")
    rejected(detect(scores=null), "score planes")
    rejected(detect(T=0), "score planes")
    rejected(detect(T=0, scores=null, q=null), "nothing")
    rejected(detect(Kq=0), "Kq")
    rejected(detect(Kq=41, ks=48), "Kq")
    rejected(detect(Kq=40, T=1), "fit")
    rejected(detect(ks=32), "fit")
    rejected(detect(ks=0), "fit")
    for bad in ({"x": odd}, {"w": odd}, {"b": odd}, {"q": odder}, {"scores": odder}):
        rejected(detect(**bad), "misaligned")
    rejected(detect(cend=extents(16, 32, 12)), "extent")
    rejected(detect(cend=extents(16, 0, 40)), "extent")
    rejected(detect(cend=extents(16, 32, 48)), "extent")
    rejected(identity(Kq=3), "identity")
    rejected(identity(cend=extents(40)), "identity")
    rejected(identity(filters=null), "filters")
    rejected(identity(T=0, scores=null, filters=ok), "filters")
    rejected(identity(filters=odd), "misaligned")
    rejected(identity(b=odder), "misaligned")
    rejected(identity(T=9), "max_targets")
    with pytest.raises(RuntimeError, match="band_detect"):
        _lib.call("hpri_band_detect", null, 1, 8, null, null, 0, 0, 0, null, null, 0, null, null, null)


def test_constructor_errors():
    st, rng = _stats(C=8, seed=9)
    tg = st.mean + 1.0
    v = rng.randn(8)
    singular = S.SpectralStats(100, st.mean, np.outer(v, v), "background")
    for whitener in ("cholesky", "pca"):
        with pytest.raises(ValueError, match="shrink"):
            D.SpectralDetector.from_statistics(singular, tg, whitener=whitener, shrink=0.0)
        D.SpectralDetector.from_statistics(singular, tg, whitener=whitener, shrink=1e-3)       # the shrinkage repairs it
    with pytest.raises(ValueError, match="shrink"):
        D.SpectralDetector.from_statistics(S.SpectralStats(100, st.mean, np.full((8, 8), np.nan)), tg)
    with pytest.raises(ValueError, match="exceeds"):
        D.SpectralDetector.from_statistics(st, st.mean + rng.randn(D.max_targets() + 1, 8))
    with pytest.raises(ValueError, match="exceeds"):
        D.SpectralDetector.sam(np.ones((D.max_targets() + 1, 8)))
    with pytest.raises(ValueError, match="bands"):
        D.SpectralDetector.from_statistics(st, np.ones(7))
    with pytest.raises(ValueError, match="bands"):
        D.SpectralDetector(np.eye(8), np.zeros(8), np.ones((1, 7)))
    with pytest.raises(ValueError, match="background mean"):
        D.SpectralDetector.from_statistics(st, st.mean)
    with pytest.raises(ValueError, match="rank"):
        D.SpectralDetector.from_statistics(st, tg, whitener="pca", rank=9)
    with pytest.raises(ValueError, match="whitener"):
        D.SpectralDetector.from_statistics(st, tg, whitener="zca")
    with pytest.raises(ValueError, match="zero"):
        D.SpectralDetector.sam(np.zeros((1, 8)))
    det = D.SpectralDetector.from_statistics(st, tg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        det(torch.zeros(1, 8, 4, 4))
    with pytest.raises(ValueError, match="score"):
        det(torch.zeros(1, 8, 4, 4), score="osp")


def test_state_dict_round_trip_is_bitwise():
    st, rng = _stats(C=11, seed=11)
    tg = st.mean + rng.randn(3, 11)
    for det, blank in ((D.SpectralDetector.from_statistics(st, tg, shrink=1e-3), D.SpectralDetector.blank(11, 3)),
                       (D.SpectralDetector.from_statistics(st, tg, whitener="pca", rank=4), D.SpectralDetector.blank(11, 3, rank=4, whitener="pca")),
                       (D.SpectralDetector.sam(tg), D.SpectralDetector.blank(11, 3, whitener="identity"))):
        sd = det.state_dict()
        assert sorted(sd) == ["ace_bias", "ace_weight", "bias", "meta", "sam_weight", "smf_bias", "smf_weight", "targets", "weight"]
        blank.load_state_dict(sd)
        for name in sd:
            assert getattr(blank, name).numpy().tobytes() == getattr(det, name).numpy().tobytes(), name
        assert blank.whitener == det.whitener and blank.rank == det.rank
        assert blank.targets.dtype == torch.float32 and np.array_equal(blank.targets.numpy(), tg.astype(np.float32))


def test_new_kernels_hold_everything_in_registers():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_codeobj
    rep = check_codeobj.run()
    rows = [k for k in rep["kernels"] if k["file"] == "detect.hip"]
    names = " ".join(k["demangled"] + " " + k["name"] for k in rows)
    for kernel in ("band_detect_kernel<true>", "band_detect_kernel<false>"):
        assert kernel in names, kernel
    assert len(rows) == 2
    for k in rows:
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
