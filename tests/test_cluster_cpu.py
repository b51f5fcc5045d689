"""Spectral k-means, the parts that need no GPU: the numpy restatement (tie rule, a planted mixture), the initialisations, the merge,
the state dict, every argument error of the C ABI and of the Python layer, the compiler's report on the new kernels, and the
conditions the GPU tests rely on for their inputs (tests/_cluster_cases.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _cluster_cases as cases
from hyperpri_amd import cluster as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ties_go_to_the_lowest_index():
    # centroids 0 and 2 coincide, 1 and 3 are mirror images about the origin: integers, every fp64 value exact
    g = np.array([[2, 0, 0], [0, 2, 0], [2, 0, 0], [0, -2, 0]], dtype=np.float32)
    w, b = K.score_rows(g)
    assert np.array_equal(w, -g) and np.array_equal(b, np.full(4, 2.0, np.float32))
    x = np.array([[2, 0, 0], [1, 0, 0], [0, 0, 1], [0, 3, 0], [0, -1, 0], [1, 1, 0]], dtype=np.float32)
    labels, z, amb = K.assign_reference(x, None, w, b)
    #            at centroid 0 = 2; nearer to 0 = 2; equidistant from all four; 1; 3; equidistant from 0, 1, 2
    assert list(labels) == [0, 0, 0, 1, 3, 0]
    assert list(amb) == [True, True, True, False, False, True]      # an exact tie or a duplicate of the winner is flagged
    assert np.array_equal(2 * z[np.arange(6), labels] + (x.astype(np.float64) ** 2).sum(axis=1), [0, 1, 5, 1, 1, 2])
    # with a pivot: d = x - pivot
    l2, z2, _ = K.assign_reference(x + 1, np.ones(3, np.float32), w, b)
    assert np.array_equal(l2, labels) and np.array_equal(z2, z)
    # a lone pixel far from the others' centroid is not ambiguous
    _, _, amb = K.assign_reference(np.array([[0, 5, 0]], np.float32), None, w[[0, 1]], b[[0, 1]])
    assert not amb.any()


def test_kmeans_reference_recovers_a_planted_mixture():
    case = cases.e2e_case()
    ref = K.kmeans_reference(case["cubes"], case["init"])
    assert ref.converged and 2 <= ref.n_iter <= 10
    assert np.array_equal(ref.labels, case["truth"].reshape(-1))
    got = ref.pivot.astype(np.float64) + ref.centers.astype(np.float64)
    n_k = np.bincount(case["truth"].reshape(-1), minlength=cases.E2E["K"])
    assert np.array_equal(ref.final.counts, n_k)
    # the mean of n_k pixels lies within a few standard errors of the planted centroid
    assert (np.abs(got - case["centroids"]) <= 6 * cases.E2E["noise"] / np.sqrt(n_k)[:, None]).all()
    x = case["cubes"].reshape(-1, cases.E2E["C"]).astype(np.float64)
    inertia = ((x - got[ref.labels]) ** 2).sum()
    assert abs(ref.final.inertia - inertia) <= 1e-6 * inertia
    # the stopping rule: one iteration at most when the tolerance is huge, max_iter binds when it is zero and the centres still move
    assert K.kmeans_reference(case["cubes"], case["init"], tol=1e9).n_iter == 1
    short = K.kmeans_reference(case["cubes"], case["init"], tol=0.0, max_iter=1)
    assert short.n_iter == 1 and not short.converged


def test_the_e2e_case_meets_no_ambiguous_pixel():
    """The condition of the end-to-end GPU test: identical labels can be demanded only where rounding cannot change one."""
    case = cases.e2e_case()
    assert K.kmeans_reference(case["cubes"], case["init"]).ambiguous == 0
    s = cases.sums_case()
    _, labels, amb = K.cluster_step_reference(s["cubes"], s["pivot"], s["centers"], return_ambiguous=True)
    assert not amb.any() and np.array_equal(labels, s["truth"].reshape(-1))


@pytest.mark.parametrize("C,Kc", cases.UNIFORM_CASES)
def test_the_uniform_cases_are_rarely_ambiguous(C, Kc):
    """The condition of the real-valued GPU tests: at most 0.5 % of the pixels of a ``uniform`` case are flagged."""
    case = cases.uniform_case(C, Kc)
    w, b = K.score_rows(case["centers"])
    _, _, amb = K.assign_reference(case["cubes"], case["pivot"], w, b)
    share = amb.mean()
    print(f"uniform C={C} K={Kc}: ambiguous share {100 * share:.3f} %")
    assert share <= 0.005
    if C == 20:
        assert share == 0


def test_initialisations_are_deterministic_per_seed():
    rng = np.random.RandomState(0)
    sample = rng.randn(500, 7)
    for init in K.INITS:
        a, b, c = (K.init_centers(sample, 6, init, seed) for seed in (3, 3, 4))
        assert a.shape == (6, 7) and np.array_equal(a, b) and not np.array_equal(a, c)
        # every centre is a sample pixel, and no pixel is taken twice
        rows = [int(np.nonzero((sample == r).all(axis=1))[0][0]) for r in a]
        assert len(set(rows)) == 6
    # D^2 sampling spreads: on two tight, distant blobs the second centre comes from the other blob
    blobs = np.concatenate([0.01 * rng.randn(200, 3), 10 + 0.01 * rng.randn(200, 3)])
    for seed in range(5):
        c = K.init_centers(blobs, 2, "k-means++", seed)
        assert abs(c[0, 0] - c[1, 0]) > 5
    # identical pixels: no distance to sample by, still k rows
    assert K.init_centers(np.ones((10, 2)), 3, "k-means++", 0).shape == (3, 2)
    with pytest.raises(ValueError, match="init"):
        K.init_centers(sample, 3, "random", 0)
    with pytest.raises(ValueError, match="at least"):
        K.init_centers(sample[:2], 3, "sample", 0)


def test_merge_cluster_sums():
    case = cases.e2e_case()
    x, pv, c = case["cubes"], case["pivot"], case["centers"]
    whole = K.cluster_step_reference(x, pv, c)
    a, b = K.cluster_step_reference(x[:1], pv, c), K.cluster_step_reference(x[1:], pv, c)
    m = K.merge_cluster_sums(a, b)
    assert np.array_equal(m.counts, whole.counts) and m.counts.dtype == np.int64
    assert np.allclose(m.sums, whole.sums, rtol=0, atol=1e-9) and abs(m.inertia - whole.inertia) <= 1e-9 * whole.inertia
    assert m.inertia == m.sq_sum + 2 * m.score_sum
    with pytest.raises(ValueError, match="shapes"):
        K.merge_cluster_sums(a, K.ClusterSums(a.counts[:2], a.sums[:2], 0.0, 0.0))
    # selections partition the pixels
    fg = K.cluster_step_reference(x, pv, c, case["masks"], "foreground")
    bg = K.cluster_step_reference(x, pv, c, case["masks"], "background")
    assert np.array_equal(fg.counts + bg.counts, whole.counts)
    assert fg.counts[0] == fg.counts.sum()               # the mask is component 0


def test_state_dict_round_trip_and_blank():
    rng = np.random.RandomState(1)
    m = K.SpectralKMeans(rng.rand(11), rng.randn(4, 11), counts=[5, 0, 7, 9], foreground_share=[0.1, 0.5, 0.9, 1.0], meta=(7, 12.5, 1))
    sd = m.state_dict()
    assert sorted(sd) == ["bias", "centers", "counts", "foreground_share", "meta", "pivot"]
    assert sd["pivot"].dtype == torch.float32 and sd["centers"].dtype == torch.float32 and sd["bias"].dtype == torch.float32
    assert sd["counts"].dtype == torch.int64 and sd["foreground_share"].dtype == torch.float64
    blank = K.SpectralKMeans.blank(11, 4)
    assert torch.isnan(blank.foreground_share).all() and blank.n_iter_ == 0 and not blank.converged_
    blank.load_state_dict(sd)
    for name in sd:
        assert getattr(blank, name).numpy().tobytes() == getattr(m, name).numpy().tobytes(), name
    assert (blank.n_iter_, blank.inertia_, blank.converged_, blank.k, blank.in_channels) == (7, 12.5, True, 4, 11)
    assert blank.centroids.dtype == np.float64
    assert np.array_equal(blank.centroids, m.pivot.numpy().astype(np.float64) + m.centers.numpy().astype(np.float64))
    c64 = m.centers.numpy().astype(np.float64)
    assert np.array_equal(m.bias.numpy(), (0.5 * (c64 ** 2).sum(axis=1)).astype(np.float32))
    with pytest.raises(RuntimeError):
        K.SpectralKMeans.blank(11, 5).load_state_dict(sd)


def test_python_argument_errors_come_before_any_device_call():
    m = K.SpectralKMeans(np.zeros(8), np.zeros((3, 8)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 8, 4, 4))
    with pytest.raises(ValueError, match="output"):
        m(torch.zeros(1, 8, 4, 4), output="probability")
    with pytest.raises(ValueError, match="exceeds"):
        K.SpectralKMeans(np.zeros(8), np.zeros((K.MAX_K + 1, 8)))
    with pytest.raises(ValueError, match="finite"):
        K.SpectralKMeans(np.zeros(8), np.full((3, 8), np.nan))
    with pytest.raises(ValueError, match="pivot"):
        K.SpectralKMeans(np.zeros(7), np.zeros((3, 8)))
    with pytest.raises(ValueError, match="centers"):
        K.SpectralKMeans(np.zeros(8), np.zeros(8))
    with pytest.raises(TypeError, match="CubeCache"):
        K.cluster_step(object(), np.zeros(8), np.zeros((3, 8)))
    with pytest.raises(ValueError, match="select"):
        K.cluster_step(object(), np.zeros(8), np.zeros((3, 8)), select="roots")
    with pytest.raises(TypeError, match="CubeCache"):
        K.SpectralKMeans.fit(object(), 3)
    with pytest.raises(ValueError, match="select"):
        K.SpectralKMeans.fit(object(), 3, select="roots")
    assert K.max_k() == K.MAX_K == 64 and K.cluster_parts() == 256


def test_argument_errors_return_minus_one_before_any_launch():
    from hyperpri_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    ok = ctypes.c_void_p(4096)                            # an aligned non-null address: never dereferenced on the host
    odd = ctypes.c_void_p(4100)                           # 4-byte aligned only
    odder = ctypes.c_void_p(4098)
    ws = lib.hpri_band_cluster_workspace_bytes(40, 5)
    assert ws > 0 and ws == lib.hpri_band_cluster_workspace_bytes(40, 32) < lib.hpri_band_cluster_workspace_bytes(40, 33)
    for cs, k in ((36, 5), (0, 5), (lib.hpri_band_max_cs() + 8, 5), (40, 0), (40, 65)):
        assert lib.hpri_band_cluster_workspace_bytes(cs, k) == 0

    def rejected(rc, word):
        msg = lib.hpri_last_error()
        assert rc == -1 and word.encode() in msg, (rc, msg)

    def assign(x=ok, pixels=100, cs=40, pivot=ok, centers=ok, bias=ok, k=5, lut=null, labels=ok, zmin=null, dist2=null, value=null):
        return lib.hpri_band_assign(x, pixels, cs, pivot, centers, bias, k, lut, labels, zmin, dist2, value, null)

    for bad in ({"x": null}, {"centers": null}, {"bias": null}):
        rejected(assign(**bad), "null")
    rejected(assign(pixels=0), "sizes")
    rejected(assign(cs=36), "multiple of 8")
    rejected(assign(cs=0), "multiple of 8")
    rejected(assign(cs=lib.hpri_band_max_cs() + 8), "multiple of 8")
    rejected(assign(k=0), "max_k")
    rejected(assign(k=65), "max_k")
    rejected(assign(labels=null), "nothing")
    rejected(assign(value=ok), "lut")
    rejected(assign(lut=ok), "lut")
    for bad in ({"x": odd}, {"pivot": odd}, {"centers": odd}, {"bias": odd}, {"zmin": odder}, {"dist2": odder}, {"value": odder, "lut": ok},
                {"value": ok, "lut": odder}):
        rejected(assign(**bad), "misaligned")

    def sums(cache=ok, dtype=0, slots=4, Hs=13, Ws=11, cs=40, masks=ok, table=ok, n=3, select=0, pivot=ok, centers=ok, bias=ok, k=5, work=ok,
             nbytes=ws, counts=ok, out=ok, totals=ok):
        return lib.hpri_band_cluster_sums(cache, dtype, slots, Hs, Ws, cs, masks, table, n, select, pivot, centers, bias, k, work, nbytes,
                                          counts, out, totals, null)

    for bad in ({"cache": null}, {"table": null}, {"work": null}, {"centers": null}, {"bias": null}, {"counts": null}, {"out": null},
                {"totals": null}):
        rejected(sums(**bad), "null")
    rejected(sums(dtype=2), "dtype")
    rejected(sums(dtype=-1), "dtype")
    for bad in ({"slots": 0}, {"Hs": 0}, {"Ws": -1}, {"n": 0}):
        rejected(sums(**bad), "sizes")
    rejected(sums(cs=36), "multiple of 8")
    rejected(sums(cs=0), "multiple of 8")
    rejected(sums(cs=lib.hpri_band_max_cs() + 8), "multiple of 8")
    rejected(sums(select=3), "select")
    rejected(sums(select=-1), "select")
    rejected(sums(select=1, masks=null), "masks")
    rejected(sums(k=0), "max_k")
    rejected(sums(k=65), "max_k")
    rejected(sums(nbytes=ws - 1), "workspace")
    rejected(sums(k=33), "workspace")
    rejected(sums(cache=odd), "aligned")
    rejected(sums(work=odd), "aligned")
    for bad in ({"pivot": odd}, {"centers": odd}, {"bias": odd}, {"counts": odd}, {"out": odd}, {"totals": odd}):
        rejected(sums(**bad), "misaligned")
    with pytest.raises(RuntimeError, match="band_assign"):
        _lib.call("hpri_band_assign", null, 1, 8, null, null, null, 1, null, null, null, null, null, null)


def test_new_kernels_hold_everything_in_registers():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_codeobj
    rep = check_codeobj.run()
    rows = [k for k in rep["kernels"] if k["file"] == "cluster.hip"]
    names = " ".join(k["demangled"] for k in rows)
    # (the half-precision instantiations keep their mangled names where the demangler does not know _Float16)
    for kernel in ("band_assign_kernel<1, true>", "band_assign_kernel<4, false>", "band_cluster_kernel<float, 1>", "band_cluster_kernelIDF16_Li4EE",
                   "band_cluster_finish_kernel"):
        assert kernel in names, kernel
    assert len(rows) == 8 + 8 + 1                        # assign: four widths with and without the distance; sums: four widths, two slot types
    for k in rows:
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0, k
        assert k["hot"] or "finish" in k["demangled"] or "DF16_" in k["name"]
    # the report still holds the kernels that moved their helpers into band_common.h
    assert sum(k["file"] == "spectral.hip" for k in rep["kernels"]) >= 18
