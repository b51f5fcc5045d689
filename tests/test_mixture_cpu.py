"""Conditions on the numpy restatement of the spectral Gaussian mixtures (hyperpri_amd/mixture.py) and on the inputs of the GPU tests
(tests/_mixture_cases.py): the reference is the density it claims to be, EM never loses likelihood, one component is the moments
pass, the ladder scene separates what it is built to separate, an fp32 emulation of the chains stays inside ``gmm_bound``, and the
integer cases are exact.  No GPU."""
import numpy as np
import pytest

import _mixture_cases as cases
from hyperpri_amd import mixture as M
from hyperpri_amd import spectral as S

U = 2.0 ** -24


def _ops(model):
    return M.gmm_operands(model["pivot"], model["weight"], model["means"], model["covariances"], model["weights"], model["classes"])


def _logpdf(z, mean, cov):
    try:
        from scipy.stats import multivariate_normal
        return multivariate_normal.logpdf(z, mean=mean, cov=cov).reshape(-1)
    except ImportError:
        e = z - mean
        return -0.5 * (np.einsum("pi,pi->p", e, np.linalg.solve(cov, e.T).T) + np.linalg.slogdet(cov)[1] + len(mean) * np.log(2 * np.pi))


@pytest.mark.parametrize("C,q,K,classes", cases.SCORE_CASES[:4])
def test_score_reference_is_the_density(C, q, K, classes):
    """Against an independent evaluation of the Gaussian densities (scipy's ``multivariate_normal.logpdf`` where scipy imports, else
    ``slogdet`` / ``solve``) on the fp64 projection: the reference works from A = L^-1 rounded to fp32, a relative 2^-24 of terms
    that add up to m, so 1e-5 (1 + m) is ample."""
    cubes, _, model = cases.model_case(C, q, K, classes, H=9, W=11)
    ops = _ops(model)
    ref = M.gmm_score_reference(cubes, ops)
    z = (cubes.reshape(-1, C) - model["pivot"]).astype(np.float64) @ model["weight"].astype(np.float64).T
    assert np.abs(ref["z"] - z).max() <= 1e-12 * np.abs(z).max()
    want = np.stack([np.log(model["weights"][k]) + _logpdf(z, ops.means[k].astype(np.float64), model["covariances"][k]) for k in range(K)], axis=1)
    assert (np.abs(ref["l"] - want) <= 1e-5 * (1 + ref["m"])).all()
    mx = want.max(axis=1)
    total = mx + np.log(np.exp(want - mx[:, None]).sum(axis=1))
    assert (np.abs(-ref["nll"] - total) <= 1e-5 * (1 + ref["m"].min(axis=1))).all()
    assert np.abs(ref["resp"].sum(axis=1) - 1).max() <= 1e-12
    assert np.abs(np.log(np.exp(ref["loglik"]).sum(axis=1)) - total).max() <= 1e-4
    assert ref["loglik"].shape == (cubes[0].size // C, classes) and ref["labels"].max() < classes


def _ladder(components):
    cubes, masks, _ = cases.ladder_scene()
    L = cases.LADDER
    fit = list(L["fit"])
    st = S.statistics_reference(cubes[fit])
    W = S.pca_basis(st, L["q"], whiten=True)[0]
    pivot = st.mean.astype(np.float32)
    inits = cases.ladder_inits(cubes, masks, pivot, W, components)
    ops, fits = M.gmm_classes_reference(cubes[fit], masks[fit], pivot, W, inits)
    ref = M.gmm_score_reference(cubes[L["held_out"]], ops)
    return cases.best_dice(ref["logit"], masks[L["held_out"]]), fits


def test_ladder_needs_a_mixture_per_class():
    """What the end-to-end GPU test asserts of the device holds for the fp64 twin with wide room: one Gaussian per class cannot
    separate interleaved materials (0.51 here), three soils and two roots can (0.97)."""
    single, fits1 = _ladder((1, 1))
    mixed, fits = _ladder((3, 2))
    assert single < 0.6 and mixed > 0.9, (single, mixed)
    assert all(f.n_iter == 1 for f in fits1)
    assert all(not f.starved and f.converged for f in fits)
    for f in fits:                                              # EM never loses likelihood
        assert (np.diff(f.history) >= -1e-9).all(), f.history


def test_em_never_loses_likelihood_from_a_poor_start():
    cubes, masks, model = cases.model_case(37, 5, 3, 1, H=20, W=25)
    z = (cubes.reshape(-1, 37) - model["pivot"]).astype(np.float64) @ model["weight"].astype(np.float64).T
    start = M.hard_init(z, z[[0, 1, 2]])
    fit = M.gmm_reference(cubes, model["pivot"], model["weight"], start, max_iter=25, tol=0.0)
    assert len(fit.history) >= 3 and (np.diff(fit.history) >= -1e-9).all(), fit.history
    assert abs(fit.weights.sum() - 1) <= 1e-12


@pytest.mark.parametrize("select", ["all", "foreground", "background"])
def test_one_component_is_the_moments_pass(select):
    """K = 1: r = 1, so the M-step of a single pass gives the mean and the (biased) covariance of the projected pixels, whatever the
    start -- ``statistics_reference``'s, projected.  The reference rounds d = x - pivot to fp32 as the device does, the statistics do
    not: a relative 2^-24 of every d[c], so the means agree within u |W| max |d| and the second moments within a few u of theirs."""
    cubes, masks, model = cases.model_case(37, 5, 1, 1, n=2, H=12, W=13)
    ops = M.gmm_operands(model["pivot"], model["weight"], np.full((1, 5), 0.25), np.eye(5)[None] * 2.0, [1.0])
    s = M.gmm_step_reference(cubes, ops, masks, select)
    st = S.statistics_reference(cubes, masks, select)
    W = ops.weight.astype(np.float64)
    n = st.count
    assert s.count == n and abs(s.N[0] - n) <= 1e-9 * n
    mean = ops.means[0].astype(np.float64) + s.S[0] / s.N[0]
    want_mean = W @ (st.mean - ops.pivot.astype(np.float64))
    dmax = np.abs(S._selected_pixels(cubes, masks, select) - ops.pivot.astype(np.float64)).max(axis=0)
    assert (np.abs(mean - want_mean) <= U * (np.abs(W) @ dmax) + 1e-12).all()
    cov = s.Q[0] / s.N[0] - np.outer(s.S[0], s.S[0]) / s.N[0] ** 2
    want_cov = W @ st.cov @ W.T * (n - 1) / n
    assert np.abs(cov - want_cov).max() <= 1e-6 * np.abs(want_cov).max()
    fit = M.gmm_reference(cubes, model["pivot"], model["weight"], (np.zeros((1, 5)), np.eye(5)[None]), masks, select, reg_covar=0.0)
    assert fit.n_iter == 1 and np.abs(fit.covariances[0] - want_cov).max() <= 1e-6 * np.abs(want_cov).max()


# ---- an fp32 emulation of the chains stays inside the bound ----------------------------------------------------------
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _emulate(x, ops, cs):
    """The contract in fp32 numpy, operation by operation (a fused multiply-add as an fp64 product and sum rounded to fp32)."""
    q, K = ops.q, ops.k
    qp = cases._rup(q, 8)
    d = x.astype(np.float32) - ops.pivot
    z = np.zeros((len(d), qp), np.float32)
    for c in range(d.shape[1]):
        z[:, :q] = _fma32(ops.weight[None, :, c], d[:, c:c + 1], z[:, :q])
    m = np.zeros((len(d), K), np.float32)
    for k in range(K):
        u = np.zeros((len(d), 32), np.float32)
        u[:, :q] = ops.a[k][None]
        for j in range(q):
            u[:, :q] = _fma32(ops.A[k][None, :, j], z[:, j:j + 1], u[:, :q])
        s = np.zeros((len(d), 4), np.float32)
        for b in range(2):
            for j in range(4):
                for g in range(4):
                    s[:, g] = _fma32(u[:, 16 * b + 4 * g + j], u[:, 16 * b + 4 * g + j], s[:, g])
        m[:, k] = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
    l = _fma32(np.float32(-0.5) * np.ones_like(m), m, ops.c[None] * np.ones_like(m))

    def lse(cols):
        mx = l[:, cols].max(axis=1)
        acc = np.zeros(len(d), np.float32)
        for k in cols:
            acc = acc + np.exp(l[:, k] - mx)
        return mx, acc
    mx, acc = lse(list(range(K)))
    resp = np.stack([np.exp(l[:, k] - mx) / acc for k in range(K)], axis=1)
    nll = -(mx + np.log(acc))
    L = np.stack([(lambda r: r[0] + np.log(r[1]))(lse(list(np.nonzero(ops.classes == c)[0]))) for c in range(ops.n_classes)], axis=1)
    assert all(v.dtype == np.float32 for v in (z, m, l, resp, nll, L))
    return {"z": z[:, :q], "m": m, "loglik": L, "resp": resp, "nll": nll}


@pytest.mark.parametrize("C,q,K,classes", cases.SCORE_CASES)
def test_fp32_emulation_stays_inside_the_bound(C, q, K, classes):
    """Also what the GPU test relies on: the bound flags at most 1 % of the pixels as having a label that rounding can flip."""
    cubes, _, model = cases.model_case(C, q, K, classes, H=16, W=25)
    ops = _ops(model)
    x = cubes.reshape(-1, C)
    got = _emulate(x, ops, cases._rup(C, 8))
    b = M.gmm_bound(x, ops)
    for name, bound in (("z", "Ez"), ("m", "Em"), ("loglik", "Eloglik"), ("resp", "Eresp"), ("nll", "Enll")):
        err = np.abs(got[name].astype(np.float64) - b[name])
        assert (err <= b[bound]).all(), (name, float((err / b[bound]).max()))
    assert (b["Eloglik"] < 0.1).all() and (b["Eresp"] <= 0.5 * b["resp"] + 1e-30).all()         # the bounds say something
    whole = M.gmm_bound(cases.model_case(C, q, K, classes)[0], ops)
    assert whole["ambiguous"].mean() <= 0.01


def test_sums_bound_covers_an_fp32_emulation():
    cubes, masks, model = cases.model_case(37, 5, 3, 1, H=16, W=25)
    ops = _ops(model)
    x = cubes.reshape(-1, 37)
    got = _emulate(x, ops, 40)
    e = got["z"][:, None, :] - ops.means[None]
    re = got["resp"][:, :, None] * e
    assert e.dtype == np.float32 and re.dtype == np.float32
    Q = np.zeros((3, 5, 5), np.float32)
    for p in range(len(x)):                                     # the run's chain, pixel by pixel
        Q = _fma32(re[p][:, :, None], e[p][:, None, :], Q)
    ref = M.gmm_step_reference(cubes, ops)
    bound = M.gmm_sums_bound(x, ops)
    assert (np.abs(Q.astype(np.float64) - ref.Q) <= bound.Q).all()
    assert (np.abs(re.astype(np.float64).sum(axis=0) - ref.S) <= bound.S).all()
    assert (np.abs(got["resp"].astype(np.float64).sum(axis=0) - ref.N) <= bound.N).all()
    assert abs(-got["nll"].astype(np.float64).sum() - ref.LL) <= bound.LL
    assert (bound.Q <= 1e-2 * np.abs(ref.Q).max()).all()


# ---- the integer cases are exact -------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 37, 238, 313])
def test_integer_cases_are_exact(C):
    """Every intermediate of the contract is an integer (l: a half) below 2^23 in magnitude, so fp32 computes it exactly in any
    order; the mirror pair and the duplicate tie for every pixel."""
    case = cases.int_case(C)
    rng = np.random.RandomState(C)
    pixels = rng.randint(-4, 5, size=(4000, C))
    d = pixels - case["pivot"].astype(np.int64)
    W = case["weight"].astype(np.int64)
    assert np.array_equal(W, case["weight"]) and np.array_equal(case["A"], case["A"].astype(np.int64))
    partial = np.cumsum(d[:, None, :] * W[None], axis=2)
    assert np.abs(partial).max() < 2 ** 23
    z, m, labels = cases.int_reference(pixels, case)
    A = case["A"].astype(np.int64)
    assert (np.abs(A).sum(axis=2).max() * np.abs(z).max() + np.abs(case["a"]).max()) < 2 ** 11
    assert m.max() < 2 ** 23 and (m >= 0).all()
    assert np.array_equal(m[:, 0], m[:, 1]) and np.array_equal(m[:, 0], m[:, -1])
    assert (labels != 1).all() and (labels != len(A) - 1).all()
    assert len(np.unique(labels)) >= 2
