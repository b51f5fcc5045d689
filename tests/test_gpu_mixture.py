"""Spectral Gaussian mixtures on the device (hyperpri_amd/mixture.py, csrc/mixture.hip) against the numpy restatement of their
contract: exact on integer data, within ``gmm_bound`` on real-valued data, labels equal to the reference's wherever rounding cannot
change them, sums exact where the responsibilities are, bit-reproducible, and end to end from a filled cache through the fits to the
evaluation of a held-out cube.  tests/test_mixture_cpu.py holds the conditions on the inputs (tests/_mixture_cases.py).  Needs a real
MI355X: ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

import _mixture_cases as cases
from conftest import record_margin
from test_gpu_spectral import DEV, _cache, _int_cubes

pytestmark = pytest.mark.gpu
SELECTS = ("all", "foreground", "background")
OUT = ("loglik", "logit", "labels", "resp", "nll")
_rup = cases._rup


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _padded(pixels, cs):
    P, C = pixels.shape
    buf = np.zeros((P, cs), dtype=np.float32)
    buf[:, :C] = pixels
    return torch.from_numpy(buf).to(DEV)


def _operands(pivot, weight, A, a, c, cs, means=None):
    """The zero-padded device operands of the C ABI: pivot (cs), weight (qp, cs), A (K, qp, qp), a (K, qp), c (K), means (K, qp)."""
    q, C = weight.shape
    K, qp = A.shape[0], _rup(q, 8)
    pv = np.zeros(cs, np.float32)
    pv[:C] = pivot
    w = np.zeros((qp, cs), np.float32)
    w[:q, :C] = weight
    Ap = np.zeros((K, qp, qp), np.float32)
    Ap[:, :q, :q] = A
    ap = np.zeros((K, qp), np.float32)
    ap[:, :q] = a
    mp = np.zeros((K, qp), np.float32)
    if means is not None:
        mp[:, :q] = means
    return [_dev(v) for v in (pv, w, Ap, ap, np.asarray(c, np.float32), mp)]


def _score(x, plane, pivot, weight, A, a, c, classes, n_classes, outputs=OUT):
    """``hpri_band_gmm_score`` itself on a (P, cs) fp32 device buffer; outputs that are not asked for keep their sentinel fill."""
    from hyperpri_amd import _lib
    from hyperpri_amd._args import _p, _stream
    P, cs = int(x.shape[0]), int(x.shape[1])
    K, q = A.shape[0], weight.shape[0]
    pv, w, Ad, ad, cd, _ = _operands(pivot, weight, A, a, c, cs)
    n = P // plane
    out = {"loglik": torch.full((n, n_classes, plane), float("nan"), device=DEV), "logit": torch.full((P,), float("nan"), device=DEV),
           "labels": torch.full((P,), 255, dtype=torch.uint8, device=DEV), "resp": torch.full((n, K, plane), float("nan"), device=DEV),
           "nll": torch.full((P,), float("nan"), device=DEV)}
    ptr = {name: (_p(out[name]) if name in outputs else None) for name in out}
    cl = (ctypes.c_int * K)(*[int(v) for v in classes])
    _lib.call("hpri_band_gmm_score", _p(x), P, plane, cs, _p(pv), _p(w), q, _p(Ad), _p(ad), _p(cd), ctypes.cast(cl, ctypes.c_void_p), K,
              n_classes, ptr["loglik"], ptr["logit"], ptr["labels"], ptr["resp"], ptr["nll"], _stream())
    torch.cuda.synchronize()
    got = {name: t.cpu().numpy() for name, t in out.items()}
    for name in out:                                            # what was not asked for stays untouched
        if name not in outputs:
            assert (got[name] == 255).all() if name == "labels" else np.isnan(got[name]).all(), name
    return got


def _by_pixel(planes):
    """(n, K, plane) -> (n * plane, K)."""
    return planes.transpose(0, 2, 1).reshape(-1, planes.shape[1])


def _sums(cache, order, select, pivot, weight, A, a, c, means):
    """``hpri_band_gmm_sums`` itself: ``(count, N (K,), S (K, q), Q (K, q, q), LL)``."""
    from hyperpri_amd import _lib
    from hyperpri_amd import mixture as M
    from hyperpri_amd._args import _p, _stream
    from hyperpri_amd.cache import _DT
    q, K = weight.shape[0], A.shape[0]
    qp = _rup(q, 8)
    pv, w, Ad, ad, cd, md = _operands(pivot, weight, A, a, c, cache.cs, means)
    table = torch.tensor(list(order), dtype=torch.int32).to(DEV)
    nbytes = M.workspace_bytes(cache.cs, q, K)
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full((2 + K * (1 + qp + qp * qp),), float("nan"), dtype=torch.float64, device=DEV)
    base = out.data_ptr()
    oN, oS, oQ = base + 8, base + 8 * (1 + K), base + 8 * (1 + K + K * qp)
    _lib.call("hpri_band_gmm_sums", _p(cache._cubes), _DT[cache.store_dtype], cache.capacity, cache.H, cache.W, cache.cs, _p(cache._masks),
              _p(table), len(order), SELECTS.index(select), _p(pv), _p(w), q, _p(Ad), _p(ad), _p(cd), _p(md), K, _p(work), nbytes, base, oN, oS,
              oQ, oQ + 8 * K * qp * qp, _stream())
    host = out.cpu().numpy()
    S = host[1 + K:1 + K + K * qp].reshape(K, qp)
    Q = host[1 + K + K * qp:-1].reshape(K, qp, qp)
    assert (S[:, q:] == 0).all() and (Q[:, q:] == 0).all() and (Q[:, :, q:] == 0).all()
    return int(host[:1].view(np.int64)[0]), host[1:1 + K].copy(), S[:, :q].copy(), Q[:, :q, :q].copy(), float(host[-1])


# ---- 1. score, exact on integers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 37, 238, 313])
def test_score_is_exact_on_integers(C):
    """Every component its own class and c = 0: the class log-likelihood is -m_k / 2 bit for bit (expf(0) = 1, logf(1) = 0), so
    ``-2 loglik`` is m_k of int64 arithmetic and the label the lowest component at the least m -- the mirror pair and the duplicate
    tie for every pixel.  63, 65 and 24960 pixels: less than a tile, one past a tile, more tiles than the grid holds at C >= 238.
    C = 313 is cs = 320: with q = 32 and K = 8 the tile is 32 pixels and two waves score (q = 5, K = 4 keep the tile of 64)."""
    cs = _rup(C, 8)
    rng = np.random.RandomState(C)
    for q, K in ((5, 4), (32, 8)) if C == 313 else ((5, 4),):
        case = cases.int_case(C, K=K, q=min(q, 5))
        if q == 32:                                             # the same rows, embedded in 32 dimensions: rows 5.. of z are zero
            w = np.zeros((32, C), np.float32)
            w[:5] = case["weight"]
            A = np.tile(np.eye(32, dtype=np.float32), (K, 1, 1))
            A[:, :5, :5] = case["A"]
            a = np.zeros((K, 32), np.float32)
            a[:, :5] = case["a"]
            case = dict(case, weight=w, A=A, a=a)
        for P in (63, 65, 24960):
            pixels = rng.randint(-4, 5, size=(P, C))
            got = _score(_padded(pixels, cs), P, case["pivot"], case["weight"], case["A"], case["a"], case["c"], case["classes"], K,
                         outputs=("loglik", "labels", "nll"))
            _, m, labels = cases.int_reference(pixels, dict(case, weight=case["weight"][:5], A=case["A"][:, :5, :5], a=case["a"][:, :5]))
            assert np.array_equal(-2.0 * _by_pixel(got["loglik"]).astype(np.float64), m.astype(np.float64)), (C, q, P)
            assert np.array_equal(got["labels"].astype(np.int64), labels), (C, q, P)
            assert (labels != 1).all() and (labels != K - 1).all()                     # the ties went to the lowest class
            assert np.isfinite(got["nll"]).all()


# ---- 2. score, real values -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,q,K,classes", cases.SCORE_CASES)
def test_score_within_the_derived_bound(C, q, K, classes):
    """One image of 47 x 53 pixels per case, every output within ``gmm_bound`` of the fp64 reference; labels equal wherever the bound
    cannot flip them (test_mixture_cpu: at most 1 % of the pixels are so excluded); one output at a time leaves the others alone."""
    from hyperpri_amd import mixture as M
    cubes, _, model = cases.model_case(C, q, K, classes)
    ops = M.gmm_operands(model["pivot"], model["weight"], model["means"], model["covariances"], model["weights"], model["classes"])
    cs = _rup(C, 8)
    pixels = cubes.reshape(-1, C)
    x = _padded(pixels, cs)
    b = M.gmm_bound(pixels, ops, cs)
    outputs = tuple(o for o in OUT if o != "logit" or classes == 2)
    got = _score(x, len(pixels), ops.pivot, ops.weight, ops.A, ops.a, ops.c, ops.classes, classes, outputs=outputs)
    key = f"mixture/score/C{C}/q{q}/K{K}"
    for name, mine, bound in (("loglik", _by_pixel(got["loglik"]), b["Eloglik"]), ("resp", _by_pixel(got["resp"]), b["Eresp"]),
                              ("nll", got["nll"], b["Enll"])) + ((("logit", got["logit"], b["Elogit"]),) if classes == 2 else ()):
        err = np.abs(mine.astype(np.float64) - b[name])
        record_margin(f"{key}/{name}", float((err / bound).max()), 1.0)
        assert (err <= bound).all(), name
    amb = b["ambiguous"]
    lab = got["labels"].astype(np.int64)
    assert lab.max() < classes and amb.mean() <= 0.01
    assert np.array_equal(lab[~amb], b["labels"][~amb])
    for name in outputs:
        alone = _score(x, len(pixels), ops.pivot, ops.weight, ops.A, ops.a, ops.c, ops.classes, classes, outputs=(name,))
        assert alone[name].tobytes() == got[name].tobytes(), name


# ---- 3. sums, exact cases --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("q", [5, 32])
def test_sums_are_exact_where_the_responsibilities_are(q, store_dtype):
    """Integer data, 0 / +-1 projection rows, A = I, a = -m for integer means: e = z - m is an integer, |e| <= 43.  K = 1: r = 1, so N is
    the count and S, Q are integers (a run's fp32 sums stay below 2048 * 43^2 < 2^23).  Two identical components: r = 1/2, every sum is
    exactly half.  A third component at a distance whose expf underflows adds exact zeros and changes nothing else.  q = 32 takes the
    second accumulator tile.  The slot table is shuffled and repeats a slot; slot 1 has no foreground."""
    C = 37
    cubes, masks = _int_cubes(70 + q, 3, cases.SLOT[0], cases.SLOT[1], C)
    cache = _cache(cubes, masks, capacity=4, store_dtype=store_dtype)
    case = cases.int_case(C, K=4, q=5)
    rng = np.random.RandomState(q)
    weight = np.zeros((q, C), np.float32)
    weight[:5] = case["weight"]
    for i in range(5, q):
        weight[i, rng.choice(C, size=8, replace=False)] = rng.choice([-1.0, 1.0], size=8)
    mean = rng.randint(-3, 4, size=q).astype(np.float32)
    order = [2, 0, 2, 1]
    xs, ms = cubes[order].astype(np.int64), masks[order]
    eye = np.eye(q, dtype=np.float32)
    far = mean + 40.0
    for select in SELECTS:
        sel = np.ones(ms.shape, bool) if select == "all" else (ms != 0) if select == "foreground" else (ms == 0)
        e = (xs[sel] - case["pivot"].astype(np.int64)) @ weight.astype(np.int64).T - mean.astype(np.int64)
        n = int(sel.sum())
        S1, Q1 = e.sum(axis=0), e.T @ e
        one = _sums(cache, order, select, case["pivot"], weight, eye[None], -mean[None], [0.0], mean[None])
        assert one[0] == n and one[1].tolist() == [float(n)], (q, select)
        assert np.array_equal(one[2][0], S1.astype(np.float64)) and np.array_equal(one[3][0], Q1.astype(np.float64)), (q, select)
        two = _sums(cache, order, select, case["pivot"], weight, np.stack([eye, eye]), np.stack([-mean, -mean]), [0.0, 0.0], np.stack([mean, mean]))
        assert two[0] == n
        for k in range(2):
            assert two[1][k] == 0.5 * n and np.array_equal(two[2][k], 0.5 * S1) and np.array_equal(two[3][k], 0.5 * Q1), (q, select, k)
        if q == 5:
            # component 2 sits 40 away in every coordinate: its expf underflows wherever l_2 - l_0 < -110, which the data keeps
            e3 = e - 40
            assert ((e3 * e3).sum(axis=1) - (e * e).sum(axis=1)).min() > 2 * 110
            three = _sums(cache, order, select, case["pivot"], weight, np.stack([eye, eye, eye]), np.stack([-mean, -mean, -far]), [0.0] * 3,
                          np.stack([mean, mean, far]))
            assert three[1][2] == 0 and (three[2][2] == 0).all() and (three[3][2] == 0).all()
            for k in range(2):
                assert three[1][k] == two[1][k] and three[2][k].tobytes() == two[2][k].tobytes() and three[3][k].tobytes() == two[3][k].tobytes()
            assert three[4] == two[4]


# ---- 4. sums, real values --------------------------------------------------------------------------------------------
def test_sums_within_the_derived_bound_reproducible_and_mergeable():
    from hyperpri_amd import mixture as M
    from hyperpri_amd import spectral as S
    s = cases.SUMS
    cubes, masks, model = cases.model_case(s["C"], s["q"], s["K"], 2, n=s["n"])
    ops = M.gmm_operands(model["pivot"], model["weight"], model["means"], model["covariances"], model["weights"], model["classes"])
    for store_dtype, name in ((torch.float32, "f32"), (torch.float16, "f16")):
        cache = _cache(cubes, masks, store_dtype=store_dtype)
        stored = cubes.astype(np.float16).astype(np.float32) if store_dtype == torch.float16 else cubes
        for select in SELECTS if name == "f32" else ("foreground",):
            ref = M.gmm_step_reference(stored, ops, masks, select)
            bound = M.gmm_sums_bound(S._selected_pixels(stored, masks, select).astype(np.float32), ops, cache.cs)
            got = M.gmm_step(cache, ops, None, select)
            assert got.count == ref.count
            for what in ("N", "S", "Q"):
                err, tol = np.abs(getattr(got, what) - getattr(ref, what)), getattr(bound, what)
                record_margin(f"mixture/sums/{name}/{select}/{what}", float((err / tol).max()), 1.0)
                assert (err <= tol).all(), (name, select, what)
            record_margin(f"mixture/sums/{name}/{select}/LL", abs(got.LL - ref.LL) / bound.LL, 1.0)
            assert abs(got.LL - ref.LL) <= bound.LL
    again = M.gmm_step(cache, ops, None, "foreground")
    assert (again.count, again.LL) == (got.count, got.LL)
    assert all(getattr(again, w).tobytes() == getattr(got, w).tobytes() for w in ("N", "S", "Q"))
    parts = M.merge_gmm_sums(M.gmm_step(cache, ops, [0, 2], "foreground"), M.gmm_step(cache, ops, [1], "foreground"))
    assert parts.count == got.count and abs(parts.LL - got.LL) <= 1e-12 * abs(got.LL)
    for w in ("N", "S", "Q"):
        assert (np.abs(getattr(parts, w) - getattr(got, w)) <= 1e-12 * np.abs(getattr(got, w)).max()).all()


def test_runs_wrap_around_the_partial_accumulators():
    """More runs than the pass has partial accumulators (256): a partial then adds several runs, in run order."""
    from hyperpri_amd import mixture as M
    from hyperpri_amd import spectral as S
    C, q = 3, 2
    Wd = (M.gmm_parts() + 1) * S.FP32_RUN + 37
    cubes, masks = _int_cubes(6, 1, 1, Wd, C)
    cache = _cache(cubes, masks)
    weight = np.array([[1, 0, -1], [0, 1, 1]], np.float32)
    pivot, mean = np.array([1, 0, 1], np.float32), np.array([1, -2], np.float32)
    e = (cubes[0, 0].astype(np.int64)[masks[0, 0] != 0] - pivot.astype(np.int64)) @ weight.astype(np.int64).T - mean.astype(np.int64)
    got = _sums(cache, [0], "foreground", pivot, weight, np.eye(q, dtype=np.float32)[None], -mean[None], [0.0], mean[None])
    assert got[0] == len(e) and got[1][0] == len(e)
    assert np.array_equal(got[2][0], e.sum(axis=0).astype(np.float64)) and np.array_equal(got[3][0], (e.T @ e).astype(np.float64))


# ---- 5. end to end ---------------------------------------------------------------------------------------------------
def test_fit_classes_end_to_end():
    import hyperpri_amd as H
    from hyperpri_amd import mixture as M
    import _crf_cases as K
    L = cases.LADDER
    cubes, masks, _ = cases.ladder_scene()
    fit, held = list(L["fit"]), L["held_out"]
    cache = _cache(cubes, masks)
    proj = H.SpectralProjection.pca(H.band_statistics(cache, fit), L["q"], whiten=True)
    n, sums = H.spectral.band_moments(cache, fit, "all")
    pivot = (sums[:L["C"]] / n).astype(np.float32)
    weight = proj.weight.cpu().numpy()
    dice = {}
    for components in ((1, 1), (3, 2)):
        inits = cases.ladder_inits(cubes, masks, pivot, weight, components)
        trace = []
        model = H.SpectralGMM.fit_classes(cache, proj, components, slots=fit, init=inits, pivot=pivot, callback=lambda c, ops, s: trace.append((c, ops, s)))
        assert model.k == sum(components) and model.q == L["q"] and model.n_classes == 2 and model.means.device.type == "cuda"
        assert not model.starved_
        assert model.classes.tolist() == [0] * components[0] + [1] * components[1]
        assert abs(float(model.weights.sum()) - 1) <= 1e-12
        if components == (1, 1):
            assert len(trace) == 2                              # the maximum-likelihood classifier: one pass per class
        # one-step parity at every EM iteration: the device's sums against the reference at the device's own parameters
        last = {}
        for c, ops, s in trace:
            select = ("background", "foreground")[c]
            ref = M.gmm_step_reference(cubes[fit], ops, masks[fit], select)
            x = H.spectral._selected_pixels(cubes[fit], masks[fit], select).astype(np.float32)
            bound = M.gmm_sums_bound(x, ops, cache.cs)
            assert s.count == ref.count
            for what in ("N", "S", "Q"):
                err, tol = np.abs(getattr(s, what) - getattr(ref, what)), getattr(bound, what)
                record_margin(f"mixture/e2e/{components[0]}{components[1]}/{what}", float((err / tol).max()), 1.0)
                assert (err <= tol).all(), (components, c, what)
            assert abs(s.LL - ref.LL) <= bound.LL
            if c in last:                                       # LL never drops by more than its bound
                assert s.LL >= last[c][0] - (bound.LL + last[c][1]), (components, c)
            last[c] = (s.LL, bound.LL)
        pred = H.gmm_split(model, [cache.batch([held])])
        val = H.validate_net(pred)
        # validate_net's pick among its 500 thresholds (for (1, 1) it lands on an empty curve point: Dice 0) and the best Dice over all
        dice[components] = (val["dice_at_threshold"], cases.best_dice(pred.logits.cpu().numpy(), masks[held]))
        logits = model(cache.batch([held]), output="logit")
        assert tuple(logits.shape) == (1, 1, cubes.shape[1], cubes.shape[2]) and bool(torch.isfinite(logits).all())
        assert pred.logits.cpu().numpy().tobytes() == logits.reshape(-1).cpu().numpy().tobytes()
        # the device's logits are the reference's at the device's parameters, within the bound
        b = M.gmm_bound(cubes[held], model.operands, cache.cs)
        err = np.abs(logits.reshape(-1).cpu().numpy().astype(np.float64) - b["logit"])
        record_margin(f"mixture/e2e/{components[0]}{components[1]}/logit", float((err / b["Elogit"]).max()), 1.0)
        assert (err <= b["Elogit"]).all()
    assert max(dice[(1, 1)]) < 0.6 and min(dice[(3, 2)]) > 0.9, dice
    # class log-likelihoods are unaries of the dense CRF
    batch = cache.batch([held, 0])
    ll = model(batch, output="loglik")
    assert tuple(ll.shape) == (2, 2, cubes.shape[1], cubes.shape[2]) and ll.is_contiguous()
    guide = H.SpectralProjection.pca(H.band_statistics(cache, fit), 1, whiten=True).to(DEV)(batch["image"])
    refined = H.dense_crf(ll, guide, **K.SCENE)
    assert tuple(refined.shape) == tuple(ll.shape) and bool(torch.isfinite(refined).all())
    assert torch.equal((ll[:, 1] - ll[:, 0]).unsqueeze(1), model(batch, output="logit"))
    for output, planes, dtype in (("labels", 1, torch.uint8), ("resp", 5, torch.float32), ("nll", 1, torch.float32)):
        y = model(batch["image"], output=output)
        assert tuple(y.shape) == (2, planes, cubes.shape[1], cubes.shape[2]) and y.dtype == dtype
    assert float((model(batch, output="resp").sum(dim=1) - 1).abs().max()) <= 1e-5
    # the state dict carries the model
    again = H.SpectralGMM.blank(L["C"], L["q"], 5, 2).to(DEV)
    again.load_state_dict(model.state_dict())
    assert again(batch, output="logit").cpu().numpy().tobytes() == model(batch, output="logit").cpu().numpy().tobytes()
    with pytest.raises(RuntimeError, match="autograd"):
        model(batch["image"].clone().requires_grad_(True))


def test_unsupervised_fit_is_deterministic_and_labels_nan():
    import hyperpri_amd as H
    L = cases.LADDER
    cubes, masks, _ = cases.ladder_scene()
    cache = _cache(cubes, masks)
    proj = H.SpectralProjection.pca(H.band_statistics(cache), L["q"], whiten=True)
    one = H.SpectralGMM.fit(cache, proj, 3, seed=3, max_iter=5)
    two = H.SpectralGMM.fit(cache, proj, 3, seed=3, max_iter=5)
    assert one.means.cpu().numpy().tobytes() == two.means.cpu().numpy().tobytes() and one.log_likelihood_ == two.log_likelihood_
    assert 1 <= one.n_iter_ <= 5 and np.isfinite(one.log_likelihood_)
    x = cubes[:1].copy()
    x[0, 0, 0, :] = np.nan
    y = one(torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).to(DEV), output="labels")
    assert int(y.max()) < 1                                     # one class: label 0 whatever the data, NaN included
    with pytest.raises(ValueError, match="two classes"):
        one(cache.batch([0]), output="logit")


# ---- 6. argument errors ----------------------------------------------------------------------------------------------
def test_argument_errors_return_the_error_code_without_a_launch():
    from hyperpri_amd import _lib
    from hyperpri_amd import mixture as M
    from hyperpri_amd._args import _p, _stream
    lib = _lib.load()
    C, cs, q, K, P = 20, 24, 5, 3, 64
    x = torch.zeros((P, cs), device=DEV)
    pv, w, A, a, c, m = _operands(np.zeros(C), np.zeros((q, C), np.float32), np.tile(np.eye(q, dtype=np.float32), (K, 1, 1)), np.zeros((K, q)), np.zeros(K), cs,
                                  np.zeros((K, q)))
    out = torch.full((P * 4,), float("nan"), device=DEV)
    lab = torch.full((P,), 255, dtype=torch.uint8, device=DEV)

    def score(**kw):
        cl = kw.get("classes", [0, 1, 1])
        arg = dict(x=_p(x), pixels=P, plane=P, cs=cs, pivot=_p(pv), weight=_p(w), q=q, A=_p(A), a=_p(a), c=_p(c),
                   classes=ctypes.cast((ctypes.c_int * len(cl))(*cl), ctypes.c_void_p), K=K, C=2, loglik=_p(out), logit=None, labels=_p(lab), resp=None,
                   nll=None)
        arg.update({k: v for k, v in kw.items() if k != "classes"})
        return lib.hpri_band_gmm_score(*arg.values(), _stream())
    assert score() == 0
    torch.cuda.synchronize()
    assert (lab.cpu().numpy() == 1).all()                       # (z = 0 for every component: class 1 holds two of the three)
    lab.fill_(255)
    bad = [dict(x=None), dict(weight=None), dict(A=None), dict(a=None), dict(c=None), dict(pixels=0), dict(plane=0), dict(plane=P - 1), dict(cs=20),
           dict(cs=328), dict(q=0), dict(q=33), dict(K=0), dict(K=9), dict(C=0), dict(C=9), dict(classes=[0, 2, 1]), dict(classes=[0, -1, 1]),
           dict(C=3, logit=_p(out)), dict(loglik=None, labels=None), dict(x=x.data_ptr() + 4), dict(loglik=out.data_ptr() + 2)]
    for kw in bad:
        assert score(**kw) == -1, kw
        assert lib.hpri_last_error()
    torch.cuda.synchronize()
    assert (lab.cpu().numpy() == 255).all()                     # nothing was launched

    cubes, masks = _int_cubes(1, 1, 5, 7, C)
    cache = _cache(cubes, masks)
    from hyperpri_amd.cache import _DT
    table = torch.zeros(1, dtype=torch.int32, device=DEV)
    nbytes = M.workspace_bytes(cache.cs, q, K)
    assert nbytes > 0 and M.workspace_bytes(20, q, K) == 0 and M.workspace_bytes(cs, 33, K) == 0 and M.workspace_bytes(cs, q, 9) == 0
    assert nbytes == M.workspace_bytes(cache.cs, q, K) and lib.hpri_band_gmm_max_components() == 8 and lib.hpri_band_gmm_max_dims() == 32 and M.gmm_parts() == 256
    work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    res = torch.full((2 + K * (1 + 8 + 64),), -7.0, dtype=torch.float64, device=DEV)

    def sums(**kw):
        base = res.data_ptr()
        arg = dict(cache=_p(cache._cubes), dtype=_DT[cache.store_dtype], slots=cache.capacity, Hs=cache.H, Ws=cache.W, cs=cache.cs, masks=_p(cache._masks),
                   table=_p(table), n=1, select=1, pivot=_p(pv), weight=_p(w), q=q, A=_p(A), a=_p(a), c=_p(c), means=_p(m), K=K, work=_p(work),
                   nbytes=nbytes, count=base, N=base + 8, S=base + 8 * (1 + K), Q=base + 8 * (1 + K + 8 * K), LL=base + 8 * (1 + K + 72 * K))
        arg.update(kw)
        return lib.hpri_band_gmm_sums(*arg.values(), _stream())
    bad = [dict(cache=None), dict(table=None), dict(work=None), dict(weight=None), dict(means=None), dict(N=None), dict(LL=None), dict(dtype=2),
           dict(slots=0), dict(Hs=0), dict(n=0), dict(cs=20), dict(select=3), dict(masks=None), dict(q=0), dict(q=33), dict(K=0), dict(K=9),
           dict(nbytes=nbytes - 1), dict(work=work.data_ptr() + 8), dict(S=res.data_ptr() + 4)]
    for kw in bad:
        assert sums(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == -7.0).all()                    # nothing was launched
    assert sums() == 0
    torch.cuda.synchronize()
    assert int(res.cpu().numpy()[:1].view(np.int64)[0]) == int((masks != 0).sum())
