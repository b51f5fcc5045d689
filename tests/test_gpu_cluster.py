"""Spectral k-means on the device (hyperpri_amd/cluster.py, csrc/cluster.hip) against the numpy restatement of its contract: exact
on integer data (every fp32 value is an integer or a half below 2^23), within bounds derived from the fp32 rounding model on
real-valued data, labels equal to the reference's wherever rounding cannot change them, bit-reproducible, and end to end from a
filled cache through fit, calibrate and ``cluster_split`` to the evaluation of a split.  tests/test_cluster_cpu.py holds the
conditions on the inputs (tests/_cluster_cases.py).  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest
import torch

import _cluster_cases as cases
from conftest import record_margin
from test_gpu_detect import SIZES
from test_gpu_spectral import DEV, U, _cache, _int_cubes, _real_cubes

pytestmark = pytest.mark.gpu
SELECTS = ("all", "foreground", "background")
KS = (1, 2, 3, 16, 17, 33, 64)


def _rup(a, m):
    return (a + m - 1) // m * m


def _padded(pixels, cs):
    """(P, C) numpy -> the zero-padded (P, cs) fp32 device buffer."""
    P, C = pixels.shape
    buf = np.zeros((P, cs), dtype=np.float32)
    buf[:, :C] = pixels
    return torch.from_numpy(buf).to(DEV)


def _rows(W, b, cs):
    """(K, C) operands -> the padded (ks, cs) rows and (ks,) bias on the device."""
    K, C = W.shape
    ks = _rup(K, 8)
    w = np.zeros((ks, cs), dtype=np.float32)
    bb = np.zeros(ks, dtype=np.float32)
    w[:K, :C], bb[:K] = W, b
    return torch.from_numpy(w).to(DEV), torch.from_numpy(bb).to(DEV)


def _assign(x, pivot, W, b, lut=None, outputs=("labels", "zmin", "dist2", "value")):
    """``hpri_band_assign`` itself on a (P, cs) fp32 device buffer; ``pivot`` (C,) or None, ``W`` (K, C), ``b`` (K,), ``lut`` (K,)."""
    from hyperpri_amd import _lib
    from hyperpri_amd._args import _p, _stream
    P, cs = int(x.shape[0]), int(x.shape[1])
    K = int(W.shape[0])
    wd, bd = _rows(np.asarray(W, np.float32), np.asarray(b, np.float32), cs)
    pv = None
    if pivot is not None:
        pv = np.zeros(cs, np.float32)
        pv[:len(pivot)] = pivot
        pv = torch.from_numpy(pv).to(DEV)
    out = {"labels": torch.full((P,), 255, dtype=torch.uint8, device=DEV)}
    for name in ("zmin", "dist2", "value"):
        out[name] = torch.full((P,), float("nan"), dtype=torch.float32, device=DEV)
    if lut is None:
        outputs = tuple(o for o in outputs if o != "value")
    ld = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float32)).to(DEV) if "value" in outputs else None
    ptr = {name: (_p(out[name]) if name in outputs else None) for name in out}
    _lib.call("hpri_band_assign", _p(x), P, cs, _p(pv), _p(wd), _p(bd), K, _p(ld), ptr["labels"], ptr["zmin"], ptr["dist2"], ptr["value"], _stream())
    torch.cuda.synchronize()
    return {name: out[name].cpu().numpy() for name in outputs}


def _int_centroids(rng, K, C):
    """Integer centroids in [-3, 3] (relative to the pivot) with a duplicate (the last repeats the first) and a mirror pair: 1 is 0
    with band 0 negated (2 against -2), so every pixel with d[0] == 0 is equidistant from 0 and 1."""
    g = rng.randint(-3, 4, size=(K, C))
    g[0, 0] = 2
    if K >= 2:
        g[1] = g[0]
        g[1, 0] = -2
    if K >= 3:
        g[K - 1] = g[0]
    return g


def _int_assign_reference(d, g):
    """int64: twice the scores ``|g|^2 - 2 g . d``, the label (lowest index of the minimum) and ``|d|^2``."""
    z2 = (g.astype(np.int64) ** 2).sum(axis=1)[None, :] - 2 * (d.astype(np.float64) @ g.astype(np.float64).T).astype(np.int64)
    labels = np.argmin(z2, axis=1)
    return labels, z2[np.arange(len(labels)), labels], (d.astype(np.int64) ** 2).sum(axis=1)


# ---- 1. exact on integers: assign ------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 37, 238, 313])
def test_assign_is_exact_on_integers(C):
    """|g . d| <= 313 * 15 and |g|^2 / 2 <= 313 * 4.5: every score is a multiple of 1/2 below 2^13, |d|^2 <= 313 * 25.  63, 65, 24960
    and 52000 pixels: less than a tile, one past a tile, many tiles, and at C >= 238 more tiles than the grid holds.  C = 313 is
    cs = 320: at K = 64 the centres leave room for a tile of 32 pixels only."""
    cs = _rup(C, 8)
    rng = np.random.RandomState(C)
    pivot = rng.randint(0, 2, size=C).astype(np.float32)
    for (n, h, w) in SIZES:
        pixels = rng.randint(-4, 5, size=(n * h * w, C))
        pixels[::7, 0] = pivot[0]                               # deliberate ties between centroids 0 and 1
        x = _padded(pixels, cs)
        d = pixels - pivot.astype(np.int64)
        for K in (KS if n == 1 else (2, 17, 64)):
            g = _int_centroids(rng, K, C)
            lut = rng.randint(-9, 10, size=K).astype(np.float32)
            got = _assign(x, pivot, -g.astype(np.float32), 0.5 * (g.astype(np.float64) ** 2).sum(axis=1), lut)
            labels, z2, s = _int_assign_reference(d, g)
            if K >= 2:
                assert (labels[::7] != 1).all()                                 # the ties went to the lower index
            assert (labels != K - 1).all() or K < 3                            # the duplicate of centroid 0 never wins
            assert np.array_equal(got["labels"].astype(np.int64), labels), (C, K, n * h * w)
            assert np.array_equal(got["zmin"].astype(np.float64) * 2, z2.astype(np.float64))
            assert np.array_equal(got["dist2"].astype(np.int64), z2 + s) and (z2 + s >= 0).all()
            assert np.array_equal(got["value"], lut[labels])
        # without a pivot d = x; one output at a time gives the same labels
        g = _int_centroids(rng, 3, C)
        labels, z2, s = _int_assign_reference(pixels, g)
        W, b = -g.astype(np.float32), 0.5 * (g.astype(np.float64) ** 2).sum(axis=1)
        assert np.array_equal(_assign(x, None, W, b, outputs=("labels",))["labels"].astype(np.int64), labels)
        assert np.array_equal(_assign(x, None, W, b, outputs=("dist2",))["dist2"].astype(np.int64), z2 + s)


# ---- 2. exact on integers: cluster sums ------------------------------------------------------------------------------
def _int_sums_reference(rows, pivot, g):
    d = rows - pivot.astype(np.int64)
    labels, z2, s = _int_assign_reference(d, g)
    K = g.shape[0]
    sums = np.zeros((K, d.shape[1]), dtype=np.int64)
    np.add.at(sums, labels, d)
    return np.bincount(labels, minlength=K), sums, z2.sum() / 2.0, float(s.sum())


@pytest.mark.parametrize("store_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("C", [3, 37, 238])
def test_cluster_sums_are_exact_on_integers(C, store_dtype):
    """Slots of 47 x 53 = 2491 pixels: two runs, a tail that is neither a multiple of 16 nor of the run.  The slot table is shuffled
    and repeats a slot.  |d| <= 5: a run's fp32 sum stays below 2^14."""
    from hyperpri_amd import cluster as K_
    cubes, masks = _int_cubes(50 + C, 3, cases.SLOT[0], cases.SLOT[1], C)
    cache = _cache(cubes, masks, capacity=4, store_dtype=store_dtype)
    rng = np.random.RandomState(C)
    pivot = rng.randint(0, 2, size=C).astype(np.float32)
    order = [2, 0, 2, 1]
    xs, ms = cubes[order].astype(np.int64), masks[order]
    for K in (1, 3, 17, 33, 64):
        g = _int_centroids(rng, K, C)
        for select in SELECTS:
            sel = np.ones(ms.shape, bool) if select == "all" else (ms != 0) if select == "foreground" else (ms == 0)
            counts, sums, zsum, ssum = _int_sums_reference(xs[sel], pivot, g)
            got = K_.cluster_step(cache, pivot, g.astype(np.float32), order, select)
            assert got.counts.dtype == np.int64 and got.sums.dtype == np.float64 and got.sums.shape == (K, C)
            assert np.array_equal(got.counts, counts), (C, K, select)
            assert np.array_equal(got.sums, sums.astype(np.float64)), (C, K, select)
            assert got.score_sum == zsum and got.sq_sum == ssum
            assert got.inertia == ssum + 2 * zsum


def test_runs_wrap_around_the_partial_accumulators_of_the_cluster_pass():
    """More runs than the pass has partial accumulators (256): a partial then adds several runs, in run order."""
    from hyperpri_amd import cluster as K_
    from hyperpri_amd import spectral as S
    W = (K_.cluster_parts() + 1) * S.FP32_RUN + 37
    cubes, masks = _int_cubes(6, 1, 1, W, 3)
    cache = _cache(cubes, masks)
    pivot = np.array([1, 0, 1], dtype=np.float32)
    g = _int_centroids(np.random.RandomState(2), 3, 3)
    counts, sums, zsum, ssum = _int_sums_reference(cubes[0, 0].astype(np.int64)[masks[0, 0] != 0], pivot, g)
    got = K_.cluster_step(cache, pivot, g.astype(np.float32), None, "foreground")
    assert np.array_equal(got.counts, counts) and np.array_equal(got.sums, sums.astype(np.float64))
    assert got.score_sum == zsum and got.sq_sum == ssum


# ---- 3. the fit labels what the prediction labels --------------------------------------------------------------------
@pytest.mark.parametrize("C,K", cases.UNIFORM_CASES + ((313, 64),))
def test_fit_and_predict_agree(C, K):
    """``counts`` of a fitting pass is the histogram of ``hpri_band_assign``'s labels over the same slots, exactly: the same d, the
    same chain, ambiguous pixels included.  (313, 64) runs both kernels with the tile of 32 pixels."""
    from hyperpri_amd import cluster as K_
    case = cases.uniform_case(C, K)
    cache = _cache(case["cubes"], case["masks"])
    W, b = K_.score_rows(case["centers"])
    labels = np.concatenate([_assign(cache._cubes[i].reshape(-1, cache.cs), case["pivot"], W, b, outputs=("labels",))["labels"] for i in range(3)])
    assert labels.max() < K
    for select in SELECTS:
        m = case["masks"].reshape(-1)
        sel = np.ones(m.shape, bool) if select == "all" else (m != 0) if select == "foreground" else (m == 0)
        got = K_.cluster_step(cache, case["pivot"], case["centers"], None, select)
        assert np.array_equal(got.counts, np.bincount(labels[sel], minlength=K)), (C, K, select)


# ---- 4. real-valued labels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K", cases.UNIFORM_CASES)
def test_labels_and_scores_within_the_derived_bound(C, K):
    """With E[k] = (cs + 1) u (|b[k]| + |W[k]| . |d|), the bound of a chain of cs fused multiply-adds: a pixel the reference does not
    flag has the reference's label; any label is a candidate within the bound; |zmin - z[label]| <= E[label].  dist2 = max(0,
    fmaf(2, zmin, s)): s is a chain of cs non-negative products, (cs + 1) u s; the fmaf rounds once; max(0, .) moves the value towards
    the non-negative truth."""
    from hyperpri_amd import cluster as K_
    case = cases.uniform_case(C, K)
    cs = _rup(C, 8)
    pixels = case["cubes"].reshape(-1, C)
    W, b = K_.score_rows(case["centers"])
    got = _assign(_padded(pixels, cs), case["pivot"], W, b)
    ref, z, amb = K_.assign_reference(pixels, case["pivot"], W, b, cs)
    E = K_.score_bound(pixels, case["pivot"], W, b, cs)
    rows = np.arange(len(ref))
    lab = got["labels"].astype(np.int64)
    assert lab.max() < K and amb.mean() <= 0.005
    assert np.array_equal(lab[~amb], ref[~amb]), f"{(lab != ref)[~amb].sum()} unflagged pixels differ"
    zmin_ref = z[rows, ref]
    gap = z[rows, lab] - zmin_ref
    room = E[rows, lab] + E[rows, ref]
    record_margin(f"cluster/candidate/C{C}/K{K}", (gap / room).max(), 1.0)
    assert (gap <= room).all()
    err = np.abs(got["zmin"].astype(np.float64) - z[rows, lab])
    record_margin(f"cluster/zmin/C{C}/K{K}", (err / E[rows, lab]).max(), 1.0)
    assert (err <= E[rows, lab]).all()
    d = (pixels - case["pivot"]).astype(np.float64)             # fp32(x - pivot), widened
    s = (d * d).sum(axis=1)
    want = np.maximum(2 * z[rows, lab] + s, 0.0)
    inner = 2 * E[rows, lab] + (cs + 1) * U * s
    tol = inner * (1 + U) + U * want
    err = np.abs(got["dist2"].astype(np.float64) - want)
    record_margin(f"cluster/dist2/C{C}/K{K}", (err / tol).max(), 1.0)
    assert (err <= tol).all()


# ---- 5. real-valued sums ---------------------------------------------------------------------------------------------
def test_cluster_sums_within_the_derived_bound():
    """On a mixture the reference flags no pixel of, the counts are exact and |sums - ref| <= (FP32_RUN u + 1e-12) sum_{p in k} |d[p][c]|:
    gamma_n for an fp32 sum of at most FP32_RUN terms, plus fp64 slack.  score_sum: every zmin within E[label]; sq_sum: every s within
    (cs + 1) u s; both then added in fp64."""
    from hyperpri_amd import cluster as K_
    from hyperpri_amd import spectral as S
    case = cases.sums_case()
    C, K = cases.SUMS["C"], cases.SUMS["K"]
    cs = _rup(C, 8)
    for store_dtype, name in ((torch.float32, "f32"), (torch.float16, "f16")):
        cache = _cache(case["cubes"], case["masks"], store_dtype=store_dtype)
        stored = case["cubes"].astype(np.float16).astype(np.float32) if store_dtype == torch.float16 else case["cubes"]
        for select in SELECTS:
            ref, labels, amb = K_.cluster_step_reference(stored, case["pivot"], case["centers"], case["masks"], select, return_ambiguous=True)
            assert not amb.any()
            got = K_.cluster_step(cache, case["pivot"], case["centers"], None, select)
            assert np.array_equal(got.counts, ref.counts), (name, select)
            rows = S._selected_pixels(stored, case["masks"], select)
            d = np.abs((rows.astype(np.float32) - case["pivot"]).astype(np.float64))
            mass = np.zeros((K, C))
            np.add.at(mass, labels, d)
            tol = (S.FP32_RUN * U + 1e-12) * mass
            err = np.abs(got.sums - ref.sums)
            live = tol > 0
            record_margin(f"cluster/sums/{name}/{select}", (err[live] / tol[live]).max() if live.any() else 0.0, 1.0)
            assert (err <= tol).all()
            W, b = K_.score_rows(case["centers"])
            E = K_.score_bound(rows, case["pivot"], W, b, cs)[np.arange(len(labels)), labels]
            _, z, _ = K_.assign_reference(rows, case["pivot"], W, b, cs)
            tol0 = E.sum() + 1e-12 * np.abs(z[np.arange(len(labels)), labels]).sum()
            record_margin(f"cluster/score_sum/{name}/{select}", abs(got.score_sum - ref.score_sum) / tol0, 1.0)
            assert abs(got.score_sum - ref.score_sum) <= tol0
            tol1 = ((cs + 1) * U + 1e-12) * ref.sq_sum
            record_margin(f"cluster/sq_sum/{name}/{select}", abs(got.sq_sum - ref.sq_sum) / tol1, 1.0)
            assert abs(got.sq_sum - ref.sq_sum) <= tol1


def test_one_cluster_is_the_moments_pass():
    """K = 1 about a zero pivot sums what ``band_moments`` sums: the count is exact.  The two passes add a run's pixels in different
    fp32 orders (an ascending chain here, interleaved sub-sums there), so they agree to fp64 accuracy -- 1e-12 relative -- exactly where
    a run's fp32 sums are exact in any order: the data of that check is the mixture rounded to multiples of 2^-12 (|x| < 2, 2048
    terms: 24 bits).  On the unrounded data both lie within FP32_RUN u sum |x| of the truth, so within twice that of each other."""
    from hyperpri_amd import cluster as K_
    from hyperpri_amd import spectral as S
    case = cases.sums_case()
    C = cases.SUMS["C"]
    exact = np.round(case["cubes"] * 4096.0) / 4096.0
    assert np.abs(exact).max() < 2 and exact.dtype == np.float32
    for cubes, name in ((exact, "dyadic"), (case["cubes"], "real")):
        cache = _cache(cubes, case["masks"])
        for select in SELECTS:
            n, sums = S.band_moments(cache, None, select)
            got = K_.cluster_step(cache, np.zeros(C), np.zeros((1, C)), None, select)
            assert got.counts.tolist() == [n]
            assert got.score_sum == 0.0
            diff = np.abs(got.sums[0] - sums[:C])
            if name == "dyadic":
                rel = (diff / np.abs(sums[:C])).max()
                record_margin(f"cluster/k1_moments/{select}", rel, 1e-12)
                assert rel <= 1e-12
            else:
                mass = np.abs(S._selected_pixels(cubes, case["masks"], select)).sum(axis=0)
                tol = 2 * (S.FP32_RUN * U + 1e-12) * mass
                record_margin(f"cluster/k1_moments_real/{select}", (diff / tol).max(), 1.0)
                assert (diff <= tol).all()


# ---- 6. reproducibility ----------------------------------------------------------------------------------------------
def test_bit_reproducible_and_independent_of_the_batch():
    from hyperpri_amd import cluster as K_
    case = cases.uniform_case(238, 8)
    cache = _cache(case["cubes"], case["masks"], out_slots=4)
    a = K_.cluster_step(cache, case["pivot"], case["centers"], None, "foreground")
    b = K_.cluster_step(cache, case["pivot"], case["centers"], None, "foreground")
    assert a.counts.tobytes() == b.counts.tobytes() and a.sums.tobytes() == b.sums.tobytes()
    assert (a.score_sum, a.sq_sum) == (b.score_sum, b.sq_sum)
    model = K_.SpectralKMeans(case["pivot"], case["centers"], foreground_share=np.linspace(0.05, 0.95, 8)).to(DEV)
    for output in K_.OUTPUTS:
        both = cache.batch([0, 2])
        x = model(both, output=output).clone()
        y = model(both, output=output).clone()
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        alone = model(cache.batch([0]), output=output)
        assert alone.cpu().numpy().tobytes() == x[:1].contiguous().cpu().numpy().tobytes()


# ---- 7. end to end ---------------------------------------------------------------------------------------------------
def test_fit_equals_the_reference_and_merges_across_a_split_slot_list():
    from hyperpri_amd import cluster as K_
    from hyperpri_amd import spectral as S
    case = cases.e2e_case()
    C, K = cases.E2E["C"], cases.E2E["K"]
    cache = _cache(case["cubes"], case["masks"])
    model = K_.SpectralKMeans.fit(cache, K, init=case["init"])
    assert model.pivot.device.type == "cuda" and model.k == K and model.in_channels == C
    ref = K_.kmeans_reference(case["cubes"], case["init"], pivot=model.pivot)
    assert ref.ambiguous == 0
    # the pivot is the fp32 mean up to the moments pass' own rounding
    flat = case["cubes"].reshape(-1, C).astype(np.float64)
    assert (np.abs(model.pivot.cpu().numpy() - flat.mean(axis=0)) <= (S.FP32_RUN + 1) * U * np.abs(flat).mean(axis=0)).all()
    assert model.n_iter_ == ref.n_iter and model.converged_ and ref.converged
    labels = model(cache.batch([0, 1, 2]), output="labels")
    assert tuple(labels.shape) == (3, 1, cases.E2E["H"], cases.E2E["W"]) and labels.dtype == torch.uint8
    assert np.array_equal(labels.cpu().numpy().reshape(-1).astype(np.int64), ref.labels)
    assert np.array_equal(model.counts.cpu().numpy(), ref.final.counts)
    # the centres: fp32(sums / n) of sums within the bound of the fitting pass, then one rounding to fp32 on either side
    d = np.abs((case["cubes"].reshape(-1, C) - ref.pivot).astype(np.float64))
    mass = np.zeros((K, C))
    np.add.at(mass, ref.labels, d)
    tol = (S.FP32_RUN * U + 1e-12) * mass / ref.final.counts[:, None] + 2 * U * np.abs(ref.centers.astype(np.float64))
    err = np.abs(model.centers.cpu().numpy().astype(np.float64) - ref.centers.astype(np.float64))
    record_margin("cluster/e2e/centers", (err / tol).max(), 1.0)
    assert (err <= tol).all()
    assert abs(model.inertia_ - ref.final.inertia) <= 1e-4 * ref.final.inertia
    assert np.array_equal(model.centroids, model.pivot.cpu().numpy().astype(np.float64) + model.centers.cpu().numpy().astype(np.float64))

    # two "ranks": this one holds slots 0 and 1, the other slot 2 and follows the same centres in lockstep
    pivot = model.pivot.cpu().numpy()
    state = {"centers": (case["init"] - pivot.astype(np.float64)).astype(np.float32)}

    def merge(mine):
        both = K_.merge_cluster_sums(mine, K_.cluster_step(cache, pivot, state["centers"], [2]))
        new = state["centers"].copy()
        nz = both.counts > 0
        new[nz] = (both.sums[nz] / both.counts[nz, None]).astype(np.float32)
        state["centers"] = new
        return both
    split = K_.SpectralKMeans.fit(cache, K, slots=[0, 1], init=case["init"], merge=merge, pivot=pivot)
    assert split.n_iter_ == model.n_iter_ and np.array_equal(split.counts.cpu().numpy(), model.counts.cpu().numpy())
    assert np.abs(split.centroids - model.centroids).max() <= 1e-10
    assert abs(split.inertia_ - model.inertia_) <= 1e-10 * model.inertia_

    # seeded initialisations from the cache: deterministic; no fit beats the planted optimum
    one = K_.SpectralKMeans.fit(cache, K, init="k-means++", seed=3, n_init=2)
    two = K_.SpectralKMeans.fit(cache, K, init="k-means++", seed=3, n_init=2)
    assert one.centers.cpu().numpy().tobytes() == two.centers.cpu().numpy().tobytes() and one.inertia_ == two.inertia_
    assert int(one.counts.sum()) == case["masks"].size and one.inertia_ >= (1 - 1e-6) * model.inertia_
    sample = K_.SpectralKMeans.fit(cache, K, init="sample", seed=1, select="background", max_iter=3)
    assert int(sample.counts.sum()) == int((case["masks"] == 0).sum())


def test_calibrate_cluster_split_and_evaluate(tmp_path):
    import hyperpri_amd as H
    from hyperpri_amd import cluster as K_
    case = cases.e2e_case()
    C, K, n = cases.E2E["C"], cases.E2E["K"], cases.E2E["n"]
    cache = _cache(case["cubes"], case["masks"])
    model = H.SpectralKMeans.fit(cache, K, init=case["init"])
    with pytest.raises(RuntimeError, match="calibrate"):
        model(cache.batch([0]), output="logit")
    table = model.calibrate(cache)
    truth = case["truth"].reshape(-1)
    labels = model(cache.batch([0, 1, 2])).cpu().numpy().reshape(-1)
    want = np.stack([np.bincount(labels[truth != 0], minlength=K), np.bincount(labels[truth == 0], minlength=K)], axis=1)
    assert table.dtype == np.int64 and np.array_equal(table, want)
    share = model.foreground_share.cpu().numpy()
    assert sorted(share.tolist()) == [0.0, 0.0, 0.0, 0.0, 1.0]              # the mask is one planted component
    pred = H.cluster_split(model, cache.epoch(batch_size=2, shuffle=False))
    assert len(pred) == n and pred.spread is None
    by_batch = torch.cat([model(bt, output="logit")[:, 0].reshape(-1).clone() for bt in cache.epoch(batch_size=2, shuffle=False)])
    assert pred.logits.cpu().numpy().tobytes() == by_batch.cpu().numpy().tobytes()
    lo, hi = np.log(2.0 ** -24) - np.log1p(-2.0 ** -24), np.log(1 - 2.0 ** -24) - np.log(2.0 ** -24)
    vals = np.unique(pred.logits.cpu().numpy())
    assert len(vals) == 2 and abs(vals[0] - lo) <= 1e-5 * abs(lo) and abs(vals[1] - hi) <= 1e-5 * hi
    val = H.validate_net(pred)
    assert val["dice_at_threshold"] > 0.9
    test = H.test_net(pred, val["best_threshold"])
    assert test["counts"]["fp"] == 0 and test["counts"]["fn"] == 0
    files = H.write_segmaps(str(tmp_path), pred, cache.epoch(batch_size=2, shuffle=False), val["best_threshold"], bands=(0, 9, 18), gamma=1.0)
    assert len(files) == n


def test_module_outputs_and_layout_paths():
    """Both logical shapes the cache hands out, the batch dict and the slow layout path give ``SpectralDetector``'s (N, 1, h, w)."""
    from hyperpri_amd import cluster as K_
    C, K = 37, 5
    cubes, masks = _int_cubes(40 + C, 3, 13, 11, C)
    rng = np.random.RandomState(C)
    pivot = rng.randint(0, 2, size=C).astype(np.float32)
    g = _int_centroids(rng, K, C)
    share = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    model = K_.SpectralKMeans(pivot, g.astype(np.float32), foreground_share=share).to(DEV)
    d = cubes[[2, 0]].reshape(-1, C).astype(np.int64) - pivot.astype(np.int64)
    labels, z2, s = _int_assign_reference(d, g)
    p = np.clip(share, 2.0 ** -24, 1 - 2.0 ** -24)
    lut = (np.log(p) - np.log1p(-p)).astype(np.float32)
    want = {"labels": labels.astype(np.uint8), "distance": (z2 + s).astype(np.float32), "score": (z2 / 2.0).astype(np.float32), "logit": lut[labels]}
    x_plain = torch.from_numpy(np.ascontiguousarray(cubes[[2, 0]].transpose(0, 3, 1, 2))).to(DEV)       # plain NCHW: the slow path
    for output in K_.OUTPUTS:
        for unsqueeze in (True, False):
            cache = _cache(cubes, masks, unsqueeze=unsqueeze)
            batch = cache.batch([2, 0])
            for arg in (batch, batch["image"], x_plain):
                y = model(arg, output=output)
                assert tuple(y.shape) == (2, 1, 13, 11) and y.is_contiguous()
                assert y.dtype == (torch.uint8 if output == "labels" else torch.float32)
                assert np.array_equal(y.cpu().numpy().reshape(-1), want[output]), output
    with pytest.raises(RuntimeError, match="autograd"):
        model(x_plain.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="bands"):
        model(x_plain[:, :C - 1].contiguous())
    # the state dict carries the model, on the device
    again = K_.SpectralKMeans.blank(C, K).to(DEV)
    again.load_state_dict(model.state_dict())
    for output in K_.OUTPUTS:
        assert torch.equal(again(x_plain, output=output), model(x_plain, output=output))
    # real cubes of another shape: labels below K whatever the data, NaN included
    real, _ = _real_cubes(3, 1, 9, 7, C)
    real[0, 0, 0, :] = np.nan
    y = model(torch.from_numpy(np.ascontiguousarray(real.transpose(0, 3, 1, 2))).to(DEV))
    assert int(y.max()) < K


# ---- the scores are the projection's chain, bit for bit ----------------------------------------------------------------
def _project(x, W, b):
    """``hpri_band_project`` itself on a (P, cs) fp32 device buffer: the (P, K) outputs of the rows ``W`` (K, C), ``b`` (K,).  A row's
    chain involves no other row, so where the launcher refuses all K rows at once (at cs = 320 sixty-four rows and its tile of 64
    pixels do not fit the LDS together) the rows go through it 32 at a time."""
    from hyperpri_amd import _lib
    from hyperpri_amd._args import _p, _stream
    P, cs = int(x.shape[0]), int(x.shape[1])
    K = int(W.shape[0])
    fits = (cs * _rup(_rup(K, 16), 32) + 64 * (_rup(cs, 32) + 2)) * 4 <= 160 * 1024
    out = []
    for k0 in range(0, K, K if fits else 32):
        k1 = min(K, k0 + (K if fits else 32))
        wd, bd = _rows(W[k0:k1], b[k0:k1], cs)
        y = torch.full((P, _rup(k1 - k0, 8)), float("nan"), dtype=torch.float32, device=DEV)
        _lib.call("hpri_band_project", _p(x), P, cs, _p(wd), _p(bd), k1 - k0, _p(y), _stream())
        torch.cuda.synchronize()
        out.append(y.cpu().numpy()[:, :k1 - k0])
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("C,K,sizes", [(37, 6, (65, 130)), (37, 33, (65, 130)), (313, 64, (70,))])
def test_assign_scores_are_bitwise_the_projection_chain(C, K, sizes):
    """The head of cluster.hip: z[k] is "bitwise the chain of hpri_band_project".  On seeded normal fp32 pixels (no pivot, random W
    and b) ``zmin`` equals the minimum over k < K of the projection's output on the same buffer and rows, bit for bit, and ``labels``
    is the lowest index of that minimum.  K = 6 is one block of 16 rows, K = 33 three; 65 and 130 pixels leave a ragged second tile;
    (313, 64) is cs = 320, where the assign tile is 32 pixels and two waves score."""
    cs = _rup(C, 8)
    rng = np.random.RandomState(1000 * C + K)
    W, b = rng.randn(K, C).astype(np.float32), rng.randn(K).astype(np.float32)
    for P in sizes:
        x = _padded(rng.randn(P, C).astype(np.float32), cs)
        z = _project(x, W, b)
        got = _assign(x, None, W, b, outputs=("labels", "zmin"))
        assert z.shape == (P, K) and np.isfinite(z).all()
        assert np.array_equal(got["zmin"].view(np.uint32), z.min(axis=1).view(np.uint32)), (C, K, P)
        assert np.array_equal(got["labels"].astype(np.int64), z.argmin(axis=1)), (C, K, P)
