"""The dense CRF on the device (hyperpri_amd/crf.py, csrc/crf.hip) against the numpy restatement of its contract: untouched logits at
zero weights, L bit for bit on one-hot integer data for every instantiation, Q^1, the last Q and L within the rounding-model bound on
real-valued data for every K, radius and class count, binary input as the two-class problem, results that do not depend on the batch,
the run, the guide's layout or the tile, the multi-class decision, and end to end from a filled cache through ``detect_split`` and
``crf_split`` to the evaluation of a split.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest
import torch

import _crf_cases as K
import _guided_cases as G
from conftest import record_margin
from test_gpu_spectral import DEV, _cache

pytestmark = pytest.mark.gpu
CASES = K.bounded_cases()
INF = float("inf")


def _launch(unary, guide, kw, output="logit", gs=None, iterations=None):
    """``hpri_dense_crf`` itself on (N, C, h, w) unaries (or binary (N, h, w)) and an (N, K, h, w) guide laid out channels-last with
    stride ``gs`` (NaN in the channels past K: they must never count): the output as a numpy array in the unaries' shape."""
    from hyperpri_amd import _lib, crf
    from hyperpri_amd._args import _p, _stream
    binary = unary.ndim == 3
    N, h, w = unary.shape[0], unary.shape[-2], unary.shape[-1]
    C = 2 if binary else unary.shape[1]
    Kg = 0 if guide is None else guide.shape[1]
    a = crf._crf_args(kw["radius"], iterations or kw["iterations"], kw["theta_alpha"], kw["theta_beta"], kw["theta_gamma"], kw["w_appearance"],
                      kw["w_smooth"], output, "test")
    mu = crf._compat(kw.get("compat"), C, "test")
    g = None
    if Kg:
        gs = Kg if gs is None else gs
        buf = np.full((N, h, w, gs), np.nan, dtype=np.float32)
        buf[..., :Kg] = guide.transpose(0, 2, 3, 1)
        g = torch.from_numpy(buf).to(DEV)
    u = torch.from_numpy(np.ascontiguousarray(unary, dtype=np.float32)).to(DEV)
    nbytes = int(_lib.load().hpri_crf_workspace_bytes(N, C, h, w))
    assert nbytes == 8 * N * C * h * w
    work = torch.full((2, N, C, h, w), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full(tuple(unary.shape), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("hpri_dense_crf", _p(u), int(binary), _p(g) if Kg else None, gs if Kg else 0, Kg, N, C, h, w, a["radius"], a["iterations"],
              a["ta"].ctypes.data, a["tg"].ctypes.data, a["b"], a["w_appearance"], a["w_smooth"], mu.ctypes.data if mu is not None else None,
              crf.CRF_OUTPUTS.index(output), _p(work), nbytes, _p(out), _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bits(t):
    return t.contiguous().cpu().numpy().tobytes()


def _frac(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bound).max())


# ---- zero weights ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kg", [0, 2])
def test_zero_weights_return_the_logits_bit_for_bit(Kg):
    from hyperpri_amd import crf
    N, C, h, w = 2, 5, K.TILE_H + 1, K.TILE_W + 1
    U = (2.0 * np.random.RandomState(1).randn(N, C, h, w)).astype(np.float32)
    I = G.real_guide(N, Kg, h, w) if Kg else None
    for mu in (None, K.compat(C)):
        kw = dict(radius=3, iterations=4, theta_alpha=2.0, theta_beta=0.5, theta_gamma=1.0, w_appearance=0.0, w_smooth=0.0, compat=mu)
        assert np.array_equal(_launch(U, I, kw, gs=8), U)
        ref, bound = crf.crf_reference(U, I, **kw), crf.crf_bound(U, I, **kw)
        e = np.exp(U.astype(np.float64) - U.astype(np.float64).max(axis=1, keepdims=True))
        assert np.abs(ref["prob"] - e / e.sum(axis=1, keepdims=True)).max() <= 1e-15         # the reference's softmax of U
        frac = _frac(np.abs(_launch(U, I, kw, "prob", gs=8) - ref["prob"]), bound["prob"])
        record_margin("crf/zero_weights/prob", frac, 1.0)
        assert frac <= 1.0
    kw["compat"] = None
    z = U[:, 1]
    assert np.array_equal(_launch(z, I, kw, gs=8), z)                                    # binary: fp32(z - 0)
    ref, bound = crf.crf_reference(z, I, **kw), crf.crf_bound(z, I, **kw)
    assert _frac(np.abs(_launch(z, I, kw, "prob", gs=8) - ref["prob"]), bound["prob"]) <= 1.0


# ---- exact on integers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kg", K.KS)
def test_one_iteration_on_one_hot_planes_is_exact(Kg):
    """A constant guide, infinite theta_alpha and theta_gamma, w_a = 2 and w_s = 1/2, logits in {-128, +128}: Q^0 is exactly one-hot,
    every k is 2.5 (w_s alone without a guide), M_l is that times a count, m one correctly rounded division, L one addition: L equals
    the reference rounded the same way, bit for bit -- for every class count, on every frame."""
    from hyperpri_amd import crf
    const = np.array([3.0, -2.0, 4.0], dtype=np.float32)[:Kg]
    seen = set()
    for C in range(2, crf.MAX_CLASSES + 1):
        r = K.RADII[(C + Kg) % 4]
        for frame in K.FRAMES[(C + Kg) % 2::2]:
            N, h, w = frame
            seen.add(frame)
            U = K.one_hot_logits(N, C, h, w, seed=C)
            I = np.broadcast_to(const[None, :, None, None], (N, Kg, h, w)).copy() if Kg else None
            kw = dict(radius=r, iterations=1, theta_alpha=INF, theta_beta=1.0, theta_gamma=INF, w_appearance=2.0 if Kg else 0.0, w_smooth=0.5)
            want = crf.crf_reference(U, I, dtype=np.float32, **kw)
            q0 = crf.crf_reference(U, I, dtype=np.float32, **{**kw, "w_smooth": 0.0, "w_appearance": 0.0})["Q"]
            assert set(np.unique(q0)) == {0.0, 1.0}                                      # softmax(U) in fp32 is exactly one-hot
            got = _launch(U, I, kw, gs=(0, 1, 3, 8)[Kg])
            assert np.array_equal(got, want["L"].astype(np.float32)), (C, r, frame)
            if h * w > 1:
                assert not np.array_equal(got, U)
    assert seen == set(K.FRAMES)


# ---- real-valued data inside the rounding-model bound ------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_q1_q_and_l_within_the_bound(case):
    name, Kg, r, C, gs, T, frame, binary, potts, _ = case
    unary, guide, kw = K.case_inputs(case)
    ref, bound = K.reference(name), K.bound(name)
    q1 = _launch(unary, guide, kw, "prob", gs, iterations=1)
    q, L = _launch(unary, guide, kw, "prob", gs), _launch(unary, guide, kw, "logit", gs)
    assert np.isfinite(q1).all() and np.isfinite(q).all() and np.isfinite(L).all()
    pick = (lambda x: x[:, 1]) if binary else (lambda x: x)
    for what, got, want, lim in (("Q1", q1, pick(ref["steps"][0]), pick(bound["steps"][0])), ("Q", q, ref["prob"], bound["prob"]),
                                 ("L", L, ref["logit"], bound["logit"])):
        frac = _frac(np.abs(got - want), lim)
        print(name, what, frac)
        record_margin(f"crf/{what}/K{Kg}/r{r}", frac, 1.0)
        assert frac <= 1.0, (name, what, frac)
    if T == 1:
        assert np.array_equal(q1, q)


# ---- binary input ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kg,r", [(0, 2), (1, 3), (3, 8)])
def test_binary_input_is_the_two_class_problem_bit_for_bit(Kg, r):
    from hyperpri_amd import dense_crf
    N, h, w = 2, K.TILE_H + 1, 2 * K.TILE_W + 3
    z = torch.from_numpy((2.0 * np.random.RandomState(r).randn(N, h, w)).astype(np.float32)).to(DEV)
    I = torch.from_numpy(G.real_guide(N, Kg, h, w, seed=r)).to(DEV) if Kg else None
    two = torch.stack([torch.zeros_like(z), z], dim=1)
    for mu in (None, K.compat(2)):
        args = (r, 3, 2.0, 0.7, 1.5, 2.0 if Kg else 0.0, 1.0, mu)
        L, Q = dense_crf(two, I, *args), dense_crf(two, I, *args, output="prob")
        lb, qb = dense_crf(z, I, *args), dense_crf(z, I, *args, output="prob")
        assert tuple(lb.shape) == (N, h, w) and tuple(L.shape) == (N, 2, h, w)
        assert _bits(lb) == _bits(L[:, 1] - L[:, 0]) and _bits(qb) == _bits(Q[:, 1])
        assert float((lb - z).abs().max()) > 0.01                                        # (and the launch did refine them)
    # Potts is the matrix -Id
    assert _bits(dense_crf(two, I, *args[:-1], -np.eye(2, dtype=np.float32))) == _bits(dense_crf(two, I, *args[:-1], None))


# ---- independence, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kg,r,C", [(1, 2, 2), (3, 1, 4), (3, 8, 8), (0, 4, 3)])
def test_a_result_depends_neither_on_the_batch_nor_on_the_run_nor_on_the_guide_layout(Kg, r, C):
    from hyperpri_amd import DenseCRF
    from hyperpri_amd import guided as GF
    N, h, w = 3, K.TILE_H + 1, 2 * K.TILE_W + 3
    U = torch.from_numpy((2.0 * np.random.RandomState(C).randn(N, C, h, w)).astype(np.float32)).to(DEV)
    I = torch.from_numpy(G.real_guide(N, Kg, h, w, seed=r)).to(DEV) if Kg else None
    mod = DenseCRF(r, 3, 2.0, 0.7, 1.5, 2.0 if Kg else 0.0, 1.0, compat=K.compat(C), output="prob")
    q = mod(U, I)
    assert tuple(q.shape) == (N, C, h, w) and bool(torch.isfinite(q).all()) and _bits(mod(U, I)) == _bits(q)      # two runs
    for n in range(N):                                                                                            # alone, and one of three
        assert _bits(mod(U[n:n + 1].contiguous(), I[n:n + 1].contiguous() if Kg else None)) == _bits(q[n:n + 1])
    if Kg:
        assert GF._guide_input(I)[1] == (Kg if Kg > 1 else 1)                            # planar: the layout pass (one plane: as it is)
        last = I.contiguous(memory_format=torch.channels_last)                          # channels-last with a stride of K: zero-copy
        src, gs = GF._guide_input(last)
        assert gs == Kg and src.data_ptr() == last.data_ptr() and _bits(mod(U, last)) == _bits(q)
        wide = torch.full((N, h, w, 8), float("nan"), device=DEV)                       # stride 8, NaN behind the guide
        wide[..., :Kg] = I.permute(0, 2, 3, 1)
        view = wide.permute(0, 3, 1, 2)[:, :Kg]
        src, gs = GF._guide_input(view)
        assert gs == 8 and src.data_ptr() == view.data_ptr() and _bits(mod(U, view)) == _bits(q)
        assert _bits(mod(U, I.unsqueeze(1))) == _bits(q)                                 # (N, 1, K, h, w)


@pytest.mark.parametrize("Kg,r,C,T", [(1, 1, 2, 4), (2, 2, 3, 3), (3, 4, 8, 2)])
def test_in_phase_pixels_of_a_periodic_image_are_equal(Kg, r, C, T):
    """Periods of 5 rows and 7 columns against tiles of 16 x 32: pixels of one phase sit at every place of a tile.  Farther than r T
    from every border their T-fold neighbourhoods are the same, so their results must be -- whatever tile or lane computed them."""
    from hyperpri_amd import dense_crf
    m = r * T
    h, w = 37 + 2 * m, 100 + 2 * m
    I = torch.from_numpy(G.periodic(2, Kg, h, w, seed=r)).to(DEV)
    U = torch.from_numpy(4.0 * G.periodic(2, C, h, w, seed=50 + r) - 2.0).to(DEV)
    for output in ("logit", "prob"):
        v = dense_crf(U, I, r, T, 2.0, 0.3, 1.5, 2.0, 1.0, K.compat(C), output)[:, :, m:h - m, m:w - m].cpu().numpy()
        assert v.shape[-2] > 2 * K.TILE_H and v.shape[-1] > 3 * K.TILE_W
        assert np.array_equal(v[..., 5:, :], v[..., :-5, :]) and np.array_equal(v[..., :, 7:], v[..., :, :-7]), output
        assert float(v.std()) > 0.01


# ---- multi-class use -------------------------------------------------------------------------------------------------
def test_the_argmax_of_the_refined_logits_is_the_references():
    import hyperpri_amd as H
    from hyperpri_amd import crf
    unary, guide, kw, lab = K.multiclass_case()
    ref, bound = crf.crf_reference(unary, guide, **kw), crf.crf_bound(unary, guide, **kw)
    top = np.sort(ref["L"], axis=1)
    decided = top[:, -1] - top[:, -2] > 2 * bound["L"].max(axis=1)
    assert decided.mean() > 0.99                                                         # (tests/test_crf_cpu.py says so of the case)
    L = H.dense_crf(torch.from_numpy(unary).to(DEV), torch.from_numpy(guide).to(DEV), **kw)
    classes = H.argmax_classes(L)
    assert classes.dtype == torch.uint8 and tuple(classes.shape) == lab[None].repeat(2, axis=0).shape
    got = classes.cpu().numpy()
    assert np.array_equal(got[decided], ref["L"].argmax(axis=1).astype(np.uint8)[decided])
    frac = _frac(np.abs(L.cpu().numpy() - ref["L"]), bound["L"])
    record_margin("crf/multiclass/L", frac, 1.0)
    assert frac <= 1.0
    assert (got == lab).mean() >= (unary.argmax(axis=1) == lab).mean() + 0.1             # and it repairs the labels


# ---- end to end ------------------------------------------------------------------------------------------------------
def _best_dice(val):
    """The best Dice 2 tp / (2 tp + fp + fn) over the thresholds of ``validate_net``'s curve, from the integer counts."""
    tp, fp, fn = (val["curve_counts"][k].cpu().numpy().astype(np.float64) for k in ("tp", "fp", "fn"))
    thr = val["thresholds"].cpu().numpy()
    return float((2 * tp / (2 * tp + fp + fn))[:len(thr)].max())


def test_statistics_guide_detect_crf_and_evaluate():
    import hyperpri_amd as H
    cubes, masks = G.blob_scene()
    n = cubes.shape[0]
    cache = _cache(cubes, masks)

    def epoch():
        return cache.epoch(batch_size=2, shuffle=False)
    proj = H.SpectralProjection.pca(H.band_statistics(cache), 1, whiten=True).to(DEV)    # one standardised principal component
    det = H.SpectralDetector.fit(cache)
    pred = H.detect_split(det, epoch(), score="ace")
    refined = H.crf_split(pred, epoch(), proj, **K.SCENE)
    assert refined is not pred and len(refined) == n and refined.spread is None
    assert refined.masks is pred.masks and refined.offsets == pred.offsets and refined.sizes == pred.sizes and refined.names == pred.names
    assert bool(torch.isfinite(refined.logits).all()) and _bits(refined.logits) != _bits(pred.logits)
    by_batch = torch.cat([H.dense_crf(det(bt, score="ace", logit=True)[:, 0].contiguous(), proj(bt["image"]), **K.SCENE).reshape(-1).clone()
                          for bt in epoch()])
    assert _bits(refined.logits) == _bits(by_batch)
    raw, val = H.validate_net(pred), H.validate_net(refined)
    raw_dice, dice = _best_dice(raw), _best_dice(val)
    print("best Dice raw", raw_dice, "refined", dice)
    assert dice >= raw_dice + 0.05 and np.isfinite(val["avg_prec"]) and np.isfinite(val["bce_loss"])
    # the stored spread is carried over; no guide at all is smoothness alone
    pred.spread = torch.zeros_like(pred.logits)
    smooth = H.crf_split(pred, epoch(), None, **{**K.SCENE, "w_appearance": 0.0})
    assert smooth.spread is pred.spread and bool(torch.isfinite(smooth.logits).all())
    with pytest.raises(ValueError, match="same order"):
        H.crf_split(pred, reversed(list(epoch())), proj, **K.SCENE)
    with pytest.raises(ValueError, match="held 2 of the 3"):
        H.crf_split(pred, list(epoch())[:1], proj, **K.SCENE)
    with pytest.raises(ValueError, match="at most 3"):
        H.crf_split(pred, epoch(), H.SpectralProjection.pca(H.band_statistics(cache), 4), **K.SCENE)
    with pytest.raises(RuntimeError, match="autograd"):
        H.dense_crf(torch.zeros(1, 4, 5, device=DEV, requires_grad=True), None, 2, 2, 1.0, 1.0, 1.0, 0.0, 1.0)
