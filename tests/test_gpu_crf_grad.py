"""The trainable dense CRF on the device (hyperpri_amd/crf.py, csrc/crf_grad.hip): the training forward bit for bit against ``dense_crf``
for every instantiation, dU == g at zero weights and on one-hot planes, every gradient inside the rounding-model bound against the fp64
restatement of the contract on every case, results that depend neither on the run, the guide's layout, the batch nor the tile, binary
input as plane 1 of the two-plane launch, and end to end ``fit_crf`` on a stored split.  No gradcheck on the device: it is fp32.
Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest
import torch

import _crf_cases as K
import _crf_grad_cases as GC
import _guided_cases as G
from conftest import record_margin
from test_crf_grad_cpu import FIT
from test_gpu_spectral import DEV, _cache

pytestmark = pytest.mark.gpu
CASES = GC.grad_cases()
INF = float("inf")
TH = (2.0, 0.7, 1.5)


def _bits(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


def _frac(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bound).max())


def _dev(x, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).requires_grad_(grad)


def _strided_guide(guide, gs):
    """An (N, K, h, w) view of a channels-last buffer with channel stride ``gs`` and NaN behind the guide."""
    N, Kg, h, w = guide.shape
    buf = torch.full((N, h, w, gs), float("nan"), device=DEV)
    buf[..., :Kg] = torch.from_numpy(guide).to(DEV).permute(0, 2, 3, 1)
    return buf.permute(0, 3, 1, 2)[:, :Kg]


def _run(unary, guide, g, kw, gs=None):
    """``crf_layer`` forward and backward: ``(out, {"unary", "w_appearance", "w_smooth", "compat"})`` as numpy arrays / floats."""
    from hyperpri_amd import crf_layer
    U = _dev(unary, True)
    I = None if guide is None else (_dev(guide) if gs is None else _strided_guide(guide, gs))
    wa = None if guide is None else torch.tensor(float(kw["w_appearance"]), device=DEV, requires_grad=True)
    ws = torch.tensor(float(kw["w_smooth"]), device=DEV, requires_grad=True)
    mu = None if kw.get("compat") is None else _dev(kw["compat"], True)
    out = crf_layer(U, I, wa, ws, mu, kw["radius"], kw["iterations"], kw["theta_alpha"], kw["theta_beta"], kw["theta_gamma"], kw["output"])
    out.backward(_dev(g))
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), {"unary": U.grad.cpu().numpy(), "w_appearance": 0.0 if wa is None else float(wa.grad),
                                        "w_smooth": float(ws.grad), "compat": None if mu is None else mu.grad.cpu().numpy()}


# ---- the training forward is dense_crf -------------------------------------------------------------------------------
@pytest.mark.parametrize("Kg", K.KS)
def test_the_forward_equals_dense_crf_bit_for_bit_for_every_instantiation(Kg):
    from hyperpri_amd import crf, crf_layer, dense_crf
    N, h, w = 2, K.TILE_H + 1, K.TILE_W + 1
    I = _dev(G.real_guide(N, Kg, h, w, seed=Kg)) if Kg else None
    for C in range(2, crf.MAX_CLASSES + 1):
        U = _dev((2.0 * np.random.RandomState(C).randn(N, C, h, w)).astype(np.float32))
        for T, output, mu in ((1, "logit", None), (3, "prob", K.compat(C)), (2, "logit", K.compat(C)), (2, "prob", None)):
            r, wa0, ws0 = K.RADII[(C + T) % 4], (1.5 if Kg else 0.0), 0.75
            want = dense_crf(U, I, r, T, *TH, wa0, ws0, mu, output)
            wa = torch.tensor(wa0, device=DEV) if Kg else None
            ws, m = torch.tensor(ws0, device=DEV), None if mu is None else _dev(mu)
            assert _bits(crf_layer(U, I, wa, ws, m, r, T, *TH, output)) == _bits(want), (C, T, output)          # nothing kept
            out = crf_layer(U, I, wa, ws.clone().requires_grad_(), m, r, T, *TH, output)                       # the stack kept
            assert out.requires_grad and _bits(out) == _bits(want), (C, T, output)
            with torch.no_grad():
                assert not crf_layer(U.clone().requires_grad_(), I, wa, ws, m, r, T, *TH, output).requires_grad
        if C == 2:
            z = U[:, 1].contiguous()
            for output in GC.OUTPUTS:
                want = dense_crf(z, I, 2, 3, *TH, 1.5 if Kg else 0.0, 0.75, None, output)
                got = crf_layer(z.clone().requires_grad_(), I, torch.tensor(1.5, device=DEV) if Kg else None, torch.tensor(0.75, device=DEV),
                                None, 2, 3, *TH, output)
                assert _bits(got) == _bits(want), output


# ---- exact results ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kg", [0, 2])
def test_zero_weights_pass_the_gradient_through_bit_for_bit(Kg):
    N, C, h, w = 2, 5, K.TILE_H + 1, K.TILE_W + 1
    rng = np.random.RandomState(1)
    U, g = (2.0 * rng.randn(N, C, h, w)).astype(np.float32), rng.randn(N, C, h, w).astype(np.float32)
    I = G.real_guide(N, Kg, h, w) if Kg else None
    for mu in (None, K.compat(C)):
        kw = dict(radius=3, iterations=4, theta_alpha=2.0, theta_beta=0.5, theta_gamma=1.0, w_appearance=0.0, w_smooth=0.0, compat=mu, output="logit")
        out, grad = _run(U, I, g, kw, gs=8 if Kg else None)
        assert np.array_equal(out, U) and np.array_equal(grad["unary"], g)
        assert np.isfinite(grad["w_smooth"]) and grad["w_smooth"] != 0.0                  # (the weights' gradients are not zero there)
    kw["compat"] = None
    out, grad = _run(U[:, 1], I, g[:, 1], kw, gs=8 if Kg else None)
    assert np.array_equal(out, U[:, 1]) and np.array_equal(grad["unary"], g[:, 1])      # binary: dz == g


@pytest.mark.parametrize("Kg", K.KS)
def test_on_one_hot_planes_the_softmax_adjoint_is_exactly_zero(Kg):
    """Logits in {-128, +128}: every Q^t is exactly one-hot, Q (x - <Q, x>) is exactly 0 in fp32, so dU == g whatever the weights, and
    the parameter gradients come from iteration T alone -- inside the bound against the reference."""
    from hyperpri_amd import crf
    rng = np.random.RandomState(Kg)
    for C in (2, 3, 8):
        r = K.RADII[(C + Kg) % 4]
        N, h, w = K.FRAMES[(C + Kg) % len(K.FRAMES)]
        U = K.one_hot_logits(N, C, h, w, seed=C)
        g = rng.randn(N, C, h, w).astype(np.float32)
        I = G.real_guide(N, Kg, h, w, seed=C) if Kg else None
        for mu in (None, K.compat(C)):
            kw = dict(radius=r, iterations=3, theta_alpha=2.0, theta_beta=0.7, theta_gamma=INF, w_appearance=2.0 if Kg else 0.0, w_smooth=0.5,
                      compat=mu, output="logit")
            _, grad = _run(U, I, g, kw)
            assert np.array_equal(grad["unary"], g), (C, mu is None)
            ref, bound = crf.crf_backward_reference(U, I, g, **kw), crf.crf_grad_bound(U, I, g, **kw)
            one = crf.crf_backward_reference(U, I, g, **{**kw, "iterations": 1})
            assert abs(ref["w_smooth"] - one["w_smooth"]) <= 1e-12 * max(1.0, abs(one["w_smooth"]))      # iteration T alone
            for key in ("w_appearance", "w_smooth"):
                frac = _frac(abs(grad[key] - ref[key]), bound[key])
                record_margin(f"crf_grad/one_hot/{key}", frac, 1.0)
                assert frac <= 1.0, (C, key, frac)
            if mu is not None:
                assert _frac(np.abs(grad["compat"] - ref["compat"]), bound["compat"]) <= 1.0
            if h * w > 1:
                assert grad["w_smooth"] != 0.0


# ---- real-valued data inside the rounding-model bound ------------------------------------------------------------------
@pytest.mark.parametrize("gcase", CASES, ids=[c[0] for c in CASES])
def test_every_gradient_lies_within_the_bound(gcase):
    name, case, output = gcase
    _, Kg, r, C, gs, T, frame, binary, potts, _ = case
    unary, guide, g, kw = GC.case_inputs(gcase)
    ref, bound = GC.reference(name), GC.bound(name)
    out, grad = _run(unary, guide, g, kw, gs if Kg else None)
    assert np.isfinite(out).all() and np.isfinite(grad["unary"]).all() and grad["unary"].shape == unary.shape
    checks = [("dU", grad["unary"], ref["unary"], bound["unary"]), ("dw_s", grad["w_smooth"], ref["w_smooth"], bound["w_smooth"])]
    if Kg:
        checks.append(("dw_a", grad["w_appearance"], ref["w_appearance"], bound["w_appearance"]))
    if not potts:
        checks.append(("dmu", grad["compat"], ref["compat"], bound["compat"]))
    for what, got, want, lim in checks:
        frac = _frac(np.abs(np.asarray(got, dtype=np.float64) - want), lim)
        print(name, what, frac)
        record_margin(f"crf_grad/{what}/K{Kg}/r{r}", frac, 1.0)
        assert frac <= 1.0, (name, what, frac)
    if frame[1] * frame[2] == 1 and output == "logit":
        assert np.array_equal(grad["unary"], g)                                          # no neighbour: dU == g


# ---- independence, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kg,r,C", [(1, 2, 2), (3, 1, 4), (3, 8, 8), (0, 4, 3)])
def test_gradients_depend_neither_on_the_run_nor_on_the_guide_layout_nor_on_the_batch(Kg, r, C):
    from hyperpri_amd import crf_layer
    N, h, w, T = 3, K.TILE_H + 1, 2 * K.TILE_W + 3, 3
    rng = np.random.RandomState(C)
    U0, g = _dev((2.0 * rng.randn(N, C, h, w)).astype(np.float32)), _dev(rng.randn(N, C, h, w).astype(np.float32))
    guide = G.real_guide(N, Kg, h, w, seed=r) if Kg else None
    mu0 = _dev(K.compat(C))

    def grads(I, sl=slice(None), output="prob"):
        U = U0[sl].clone().requires_grad_()
        wa = torch.tensor(2.0, device=DEV, requires_grad=True) if Kg else None
        ws, mu = torch.tensor(1.0, device=DEV, requires_grad=True), mu0.clone().requires_grad_()
        crf_layer(U, I, wa, ws, mu, r, T, *TH, output).backward(g[sl].contiguous())
        return [_bits(t.grad) for t in (U, ws, mu) + ((wa,) if Kg else ())], U.grad
    I = _dev(guide) if Kg else None
    first, dU = grads(I)
    assert bool(torch.isfinite(dU).all()) and grads(I)[0] == first                       # two runs: every gradient, bit for bit
    if Kg:
        for layout in (I.contiguous(memory_format=torch.channels_last), _strided_guide(guide, 8), I.unsqueeze(1)):
            assert grads(layout)[0] == first
    for n in range(N):                                                                   # alone, and one of three
        alone = grads(I[n:n + 1].contiguous() if Kg else None, slice(n, n + 1))[1]
        assert _bits(alone) == _bits(dU[n:n + 1])
    assert grads(I, output="logit")[0] != first


@pytest.mark.parametrize("Kg,r,C,T", [(1, 1, 2, 3), (2, 2, 3, 2), (3, 4, 8, 1)])
def test_in_phase_pixels_of_a_periodic_problem_have_equal_gradients(Kg, r, C, T):
    """Periods of 5 rows and 7 columns against tiles of 16 x 32: pixels of one phase sit at every place of a tile.  Farther than 2 r T
    from every border (r T for the forward's Q, r T more for the backward) their gradients must be equal -- whatever tile or lane
    computed them, and however far the frame extends beyond."""
    from hyperpri_amd import crf_layer
    m = 2 * r * T
    h, w = 37 + 2 * m, 100 + 2 * m
    I = torch.from_numpy(G.periodic(2, Kg, h, w, seed=r)).to(DEV)
    g = torch.from_numpy(G.periodic(2, C, h, w, seed=90 + r) - 0.5).to(DEV)
    for output in GC.OUTPUTS:
        U = torch.from_numpy(4.0 * G.periodic(2, C, h, w, seed=50 + r) - 2.0).to(DEV).requires_grad_()
        crf_layer(U, I, torch.tensor(2.0, device=DEV), torch.tensor(1.0, device=DEV), _dev(K.compat(C)), r, T, 2.0, 0.3, 1.5, output).backward(g)
        v = U.grad[:, :, m:h - m, m:w - m].cpu().numpy()
        assert v.shape[-2] > 2 * K.TILE_H and v.shape[-1] > 3 * K.TILE_W
        assert np.array_equal(v[..., 5:, :], v[..., :-5, :]) and np.array_equal(v[..., :, 7:], v[..., :, :-7]), output
        assert float(v.std()) > 0.01


@pytest.mark.parametrize("Kg,r", [(0, 2), (1, 3), (3, 8)])
def test_binary_input_gives_the_bits_of_plane_one_of_the_two_plane_launch(Kg, r):
    from hyperpri_amd import crf_layer
    N, h, w = 2, K.TILE_H + 1, 2 * K.TILE_W + 3
    rng = np.random.RandomState(r)
    z0, g = _dev((2.0 * rng.randn(N, h, w)).astype(np.float32)), _dev(rng.randn(N, h, w).astype(np.float32))
    I = _dev(G.real_guide(N, Kg, h, w, seed=r)) if Kg else None
    for mu0 in (None, K.compat(2)):
        for output in GC.OUTPUTS:
            res = []
            for binary in (True, False):
                z = z0.clone().requires_grad_()
                U = z if binary else torch.stack([torch.zeros_like(z), z], dim=1)
                wa = torch.tensor(2.0, device=DEV, requires_grad=True) if Kg else None
                ws = torch.tensor(1.0, device=DEV, requires_grad=True)
                mu = None if mu0 is None else _dev(mu0, True)
                out = crf_layer(U, I, wa, ws, mu, r, 3, *TH, output)
                go = g if binary else (torch.stack([-g, g], dim=1) if output == "logit" else torch.stack([torch.zeros_like(g), g], dim=1))
                out.backward(go)
                res.append([_bits(t.grad) for t in (z, ws) + ((wa,) if Kg else ()) + ((mu,) if mu is not None else ())])
                assert float((z.grad - g).abs().max()) > 1e-3
            assert res[0] == res[1], (mu0 is None, output)


def test_what_is_not_differentiable_raises():
    from hyperpri_amd import crf_layer
    U = torch.zeros(1, 3, 4, 5, device=DEV, requires_grad=True)
    I = torch.zeros(1, 1, 4, 5, device=DEV, requires_grad=True)
    wa, ws = torch.tensor(1.0, device=DEV), torch.tensor(1.0, device=DEV, requires_grad=True)
    with pytest.raises(RuntimeError, match="guide is not differentiable"):
        crf_layer(U, I, wa, ws, None, 2, 2, 1.0, 1.0, 1.0)
    out = crf_layer(U, I.detach(), wa, ws, None, 2, 2, 1.0, 1.0, 1.0)
    (gw,) = torch.autograd.grad((out * out).sum(), ws, create_graph=True)      # (a gradient of the output that itself requires grad)
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):
        gw.backward()
    neg = crf_layer(U, I.detach(), -wa, -ws.detach(), None, 2, 2, 1.0, 1.0, 1.0)          # a repulsive CRF is no error
    assert bool(torch.isfinite(neg).all())


# ---- end to end ------------------------------------------------------------------------------------------------------
def _best_dice(val):
    tp, fp, fn = (val["curve_counts"][k].cpu().numpy().astype(np.float64) for k in ("tp", "fp", "fn"))
    thr = val["thresholds"].cpu().numpy()
    return float((2 * tp / (2 * tp + fp + fn))[:len(thr)].max())


def test_fit_crf_lowers_the_bce_and_raises_the_dice_of_a_stored_split():
    """``fit_crf`` from w_a = w_s = 0 with SCENE's radius, iterations and thetas, one standardised principal component as the guide,
    FIT's Adam steps: the BCE after fitting is below the BCE before, the best Dice of ``crf_split`` with the fitted layer above that of
    the unrefined prediction (tests/test_crf_grad_cpu.py shows the fp64 reference meets both with room).  The four numbers are printed
    and recorded."""
    import hyperpri_amd as H
    cubes, masks = G.blob_scene()
    cache = _cache(cubes, masks)

    def epoch():
        return cache.epoch(batch_size=2, shuffle=False)
    proj = H.SpectralProjection.pca(H.band_statistics(cache), 1, whiten=True).to(DEV)
    pred = H.detect_split(H.SpectralDetector.fit(cache), epoch(), score="ace")
    kw = {k: v for k, v in K.SCENE.items() if not k.startswith("w_")}
    layer = H.CRFLayer(w_appearance=0.0, w_smooth=0.0, **kw).to(DEV)
    assert H.fit_crf(pred, epoch(), proj, layer, FIT["steps"], FIT["lr"]) is layer
    fitted = layer.frozen().get_extra_state()
    fitted.pop("output")
    assert fitted["w_appearance"] > 0.0 and fitted["w_smooth"] > 0.0
    refined = H.crf_split(pred, epoch(), proj, **fitted)
    raw, val = H.validate_net(pred), H.validate_net(refined)
    before, after, raw_dice, dice = float(raw["bce_loss"]), float(val["bce_loss"]), _best_dice(raw), _best_dice(val)
    print("BCE", before, "->", after, "best Dice", raw_dice, "->", dice, "w_a", fitted["w_appearance"], "w_s", fitted["w_smooth"])
    for key, v in (("bce_before", before), ("bce_after", after), ("dice_raw", raw_dice), ("dice_fitted", dice)):
        record_margin(f"crf_grad/fit/{key}", v, 1.0)
    assert after < before and dice > raw_dice
