"""The trainable dense CRF without a GPU (hyperpri_amd/crf.py): the backward's contract restated in numpy against torch.autograd through
an fp64 restatement of the forward, the rounding-model bound against an fp32 emulation of the device on every case the GPU tests use
(and against single mutations of the contract, which must leave it by orders of magnitude), the module's state, the argument errors,
the ABI, the code objects, and the end-to-end fit on the reference."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import _crf_cases as K
import _crf_grad_cases as GC
import _guided_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = GC.grad_cases()
INF = float("inf")
FIT = dict(steps=30, lr=0.2)                       # the end-to-end fit, here on the reference and in tests/test_gpu_crf_grad.py on the device


def _frac(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bound).max())


def _worst(got, ref, bound):
    """The largest used fraction over dU and the parameter gradients."""
    worst = _frac(np.abs(got["unary"] - ref["unary"]), bound["unary"])
    for key in ("w_appearance", "w_smooth"):
        worst = max(worst, _frac(abs(got[key] - ref[key]), bound[key]))
    if ref["compat"] is not None:
        worst = max(worst, _frac(np.abs(got["compat"] - ref["compat"]), bound["compat"]))
    return worst


# ---- the restated contract against autograd ----------------------------------------------------------------------------
def _torch_forward(U, I, a, wa, ws, mu, binary, output):
    """The forward in fp64 torch: the pairwise weight is ``w_a (ta ta) e + w_s (tg tg)`` with the fp32 table products the backward's
    contract names (the case table's weights are powers of two, for which the forward's rounded ``(w ta) ta`` is the same number)."""
    from hyperpri_amd import guided
    if binary:
        U = torch.stack([torch.zeros_like(U), U], dim=1)
    N, C, h, w = U.shape
    r, T = a["radius"], a["iterations"]
    PA = torch.from_numpy((a["ta"][:, None] * a["ta"][None, :]).astype(np.float32).astype(np.float64))
    PS = torch.from_numpy((a["tg"][:, None] * a["tg"][None, :]).astype(np.float32).astype(np.float64))
    den = torch.from_numpy(guided._counts(h, w, r) - 1.0)
    pad = torch.nn.functional.pad
    Ip = None if I is None else pad(I, (r, r, r, r))
    Q = torch.softmax(U, dim=1)
    L = U
    for _ in range(T):
        Qp = pad(Q, (r, r, r, r))
        M = torch.zeros_like(U)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dy == 0 and dx == 0:
                    continue
                k = ws * PS[abs(dy), abs(dx)]
                if I is not None:
                    d2 = ((Ip[:, :, r + dy:r + dy + h, r + dx:r + dx + w] - I) ** 2).sum(dim=1, keepdim=True)
                    k = k + wa * PA[abs(dy), abs(dx)] * torch.exp(-d2 * a["b"])
                M = M + k * Qp[:, :, r + dy:r + dy + h, r + dx:r + dx + w]
        m = torch.where(den > 0, M / den.clamp(min=1.0), torch.zeros_like(M))
        L = U + m if mu is None else U - torch.einsum("lk,nkhw->nlhw", mu, m)
        Q = torch.softmax(L, dim=1)
    if binary:
        return L[:, 1] - L[:, 0] if output == "logit" else Q[:, 1]
    return L if output == "logit" else Q


SMALL = [c for c in CASES if c[1][6][1] * c[1][6][2] <= 20 * 40]


@pytest.mark.parametrize("frame", [(1, 1), (3, 5), (11, 13)])
@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("Kg", [0, 1, 3])
def test_the_reference_equals_autograd_through_an_fp64_forward(Kg, C, r, frame):
    """tests/test_crf_cpu.py's grid for the forward's oracle, here for the backward: Potts and the non-symmetric mu, both outputs,
    binary input for C = 2; T = 3 and weights of 1 and 1/2, at which the derived worst-case tolerance on dU is still below 1e-6."""
    from hyperpri_amd import crf
    h, w = frame
    N, T, wa0, ws0 = 2, 3, (1.0 if Kg else 0.0), 0.5
    rng = np.random.RandomState(10 * Kg + C + r)
    unary = (2.0 * rng.randn(N, C, h, w)).astype(np.float32)
    guide = G.real_guide(N, Kg, h, w, seed=r) if Kg else None
    th = dict(theta_alpha=2.0, theta_beta=0.7, theta_gamma=1.5)
    a = crf._crf_args(r, T, th["theta_alpha"], th["theta_beta"], th["theta_gamma"], 0.0, 0.0, "logit", "test")
    for mu0 in (None, K.compat(C)):
        for output in GC.OUTPUTS:
            for binary in ((False, True) if C == 2 else (False,)):
                un = unary[:, 1] if binary else unary
                g = rng.randn(*un.shape).astype(np.float32)
                U = torch.from_numpy(un.astype(np.float64)).requires_grad_()
                I = None if guide is None else torch.from_numpy(guide.astype(np.float64))
                wa = torch.tensor(wa0, dtype=torch.float64, requires_grad=True)
                ws = torch.tensor(ws0, dtype=torch.float64, requires_grad=True)
                mu = None if mu0 is None else torch.from_numpy(mu0.astype(np.float64)).requires_grad_()
                out = _torch_forward(U, I, a, wa, ws, mu, binary, output)
                (out * torch.from_numpy(g.astype(np.float64))).sum().backward()
                ref = crf.crf_backward_reference(un, guide, g, r, T, w_appearance=wa0, w_smooth=ws0, compat=mu0, output=output, **th)
                mu_sum = 1.0 if mu0 is None else float(np.abs(mu0).sum(axis=0).max())
                tol_u, tol_p = GC.fp64_grad_tolerance((2 * r + 1) ** 2, C, T, wa0 + ws0, mu_sum, float(np.abs(un).max()), float(np.abs(g).max()))
                tol_sum = N * h * w * tol_p
                assert tol_u <= 1e-6 and tol_sum <= 1e-3, (tol_u, tol_sum)          # worst-case gains; the differences seen are near 1e-15
                assert ref["unary"].shape == un.shape and np.abs(ref["unary"] - U.grad.numpy()).max() <= tol_u, (output, binary)
                assert abs(ref["w_smooth"] - float(ws.grad)) <= tol_sum
                assert abs(ref["w_appearance"] - float(wa.grad)) <= tol_sum if Kg else ref["w_appearance"] == 0.0
                if mu0 is None:
                    assert ref["compat"] is None
                else:
                    assert np.abs(ref["compat"] - mu.grad.numpy()).max() <= tol_sum
                    assert np.abs(ref["compat"]).max() > 0 or h * w == 1
                if h * w == 1 and output == "logit":                                    # no neighbour: dU = g
                    assert np.array_equal(ref["unary"], g.astype(np.float64))
    # Potts is the matrix -Id
    g = rng.randn(*unary.shape).astype(np.float32)
    one = crf.crf_backward_reference(unary, guide, g, r, T, w_appearance=wa0, w_smooth=ws0, **th)
    two = crf.crf_backward_reference(unary, guide, g, r, T, w_appearance=wa0, w_smooth=ws0, compat=-np.eye(C, dtype=np.float32), **th)
    assert np.array_equal(one["unary"], two["unary"]) and one["w_smooth"] == two["w_smooth"]


# ---- the bound is not vacuous ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("gcase", CASES, ids=[c[0] for c in CASES])
def test_an_fp32_emulation_of_the_device_stays_inside_the_bound(gcase):
    from hyperpri_amd import crf
    name = gcase[0]
    unary, guide, g, kw = GC.case_inputs(gcase)
    ref, bound = GC.reference(name), GC.bound(name)
    emu = crf.crf_backward_reference(unary, guide, g, dtype=np.float32, **kw)
    assert bound["unary"].shape == ref["unary"].shape and np.isfinite(bound["unary"]).all()
    assert _worst(emu, ref, bound) <= 1.0
    # and it is a bound worth having: a few hundredths of the gradient's size at the very most (the forward's bound on Q^(t-1), which
    # crf_bound lets grow to 1e-2 over five iterations, passes through here); the parameters' bounds add it up over every pixel
    assert bound["unary"].max() <= 5e-2 * max(1.0, np.abs(ref["unary"]).max())


MUTATIONS = {"centre included": "centre", "division by n_j": "nj", "mu instead of mu^T": "mu", "no inner product": "no_inner",
             "one iteration fewer": "short", "no gL^0": "no_gl0"}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_a_single_mutation_of_the_contract_leaves_the_bound(mutation):
    from hyperpri_amd import crf
    broken = []
    for gcase in SMALL:
        name, case, output = gcase
        _, Kg, r, C, gs, T, (N, h, w), binary, potts, _ = case
        if h * w == 1 or (mutation == "mu instead of mu^T" and potts) or (mutation == "one iteration fewer" and T == 1):
            continue
        unary, guide, g, kw = GC.case_inputs(gcase)
        got = crf.crf_backward_reference(unary, guide, g, _variant=MUTATIONS[mutation], **kw)
        worst = _worst(got, GC.reference(name), GC.bound(name))
        if worst > 1.0:
            broken.append((name, worst))
    assert broken, mutation
    assert max(v for _, v in broken) > 100.0, broken


def test_the_cases_cover_every_kernel_both_outputs_and_both_inputs():
    base = [c[1] for c in CASES]
    assert {(c[1], c[2], c[3]) for c in base} == {(k, r, C) for k in K.KS for r in K.RADII for C in K.CS} and len(CASES) == 48
    assert {c[6] for c in base} == set(G.FRAMES) and {c[5] for c in base} == {1, 2, 5}
    for sel in (lambda c: c[7], lambda c: c[3] == 2 and not c[7], lambda c: c[8], lambda c: not c[8], lambda c: c[5] == 1, lambda c: c[5] == 5):
        assert {o for _, c, o in CASES if sel(c)} == set(GC.OUTPUTS)
    assert SMALL and any(c[1][5] == 5 for c in SMALL) and any(not c[1][8] for c in SMALL)


# ---- the module ------------------------------------------------------------------------------------------------------
def test_the_layer_carries_weights_as_parameters_and_the_rest_as_extra_state():
    from hyperpri_amd import CRFLayer
    mu = K.compat(3)
    src = CRFLayer(3, 5, INF, 0.5, 2.0, 4.0, 1.0, compat=mu, output="prob")
    assert {n for n, _ in src.named_parameters()} == {"w_appearance", "w_smooth"}
    sd = src.state_dict()
    assert set(sd) == {"w_appearance", "w_smooth", "_extra_state"}
    assert sd["_extra_state"] == {"radius": 3, "iterations": 5, "theta_alpha": INF, "theta_beta": 0.5, "theta_gamma": 2.0, "output": "prob",
                                  "learn_compat": False, "compat": mu.tolist()}
    assert sd["w_appearance"].dtype == torch.float32 and sd["w_appearance"].dim() == 0 and float(sd["w_appearance"]) == 4.0
    dst = CRFLayer(1, 1, 1.0, 1.0, 1.0, 0.0, 0.0)
    dst.load_state_dict(sd)
    assert dst.get_extra_state() == src.get_extra_state() and float(dst.w_smooth) == 1.0 and float(dst.w_appearance) == 4.0
    assert np.array_equal(dst._fixed_compat.numpy(), mu) and "radius=3" in repr(dst)
    with pytest.raises(ValueError, match="iterations"):
        dst.load_state_dict({**sd, "_extra_state": {**sd["_extra_state"], "iterations": 40}})
    learn = CRFLayer(3, 5, INF, 0.5, 2.0, 4.0, 1.0, compat=mu, learn_compat=True)
    assert {n for n, _ in learn.named_parameters()} == {"w_appearance", "w_smooth", "compat"} and learn.get_extra_state()["compat"] is None
    with pytest.raises(ValueError, match="learn_compat"):
        learn.load_state_dict(sd, strict=False)
    with pytest.raises(ValueError, match="learn_compat"):
        CRFLayer(3, 5, INF, 0.5, 2.0, 4.0, 1.0, learn_compat=True)
    bare = CRFLayer(2, 2, 1.0, 1.0, 1.0, None, 0.5)                                        # no guide: w_appearance fixed at 0, no parameter
    assert {n for n, _ in bare.named_parameters()} == {"w_smooth"} and set(bare.state_dict()) == {"w_smooth", "_extra_state"}
    assert bare.frozen().w_appearance == 0.0
    for bad in (dict(radius=0), dict(output="label"), dict(w_smooth=INF), dict(theta_beta=0.0)):
        args = dict(radius=2, iterations=2, theta_alpha=1.0, theta_beta=1.0, theta_gamma=1.0, w_appearance=1.0, w_smooth=1.0, output="logit")
        with pytest.raises(ValueError, match=next(iter(bad))):
            CRFLayer(**{**args, **bad})


def test_frozen_and_from_crf_are_inverse_to_each_other():
    from hyperpri_amd import CRFLayer, DenseCRF
    for mu in (None, K.compat(4)):
        for learn in ((False, True) if mu is not None else (False,)):
            crf = DenseCRF(3, 5, 2.0, 0.5, INF, 4.0, 0.75, compat=mu, output="prob")
            layer = CRFLayer.from_crf(crf, learn_compat=learn)
            assert isinstance(layer, CRFLayer) and layer.frozen().get_extra_state() == crf.get_extra_state()
            again = CRFLayer.from_crf(layer.frozen(), learn_compat=learn)
            assert again.get_extra_state() == layer.get_extra_state()
            assert all(torch.equal(a, b) for a, b in zip(again.parameters(), layer.parameters()))
    smooth = DenseCRF(2, 2, 1.0, 1.0, 1.0, 0.0, 0.5)
    assert CRFLayer.from_crf(smooth, guided=False).w_appearance is None
    assert CRFLayer.from_crf(smooth, guided=False).frozen().get_extra_state() == smooth.get_extra_state()
    with pytest.raises(ValueError, match="guided"):
        CRFLayer.from_crf(DenseCRF(2, 2, 1.0, 1.0, 1.0, 1.0, 0.5), guided=False)
    neg = CRFLayer(2, 2, 1.0, 1.0, 1.0, 1.0, -0.5)                                         # a repulsive layer trains; dense_crf does not take it
    with pytest.raises(ValueError, match="w_smooth"):
        neg.frozen()


def test_argument_errors():
    from hyperpri_amd import CRFLayer, crf_layer
    from hyperpri_amd import crf
    U, I = torch.zeros(2, 3, 4, 5), torch.zeros(2, 2, 4, 5)
    wa, ws = torch.tensor(1.0), torch.tensor(1.0)
    th = (2, 3, 2.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="radius"):
        crf_layer(U, I, wa, ws, None, 0, *th[1:])
    with pytest.raises(ValueError, match="iterations"):
        crf_layer(U, I, wa, ws, None, 2, 17, *th[2:])
    with pytest.raises(ValueError, match="theta_beta"):
        crf_layer(U, I, wa, ws, None, 2, 3, 2.0, 0.0, 1.0)
    with pytest.raises(ValueError, match="output"):
        crf_layer(U, I, wa, ws, None, *th, output="label")
    with pytest.raises(ValueError, match="float32 unary"):
        crf_layer(U.double(), I, wa, ws, None, *th)
    with pytest.raises(ValueError, match="unaries"):
        crf_layer(torch.zeros(2, 9, 4, 5), I, wa, ws, None, *th)
    with pytest.raises(ValueError, match="frame"):
        crf_layer(U, torch.zeros(2, 2, 4, 6), wa, ws, None, *th)
    for bad in (1.0, torch.ones(1), torch.tensor(1.0, dtype=torch.float64)):
        with pytest.raises(ValueError, match="w_appearance"):
            crf_layer(U, I, bad, ws, None, *th)
        with pytest.raises(ValueError, match="w_smooth"):
            crf_layer(U, I, wa, bad, None, *th)
    with pytest.raises(ValueError, match="without a guide"):
        crf_layer(U, None, wa, ws, None, *th)
    for bad in (torch.zeros(2, 2), torch.zeros(3, 3, dtype=torch.float64), np.zeros((3, 3), np.float32)):
        with pytest.raises(ValueError, match="compat"):
            crf_layer(U, I, wa, ws, bad, *th)
    with pytest.raises(ValueError, match="empty"):
        crf_layer(torch.zeros(2, 3, 0, 5), None, None, ws, None, *th)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crf_layer(U, I, wa, ws, torch.zeros(3, 3), *th)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CRFLayer(*th, 1.0, 1.0)(U, I)
    with pytest.raises(ValueError, match="takes a guide"):
        CRFLayer(*th, 1.0, 1.0)(U)
    with pytest.raises(ValueError, match="takes none"):
        CRFLayer(*th, None, 1.0)(U, I)
    g = np.zeros((2, 3, 4, 5), np.float32)
    with pytest.raises(ValueError, match="gradient"):
        crf.crf_backward_reference(U.numpy(), I.numpy(), g[:, :2], *th, 1.0, 1.0)
    with pytest.raises(ValueError, match="without a guide"):
        crf.crf_backward_reference(U.numpy(), None, g, *th, 1.0, 1.0)
    with pytest.raises(ValueError, match="non-negative"):
        crf.crf_grad_bound(U.numpy(), I.numpy(), g, *th, 1.0, -1.0)
    neg = crf.crf_backward_reference(U.numpy() + 1.0, I.numpy(), g + 1.0, *th, -1.0, -0.5)     # a repulsive CRF is no error
    assert np.isfinite(neg["unary"]).all()


def test_fit_crf_checks_its_arguments_before_any_launch():
    import hyperpri_amd as H
    pred = H.SplitPrediction(torch.zeros(40), torch.zeros(40), [0, 20, 40], [(4, 5), (4, 5)], ["a", "b"], None)
    layer = H.CRFLayer(2, 3, 2.0, 1.0, 1.0, 1.0, 1.0)
    guide = lambda image: image[:, :1]                                                   # noqa: E731
    with pytest.raises(ValueError, match="CRFLayer"):
        H.fit_crf(pred, [], guide, H.DenseCRF(2, 3, 2.0, 1.0, 1.0, 1.0, 1.0), 3, 0.1)
    with pytest.raises(ValueError, match="steps"):
        H.fit_crf(pred, [], guide, layer, 0, 0.1)
    with pytest.raises(ValueError, match="logit"):
        H.fit_crf(pred, [], guide, H.CRFLayer(2, 3, 2.0, 1.0, 1.0, 1.0, 1.0, output="prob"), 3, 0.1)
    with pytest.raises(ValueError, match="held 0 of the 2"):
        H.fit_crf(pred, [], guide, layer, 3, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.fit_crf(pred, [{"image": torch.zeros(2, 6, 4, 5), "index": ["a", "b"]}], guide, layer, 3, 0.1)


# ---- the ABI and the code objects ------------------------------------------------------------------------------------
ENTRIES = ("hpri_crf_train_workspace_bytes", "hpri_dense_crf_train_forward", "hpri_dense_crf_backward")


def test_the_header_declares_and_the_library_exports_the_entry_points():
    from hyperpri_amd import _lib
    decls = _lib.parse_header()
    src = open(os.path.join(ROOT, "include", "hyperpri_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in decls and re.search(r"\b" + name + r"\s*\(", src) and hasattr(lib, name) and hasattr(_lib.load_f16(), name), name
    assert len(decls["hpri_dense_crf_train_forward"][1]) == 23 and len(decls["hpri_dense_crf_backward"][1]) == 26
    assert "crf_grad.hip" in __import__("hyperpri_amd.build", fromlist=["SOURCES"]).SOURCES
    N, C, h, w, T = 2, 5, 37, 130, 4
    tiles = N * 3 * 5
    assert lib.hpri_crf_train_workspace_bytes(N, C, h, w, T) == 8 * T * tiles * (2 + C * C) + 4 * (T + 2) * N * C * h * w
    for bad in ((0, 2, 4, 4, 1), (1, 9, 4, 4, 1), (1, 2, 4, 4, 0), (1, 2, 4, 4, 17)):
        assert lib.hpri_crf_train_workspace_bytes(*bad) == 0, bad
    # bad arguments return before any launch
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    t = ctypes.cast((ctypes.c_float * 9)(*([1.0] * 9)), ctypes.c_void_p)
    big = 1 << 20
    fwd = [p, 0, p, 1, 1, 1, 2, 4, 4, 2, 2, t, t, 0.5, p, p, null, 0, 1, p, big, p, null]
    for pos, v in {0: null, 11: null, 15: null, 21: null, 14: null, 1: 2, 4: 4, 6: 9, 9: 0, 10: 17, 13: 0.0, 17: 2, 18: 2, 19: odd, 20: 8}.items():
        args = list(fwd)
        args[pos] = v
        assert lib.hpri_dense_crf_train_forward(*args) == -1, (pos, v)
        assert b"dense_crf_train_forward" in lib.hpri_last_error()
    bwd = [p, p, 0, p, 1, 1, 1, 2, 4, 4, 2, 2, t, t, 0.5, p, p, null, 0, p, big, p, p, p, null, null]
    for pos, v in {0: null, 1: null, 16: null, 19: null, 21: null, 15: null, 2: 2, 5: 4, 7: 9, 10: 9, 11: 0, 14: -1.0, 18: 2, 19: odd, 20: 8,
                   24: p}.items():                                                       # (24: grad_compat without compat)
        args = list(bwd)
        args[pos] = v
        assert lib.hpri_dense_crf_backward(*args) == -1, (pos, v)
        assert b"dense_crf_backward" in lib.hpri_last_error()
    assert lib.hpri_dense_crf_backward(*(bwd[:3] + [null, 0, 0] + bwd[6:])) == -1          # grad_w_a without a guide


def test_the_backward_kernels_hold_everything_in_registers():
    """tools/check_codeobj.py's report, as tests/test_crf_cpu.py reads it for the forward: all 28 instantiations are there, gated, with
    zero scratch and no spilled register, vector or scalar, and two workgroups of 512 lanes fit a CU's registers."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_codeobj as C
    rep = C.run()
    rows = {k["demangled"].split("(")[0].replace("void ", ""): k for k in rep["kernels"] if k["file"] == "crf_grad.hip"}
    want = [f"crf_back_kernel<{k}, {c}>" for k in range(4) for c in range(2, 9)]
    assert sorted(n for n in rows if n.startswith("crf_back_kernel")) == sorted(want)
    for name in want + ["crf_grad_start_kernel", "crf_grad_finish_kernel"]:
        k = rows[name]
        assert k["clean"] and k["scratch"] == 0 and k["vgpr_spill"] == 0 and k.get("sgpr_spill", 0) == 0, k
    for name in want:
        k = rows[name]
        assert k["hot"] and k["vgprs"] + k.get("agprs", 0) <= 128 and k["max_flat_wg"] == 512, k


# ---- end to end on the reference -------------------------------------------------------------------------------------
def test_fitting_the_reference_on_the_scene_lowers_the_bce_and_raises_the_dice():
    """What tests/test_gpu_crf_grad.py asserts of ``fit_crf``, on the fp64 reference: Adam on the BCE from w_a = w_s = 0."""
    from hyperpri_amd import crf
    ace, logit, guide, masks = K.scene()
    y = (masks != 0).astype(np.float64)
    kw = {k: v for k, v in K.SCENE.items() if not k.startswith("w_")}

    def bce(z):
        return float((np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))).mean())
    w = np.zeros(2)
    m, v = np.zeros(2), np.zeros(2)
    before = bce(crf.crf_reference(logit, guide, w_appearance=0.0, w_smooth=0.0, **kw)["logit"])
    assert before == bce(logit.astype(np.float64))
    for step in range(1, FIT["steps"] + 1):
        wa, ws = (float(np.float32(max(x, 0.0))) for x in w)                             # (crf_reference takes non-negative weights)
        z = crf.crf_reference(logit, guide, w_appearance=wa, w_smooth=ws, **kw)["logit"]
        g = ((1.0 / (1.0 + np.exp(-z)) - y) / z.size).astype(np.float32)
        grad = crf.crf_backward_reference(logit, guide, g, w_appearance=wa, w_smooth=ws, **kw)
        gw = np.array([grad["w_appearance"], grad["w_smooth"]])
        m, v = 0.9 * m + 0.1 * gw, 0.999 * v + 0.001 * gw * gw
        w = w - FIT["lr"] * (m / (1 - 0.9 ** step)) / (np.sqrt(v / (1 - 0.999 ** step)) + 1e-8)
    wa, ws = (float(np.float32(max(x, 0.0))) for x in w)
    fitted = crf.crf_reference(logit, guide, w_appearance=wa, w_smooth=ws, **kw)
    after, raw, dice = bce(fitted["logit"]), G.best_dice(ace, masks), G.best_dice(fitted["prob"], masks)
    print("BCE", before, "->", after, "best Dice", raw, "->", dice, "w", wa, ws)
    assert after <= 0.8 * before and dice >= raw + 0.03, (before, after, raw, dice)        # with room: the device test asserts < and >
