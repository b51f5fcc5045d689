"""CPU-side checks of the device sort, the Lovasz hinge and the ranking metrics (no GPU): the numpy restatement of the loss against
the published formulation under torch autograd in fp64, the tie rule, the pure host functions of csrc/sort.hip and the argument
errors of its launchers (nothing is launched), and the placement error of the module."""
import ctypes

import numpy as np
import pytest
import torch

import _sort_cases as C


def _logits(rng, shape):
    """Distinct multiples of 1/1024 below 8 in magnitude: e = 1 - x s is exact in fp32, so the fp32 errors of the reference and the
    fp64 errors of the torch side are the same numbers, and no two are equal."""
    n = int(np.prod(shape))
    return ((rng.permutation(8000)[:n] - 4000) / 1024.0).reshape(shape)


def _cases():
    rng = np.random.RandomState(3)
    out = {}
    out["tie_free"] = (_logits(rng, (3, 1, 7, 9)), (rng.rand(3, 1, 7, 9) < 0.4).astype(np.float64), None)
    y = np.zeros((3, 1, 4, 5))
    y[0] = 1.0                                              # image 0 all positive, image 1 all negative, image 2 mixed
    y[2, 0, 1] = 1.0
    out["degenerate_groups"] = (_logits(rng, (3, 1, 4, 5)), y, None)
    out["all_negative"] = (_logits(rng, (2, 1, 3, 3)), np.zeros((2, 1, 3, 3)), None)
    out["all_positive"] = (_logits(rng, (2, 1, 3, 3)), np.ones((2, 1, 3, 3)), None)
    out["single_pixel"] = (_logits(rng, (4, 1, 1, 1)), np.array([1.0, 0.0, 1.0, 0.0]).reshape(4, 1, 1, 1), None)
    y = (rng.rand(3, 1, 6, 5) < 0.5).astype(np.float64)
    y[0] = 255.0                                            # a whole group hidden
    y[1, 0, :3] = 255.0                                     # part of one
    out["ignore"] = (_logits(rng, (3, 1, 6, 5)), y, 255)
    return out


CASES = _cases()


@pytest.mark.parametrize("per_image", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_matches_the_published_formulation_under_autograd(name, per_image):
    """Loss and gradient within 1e-12 of torch.sort, cumulative sums and dot(relu(e_sorted), grad) in fp64."""
    import hyperpri_amd as H
    x, y, ignore = CASES[name]
    loss, grad = H.lovasz_hinge_reference(x, y, per_image, ignore)
    tl, tg = C.lovasz_torch(x, y, per_image, ignore)
    assert grad.shape == x.shape and grad.dtype == np.float64
    assert abs(loss - tl) <= 1e-12 and np.abs(grad - tg).max() <= 1e-12
    assert np.abs(tg).max() > 0


def test_tie_rule_all_logits_zero():
    """All logits 0: every error is 1, so the order is the index order and the gradient is decided by it alone."""
    import hyperpri_amd as H
    y = np.array([[0, 1, 1, 0, 1, 0, 0, 1]], dtype=np.float64)
    x = np.zeros_like(y)
    loss, grad = H.lovasz_hinge_reference(x, y, True, None)
    G1 = 4
    P = np.cumsum(y[0])
    r = np.arange(8)
    J = 1.0 - (G1 - P) / (G1 + (r + 1 - P))
    w = np.diff(J, prepend=0.0)
    assert np.abs(grad[0] - np.where(y[0] > 0, -w, w)).max() <= 1e-15
    assert abs(loss - w.sum()) <= 1e-15 and abs(loss - 1.0) <= 1e-15        # the weights telescope to J_{n-1} = 1
    tl, tg = C.lovasz_torch(x, y, True, None)
    assert abs(loss - tl) <= 1e-12 and np.abs(grad - tg).max() <= 1e-12


def test_size_functions_are_pure_host_functions():
    from hyperpri_amd import _lib
    lib = _lib.load()
    T = lib.hpri_sort_tile()
    assert T > 0 and T % 64 == 0
    prev = 0
    for L in (1, 2, T - 1, T, T + 1, 3 * T + 5, 588544, 8_800_000):
        b = lib.hpri_sort_workspace_bytes(1, L)
        assert b > 0 and b >= prev and b >= 16 * L
        prev = b
    assert lib.hpri_sort_workspace_bytes(3, T + 3) > lib.hpri_sort_workspace_bytes(1, T + 3)
    assert lib.hpri_sort_workspace_bytes(0, 5) == 0 and lib.hpri_sort_workspace_bytes(1, 0) == 0
    assert lib.hpri_sort_workspace_bytes(2, 2 ** 30) == 0
    assert lib.hpri_lovasz_hinge_workspace_bytes(2, 588544, 1) > lib.hpri_sort_workspace_bytes(2, 588544)
    assert lib.hpri_lovasz_hinge_workspace_bytes(2, 588544, 0) > lib.hpri_sort_workspace_bytes(1, 2 * 588544)
    assert lib.hpri_lovasz_hinge_workspace_bytes(2, 2 ** 30, 0) == 0 and lib.hpri_lovasz_hinge_workspace_bytes(0, 4, 1) == 0
    assert lib.hpri_ranking_workspace_bytes(8_800_000) > lib.hpri_sort_workspace_bytes(1, 8_800_000)
    assert lib.hpri_ranking_workspace_bytes(0) == 0 and lib.hpri_ranking_workspace_bytes(2 ** 31) == 0


def test_bad_arguments_are_rejected_without_launch():
    from hyperpri_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)            # a 16-byte aligned host address: never dereferenced
    # the sort
    assert lib.hpri_sort_keys_f32(null, 1, 4, 1, p, null, p, 1 << 20, null) == -1 and b"null" in lib.hpri_last_error()
    assert lib.hpri_sort_keys_f32(p, 1, 4, 1, null, null, p, 1 << 20, null) == -1
    assert lib.hpri_sort_keys_f32(p, 1, 4, 1, p, null, null, 1 << 20, null) == -1
    assert lib.hpri_sort_keys_f32(p, 1, 0, 1, p, null, p, 1 << 20, null) == -1 and len(lib.hpri_last_error()) > 0
    assert lib.hpri_sort_keys_f32(p, 1, -3, 1, p, null, p, 1 << 20, null) == -1
    assert lib.hpri_sort_keys_f32(p, 0, 4, 1, p, null, p, 1 << 20, null) == -1
    assert lib.hpri_sort_keys_f32(p, 2, 2 ** 30, 1, p, null, p, 1 << 20, null) == -1 and b"2^31" in lib.hpri_last_error()
    assert lib.hpri_sort_keys_f32(p, 1, 4, 1, p, null, p, lib.hpri_sort_workspace_bytes(1, 4) - 1, null) == -3
    assert b"workspace" in lib.hpri_last_error()
    # the loss
    assert lib.hpri_lovasz_hinge_fwd(null, p, 1, 4, 1, 0, 0, p, p, p, 1 << 20, null) == -1 and b"null" in lib.hpri_last_error()
    assert lib.hpri_lovasz_hinge_fwd(p, p, 1, 4, 1, 0, 0, p, null, p, 1 << 20, null) == -1
    assert lib.hpri_lovasz_hinge_fwd(p, p, 1, 0, 1, 0, 0, p, p, p, 1 << 20, null) == -1
    assert lib.hpri_lovasz_hinge_fwd(p, p, 0, 4, 1, 0, 0, p, p, p, 1 << 20, null) == -1
    assert lib.hpri_lovasz_hinge_fwd(p, p, 2, 2 ** 30, 0, 0, 0, p, p, p, 1 << 20, null) == -1 and b"2^31" in lib.hpri_last_error()
    assert lib.hpri_lovasz_hinge_fwd(p, p, 1, 4, 1, 0, 0, p, p, p, lib.hpri_lovasz_hinge_workspace_bytes(1, 4, 1) - 1, null) == -3
    assert lib.hpri_lovasz_hinge_bwd(null, 4, null, p, null) == -1 and lib.hpri_lovasz_hinge_bwd(p, 0, null, p, null) == -1
    assert lib.hpri_lovasz_hinge_bwd(p, 2 ** 31, null, p, null) == -1
    # the ranking sums
    assert lib.hpri_ranking_sums(null, p, 0, 4, p, p, 1 << 20, null) == -1 and b"null" in lib.hpri_last_error()
    assert lib.hpri_ranking_sums(p, p, 0, 0, p, p, 1 << 20, null) == -1
    assert lib.hpri_ranking_sums(p, p, 0, 2 ** 31, p, p, 1 << 20, null) == -1
    assert lib.hpri_ranking_sums(p, p, 2, 4, p, p, 1 << 20, null) == -1
    assert lib.hpri_ranking_sums(p, p, 0, 4, p, p, lib.hpri_ranking_workspace_bytes(4) - 1, null) == -3


def test_cpu_tensors_fail_loudly():
    import hyperpri_amd as H
    x, y = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.LovaszHingeLoss()(x, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.ranking_metrics(x, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.sort_scores(x)
    with pytest.raises(ValueError):
        H.LovaszHingeLoss(ignore_index=0.5)
    from hyperpri_amd import losses, metrics, trainer
    assert trainer.LovaszHingeLoss is losses.LovaszHingeLoss is H.LovaszHingeLoss
    assert trainer.ranking_metrics is metrics.ranking_metrics and trainer.sort_scores is metrics.sort_scores


def test_ranking_reference_on_small_known_inputs():
    import hyperpri_amd as H
    r = H.ranking_reference([0.9, 0.8, 0.7, 0.6], [1, 0, 1, 0])
    assert r["roc_auc"] == 0.75 and r["avg_prec"] == pytest.approx(0.5 * (1.0 + 2.0 / 3.0), abs=1e-15)
    r = H.ranking_reference([0.5] * 6, [1, 0, 1, 0, 0, 0])
    assert r["roc_auc"] == 0.5 and r["avg_prec"] == pytest.approx(2.0 / 6.0, abs=1e-15)
    assert np.isnan(H.ranking_reference([0.1, 0.2], [0, 0])["roc_auc"]) and np.isnan(H.ranking_reference([0.1, 0.2], [0, 0])["avg_prec"])
    assert np.isnan(H.ranking_reference([0.1, 0.2], [1, 1])["roc_auc"]) and H.ranking_reference([0.1, 0.2], [1, 1])["avg_prec"] == 1.0
