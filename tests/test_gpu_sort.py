"""The device sort (csrc/sort.hip) and its two consumers on the GPU.

* sort_scores: the permutation is BIT-EQUAL to torch.sort(stable=True) on the CPU copy, for one group of each length of
  _sort_cases.lengths(T) (T = hpri_sort_tile()) and for 3 groups of the odd length T + 3, both directions, eight key sets each chosen
  to break one thing; the sorted keys come back with their original bits.
* LovaszHingeLoss against lovasz_hinge_reference (numpy fp64; tests/test_sort_cpu.py holds it against torch autograd).  Bounds, with
  u = 2^-24: the gradient is exactly 0 where e <= 0 and within 2 u relative elsewhere -- the coefficient -s w / groups is formed in
  fp64 and rounded once, the backward multiplies it by the upstream scalar and rounds once; the loss is within (u + n 2^-52)
  relative -- fp64 sums of the same non-negative terms in another order (n terms), rounded once to fp32.  The inputs make e exact
  in fp32 (multiples of 1/1024), so the reference and the kernels order the same numbers.
* ranking_metrics: roc_auc bit-equal to the integer restatement ranking_reference; avg_prec within 4 runs 2^-53 relative of the
  existing average_precision (both are fp64 sums of the same `runs` non-negative terms, each term a few roundings).
"""
import numpy as np
import pytest
import torch

import _sort_cases as C
from conftest import record_margin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _tile():
    from hyperpri_amd import _lib
    return int(_lib.load().hpri_sort_tile())


# -- the sort ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.KEY_SETS)
def test_permutation_is_bit_equal_to_torch_stable_sort(name):
    import hyperpri_amd as H
    T = _tile()
    shapes = [(1, L) for L in C.lengths(T)] + [(3, T + 3)]
    for G, L in shapes:
        k = C.keys(name, G * L, seed=G).reshape(G, L)
        if name in ("sorted", "reversed") and G > 1:
            k = np.stack([C.keys(name, L, seed=g) for g in range(G)])
        dk = torch.from_numpy(k).to(DEV)
        for descending in (True, False):
            perm, out = H.sort_scores(dk, descending=descending, groups=G)
            want, _ = C.torch_order(k, descending)
            got = perm.cpu().numpy()
            assert perm.dtype == torch.int32 and got.shape == (G, L)
            bad = np.nonzero(got != want)
            assert bad[0].size == 0, (name, G, L, descending, bad[0][:4], bad[1][:4], got[bad][:4], want[bad][:4])
            gathered = np.take_along_axis(k, want.astype(np.int64), axis=1)
            assert np.array_equal(out.cpu().numpy().view(np.uint32), gathered.view(np.uint32)), (name, G, L, descending)


def test_sort_is_reproducible_and_flat_input_is_one_group():
    import hyperpri_amd as H
    T = _tile()
    k = torch.from_numpy(C.keys("three", 3 * T + 5, seed=9)).to(DEV)
    a, av = H.sort_scores(k)
    b, bv = H.sort_scores(k)
    assert a.shape == (1, 3 * T + 5) and torch.equal(a, b) and torch.equal(av, bv)
    with pytest.raises(ValueError):
        H.sort_scores(k, groups=2)


def test_groups_skip_their_own_passes():
    """Three groups whose digits differ in which passes are the identity (all keys equal: all four; one low byte: three; distinct
    values: none): every group's workgroups decide for themselves, and find their data in the buffer their last pass wrote."""
    import hyperpri_amd as H
    L = _tile() + 3
    k = np.stack([C.keys("equal", L), C.keys("low_byte", L, seed=1), C.keys("distinct", L, seed=2)])
    for descending in (True, False):
        perm, out = H.sort_scores(torch.from_numpy(k).to(DEV), descending=descending, groups=3)
        want, _ = C.torch_order(k, descending)
        assert np.array_equal(perm.cpu().numpy(), want), descending
        assert np.array_equal(out.cpu().numpy().view(np.uint32), np.take_along_axis(k, want.astype(np.int64), axis=1).view(np.uint32))


# -- more tiles than one round of the scans takes -------------------------------------------------------------------------------------
def test_more_tiles_than_the_scan_takes_in_one_round():
    """L = 256 T + 1: sort_scan_kernel walks the tile counts of a digit 256 at a time, and the consumers' sums over the earlier tiles
    stride by 256 -- at 257 tiles each of those loops takes its second round.  The same checks as above at that one size."""
    import hyperpri_amd as H
    T = _tile()
    n = 256 * T + 1
    for name in ("distinct", "three"):
        k = C.keys(name, n, seed=2)
        perm, out = H.sort_scores(torch.from_numpy(k).to(DEV))
        want, _ = C.torch_order(k[None], True)
        assert np.array_equal(perm.cpu().numpy(), want), name
        assert np.array_equal(out.cpu().numpy().view(np.uint32), k[want.astype(np.int64)].view(np.uint32)), name
    x, y = C.exact_case((1, 1, 1, n), 41)
    _check(f"exact/1x1x1x{n}", x, y, True)
    rng = np.random.RandomState(6)
    s = (rng.randint(0, 16, n) / np.float32(16)).astype(np.float32)
    t = rng.rand(n) < 0.3
    sd, td = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    got, ref, ap = H.ranking_metrics(sd, td), H.ranking_reference(s, t), H.average_precision(sd, td)
    assert got["roc_auc"] == ref["roc_auc"]
    tol = 4 * 16 * 2.0 ** -53 * abs(ap)
    record_margin(f"ranking/avg_prec/levels16/{n}", abs(got["avg_prec"] - ap), tol)
    assert abs(got["avg_prec"] - ap) <= tol and abs(got["avg_prec"] - ref["avg_prec"]) <= tol


# -- the Lovasz hinge ------------------------------------------------------------------------------------------------------------------
def _shapes():
    T = _tile()
    hw = 2 * T + 7
    h = next(d for d in range(int(hw ** 0.5), 0, -1) if hw % d == 0)
    return [(1, 1, 1, 1), (1, 1, 5, 3), (3, 1, 37, 53), (2, 1, h, hw // h)]


def _run(x, y, per_image, ignore_index=None, scale=None):
    import hyperpri_amd as H
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).requires_grad_(True)
    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(DEV)
    loss = H.LovaszHingeLoss(per_image=per_image, ignore_index=ignore_index)(xd, yd)
    (loss if scale is None else loss * scale).backward()
    return loss.detach().cpu().numpy(), xd.grad.detach().cpu().numpy()


def _check(tag, x, y, per_image, ignore_index=None):
    import hyperpri_amd as H
    loss, grad = _run(x, y, per_image, ignore_index)
    ref_loss, ref_grad = H.lovasz_hinge_reference(x, y, per_image, ignore_index)
    x32, y32 = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    e = np.float32(1) - x32 * np.where(y32 >= 0.5, np.float32(1), np.float32(-1)).astype(np.float32)
    off = ~(e > 0) if ignore_index is None else (~(e > 0) | (y32 == ignore_index))
    assert np.all(grad[off] == 0) and np.all(ref_grad[off] == 0), tag
    zero, nz = ~off & (ref_grad == 0), ~off & (ref_grad != 0)
    assert np.all(grad[zero] == 0), tag                     # (weights that are exactly 0: G1 == 0 beyond rank 0)
    gerr = float((np.abs(grad[nz] - ref_grad[nz]) / np.abs(ref_grad[nz])).max()) if nz.any() else 0.0
    ltol = (U + x32.size * 2.0 ** -52) * abs(ref_loss)
    lerr = abs(float(loss) - ref_loss)
    print(f"lovasz {tag} per_image {per_image}: loss {float(loss)!r} (fp64 {ref_loss!r}) error {lerr:.3e} of {ltol:.3e}; "
          f"gradient {gerr / U:.3f} u of 2 u")
    record_margin(f"lovasz/loss/{tag}/img{int(per_image)}", lerr, max(ltol, 1e-300))
    record_margin(f"lovasz/grad/{tag}/img{int(per_image)}", gerr, 2 * U)
    assert lerr <= ltol, tag
    assert gerr <= 2 * U, tag
    return loss, grad


@pytest.mark.parametrize("per_image", [True, False])
def test_exact_inputs_match_the_reference(per_image):
    for i, shape in enumerate(_shapes()):
        x, y = C.exact_case(shape, 20 + i)
        loss, grad = _check("exact/" + "x".join(map(str, shape)), x, y, per_image)
        assert np.isfinite(loss) and (np.prod(shape) == 1 or np.abs(grad).max() > 0)


@pytest.mark.parametrize("per_image", [True, False])
def test_ties_follow_the_stable_order(per_image):
    """All logits 0 (every error is 1: the index order decides everything), and a plateau case of 3 distinct logit values."""
    rng = np.random.RandomState(5)
    for i, shape in enumerate(_shapes()):
        y = (rng.rand(*shape) < 0.35).astype(np.float32)
        _check("zeros/" + "x".join(map(str, shape)), np.zeros(shape, dtype=np.float32), y, per_image)
        x = np.array([-0.5, 0.25, 0.75], dtype=np.float32)[rng.randint(0, 3, size=shape)]
        _check("plateau/" + "x".join(map(str, shape)), x, y, per_image)


@pytest.mark.parametrize("per_image", [True, False])
def test_degenerate_groups_and_ignore_index(per_image):
    T = _tile()
    shape = (3, 1, 7, (T + 9) // 7 + 1)
    x, y = C.exact_case(shape, 31)
    _check("no_positive", x, np.zeros(shape, dtype=np.float32), per_image)
    # (x was built for y: keep its e pattern but call every pixel positive -- e = 1 - x stays exact)
    _check("all_positive", x, np.ones(shape, dtype=np.float32), per_image)
    y1 = y.copy()
    y1[1] = 0                                               # one image of the batch empty while the others are not
    _check("one_empty", x, y1, per_image)
    y2 = y.copy()
    y2[0] = 255                                             # a whole group hidden
    y2[2, 0, :3] = 255                                      # part of one
    loss, grad = _check("ignore", x, y2, per_image, ignore_index=255)
    assert np.all(grad[y2 == 255] == 0) and np.abs(grad[1]).max() > 0
    y3 = np.full(shape, 255, dtype=np.float32)              # nothing left at all: the loss is 0 and so is the gradient
    loss, grad = _run(x, y3, per_image, 255)
    assert float(loss) == 0.0 and np.all(grad == 0)


def test_two_runs_give_identical_bytes_and_the_upstream_gradient_scales_exactly():
    shape = _shapes()[-1]
    rng = np.random.RandomState(8)
    x = rng.randn(*shape).astype(np.float32)
    y = (rng.rand(*shape) < 0.3).astype(np.float32)
    l1, g1 = _run(x, y, True)
    l2, g2 = _run(x, y, True)
    assert l1.tobytes() == l2.tobytes() and g1.tobytes() == g2.tobytes()
    l3, g3 = _run(x, y, True, scale=3.0)
    assert l3.tobytes() == l1.tobytes() and g3.tobytes() == (g1 * np.float32(3)).tobytes()
    assert np.abs(g1).max() > 0


def test_segmentation_model_takes_one_training_step_under_the_lovasz_hinge():
    """SegmentationModel(net, criterion=LovaszHingeLoss()) on the tiny UNet-3 shape (2, 3, 36, 50): the step's loss is the criterion
    called on the model's own logits, bit for bit, and every parameter receives a finite gradient."""
    import hyperpri_amd as H
    torch.manual_seed(4)
    net = H.UNet(3, 1, bilinear=False).to(DEV).train()
    rng = np.random.RandomState(4)
    image = torch.from_numpy(rng.rand(2, 3, 36, 50).astype(np.float32)).to(DEV)
    mask = torch.from_numpy((rng.rand(2, 1, 36, 50) < 0.3).astype(np.float32)).to(DEV)
    crit = H.LovaszHingeLoss()
    model = H.SegmentationModel(net, criterion=crit)
    logits, loss = model._step("tr", {"image": image, "mask": mask}, model.threshold)
    assert type(loss.grad_fn).__name__.startswith("_LovaszHingeFn")
    loss.backward()
    again = crit(logits.detach(), mask)
    assert loss.detach().cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    ref, _ = H.lovasz_hinge_reference(logits.detach().cpu().numpy(), mask.cpu().numpy(), True, None)
    assert abs(float(loss.detach()) - ref) <= (U + logits.numel() * 2.0 ** -52) * abs(ref)
    grads = [p.grad for p in net.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    step = H.SegmentationModel(net, criterion=crit).training_step({"image": image, "mask": mask})
    assert step.requires_grad and float(step.detach()) == pytest.approx(float(loss.detach()), rel=1e-4)


# -- ranking ---------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


@pytest.mark.parametrize("kind", ["tie_free", "levels16", "all_equal", "no_positive", "no_negative"])
def test_ranking_metrics(kind):
    import hyperpri_amd as H
    T = _tile()
    for n in (1, T + 1, 3 * T + 5):
        rng = np.random.RandomState(n % 1000 + len(kind))
        if kind == "tie_free":
            s = (rng.permutation(n).astype(np.float32) + np.float32(0.5)) / np.float32(n)
        elif kind == "all_equal":
            s = np.full(n, 0.25, dtype=np.float32)
        else:
            s = (rng.randint(0, 16, n) / np.float32(16)).astype(np.float32)
        t = (rng.rand(n) < 0.3)
        if kind == "no_positive":
            t[:] = False
        elif kind == "no_negative":
            t[:] = True
        elif n > 1:
            t[0], t[1] = True, False
        sd = torch.from_numpy(s).to(DEV)
        ref = H.ranking_reference(s, t)
        for td in (torch.from_numpy(t).to(DEV), torch.from_numpy(t.astype(np.float32)).to(DEV), torch.from_numpy(t.astype(np.int64)).to(DEV)):
            got = H.ranking_metrics(sd, td)
            assert _same(got["roc_auc"], ref["roc_auc"]), (kind, n, got, ref)            # bit-equal: an exact integer over an integer
            ap = H.average_precision(sd, td)
            runs = int(np.unique(s).size)
            if np.isnan(ap):
                assert np.isnan(got["avg_prec"]) and not t.any()
            else:
                tol = 4 * runs * 2.0 ** -53 * abs(ap)
                err = abs(got["avg_prec"] - ap)
                record_margin(f"ranking/avg_prec/{kind}/{n}", err, tol)
                assert err <= tol, (kind, n, got["avg_prec"], ap, err, tol)
                assert abs(got["avg_prec"] - ref["avg_prec"]) <= tol
        if kind == "all_equal" and n > 1:
            assert got["roc_auc"] == 0.5
        if kind in ("no_positive", "no_negative") or n == 1:
            assert np.isnan(got["roc_auc"])
        print(f"ranking {kind} n {n}: {got}")
