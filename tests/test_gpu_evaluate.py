"""Evaluation on the device (hyperpri_amd/evaluate.py, csrc/segmap.hip) against host restatements of the reference's
``eval_color_segmaps`` / ``validate_net`` / ``test_net`` (PLTrainer.py:219-267, 533-609, 631-661).

Tolerances.  Class maps, PR-curve counts, the threshold pick and the confusion counts are integers or picks among them: exact.
Every probability the tests decide on is kept at least 1e-5 away from every threshold it meets (and any two probabilities at
least 16 ulp apart), so the one or two ulp between the device's and the host's fp32 sigmoid cannot change a decision, an order
or a tie.  The picture is compared within ONE level per channel, no pixel exempt: a few ulp of powf and one fused multiply-add
can move ``out * 255 + 0.5`` across a rounding boundary, and no more.  BCE: 1e-6 relative against fp64 (the bound of
test_bce_with_logits_matches_torch_cpu); AP: 1e-9 (the bound of test_average_precision_matches_sklearn).  Needs a real MI355X."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch
from torch import nn

from oracle import hyperpri_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = torch.tensor([[0, 0, 0], [202, 0, 32], [5, 133, 176], [155, 191, 133]], dtype=torch.uint8)


def _u(seed, shape):
    return torch.from_numpy(O._u(seed, int(np.prod(shape))).reshape(shape).copy())


def _restate(image, x, m, thr, bands, gamma, alpha, palette):
    """eval_color_segmaps' arithmetic in fp32 on the host, with the library's clamp / NaN rule: (rgb (N,h,w,3), classes (N,h,w))."""
    v = torch.nan_to_num(image[:, list(bands)].float(), nan=0.0).clamp(0, 1)
    base = v if gamma == 1 else v ** (1 / gamma)
    s = torch.sigmoid(x.float()) > thr
    g = m.to(torch.int32) != 0
    cls = s.to(torch.uint8) + 2 * g.to(torch.uint8)
    table = torch.tensor([[0.0, 0.0, 0.0], *palette], dtype=torch.float32)
    a = torch.tensor(alpha, dtype=torch.float32)
    out = a * table[cls.long()] + (1 - a) * base.permute(0, 2, 3, 1)
    return (out * 255 + 0.5).to(torch.uint8), cls


def _logits_clear_of(seed, shape, thr):
    """Logits in (-3, 3) whose fp32 sigmoid stays 1e-5 away from ``thr``: any that come closer are moved."""
    x = _u(seed, shape) * 6 - 3
    near = (torch.sigmoid(x) - thr).abs() < 1e-5
    x[near] += 0.01
    assert not bool(((torch.sigmoid(x) - thr).abs() < 1e-5).any())
    return x


def _check_overlay(image_dev, image_host, x, m, thr, want_bands, want_gamma, alpha=0.6, **kw):
    """``kw`` goes to color_segmaps; ``want_bands`` / ``want_gamma`` are what the restatement uses (the defaults, when kw names none)."""
    import hyperpri_amd as H
    rgb, cls = H.color_segmaps(image_dev, x.to(DEV), m.to(DEV), thr, alpha=alpha, return_classes=True, **kw)
    assert rgb.dtype == torch.uint8 and cls.dtype == torch.uint8 and rgb.is_cuda and cls.is_cuda
    want_rgb, want_cls = _restate(image_host, x, m, thr, want_bands, want_gamma, alpha, H.evaluate.PALETTE)
    assert tuple(rgb.shape) == tuple(want_rgb.shape) and tuple(cls.shape) == tuple(want_cls.shape)
    assert torch.equal(cls.cpu(), want_cls)
    diff = int((rgb.cpu().int() - want_rgb.int()).abs().max())
    print(f"overlay {tuple(image_host.shape)} bands {want_bands} gamma {want_gamma} alpha {alpha}: max level difference {diff}")
    assert diff <= 1
    assert torch.equal(H.color_segmaps(image_dev, x.to(DEV), m.to(DEV), thr, alpha=alpha, **kw), rgb)     # without the class map
    return rgb.cpu(), cls.cpu()


def test_overlay_channels_last_cube():
    """A 238-band cube in the cache's layout (cs = 240, zero pad channels, viewed (N,1,C,h,w)); w = 13: three quads and a tail;
    9 * 13 is odd, so quads of the second image start at every alignment."""
    N, C, cs, h, w = 2, 238, 240, 9, 13
    bands, thr = (125, 49, 0), 0.4
    buf = torch.zeros(N, h, w, cs)
    buf[..., :C] = _u(71, (N, h, w, C))
    for (n, y, x0), vals in {(0, 0, 0): (-0.3, 1.7, float("nan")), (0, 4, 12): (float("nan"), -0.3, 1.7), (1, 8, 5): (1.7, float("nan"), -0.3),
                             (1, 3, 12): (float("nan"),) * 3, (1, 0, 3): (float("inf"), -float("inf"), 1.0)}.items():
        for b, v in zip(bands, vals):
            buf[n, y, x0, b] = v
    dev = buf.to(DEV)
    image = dev[:, :, :, :C].permute(0, 3, 1, 2).unsqueeze(1)              # as CubeCache._gather hands it out
    image._hpri_zero_padded = True
    assert image.stride()[2:] == (1, w * cs, cs)
    x = _logits_clear_of(72, (N, h, w), thr)
    m = (_u(73, (N, h, w)) > 0.5).float()
    _, cls = _check_overlay(image, buf[..., :C].permute(0, 3, 1, 2), x, m, thr, bands, 2.2)
    assert sorted(cls.unique().tolist()) == [0, 1, 2, 3]
    # the defaults of a cube with more than three bands are these bands and this gamma
    import hyperpri_amd as H
    assert torch.equal(H.color_segmaps(image, x.to(DEV), m.to(DEV), thr), H.color_segmaps(image, x.to(DEV), m.to(DEV), thr, bands=bands, gamma=2.2))


@pytest.mark.parametrize("shape,bands,gamma,kw", [((1, 3, 8, 12), (0, 1, 2), 1.0, {}),
                                                   ((2, 5, 7, 10), (4, 0, 2), 2.2, {"bands": (4, 0, 2)})])
def test_overlay_contiguous_tensors(shape, bands, gamma, kw):
    import hyperpri_amd as H
    N, C, h, w = shape
    thr = 0.55
    img = _u(81, shape) * 1.2 - 0.1                                        # some values outside [0, 1]
    img[0, bands[1], 1, 2] = float("nan")
    x = _logits_clear_of(82, (N, 1, h, w), thr)                            # (N,1,h,w) logits and masks, as the networks return them
    m = (_u(83, (N, 1, h, w)) > 0.5).float()
    dev = img.to(DEV)
    _, cls = _check_overlay(dev, img, x[:, 0], m[:, 0], thr, bands, gamma, **kw)
    assert sorted(cls.unique().tolist()) == [0, 1, 2, 3]
    # alpha = 0: the bare pseudo-RGB picture; alpha = 1: the bare class colours on black -- the latter exactly
    bare, _ = _check_overlay(dev, img, x[:, 0], m[:, 0], thr, bands, gamma, alpha=0.0, **kw)
    v = torch.nan_to_num(img[:, list(bands)], nan=0.0).clamp(0, 1)
    v = v if gamma == 1 else v ** (1 / gamma)
    assert int((bare.int() - (v.permute(0, 2, 3, 1) * 255 + 0.5).to(torch.uint8).int()).abs().max()) <= 1
    flat, _ = _check_overlay(dev, img, x[:, 0], m[:, 0], thr, bands, gamma, alpha=1.0, **kw)
    assert torch.equal(flat, LEVELS[cls.long()])
    # an integer mask and a 5-D (N,1,C,h,w) view of the same tensor give the same picture
    assert torch.equal(H.color_segmaps(dev.unsqueeze(1), x.to(DEV), m.to(DEV).to(torch.int32), thr, alpha=1.0, **kw).cpu(), flat)


class _Replay(nn.Module):
    """A "network" that returns precomputed logits, one tensor per call."""

    def __init__(self, outs):
        super().__init__()
        self.outs, self.calls = outs, 0

    def forward(self, x):
        self.calls += 1
        return self.outs[self.calls - 1]


def _separated_probabilities(n):
    """Probabilities drawn as test_pr_curve_histogram_exact_and_best_threshold draws them, then moved until the fp32
    ``sigmoid(logit(p))`` of every one is at least 1e-5 (2e-5 asked for) away from every k/499 and every j/100 and at least 16 ulp
    (a relative 2e-6) away from every other one.  Returns (logits, host probabilities)."""
    p = (_u(51, (n,)) ** 2).double()
    p[:8] = torch.tensor([0.0, 1.0, 0.5, 0.25, 1.0 / 499, 498.0 / 499, 0.1, 0.998], dtype=torch.float64)
    p = 1e-4 + p * (1 - 2e-4)                                                   # off 0 and 1, where logit() is infinite
    for _ in range(20):
        x = torch.logit(p).float()
        ph = torch.sigmoid(x).double()
        bad = torch.zeros(n, dtype=torch.bool)
        for grid in (499, 100):
            bad |= (ph - torch.round(ph * grid) / grid).abs() < 2e-5
        order = torch.argsort(ph)
        close = (ph[order][1:] - ph[order][:-1]) < 2e-6 * ph[order][1:]
        bad[order[1:][close]] = True
        if not bool(bad.any()):
            return x, ph.float()
        p[bad] += torch.where(p[bad] < 0.5, 1.7e-4, -1.7e-4)
    raise AssertionError("the probabilities did not separate")


def test_validate_and_test_net_reproduce_the_host_exactly():
    import hyperpri_amd as H
    n_img, h, w = 11, 16, 24
    n = n_img * h * w
    x, ph = _separated_probabilities(n)
    t = (_u(52, (n,)) < ph).float()
    xs, ts = x.view(n_img, 1, h, w), t.view(n_img, 1, h, w)
    cuts = [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10), (10, 11)]                # five batches of 2 and one of 1
    names = [f"img{i:02d}" for i in range(n_img)]
    net = _Replay([xs[a:b].to(DEV) for a, b in cuts])
    dummy = torch.zeros(2, 3, h, w, device=DEV)
    pred = H.predict_split(net, ({"image": dummy[:b - a], "mask": ts[a:b].to(DEV), "index": names[a:b]} for a, b in cuts))
    assert net.calls == 6 and len(pred) == n_img and pred.names == names
    assert pred.offsets == [i * h * w for i in range(n_img + 1)] and pred.sizes == [(h, w)] * n_img
    assert torch.equal(pred.logits.cpu(), x) and torch.equal(pred.masks.cpu(), t)
    assert torch.equal(pred.image(10)[0].cpu(), xs[10, 0]) and torch.equal(pred.image(3)[1].cpu(), ts[3, 0])

    val = H.validate_net(pred)
    oprec, orec, oth, otp, ofp, ofn = O.pr_curve_binned(ph, t, 500)
    cc = val["curve_counts"]
    assert torch.equal(cc["tp"], otp) and torch.equal(cc["fp"], ofp) and torch.equal(cc["fn"], ofn)
    best = O.best_dice_threshold(oprec, orec, oth)                              # picked on the unpatched curve
    assert (val["best_threshold"], val["best_precision"], val["best_recall"]) == best
    assert val["dice"] == 2 * best[1] * best[2] / (best[1] + best[2])
    patched = oprec.clone()
    assert patched[-2] < 1e-6                                                   # no probability reaches 1: the reference's patch applies
    patched[-2] = (1 + patched[-3]) / 2
    assert torch.equal(val["precision"], patched) and torch.equal(val["recall"], orec) and torch.equal(val["thresholds"], oth)

    def check_counts(got, thr):
        tp, fp, fn, tn = O.seg_counts(ph, t, thr, is_logits=False)
        assert got["counts"] == {"tp": tp, "fp": fp, "fn": fn, "tn": tn}
        assert min(tp, fp, fn, tn) > 0
        assert abs(got["acc"] - (tp + tn) / n) < 1e-6 and abs(got["pos_iou"] - tp / (tp + fp + fn)) < 1e-6
        want = [[tn / (tn + fp), fp / (tn + fp)], [fn / (fn + tp), tp / (fn + tp)]]
        assert np.abs(np.array(got["confusion"]) - np.array(want)).max() < 1e-6
        return 2 * tp / (2 * tp + fp + fn)

    assert abs(val["dice_at_threshold"] - check_counts(val, best[0])) < 1e-6
    ref_bce = float(O.bce_with_logits(x.double(), t.double()))
    print(f"bce {val['bce_loss']!r} (fp64 {ref_bce!r}), AP {val['avg_prec']!r}, best threshold {best[0]}")
    assert abs(val["bce_loss"] - ref_bce) <= 1e-6 * abs(ref_bce)
    want_ap = O.average_precision(ph, t)
    assert abs(val["avg_prec"] - want_ap) < 1e-9, (val["avg_prec"], want_ap)

    test = H.test_net(pred, 0.37)
    assert abs(test["dice"] - check_counts(test, 0.37)) < 1e-6
    assert abs(test["avg_prec"] - want_ap) < 1e-9
    assert set(test) == {"acc", "dice", "pos_iou", "avg_prec", "confusion", "counts"}


def test_predict_split_runs_a_real_network_in_eval_and_restores_it():
    import hyperpri_amd as H
    net = H.UNet(3, 1, bilinear=False)
    net.load_state_dict(O.synth_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())))
    net = net.to(DEV).train()
    xs = [_u(91 + i, (2, 3, 36, 50)).to(DEV) for i in range(2)]
    ms = [(_u(95 + i, (2, 1, 36, 50)) > 0.8).float().to(DEV) for i in range(2)]
    net.eval()
    with torch.no_grad():
        want = torch.cat([net(x).reshape(-1) for x in xs])
    net.train()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    pred = H.predict_split(net, [{"image": x, "mask": m, "index": [2 * i, 2 * i + 1]} for i, (x, m) in enumerate(zip(xs, ms))])
    assert net.training and all(mod.training for mod in net.modules())
    after = net.state_dict()
    assert any(k.endswith("num_batches_tracked") for k in before)
    for k, v in before.items():                                                 # running_mean / running_var / num_batches_tracked among them
        assert torch.equal(after[k], v), k
    assert torch.equal(pred.logits, want)
    assert torch.equal(pred.masks, torch.cat([m.reshape(-1) for m in ms]))
    assert not pred.logits.requires_grad and not pred.masks.requires_grad
    assert pred.names == [0, 1, 2, 3] and pred.offsets == [i * 36 * 50 for i in range(5)]
    net.eval()                                                                  # an eval() network stays in eval()
    H.predict_split(net, [{"image": xs[0], "mask": ms[0], "index": [0, 1]}])
    assert not net.training


class _TwoBands(nn.Module):
    def forward(self, x):                       # (N,1,C,h,w) -> (N,1,h,w)
        return x[:, :, 3] + x[:, :, 7]


def test_from_the_cache_to_files(tmp_path):
    import hyperpri_amd as H
    Hs, Ws, B, lo, hi = 12, 20, 16, 2, 14
    cubes = [_u(101 + i, (Hs, Ws, B)).numpy() for i in range(3)]
    masks = [(_u(111 + i, (Hs, Ws)) > 0.6).to(torch.uint8).numpy() for i in range(3)]
    names = ["plant_a", "plant_b", "plant_c"]
    cache = H.CubeCache(capacity=3, height=Hs, width=Ws, bands=B, hsi_lo=lo, hsi_hi=hi, device=DEV)
    cache.fill(zip(cubes, masks, names))
    net = _TwoBands()
    pred = H.predict_split(net, cache.epoch(batch_size=2, shuffle=False))
    assert pred.names == names and pred.offsets == [0, 240, 480, 720] and pred.sizes == [(Hs, Ws)] * 3
    for i in range(3):
        lg, mk = pred.image(i)
        assert torch.equal(lg.cpu(), torch.from_numpy(cubes[i][:, :, lo + 3] + cubes[i][:, :, lo + 7]))
        assert torch.equal(mk.cpu(), torch.from_numpy(masks[i]).float())
    thr, bands = 0.7, (5, 2, 0)
    assert float((torch.sigmoid(pred.logits.cpu()) - thr).abs().min()) > 1e-5       # no class hangs on an ulp of the sigmoid
    paths = H.write_segmaps(str(tmp_path / "maps"), pred, cache.epoch(batch_size=2, shuffle=False), thr, bands=bands)
    try:
        from PIL import Image
        ext, read = ".png", lambda p: np.asarray(Image.open(p).convert("RGB"))
    except ImportError:
        ext, read = ".npy", np.load
    assert sorted(os.listdir(tmp_path / "maps")) == [f"{nm}_seg{ext}" for nm in names]
    assert paths == [str(tmp_path / "maps" / f"{nm}_seg{ext}") for nm in names]
    seen = set()
    for i, path in enumerate(paths):
        lg, mk = pred.image(i)
        direct, cls = H.color_segmaps(cache.batch([i])["image"], lg, mk, thr, bands=bands, return_classes=True)
        assert np.array_equal(read(path), direct[0].cpu().numpy())
        seen |= set(cls.unique().tolist())
        # the same cube as a plain contiguous (1,C,h,w) tensor: the other layout, the same picture
        plain = torch.from_numpy(cubes[i][:, :, lo:hi].copy()).permute(2, 0, 1)[None].contiguous().to(DEV)
        assert torch.equal(H.color_segmaps(plain, lg, mk, thr, bands=bands), direct)
        want, _ = _restate(plain.cpu(), lg.cpu()[None], mk.cpu()[None], thr, bands, 2.2, 0.6, H.evaluate.PALETTE)
        assert int((direct.cpu().int() - want.int()).abs().max()) <= 1
    assert seen == {0, 1, 2, 3}
    with pytest.raises(ValueError, match="same order"):
        H.write_segmaps(str(tmp_path / "maps"), pred, cache.epoch(batch_size=2, shuffle=True, generator=torch.Generator().manual_seed(1)),
                        thr, bands=bands)
