"""Test-time augmentation on the device: hpri_tta_merge (csrc/tta.hip) against the numpy restatement of hyperpri_amd/tta.py, the
cache's views against ``apply_view``, and the plumbing through predict_split / evaluate_multiclass.  Needs a real MI355X: ``-m gpu``.

Tolerances.  The logit mode is compared bit for bit with a numpy fp32 loop in view order.  The prob mode is compared with fp64:
|out - ref| <= (V + c) 2^-23 + 2^-23 |ref|, where c is MEASURED per session: four times the largest error (in units of 2^-23, rounded
up) of a V = 1, ``id`` merge over a ramp of 4096 logits on [-30, 30] -- the device's expf / logf / division error, which nothing
here can state in advance.  c above 64 fails the session.  The binary spread gets (V + c) 2^-23, the multi-class spread is exact on
inputs built with a top-two gap of at least 0.5 in every view and in the merged output.
Observed on an MI355X: see DESIGN.md, "Test-time augmentation"."""
import ctypes
import functools
import math
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import record_margin
from oracle import hyperpri_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -23
ALL = ("id", "flip_h", "flip_w", "rot180", "rot90", "rot270", "transpose", "antitranspose")
SHAPES = [(1, 1, 1, 1), (1, 1, 33, 1), (2, 1, 37, 70), (1, 3, 31, 65), (1, 64, 8, 9), (2, 2, 64, 96)]
VIEW_SETS = [("id",), ALL, ("rot90", "flip_h", "antitranspose"), ("id", "flip_w", "flip_h", "rot180")]
CASES = [(s, v) for s in SHAPES for v in VIEW_SETS]
IDS = ["x".join(map(str, s)) + "-" + ("all8" if v == ALL else "+".join(v)) for s, v in CASES]
GUARD = 64


def _u(seed, shape):
    return torch.from_numpy(O._u(seed, int(np.prod(shape))).reshape(shape).copy())


def _merge_raw(arrays, views, mode, spread):
    """hpri_tta_merge on NaN-poisoned buffers with GUARD floats behind each, which must stay NaN.  Returns (out, spread) as numpy."""
    from hyperpri_amd import _lib, tta
    from hyperpri_amd.engine import _p
    xs = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]
    N, K, hv, wv = arrays[0].shape
    h, w = (wv, hv) if tta.view_transposes(views[0]) else (hv, wv)
    out = torch.full((N * K * h * w + GUARD,), float("nan"), device=DEV)
    sp = torch.full((N * h * w + GUARD,), float("nan"), device=DEV) if spread else None
    V = len(views)
    ptrs = (ctypes.c_void_p * V)(*[x.data_ptr() for x in xs])
    codes = (ctypes.c_int * V)(*[tta.view_code(v) for v in views])
    with torch.cuda.device(DEV):
        _lib.call("hpri_tta_merge", ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(codes, ctypes.c_void_p), V, N, K, h, w, mode,
                  _p(out), _p(sp), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isnan(o[-GUARD:]).all(), "the merge wrote behind its output"
    o = o[:-GUARD].reshape(N, K, h, w)
    if sp is None:
        return o, None
    s = sp.cpu().numpy()
    assert np.isnan(s[-GUARD:]).all(), "the merge wrote behind its spread map"
    return o, s[:-GUARD].reshape(N, h, w)


@functools.lru_cache(maxsize=None)
def _c_bound():
    """c of the module docstring, measured once."""
    from hyperpri_amd import tta
    ramp = np.linspace(-30.0, 30.0, 4096).astype(np.float32).reshape(1, 1, 64, 64)
    got, _ = _merge_raw([ramp], ("id",), 1, False)
    want, _ = tta.tta_merge_reference([ramp], ("id",), "prob")
    err = float(np.abs(got.astype(np.float64) - want).max())
    c = int(math.ceil(4 * err / U))
    print(f"tta: largest error of a V = 1 id prob merge on the ramp: {err:.3e} = {err / U:.2f} x 2^-23 -> c = {c}")
    record_margin("tta_c_bound", c, 64)
    assert c <= 64, f"c = {c}: the device's expf / logf / division are further off than the contract can absorb"
    return c


@functools.lru_cache(maxsize=None)
def _inputs(shape, views):
    """One (N, K, hv, wv) fp32 array per view: 4 randn with about 1 % of the entries at +-40 and +-200."""
    from hyperpri_amd import tta
    N, K, h, w = shape
    rng = np.random.default_rng(1000 * h + 10 * w + K + len(views))
    arrays = []
    for v in views:
        hv, wv = tta.view_shape(v, h, w)
        a = (4 * rng.standard_normal((N, K, hv, wv))).astype(np.float32)
        pick = rng.random(a.shape)
        for i, val in enumerate((40.0, -40.0, 200.0, -200.0)):
            a[(pick >= 0.0025 * i) & (pick < 0.0025 * (i + 1))] = val
        arrays.append(a)
    if N * K * h * w >= 400:
        assert any((np.abs(a) == 200).any() for a in arrays)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def _voting_inputs(shape, views):
    """K > 1 inputs on which every argmax is beyond rounding: per frame pixel a majority class wins in all views but at most V // 3
    dissenters (and none at all on about 40 % of the pixels); a winner is 8 + noise, everything else noise in [0, 0.25).  The
    top-two gap of every view, of the mean logits and of the log mean softmax is checked to be at least 0.5 here, in fp64."""
    from hyperpri_amd import tta
    N, K, h, w = shape
    V = len(views)
    rng = np.random.default_rng(7 + 1000 * h + K + V)
    major = rng.integers(0, K, (N, h, w))
    arrays = []
    dissent = np.zeros((V, N, h, w), dtype=bool)
    for _ in range(V // 3):
        who = rng.integers(0, V, (N, h, w))
        n_, y_, x_ = np.nonzero(rng.random((N, h, w)) < 0.6)          # (the other pixels keep a unanimous vote)
        dissent[who[n_, y_, x_], n_, y_, x_] = True
    frames = []
    for v in range(V):
        other = (major + rng.integers(1, K, (N, h, w))) % K
        win = np.where(dissent[v], other, major)
        a = 0.25 * rng.random((N, K, h, w))
        np.put_along_axis(a, win[:, None], 8.0 + np.take_along_axis(a, win[:, None], 1), 1)
        frames.append(a.astype(np.float32))
        arrays.append(np.ascontiguousarray(tta.apply_view(frames[-1], views[v])))

    def gap(x):
        top = np.sort(x, axis=1)
        return float((top[:, -1] - top[:, -2]).min())
    f64 = [a.astype(np.float64) for a in frames]
    assert all(gap(a) >= 0.5 for a in f64)
    for merge in ("logit", "prob"):
        out, _ = tta.tta_merge_reference(arrays, views, merge)
        assert gap(out) >= 0.5, (shape, views, merge, gap(out))
    if V >= 3 and N * h * w >= 100:
        assert dissent.any()
    return tuple(arrays)


def _check_prob(key, got, want, V, c):
    tol = (V + c) * U + U * np.abs(want)
    err = np.abs(got.astype(np.float64) - want)
    assert np.isfinite(got).all(), key
    worst = float((err / tol).max())
    record_margin("tta_merge_prob", worst, 1.0)
    assert worst <= 1.0, (key, worst, float(err.max()))
    return float(err.max())


@pytest.mark.parametrize("shape,views", CASES, ids=IDS)
def test_merge_kernel_against_the_restatement(shape, views):
    from hyperpri_amd import tta
    c = _c_bound()
    N, K, h, w = shape
    V = len(views)
    arrays = _inputs(shape, views)
    worst_out = worst_sp = 0.0
    for mode, merge in ((0, "logit"), (1, "prob")):
        for spread in (False, True):
            got, sp = _merge_raw(arrays, views, mode, spread)
            assert not np.isnan(got).any() and (sp is None or not np.isnan(sp).any())        # every element was written
            if mode == 0:
                want, _ = tta.tta_merge_reference(arrays, views, "logit", dtype=np.float32)
                assert want.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), (shape, views, spread)
            else:
                want, _ = tta.tta_merge_reference(arrays, views, "prob")
                worst_out = max(worst_out, _check_prob((shape, views, spread), got, want, V, c))
            if spread and K == 1:
                _, want_sp = tta.tta_merge_reference(arrays, views, merge, spread=True)
                err = float(np.abs(sp.astype(np.float64) - want_sp).max())
                worst_sp = max(worst_sp, err)
                record_margin("tta_spread_binary", err / ((V + c) * U), 1.0)
                assert err <= (V + c) * U, (shape, views, merge, err)
            elif spread:
                voting = _voting_inputs(shape, views)
                got_v, sp_v = _merge_raw(voting, views, mode, True)
                want_v, want_sp = tta.tta_merge_reference(voting, views, merge, spread=True)
                assert np.array_equal(got_v.argmax(1), want_v.argmax(1))
                assert np.array_equal(sp_v, (want_sp * V).round().astype(np.float32) / np.float32(V)), (shape, views, merge)
    print(f"tta merge {shape} {views}: max |out - fp64| {worst_out:.3e}, max |spread - fp64| {worst_sp:.3e} (c = {c})")
    if V == 1:                                                       # one id view in logit mode: the input bits
        got, _ = _merge_raw(arrays, views, 0, False)
        assert np.array_equal(got.view(np.int32), arrays[0].view(np.int32))


@pytest.mark.parametrize("shape,views", CASES, ids=IDS)
def test_merge_kernel_is_deterministic(shape, views):
    arrays = _inputs(shape, views)
    for mode in (0, 1):
        for spread in (False, True):
            a, sa = _merge_raw(arrays, views, mode, spread)
            b, sb = _merge_raw(arrays, views, mode, spread)
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
            assert sa is None or np.array_equal(sa.view(np.int32), sb.view(np.int32))


def test_merge_propagates_nan_and_the_wrapper_checks_shapes():
    import hyperpri_amd as H
    x = np.zeros((1, 1, 5, 7), dtype=np.float32)
    x[0, 0, 2, 3] = np.nan
    for mode in (0, 1):
        got, sp = _merge_raw([x, np.zeros((1, 1, 7, 5), dtype=np.float32)], ("id", "transpose"), mode, True)
        assert np.isnan(got[0, 0, 2, 3]) and np.isnan(got).sum() == 1 and np.isnan(sp[0, 2, 3]) and np.isnan(sp).sum() == 1
    k = np.zeros((1, 3, 5, 7), dtype=np.float32)
    k[0, 1, 4, 6] = np.nan
    got, _ = _merge_raw([k], ("id",), 1, False)
    assert np.isnan(got[0, :, 4, 6]).all() and np.isnan(got).sum() == 3
    t = torch.zeros((1, 1, 5, 7), device=DEV)
    with pytest.raises(ValueError, match="view 'rot90'"):
        H.tta_merge([t, t], ("id", "rot90"))
    out, sp = H.tta_merge([t, t.transpose(-2, -1).contiguous()], ("id", "rot90"), "prob", True)
    assert out.shape == (1, 1, 5, 7) and sp.shape == (1, 5, 7) and not out.any() and not sp.any()


# ---- cache views -------------------------------------------------------------------------------------------------------
_CACHES = {}


def _cache(frame, store, out_slots=2):
    key = (frame, store, out_slots)
    if key not in _CACHES:
        from hyperpri_amd.cache import CubeCache
        Hs, Ws = frame
        cubes = [_u(500 + k + 10 * Hs, (Hs, Ws, 14)) for k in range(3)]
        masks = [(_u(600 + k + 10 * Hs, (Hs, Ws)) * 3).to(torch.uint8) for k in range(3)]
        cache = CubeCache(3, Hs, Ws, 14, hsi_lo=2, hsi_hi=13, device=DEV, store_dtype=store, out_slots=out_slots)
        cache.fill((cubes[k], masks[k], f"box{k}") for k in range(3))
        _CACHES[key] = cache
    return _CACHES[key]


def _underlying(x, cs):
    x4 = x.squeeze(1) if x.dim() == 5 else x
    N, _, h, w = x4.shape
    return torch.as_strided(x4, (N, h, w, cs), (h * w * cs, w * cs, cs, 1))


@pytest.mark.parametrize("store", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("frame", [(13, 22), (12, 21)], ids=["13x22", "12x21"])
def test_cache_views_are_bit_equal_to_apply_view(frame, store):
    import hyperpri_amd as H
    from hyperpri_amd import tta
    cache = _cache(frame, store)
    assert (cache.C, cache.cs) == (11, 16)
    plain = cache.batch([2, 0])
    image, mask = plain["image"].clone(), plain["mask"].clone()
    assert image.shape == (2, 1, 11, *frame) and mask.shape == (2, 1, *frame)
    for v in ALL:
        for b in cache._out + cache._mout:
            b.fill_(float("nan"))
        got = cache.view([2, 0], v)
        assert got["index"] == ["box2", "box0"]
        hv, wv = tta.view_shape(v, *frame)
        assert got["image"].shape == (2, 1, 11, hv, wv) and got["mask"].shape == (2, 1, hv, wv), v
        assert torch.equal(got["image"], H.apply_view(image, v)), v
        assert torch.equal(got["mask"], H.apply_view(mask, v)), v
        pad = _underlying(got["image"], cache.cs)[..., cache.C:]
        assert pad.shape == (2, hv, wv, 5) and not pad.any() and not torch.isnan(pad).any(), v
        assert getattr(got["image"], "_hpri_zero_padded", False)
    with pytest.raises(ValueError, match="unknown view"):
        cache.view([0], "rot45")
    with pytest.raises(IndexError):
        cache.view([3], "id")


# ---- a network whose answer is known exactly ----------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    """NOT equivariant: band 0 plus a ramp over the coordinates of whatever frame it is shown."""

    @staticmethod
    def ramp(hv, wv, device):
        i = torch.arange(hv, dtype=torch.float32, device=device)[:, None]
        j = torch.arange(wv, dtype=torch.float32, device=device)[None, :]
        return 0.375 * i - 0.25 * j + 0.5 * ((i * 3 + j) % 7) - 1.0

    def forward(self, x):
        band0 = x[:, 0, 0] if x.dim() == 5 else x[:, 0]
        return (band0 * 6.0 + self.ramp(band0.shape[-2], band0.shape[-1], band0.device)).unsqueeze(1)


def _stub_views(image):
    """What _Stub answers for every view of ``image`` (CPU, the same fp32 operations), as numpy (N, 1, hv, wv) arrays."""
    import hyperpri_amd as H
    stub = _Stub()
    return [stub(H.apply_view(image, v).contiguous()).numpy() for v in ALL]


@pytest.mark.parametrize("merge", ["logit", "prob"])
def test_predict_split_with_a_stub_network(merge):
    import hyperpri_amd as H
    from hyperpri_amd import tta
    c = _c_bound()
    cache = _cache((13, 22), torch.float32)
    images, masks = [], []
    for slots in ([0, 1], [2]):
        b = cache.batch(slots)
        images.append(b["image"].cpu().contiguous())
        masks.append(b["mask"].cpu().clone())
    want, want_sp = [], []
    for image in images:
        o, s = tta.tta_merge_reference(_stub_views(image), ALL, merge, spread=True, dtype=np.float32 if merge == "logit" else np.float64)
        want.append(o.reshape(-1))
        want_sp.append(s.reshape(-1))
    want, want_sp = np.concatenate(want), np.concatenate(want_sp)
    settings = H.TTA(views=ALL, merge=merge, spread=True)
    fallback = [{"image": im.to(DEV), "mask": m.to(DEV), "index": nm} for im, m, nm in zip(images, masks, (["box0", "box1"], ["box2"]))]
    stub = _Stub().to(DEV).train()
    for batches in (cache.epoch_views(2, settings.views), fallback):
        pred = H.predict_split(stub, batches, tta=settings)
        assert stub.training
        assert pred.names == ["box0", "box1", "box2"] and pred.sizes == [(13, 22)] * 3 and pred.offsets == [0, 286, 572, 858]
        assert torch.equal(pred.masks.cpu(), torch.cat([m.reshape(-1) for m in masks]))
        got = pred.logits.cpu().numpy()
        if merge == "logit":
            assert np.array_equal(got.view(np.int32), want.view(np.int32))
        else:
            _check_prob(("stub", merge), got, want, 8, c)
        assert pred.spread.shape == pred.logits.shape
        assert float(np.abs(pred.spread.cpu().numpy().astype(np.float64) - want_sp).max()) <= (8 + c) * U
    stub.eval()
    H.predict_split(stub, fallback, tta=H.TTA(views=("id",)))
    assert not stub.training


def test_identity_view_in_logit_mode_is_the_plain_prediction():
    import hyperpri_amd as H
    net = H.UNet(3, 1, bilinear=False)
    net.load_state_dict(O.synth_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())))
    net = net.to(DEV).train()
    batch = {"image": _u(91, (2, 3, 36, 52)).to(DEV), "mask": (_u(95, (2, 1, 36, 52)) > 0.8).float().to(DEV), "index": ["a", "b"]}
    plain = H.predict_split(net, [batch])
    same = H.predict_split(net, [batch], tta=H.TTA(views=("id",), merge="logit"))
    assert net.training
    assert torch.equal(plain.logits.view(torch.int32), same.logits.view(torch.int32)) and torch.equal(plain.masks, same.masks)
    assert (plain.offsets, plain.sizes, plain.names) == (same.offsets, same.sizes, same.names)
    assert plain.spread is None and same.spread is None


# ---- real networks ------------------------------------------------------------------------------------------------------
def test_unet_with_all_eight_views(tmp_path):
    import hyperpri_amd as H
    from hyperpri_amd import tta
    c = _c_bound()
    net = H.UNet(3, 1, bilinear=False)
    net.load_state_dict(O.synth_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())))
    net = net.to(DEV).train()
    x = _u(191, (2, 3, 36, 52)).to(DEV)
    batch = {"image": x, "mask": (_u(195, (2, 1, 36, 52)) > 0.8).float().to(DEV), "index": ["a", "b"]}
    net.eval()
    with torch.inference_mode():
        per_view = [net(H.apply_view(x, v).contiguous()).float().cpu().numpy() for v in ALL]
    net.train()
    assert per_view[4].shape == (2, 1, 52, 36)
    pred = H.predict_split(net, [batch], tta=H.TTA(views=ALL, merge="prob", spread=True))
    assert net.training
    want, want_sp = tta.tta_merge_reference(per_view, ALL, "prob", spread=True)
    err = _check_prob("unet", pred.logits.cpu().numpy(), want.reshape(-1), 8, c)
    print(f"UNet(3, 1) eight views: max |merged - fp64 merge of its own outputs| {err:.3e}")
    sp = pred.spread.cpu().numpy()
    assert sp.shape == (2 * 36 * 52,) and sp.min() >= 0.0 and sp.max() <= 0.5
    assert float(np.abs(sp.astype(np.float64) - want_sp.reshape(-1)).max()) <= (8 + c) * U
    # not the plain prediction: the network is not equivariant
    assert not torch.equal(pred.logits, H.predict_split(net, [batch]).logits)
    val = H.validate_net(pred)
    assert 0.0 <= val["best_threshold"] <= 1.0 and math.isfinite(val["bce_loss"])
    test = H.test_net(pred, val["best_threshold"])
    assert 0.0 <= test["acc"] <= 1.0
    paths = H.write_spreadmaps(str(tmp_path / "spread"), pred)
    assert [os.path.basename(p).rsplit(".", 1)[0] for p in paths] == ["a_spread", "b_spread"] and all(os.path.exists(p) for p in paths)
    with pytest.raises(ValueError, match="no spread"):
        H.write_spreadmaps(str(tmp_path / "none"), H.predict_split(net, [batch]))


def test_spectral_unet_multiclass_with_the_default_views(tmp_path):
    import hyperpri_amd as H
    from hyperpri_amd import tta
    net = H.SpectralUNET(10, 3, 4)
    net.load_state_dict(O.synth_state_dict(OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())))
    net = net.to(DEV).train()
    xs = _u(291, (3, 10, 19, 26))
    ts = (_u(295, (3, 19, 26)) * 3).long().clamp(max=2)
    names = ["p", "q", "r"]
    batches = [{"image": xs[a:b].to(DEV), "mask": ts[a:b].to(torch.uint8).to(DEV), "index": names[a:b]} for a, b in ((0, 2), (2, 3))]
    settings = H.TTA(merge="prob", spread=True)
    net.eval()
    with torch.inference_mode():
        per_view = [torch.cat([net(H.apply_view(b["image"], v).contiguous()).float() for b in batches]).cpu().numpy() for v in settings.views]
    net.train()
    logp, want_sp = tta.tta_merge_reference(per_view, settings.views, "prob", spread=True)
    ref = float(torch.nn.CrossEntropyLoss()(torch.from_numpy(logp), ts))
    out = H.evaluate_multiclass(net, batches, 3, tta=settings, segmap_dir=str(tmp_path / "maps"), bands=(2, 1, 0), gamma=1.0)
    assert net.training and out["names"] == names
    print(f"evaluate_multiclass with TTA: ce_loss {out['ce_loss']!r} (fp64 {ref!r})")
    assert abs(out["ce_loss"] - ref) <= 1e-6 * abs(ref)
    assert int(np.sum(out["confusion"])) == ts.numel()
    assert out["spread_paths"] == [str(tmp_path / "maps" / f"{nm}_spread.npy") for nm in names]
    for i, p in enumerate(out["spread_paths"]):
        m = np.load(p)
        assert m.shape == (19, 26) and m.dtype == np.float32 and set(np.unique(m)) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    assert len(out["paths"]) == 3
    plain = H.evaluate_multiclass(net, batches, 3)
    assert "spread_paths" not in plain and plain["ce_loss"] != out["ce_loss"]
