"""Device-resident cube cache (hyperpri_amd/cache.py, csrc/cache.hip): bit-exact data movement against a torch
restatement of ``dataset.py:267-270`` + crop + flips, in-place consumption by the networks (bit-identical loss, logits and
gradients), output-buffer reuse without host synchronisation, and epochs that reproduce the host planner.
Needs a real MI355X: ``-m gpu``."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import hyperpri_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _u(seed, shape):
    return torch.from_numpy(O._u(seed, int(np.prod(shape))).reshape(shape).copy())


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _want(cubes, masks, rows, lo, hi, h, w, unsqueeze=True):
    """The restatement: ``cube[idx][top:top+h, left:left+w, lo:hi]``, flipped, permuted as dataset.py:267-270 (same for masks)."""
    xs, ms = [], []
    for idx, top, left, flags in rows:
        c = cubes[idx][top:top + h, left:left + w, lo:hi]
        m = masks[idx][top:top + h, left:left + w]
        dims = [d for d, bit in ((0, 1), (1, 2)) if flags & bit]
        if dims:
            c, m = torch.flip(c, dims), torch.flip(m, dims)
        c = c.permute(2, 0, 1)
        xs.append(c.unsqueeze(0) if unsqueeze else c)
        ms.append(m.unsqueeze(0).float())
    return torch.stack(xs), torch.stack(ms)


def _underlying(x, cs):
    """The padded (N, h, w, cs) buffer behind a batch's image."""
    x4 = x.squeeze(1) if x.dim() == 5 else x
    N, _, h, w = x4.shape
    return torch.as_strided(x4, (N, h, w, cs), (h * w * cs, w * cs, cs, 1))


# (Hs, Ws, h, w, top, left): the window equal to the frame, one in every corner (touching two borders each), each single border,
# an interior one, one-pixel-wide / -high windows, and a frame whose rows span several work items of the gather (w * cs/4 > 1024)
GEOMETRIES = [(9, 14, 9, 14, 0, 0), (12, 20, 5, 7, 0, 0), (12, 20, 5, 7, 0, 13), (12, 20, 5, 7, 7, 0), (12, 20, 5, 7, 7, 13),
              (12, 20, 6, 8, 3, 0), (12, 20, 6, 8, 0, 5), (12, 20, 6, 8, 3, 12), (12, 20, 6, 8, 6, 5), (12, 20, 6, 8, 3, 5),
              (12, 20, 12, 1, 0, 19), (12, 20, 1, 20, 11, 0), (5, 40, 4, 37, 1, 2)]


@pytest.mark.parametrize("src_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("store_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("flip_h,flip_w", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("B,lo,hi", [(299, 25, 263), (13, 12, 13), (8, 0, 8), (11, 2, 9)])
def test_gather_is_bit_exact(B, lo, hi, geom, flip_h, flip_w, store_dtype, src_dtype):
    from hyperpri_amd.cache import CubeCache
    Hs, Ws, h, w, top, left = geom
    C = hi - lo
    cache = CubeCache(3, Hs, Ws, B, hsi_lo=lo, hsi_hi=hi, device=DEV, store_dtype=store_dtype, out_slots=1)
    cache._cubes.fill_(float("nan"))                       # whatever the store pass does not write shows up below
    cubes = [_u(300 + k, (Hs, Ws, B)).to(src_dtype) for k in range(3)]
    masks = [(_u(400 + k, (Hs, Ws)) > 0.6).to(torch.uint8) for k in range(3)]
    for k in range(3):
        cache.put(k, cubes[k].numpy() if k == 1 else cubes[k].to(DEV) if k == 2 else cubes[k], masks[k], name=f"box{k}")
    assert len(cache) == 3
    cache.batch([0, 1], patch=(h, w), top=top, left=left)   # a first tenant of the (single) output buffer ...
    cache._out[0].fill_(float("nan"))                       # ... and poison: every element must be rewritten
    cache._mout[0].fill_(float("nan"))
    idx = [2, 0]
    out = cache.batch(idx, top=top, left=left, flip_h=flip_h, flip_w=flip_w, patch=(h, w))
    rounded = [c.half().float() if torch.float16 in (store_dtype, src_dtype) else c for c in cubes]    # rounded ONCE to half
    rows = [(i, top, left, flip_h | (flip_w << 1)) for i in idx]
    want_x, want_m = _want(rounded, masks, rows, lo, hi, h, w)
    x, m = out["image"], out["mask"]
    assert x.dtype == torch.float32 and tuple(x.shape) == (2, 1, C, h, w) and tuple(m.shape) == (2, 1, h, w)
    assert torch.equal(x.cpu(), want_x)
    assert m.dtype == torch.float32 and torch.equal(m.cpu(), want_m)
    assert out["index"] == ["box2", "box0"]
    assert getattr(x, "_hpri_zero_padded", False)
    cs = (C + 7) // 8 * 8
    assert x.stride(2) == 1 and x.stride(4) == cs and x.data_ptr() % 16 == 0
    under = _underlying(x, cs)
    assert torch.equal(under[..., :C].cpu(), want_x.squeeze(1).permute(0, 2, 3, 1))
    assert torch.count_nonzero(under[..., C:]) == 0 and not torch.isnan(under).any()       # pad channels [C, cs) are zero


def test_put_takes_numpy_and_torch_on_host_and_device_and_batch_validates():
    from hyperpri_amd.cache import CubeCache
    cache = CubeCache(4, 8, 10, 9, hsi_lo=1, hsi_hi=8, device=DEV, unsqueeze_hsi=False)
    cube = _u(90, (8, 10, 9))
    mask = (_u(91, (8, 10)) > 0.5)
    cache.put(0, cube.numpy(), mask.numpy())
    cache.put(1, cube, mask.float().reshape(1, 8, 10))
    cache.put(2, cube.to(DEV), mask.to(DEV))
    assert cache.fill([]) == 0
    with pytest.raises(IndexError):
        cache.batch([3])                                    # an empty slot
    with pytest.raises(ValueError, match="leaves"):
        cache.batch([0], top=5, patch=(4, 4))               # a window outside the frame
    with pytest.raises(ValueError):
        cache.put(3, cube[..., :8], mask)
    out = cache.batch([0, 1, 2])
    want = cube[..., 1:8].permute(2, 0, 1)
    assert tuple(out["image"].shape) == (3, 7, 8, 10) and out["index"] == [0, 1, 2]
    for k in range(3):
        assert torch.equal(out["image"][k].cpu(), want) and torch.equal(out["mask"][k, 0].cpu(), mask.float())


def _tiny_cubenet(precision=None):
    import hyperpri_amd as H
    net = H.CubeNET(6, 1, first_depth=64, bilinear=False)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())
    net.load_state_dict(O.synth_state_dict(shapes))
    net = net.to(DEV).train()
    return H.set_precision(net, precision) if precision else net


def _step(net, x, mask, log_calls=False):
    import hyperpri_amd.engine as E
    calls = []
    orig = E._lib.call
    if log_calls:
        E._lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        logits = net(x)
        loss = torch.nn.BCEWithLogitsLoss()(logits, mask)
        loss.backward()
    finally:
        E._lib.call = orig
    grads = [p.grad.clone() for p in net.parameters()]
    for p in net.parameters():
        p.grad = None
    return loss.detach().clone(), logits.detach().clone(), grads, calls


def _tiny_cache(n=2, **kw):
    from hyperpri_amd.cache import CubeCache
    cubes = [_u(1235 + k, (36, 50, 9)) for k in range(n)]                # 9 bands on "disk", the net takes [2:8]
    masks = [(_u(4321 + k, (36, 50)) > 0.9).to(torch.uint8) for k in range(n)]
    cache = CubeCache(n, 36, 50, 9, hsi_lo=2, hsi_hi=8, device=DEV, **kw)
    assert cache.fill((cubes[k].numpy(), masks[k].numpy(), f"box{k}") for k in range(n)) == n
    return cache, cubes, masks


def test_cubenet_consumes_cached_batch_in_place_bit_identical():
    cache, cubes, masks = _tiny_cache()
    rows = [(1, 0, 0, 2), (0, 0, 0, 1)]
    want_x, want_m = _want(cubes, masks, rows, 2, 8, 36, 50)
    x_ref, m_ref = want_x.contiguous().to(DEV), want_m.to(DEV)            # what dataset.py would hand over: (N,1,C,H,W) contiguous
    loss, logits, grads, _ = _step(_tiny_cubenet(), x_ref, m_ref)
    out = cache.batch([1, 0], flip_h=[0, 1], flip_w=[1, 0])
    assert torch.equal(out["image"], x_ref) and torch.equal(out["mask"], m_ref)
    loss2, logits2, grads2, calls = _step(_tiny_cubenet(), out["image"], out["mask"], log_calls=True)
    assert calls and not any(c.startswith("hpri_nchw_to_nhwc") for c in calls)            # consumed in place
    assert torch.equal(loss2, loss) and torch.equal(logits2, logits)
    assert len(grads) == len(grads2) and all(torch.equal(a, b) for a, b in zip(grads2, grads))


def test_bf16_step_from_the_cache_equals_a_stager_fed_step():
    from hyperpri_amd.ingest import CubeStager
    cache, cubes, masks = _tiny_cache()
    m_ref = torch.stack([m.unsqueeze(0).float() for m in masks]).to(DEV)
    st = CubeStager(2, 36, 50, 9, hsi_lo=2, hsi_hi=8, device=DEV)
    np.copyto(st.host_slot(), torch.stack(cubes).numpy())
    xs = st.submit()
    loss, logits, grads, calls_s = _step(_tiny_cubenet("bf16"), xs, m_ref, log_calls=True)
    st.release()
    out = cache.batch([0, 1])
    assert torch.equal(out["image"], xs) and torch.equal(out["mask"], m_ref)
    loss2, logits2, grads2, calls_c = _step(_tiny_cubenet("bf16"), out["image"], out["mask"], log_calls=True)
    calls_s, calls_c = ([c for c in cs if c != "hpri_set_item_queue"] for cs in (calls_s, calls_c))    # (first use of a stream registers one)
    assert calls_c == calls_s and not any(c.startswith("hpri_nchw_to_nhwc") for c in calls_c)   # the same zero-copy route
    assert torch.equal(loss2, loss) and torch.equal(logits2, logits)
    assert all(torch.equal(a, b) for a, b in zip(grads2, grads))


def test_spectral_unet_takes_4d_cached_batch():
    import hyperpri_amd as H
    from hyperpri_amd.cache import CubeCache

    def mk():
        net = H.SpectralUNET(22, 1, 48)
        shapes = OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())
        net.load_state_dict(O.synth_state_dict(shapes))
        return net.to(DEV).train()
    cubes = [_u(1238 + k, (12, 20, 22)) for k in range(2)]
    masks = [(_u(77 + k, (12, 20)) > 0.8).to(torch.uint8) for k in range(2)]
    cache = CubeCache(2, 12, 20, 22, device=DEV, unsqueeze_hsi=False)
    cache.fill((cubes[k], masks[k], k) for k in range(2))
    out = cache.batch([0, 1], flip_w=1)
    want_x, want_m = _want(cubes, masks, [(0, 0, 0, 2), (1, 0, 0, 2)], 0, 22, 12, 20, unsqueeze=False)
    assert tuple(out["image"].shape) == (2, 22, 12, 20) and torch.equal(out["image"].cpu(), want_x)
    a = _step(mk(), want_x.contiguous().to(DEV), want_m.to(DEV))
    b = _step(mk(), out["image"], out["mask"], log_calls=True)
    assert not any(c.startswith("hpri_nchw_to_nhwc") for c in b[3])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))


@pytest.mark.parametrize("out_slots", [1, 2])
def test_output_buffers_are_reused_safely_without_synchronising(out_slots):
    """Six consecutive training steps over one epoch, nothing between them but stream order: every step's gradients equal the
    ones of a run that synchronises and clones each batch first (a gather that overtook a reader of its buffer -- the weight
    gradient of the first layer runs on the engine's second stream -- would change them)."""
    cache, _, _ = _tiny_cache(12, out_slots=out_slots)
    kw = dict(batch_size=2, shuffle=True, patch=(32, 48), random_crop=True, flips=True)
    net = _tiny_cubenet()
    fast = []
    for batch in cache.epoch(generator=_gen(21), **kw):
        fast.append(_step(net, batch["image"], batch["mask"])[2])
    assert len(fast) == 6
    torch.cuda.synchronize()
    net = _tiny_cubenet()
    slow = []
    for batch in cache.epoch(generator=_gen(21), **kw):
        torch.cuda.synchronize()
        x, m = batch["image"].contiguous().clone(), batch["mask"].clone()
        torch.cuda.synchronize()
        slow.append(_step(net, x, m)[2])
        torch.cuda.synchronize()
    assert len(slow) == 6
    for ga, gb in zip(fast, slow):
        assert all(torch.equal(a, b) for a, b in zip(ga, gb))
    assert not all(torch.equal(a, b) for a, b in zip(fast[0], fast[1]))          # (the steps do see different data)


def test_epoch_reproduces_the_host_plan_and_two_epochs_differ():
    from hyperpri_amd.cache import plan_epoch
    cache, cubes, masks = _tiny_cache(7)
    kw = dict(patch=(20, 31), shuffle=True, random_crop=True, flips=True)
    plan = plan_epoch(7, 3, (36, 50), generator=_gen(5), **kw)
    g = _gen(5)
    got = [(b["image"].clone(), b["mask"].clone(), b["index"]) for b in cache.epoch(3, generator=g, **kw)]
    assert torch.equal(cache.last_plan.table, plan.table) and [x.shape[0] for x, _, _ in got] == [3, 3, 1]
    for (x, m, names), (s, e) in zip(got, plan.batches):
        rows = [tuple(r) for r in plan.table[s:e].tolist()]
        want_x, want_m = _want(cubes, masks, rows, 2, 8, 20, 31)
        assert torch.equal(x.cpu(), want_x) and torch.equal(m.cpu(), want_m)
        assert names == [f"box{r[0]}" for r in rows]
    assert sorted(n for _, _, names in got for n in names) == sorted(f"box{k}" for k in range(7))
    second = [b["image"].clone() for b in cache.epoch(3, generator=g, **kw)]      # the same generator, one epoch on
    assert not torch.equal(cache.last_plan.table, plan.table)
    assert not all(torch.equal(a, b[0]) for a, b in zip(second, got))
    dropped = list(cache.epoch(3, generator=_gen(5), drop_last=True, **kw))
    assert [b["image"].shape[0] for b in dropped] == [3, 3]
    plain = list(cache.epoch(4, shuffle=False))
    assert [b["index"] for b in plain] == [[f"box{k}" for k in range(4)], [f"box{k}" for k in range(4, 7)]]


def test_full_size_batches_match_the_restatement_on_the_device():
    """Three 299-band 608 x 968 cubes, bands [25:263], batch 2: whole frames with flips, then 512 x 512 windows pushed into
    opposite corners -- compared on the device (about 7 GB with the sources and the expected values)."""
    from hyperpri_amd.cache import CubeCache
    H_, W_, B, lo, hi = 608, 968, 299, 25, 263
    base = _u(7001, (H_, W_, B))
    cubes = [base.to(DEV)]
    cubes.append(1.0 - cubes[0])
    cubes.append(cubes[0] * 0.5 + 0.25)
    masks = [(_u(7100 + k, (H_, W_)) > 0.7).to(torch.uint8).to(DEV) for k in range(3)]
    cache = CubeCache(3, H_, W_, B, hsi_lo=lo, hsi_hi=hi, device=DEV, out_slots=1)
    cache.put(0, base.numpy(), masks[0])                    # host source: pinned staging at full size
    cache.put(1, cubes[1], masks[1])
    cache.put(2, cubes[2], masks[2])
    cache.release_staging()
    del base
    out = cache.batch([2, 0], flip_h=[1, 0], flip_w=[0, 1])
    want_x, want_m = _want(cubes, masks, [(2, 0, 0, 1), (0, 0, 0, 2)], lo, hi, H_, W_)
    assert tuple(out["image"].shape) == (2, 1, 238, H_, W_)
    assert torch.equal(out["image"], want_x) and torch.equal(out["mask"], want_m)
    assert torch.count_nonzero(_underlying(out["image"], 240)[..., 238:]) == 0
    del want_x, out
    out = cache.batch([1, 2], top=[96, 0], left=[0, 456], flip_h=[1, 1], flip_w=[1, 0], patch=512)
    want_x, want_m = _want(cubes, masks, [(1, 96, 0, 3), (2, 0, 456, 1)], lo, hi, 512, 512)
    assert torch.equal(out["image"], want_x) and torch.equal(out["mask"], want_m)


def test_slot_offsets_beyond_2_31_elements():
    """460 slots of 608 x 968 x 8 halves hold 2.17 G elements (4.3 GB): the last slot starts past 2^31, where 32-bit slot
    arithmetic would wrap into an earlier slot."""
    from hyperpri_amd.cache import CubeCache
    H_, W_, n = 608, 968, 460
    assert (n - 1) * H_ * W_ * 8 > 2 ** 31
    cache = CubeCache(n, H_, W_, 8, device=DEV, store_dtype=torch.float16, out_slots=1)
    cache._cubes.zero_()
    cubes = {k: _u(7200 + k, (H_, W_, 8)) for k in (0, n - 1)}
    masks = {k: (_u(7300 + k, (H_, W_)) > 0.7).to(torch.uint8) for k in (0, n - 1)}
    for k in cubes:
        cache.put(k, cubes[k], masks[k])
    out = cache.batch([n - 1, 0], top=[0, 96], left=[456, 0], flip_w=[1, 0], patch=512)
    rounded = {k: c.half().float() for k, c in cubes.items()}
    want_x, want_m = _want(rounded, masks, [(n - 1, 0, 456, 2), (0, 96, 0, 0)], 0, 8, 512, 512)
    assert torch.equal(out["image"].cpu(), want_x) and torch.equal(out["mask"].cpu(), want_m)
