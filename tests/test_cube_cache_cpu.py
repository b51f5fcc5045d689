"""Device-resident cube cache (hyperpri_amd/cache.py, csrc/cache.hip) -- CPU half: the new C-ABI entry points exist and
reject bad arguments without a launch, and the epoch planner (a pure host function) is deterministic, follows the
documented draw order and only plans windows inside the frame.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hpri_hwb_store", "hpri_cube_gather", "hpri_mask_gather")


def test_new_symbols_are_declared_and_exported():
    from hyperpri_amd import _lib
    header = open(os.path.join(ROOT, "include", "hyperpri_hip.h")).read()
    declared = set(re.findall(r"\b(hpri_\w+)\s*\(", header))
    decls = _lib.parse_header()
    lib = _lib.load()
    for n in NEW:
        assert n in declared and n in decls and hasattr(lib, n), n
    assert hasattr(_lib.load_f16(), "hpri_cube_gather")            # built into both product libraries


def test_store_rejects_bad_arguments_without_launch():
    from hyperpri_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(4096)                 # never dereferenced: every call below must fail its argument checks
    assert lib.hpri_hwb_store(null, 0, one, 0, 10, 8, 0, 8, 8, null) == -1 and b"null" in lib.hpri_last_error()
    assert lib.hpri_hwb_store(one, 0, null, 1, 10, 8, 0, 8, 8, null) == -1
    assert lib.hpri_hwb_store(one, 0, one, 1, 10, 8, 4, 8, 8, null) == -1 and b"band range" in lib.hpri_last_error()   # lo + C > B
    assert lib.hpri_hwb_store(one, 0, one, 0, 10, 8, 4, 8, 8, null) == -1
    assert lib.hpri_hwb_store(one, 0, one, 1, 10, 12, 0, 6, 6, null) == -1                      # cs not a multiple of 8
    assert lib.hpri_hwb_store(one, 0, one, 0, 10, 12, 0, 12, 12, null) == -1                    # (12 % 4 == 0 is not enough)
    assert lib.hpri_hwb_store(one, 0, one, 1, 10, 12, 0, 12, 8, null) == -1                     # cs < C
    assert lib.hpri_hwb_store(one, 2, one, 0, 10, 8, 0, 8, 8, null) == -1                       # unknown dtypes
    assert lib.hpri_hwb_store(one, 0, one, 2, 10, 8, 0, 8, 8, null) == -1
    with pytest.raises(RuntimeError, match="hpri_hwb_store"):
        _lib.call("hpri_hwb_store", null, 0, null, 0, 10, 8, 0, 8, 8, null)


def test_gathers_reject_bad_arguments_without_launch():
    from hyperpri_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(4096)
    ok = dict(slots=3, Hs=12, Ws=20, cs=8, N=2, h=12, w=20)

    def cube(cache=one, dt=0, table=one, dst=one, **kw):
        a = dict(ok, **kw)
        return lib.hpri_cube_gather(cache, dt, a["slots"], a["Hs"], a["Ws"], a["cs"], table, a["N"], a["h"], a["w"], dst, null)

    def mask(masks=one, table=one, dst=one, **kw):
        a = dict(ok, **kw)
        return lib.hpri_mask_gather(masks, a["slots"], a["Hs"], a["Ws"], table, a["N"], a["h"], a["w"], dst, null)
    for fn in (cube, mask):
        assert fn(null) == -1 and b"null" in lib.hpri_last_error()
        assert fn(table=null) == -1
        assert fn(dst=null) == -1
        assert fn(h=13) == -1 and b"window" in lib.hpri_last_error()       # a window outside the frame
        assert fn(w=21) == -1 and b"window" in lib.hpri_last_error()
        assert fn(h=0) == -1
        assert fn(slots=0) == -1
        assert fn(N=0) == -1
    assert cube(cs=12) == -1 and b"multiple of 8" in lib.hpri_last_error()  # unaligned channel stride
    assert cube(cs=4) == -1
    assert cube(dt=2) == -1
    assert cube(cache=ctypes.c_void_p(4100)) == -1                          # not 16-byte aligned
    assert cube(table=ctypes.c_void_p(4100)) == -1


def test_cache_needs_a_rocm_device():
    import hyperpri_amd as H
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.CubeCache(4, 12, 20, 9, device="cpu")
    with pytest.raises(ValueError, match="band range"):
        H.CubeCache(4, 12, 20, 9, hsi_lo=5, hsi_hi=12, device="cpu")
    assert H.CubeCache.planned_bytes(45, 608, 968, 238) == 45 * 608 * 968 * (240 * 4 + 1)
    assert H.CubeCache.planned_bytes(45, 608, 968, 238, torch.float16) == 45 * 608 * 968 * (240 * 2 + 1)


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def test_planner_is_deterministic_and_follows_the_documented_draws():
    from hyperpri_amd.cache import plan_epoch
    kw = dict(patch=(32, 48), shuffle=True, random_crop=True, flips=True)
    a = plan_epoch(45, 2, (608, 968), generator=_gen(7), **kw)
    b = plan_epoch(45, 2, (608, 968), generator=_gen(7), **kw)
    assert torch.equal(a.order, b.order) and torch.equal(a.table, b.table) and a.batches == b.batches
    c = plan_epoch(45, 2, (608, 968), generator=_gen(8), **kw)
    assert not torch.equal(a.table, c.table)
    # the documented draw order, restated: randperm, top, left, flip_h, flip_w -- all over n, from one generator
    g = _gen(7)
    order = torch.randperm(45, generator=g)
    top = torch.randint(0, 608 - 32 + 1, (45,), generator=g)
    left = torch.randint(0, 968 - 48 + 1, (45,), generator=g)
    fh = torch.randint(0, 2, (45,), generator=g)
    fw = torch.randint(0, 2, (45,), generator=g)
    assert torch.equal(a.order, order)
    assert a.table.dtype == torch.int32 and tuple(a.table.shape) == (45, 4)
    assert torch.equal(a.table.long(), torch.stack([order, top, left, fh + 2 * fw], 1))
    assert a.window == (32, 48)
    # two epochs from ONE generator differ
    g = _gen(7)
    e1 = plan_epoch(45, 2, (608, 968), generator=g, **kw)
    e2 = plan_epoch(45, 2, (608, 968), generator=g, **kw)
    assert not torch.equal(e1.order, e2.order) and not torch.equal(e1.table, e2.table)


def test_planner_sample_order_is_randperm_or_range():
    from hyperpri_amd.cache import plan_epoch
    for n in (1, 5, 44, 45):
        p = plan_epoch(n, 2, (36, 50), shuffle=True, generator=_gen(n))
        assert torch.equal(p.order, torch.randperm(n, generator=_gen(n)))
        q = plan_epoch(n, 2, (36, 50), shuffle=False, generator=_gen(n))
        assert torch.equal(q.order, torch.arange(n))
        assert torch.count_nonzero(q.table[:, 1:]) == 0                      # whole frame, no flips: top = left = flags = 0


@pytest.mark.parametrize("frame,patch", [((608, 968), (512, 512)), ((36, 50), (36, 50)), ((36, 50), 7), ((9, 14), (1, 14)),
                                         ((9, 14), (9, 1))])
@pytest.mark.parametrize("random_crop", [False, True])
def test_planned_windows_lie_inside_the_frame(frame, patch, random_crop):
    from hyperpri_amd.cache import plan_epoch
    H, W = frame
    p = plan_epoch(200, 3, frame, patch=patch, random_crop=random_crop, flips=True, generator=_gen(3))
    h, w = p.window
    t = p.table.long()
    assert bool((t[:, 1] >= 0).all()) and bool((t[:, 1] + h <= H).all())
    assert bool((t[:, 2] >= 0).all()) and bool((t[:, 2] + w <= W).all())
    assert bool((t[:, 3] >= 0).all()) and bool((t[:, 3] <= 3).all())
    if random_crop and h < H:
        assert len(set(t[:, 1].tolist())) > 1
    if not random_crop:
        assert set(t[:, 1].tolist()) == {(H - h) // 2} and set(t[:, 2].tolist()) == {(W - w) // 2}    # centred
    with pytest.raises(ValueError, match="does not fit"):
        plan_epoch(4, 2, frame, patch=(H + 1, W))


def test_every_index_appears_exactly_once_without_drop_last():
    from hyperpri_amd.cache import plan_epoch
    for n, bs in [(45, 2), (44, 2), (7, 3), (3, 5), (1, 1)]:
        p = plan_epoch(n, bs, (36, 50), generator=_gen(11))
        assert sorted(p.order.tolist()) == list(range(n))
        assert torch.equal(p.table[:, 0].long(), p.order)
        covered = [i for s, e in p.batches for i in range(s, e)]
        assert covered == list(range(n)) and all(0 < e - s <= bs for s, e in p.batches)
        assert len(p.batches) == (n + bs - 1) // bs
        d = plan_epoch(n, bs, (36, 50), drop_last=True, generator=_gen(11))
        assert len(d.batches) == n // bs and all(e - s == bs for s, e in d.batches)
        assert torch.equal(d.order, p.order[:n - n % bs])                      # the same draws, the tail dropped
