"""Test-time augmentation, the host side (hyperpri_amd/tta.py, cache.view_warp_entries) and the argument checks of hpri_tta_merge:
no GPU needed."""
import ctypes

import numpy as np
import pytest
import torch


def test_views_against_numpy_and_their_index_maps():
    import hyperpri_amd as H
    from hyperpri_amd import tta
    assert H.VIEW_NAMES == ("id", "flip_h", "flip_w", "rot180", "rot90", "rot270", "transpose", "antitranspose")
    assert [tta.view_code(v) for v in H.VIEW_NAMES] == list(range(8))
    a = np.arange(15).reshape(3, 5)
    want = {"id": a, "flip_h": a[::-1], "flip_w": a[:, ::-1], "rot180": a[::-1, ::-1], "rot90": np.rot90(a, 1), "rot270": np.rot90(a, 3),
            "transpose": a.T, "antitranspose": np.rot90(a, 2).T}
    seen = []
    for v in H.VIEW_NAMES:
        got = H.apply_view(a, v)
        assert got.shape == tta.view_shape(v, 3, 5) == ((5, 3) if tta.view_transposes(v) else (3, 5))
        assert np.array_equal(got, want[v]), v
        assert np.array_equal(H.invert_view(got, v), a), v
        rows, cols = tta.forward_index(v, 3, 5)
        assert np.array_equal(got, a[rows, cols]), v
        rows, cols = tta.inverse_index(v, 3, 5)
        assert rows.shape == (3, 5) and np.array_equal(got[rows, cols], a), v
        t = H.apply_view(torch.from_numpy(a.copy()), v)                 # tensors: the same views, over the last two axes
        assert np.array_equal(t.numpy(), got) and np.array_equal(H.invert_view(t, v).numpy(), a), v
        batch = np.stack([a, a + 100])[None]
        assert np.array_equal(H.apply_view(batch, v)[0, 1], got + 100), v
        seen.append(got)
    assert np.array_equal(H.apply_view(torch.from_numpy(a.copy()), "rot90").numpy(), torch.rot90(torch.from_numpy(a.copy()), 1, (-2, -1)).numpy())
    for i in range(8):
        for j in range(i + 1, 8):
            assert seen[i].shape != seen[j].shape or not np.array_equal(seen[i], seen[j]), (i, j)
    with pytest.raises(ValueError, match="unknown view"):
        H.apply_view(a, "rot45")


def test_tta_validation():
    import hyperpri_amd as H
    t = H.TTA()
    assert t.views == ("id", "flip_w", "flip_h", "rot180") and t.merge == "prob" and t.spread is False and t.mode == 1
    assert H.TTA(views=["rot90", "id"], merge="logit").codes == [4, 0] and H.TTA(merge="logit").mode == 0
    assert len(H.TTA(views=H.VIEW_NAMES).views) == 8
    with pytest.raises(ValueError, match="1 to 8"):
        H.TTA(views=())
    with pytest.raises(ValueError, match="1 to 8"):
        H.TTA(views=H.VIEW_NAMES + ("id",))
    with pytest.raises(ValueError, match="unknown view"):
        H.TTA(views=("id", "rot45"))
    with pytest.raises(ValueError, match="twice"):
        H.TTA(views=("id", "flip_w", "id"))
    with pytest.raises(ValueError, match="merge"):
        H.TTA(merge="median")


def test_merge_launcher_rejects_bad_arguments_without_a_launch():
    from hyperpri_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    some = ctypes.c_void_p(4096)                                        # never dereferenced: every call below fails its checks

    def call(ptrs, codes, V, N=1, K=1, h=4, w=4, mode=0, out=some, views=True, code_array=True):
        p = (ctypes.c_void_p * 9)(*ptrs)
        c = (ctypes.c_int * 9)(*codes)
        rc = lib.hpri_tta_merge(ctypes.cast(p, ctypes.c_void_p) if views else null, ctypes.cast(c, ctypes.c_void_p) if code_array else null,
                                V, N, K, h, w, mode, out, null, null)
        return rc, lib.hpri_last_error()
    ok_p, ok_c = [4096] * 9, [0] * 9
    for kw in (dict(views=False), dict(code_array=False), dict(out=null)):
        rc, msg = call(ok_p, ok_c, 1, **kw)
        assert rc == -1 and b"null" in msg, kw
    rc, msg = call([4096, 0] + [4096] * 7, ok_c, 2)
    assert rc == -1 and b"null view" in msg
    for V in (0, 9):
        rc, msg = call(ok_p, ok_c, V)
        assert rc == -1 and b"views" in msg, V
    for K in (0, 65):
        rc, msg = call(ok_p, ok_c, 1, K=K)
        assert rc == -1 and b"classes" in msg, K
    rc, msg = call(ok_p, [0, 8] + [0] * 7, 2)
    assert rc == -1 and b"view code" in msg
    rc, msg = call(ok_p, [-1] + [0] * 8, 1)
    assert rc == -1 and b"view code" in msg
    for kw in (dict(h=0), dict(w=0), dict(h=-3), dict(w=-1), dict(N=0)):
        rc, msg = call(ok_p, ok_c, 1, **kw)
        assert rc == -1 and b"sizes" in msg, kw
    rc, msg = call(ok_p, ok_c, 1, mode=2)
    assert rc == -1 and b"mode" in msg
    with pytest.raises(RuntimeError, match="tta_merge"):
        _lib.call("hpri_tta_merge", null, null, 1, 1, 1, 4, 4, 0, null, null, null)


def _warp_coordinates(entry, window):
    """What cache_warp.hip computes for every output pixel of ``window`` = (h, w) from one entry, in numpy fp32 (fma(a, b, c) with
    a in {0, +-1} is the product, exact, plus c: one rounding either way)."""
    f = entry[4:12].view(np.float32)
    a00, a01, cx, a10, a11, cy, gain, offset = (np.float32(v) for v in f)
    h, w = window
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    u = x.astype(np.float32) - np.float32(0.5) * np.float32(w - 1)
    v = y.astype(np.float32) - np.float32(0.5) * np.float32(h - 1)
    sx = a00 * u + (a01 * v + cx)
    sy = a10 * u + (a11 * v + cy)
    assert sx.dtype == np.float32 and sy.dtype == np.float32
    return sx, sy, float(gain), float(offset)


@pytest.mark.parametrize("frame", [(13, 22), (12, 21)])
def test_quarter_turn_warp_entries_are_exact(frame):
    from hyperpri_amd import tta
    from hyperpri_amd.cache import view_warp_entries
    H_, W_ = frame
    for view in ("rot90", "rot270", "transpose", "antitranspose"):
        e = view_warp_entries([2, 0], view, frame).numpy()
        assert e.shape == (2, 16) and e.dtype == np.int32
        assert e[:, 0].tolist() == [2, 0] and not e[:, 1:4].any() and not e[:, 12:].any()        # slot; no band dropped
        for row in e:
            m = row[[4, 5, 7, 8]].view(np.float32)
            assert all(float(v) in (0.0, 1.0, -1.0) for v in m) and sorted(abs(m).tolist()) == [0.0, 0.0, 1.0, 1.0]
            assert not np.signbit(m[m == 0]).any()
            assert row[6:7].view(np.float32)[0] == np.float32((W_ - 1) / 2) and row[9:10].view(np.float32)[0] == np.float32((H_ - 1) / 2)
            sx, sy, gain, offset = _warp_coordinates(row, (W_, H_))
            assert gain == 1.0 and offset == 0.0
            rows, cols = tta.forward_index(view, H_, W_)                # view[i, j] = frame[rows, cols]
            assert rows.shape == (W_, H_)
            assert np.array_equal(sy, rows.astype(np.float32)) and np.array_equal(sx, cols.astype(np.float32)), view
    with pytest.raises(ValueError, match="swap"):
        view_warp_entries([0], "flip_h", frame)


def test_merge_reference():
    import hyperpri_amd as H
    rng = np.random.default_rng(5)
    x = (4 * rng.standard_normal((2, 1, 3, 5))).astype(np.float32)
    out, sp = H.tta_merge_reference([x], ["id"], "logit", dtype=np.float32)
    assert out.dtype == np.float32 and np.array_equal(out, x) and sp is None
    out, _ = H.tta_merge_reference([x], ["id"], "logit")
    assert out.dtype == np.float64 and np.array_equal(out, x.astype(np.float64))
    # a pair (s, -s): mean probability 1/2, logit 0, spread |p - 1/2|
    s = 4 * rng.standard_normal((2, 1, 3, 5))
    out, sp = H.tta_merge_reference([s, -s], ["id", "id"], "prob", spread=True)
    assert np.abs(out).max() < 1e-15
    np.testing.assert_allclose(sp, np.abs(1 / (1 + np.exp(-s[:, 0])) - 0.5), rtol=0, atol=1e-15)
    # the same through views: the network's output for a view is the view of its output for the frame
    out2, sp2 = H.tta_merge_reference([H.apply_view(s, "rot90"), H.apply_view(-s, "antitranspose")], ["rot90", "antitranspose"], "prob", True)
    assert np.array_equal(out2, out) and np.array_equal(sp2, sp)
    # softmax mode: log-probabilities
    k = 4 * rng.standard_normal((2, 3, 3, 5))
    views = ("id", "flip_h", "rot270")
    out, sp = H.tta_merge_reference([H.apply_view(k + i, v) for i, v in enumerate(views)], views, "prob", spread=True)
    assert out.shape == (2, 3, 3, 5) and sp.shape == (2, 3, 5)
    np.testing.assert_allclose(np.exp(out).sum(axis=1), 1.0, rtol=0, atol=1e-14)
    e = np.exp(k - k.max(1, keepdims=True))
    np.testing.assert_allclose(np.exp(out), e / e.sum(1, keepdims=True), rtol=1e-13)          # (a shift per view changes no softmax)
    assert not sp.any()
    # the multi-class spread: one of two views votes for another class everywhere
    a = np.zeros((1, 3, 2, 2)); a[:, 0] = 3.0
    b = np.zeros((1, 3, 2, 2)); b[:, 2] = 1.0
    out, sp = H.tta_merge_reference([a, b], ("id", "flip_w"), "logit", spread=True)
    assert np.array_equal(out.argmax(1), np.zeros((1, 2, 2))) and np.array_equal(sp, np.full((1, 2, 2), 0.5))
    # the clamp keeps the logit finite, NaN goes through
    big = np.array([[[[200.0, -200.0, np.nan]]]])
    out, sp = H.tta_merge_reference([big], ["id"], "prob", spread=True)
    assert np.isfinite(out[0, 0, 0, :2]).all() and out[0, 0, 0, 0] > 87 and out[0, 0, 0, 1] < -87 and np.isnan(out[0, 0, 0, 2])
    with pytest.raises(ValueError):
        H.tta_merge_reference([x, x], ["id"], "prob")


def test_public_names_and_defaults():
    import inspect
    import hyperpri_amd as H
    for name in ("TTA", "VIEW_NAMES", "apply_view", "invert_view", "tta_merge_reference", "tta_merge", "write_spreadmaps"):
        assert hasattr(H, name), name
    assert inspect.signature(H.predict_split).parameters["tta"].default is None
    assert inspect.signature(H.evaluate_multiclass).parameters["tta"].default is None
    fields = list(H.SplitPrediction.__dataclass_fields__)
    assert fields[-1] == "spread" and H.SplitPrediction.__dataclass_fields__["spread"].default is None
    assert hasattr(H.CubeCache, "view") and hasattr(H.CubeCache, "epoch_views")
    with pytest.raises(TypeError, match="TTA"):
        H.predict_split(torch.nn.Identity(), [], tta="prob")
