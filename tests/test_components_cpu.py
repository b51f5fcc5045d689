"""Connected components without a GPU (hyperpri_amd/components.py, csrc/components.hip): the numpy restatements of the contract
against scipy.ndimage where scipy imports and against hand-counted maps where it does not; the argument checks of the hpri_cc_*
entry points (an error code and a message, no launch); the "no CPU fallback" errors of the public functions.  Everything here is
an integer: every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

import _components_patterns as P
from hyperpri_amd import components as C


def test_exports_and_tile_constants():
    import hyperpri_amd as H
    from hyperpri_amd import _lib
    for name in ("label_components", "component_table", "clean_mask", "components_reference", "clean_reference", "clean_prediction",
                 "object_metrics", "TILE_H", "TILE_W", "CLEAN_LOGIT"):
        assert hasattr(H, name), name
    lib = _lib.load()
    assert (lib.hpri_cc_tile_h(), lib.hpri_cc_tile_w()) == (H.TILE_H, H.TILE_W) == (C.TILE_H, C.TILE_W)
    assert H.CLEAN_LOGIT == 16.0
    n = 3 * 76 * 121
    assert lib.hpri_cc_workspace_ints(3, 76, 121) == 4 * n + (n + 3) // 4 + 2 * 3 * 76
    assert lib.hpri_cc_workspace_ints(0, 76, 121) == 0
    # fp32 sigmoid(+-CLEAN_LOGIT) lies strictly inside (0, 1) and on the right side of every threshold in [1e-6, 1 - 1e-6]
    s = torch.sigmoid(torch.tensor([-H.CLEAN_LOGIT, H.CLEAN_LOGIT], dtype=torch.float32))
    assert 0.0 < float(s[0]) < 1e-6 and 1.0 - 1e-6 < float(s[1]) < 1.0
    assert not bool(s[0] > torch.tensor(1e-6, dtype=torch.float32)) and bool(s[1] > torch.tensor(1 - 1e-6, dtype=torch.float32))


def test_reference_on_hand_counted_maps():
    a = np.array([[1, 0, 0, 1, 1],
                  [0, 1, 0, 0, 0],
                  [0, 0, 0, 1, 0],
                  [1, 1, 0, 1, 0]], dtype=np.uint8)
    l4, c4 = C.components_reference(a, 4)
    assert c4.tolist() == [5]
    assert l4.tolist() == [[1, 0, 0, 2, 2], [0, 3, 0, 0, 0], [0, 0, 0, 4, 0], [5, 5, 0, 4, 0]]
    l8, c8 = C.components_reference(a, 8)
    assert c8.tolist() == [4]
    assert l8.tolist() == [[1, 0, 0, 2, 2], [0, 1, 0, 0, 0], [0, 0, 0, 3, 0], [4, 4, 0, 3, 0]]
    # two images never merge; labels restart per image
    s = np.ones((2, 2, 3), dtype=bool)
    l, c = C.components_reference(s, 4)
    assert c.tolist() == [1, 1] and l.max() == 1
    t = C.table_reference(l8, c8, truth=np.array([[1, 0, 0, 0, 0], [0, 2, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0.5, 0]]))
    assert t["area"].tolist() == [2, 2, 2, 2] and t["overlap"].tolist() == [2, 0, 0, 0]
    assert (t["y0"].tolist(), t["x0"].tolist(), t["y1"].tolist(), t["x1"].tolist()) == ([0, 0, 2, 3], [0, 3, 3, 0], [1, 0, 3, 3], [1, 4, 3, 1])
    with pytest.raises(ValueError, match="connectivity"):
        C.components_reference(a, 6)


def test_clean_reference_on_hand_counted_maps():
    a = np.array([[0, 0, 0, 0, 0, 0, 0],
                  [0, 1, 1, 1, 0, 0, 0],
                  [0, 1, 0, 1, 0, 1, 0],
                  [0, 1, 1, 0, 0, 0, 0],
                  [0, 0, 0, 0, 0, 1, 1]], dtype=np.uint8)
    # foreground 8: the ring is closed through the diagonal, the background is 4-connected, (2, 2) is a hole of one pixel
    m, st = C.clean_reference(a, min_area=2, max_hole=1, connectivity=8)
    assert st == {"components_removed": 1, "pixels_removed": 1, "holes_filled": 1, "pixels_filled": 1}
    want = a.copy(); want[2, 5] = 0; want[2, 2] = 1
    assert m.dtype == np.uint8 and np.array_equal(m, want)
    # foreground 4: the ring is open at its lower right corner, the background is 8-connected and (2, 2) leaks out through (3, 3)
    m, st = C.clean_reference(a, min_area=2, max_hole=1, connectivity=4)
    assert st == {"components_removed": 1, "pixels_removed": 1, "holes_filled": 0, "pixels_filled": 0}
    # neutral settings return the input
    m, st = C.clean_reference(a, 0, 0, 8)
    assert np.array_equal(m, a) and not any(st.values())
    with pytest.raises(ValueError, match="negative"):
        C.clean_reference(a, -1, 0, 8)


@pytest.mark.parametrize("shape", P.SHAPES)
def test_references_match_scipy(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    structures = {4: ndimage.generate_binary_structure(2, 1), 8: np.ones((3, 3), dtype=int)}
    h, w = shape
    for name, a in P.all_patterns(shape):
        for conn, structure in structures.items():
            labels, counts = P.reference(name, shape, conn)
            assert labels.dtype == np.int32 and counts.dtype == np.int32
            for n in range(P.N):
                want, cnt = ndimage.label(a[n], structure=structure)
                assert cnt == counts[n] and np.array_equal(want, labels[n]), (name, conn, n)
            # speck removal against scipy's labels and areas, hole filling against binary_fill_holes
            got, st = C.clean_reference(a, min_area=4, max_hole=0, connectivity=conn)
            removed = pixels = 0
            for n in range(P.N):
                lab, cnt = ndimage.label(a[n], structure=structure)
                area = np.bincount(lab.reshape(-1), minlength=cnt + 1)
                small = area < 4
                small[0] = False
                assert np.array_equal(got[n].astype(bool), a[n] & ~small[lab]), (name, conn, n)
                removed += int(small.sum()); pixels += int(area[small].sum())
            assert (st["components_removed"], st["pixels_removed"], st["holes_filled"]) == (removed, pixels, 0)
        filled, st = C.clean_reference(a, min_area=0, max_hole=h * w, connectivity=8)
        for n in range(P.N):
            assert np.array_equal(filled[n].astype(bool), ndimage.binary_fill_holes(a[n])), (name, n)
        assert st["pixels_filled"] == int(filled.sum()) - int(a.sum()) and st["pixels_removed"] == 0


def test_checkerboard_counts():
    for shape in P.SHAPES:
        a = P.pattern("checkerboard", shape)
        assert P.reference("checkerboard", shape, 4)[1].tolist() == [int(a[n].sum()) for n in range(P.N)]
        if min(shape) > 1:
            assert P.reference("checkerboard", shape, 8)[1].tolist() == [1, 1, 1]


def _host(n, dtype=ctypes.c_int):
    buf = (dtype * n)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_entry_points_reject_bad_arguments_without_launch():
    from hyperpri_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    keep, p = _host(64)                    # a HOST buffer: never dereferenced, every call below fails before its first launch
    ws = 10 ** 6

    def rejected(rc, word):
        assert rc == -1, rc
        assert word.encode() in lib.hpri_last_error(), lib.hpri_last_error()

    # hpri_cc_label(pred, kind, thr, is_logits, invert, N, h, w, connectivity, labels, counts, workspace, ws_ints, stream)
    rejected(lib.hpri_cc_label(null, 0, 0.5, 1, 0, 1, 2, 2, 8, p, p, p, ws, null), "null")
    rejected(lib.hpri_cc_label(p, 0, 0.5, 1, 0, 1, 2, 2, 8, null, p, p, ws, null), "null")
    rejected(lib.hpri_cc_label(p, 0, 0.5, 1, 0, 1, 2, 2, 8, p, null, p, ws, null), "null")
    rejected(lib.hpri_cc_label(p, 0, 0.5, 1, 0, 1, 2, 2, 8, p, p, null, ws, null), "null")
    for conn in (0, 1, 5, 6, 16, -4):
        rejected(lib.hpri_cc_label(p, 0, 0.5, 1, 0, 1, 2, 2, conn, p, p, p, ws, null), "connectivity")
    for N, h, w in ((0, 2, 2), (1, 0, 2), (1, 2, -1)):
        rejected(lib.hpri_cc_label(p, 0, 0.5, 1, 0, N, h, w, 8, p, p, p, ws, null), "sizes")
    rejected(lib.hpri_cc_label(p, 0, 0.5, 1, 0, 4, 32768, 16384, 8, p, p, p, ws, null), "2^31")
    rejected(lib.hpri_cc_label(p, 3, 0.5, 1, 0, 1, 2, 2, 8, p, p, p, ws, null), "pred_kind")
    assert lib.hpri_cc_label(p, 0, 0.5, 1, 0, 1, 2, 2, 8, p, p, p, 3, null) == -3 and b"workspace" in lib.hpri_last_error()
    # hpri_cc_measure(labels, counts, truth, truth_kind, N, h, w, table, table_rows, offsets, stream)
    rejected(lib.hpri_cc_measure(null, p, null, 0, 1, 2, 2, p, 4, p, null), "null")
    rejected(lib.hpri_cc_measure(p, null, null, 0, 1, 2, 2, p, 4, p, null), "null")
    rejected(lib.hpri_cc_measure(p, p, null, 0, 1, 2, 2, p, 4, null, null), "null")
    rejected(lib.hpri_cc_measure(p, p, null, 0, 1, 2, 2, null, 4, p, null), "table")
    rejected(lib.hpri_cc_measure(p, p, null, 0, 1, 2, 2, p, -1, p, null), "table")
    rejected(lib.hpri_cc_measure(p, p, null, 0, 1, 0, 2, p, 4, p, null), "sizes")
    rejected(lib.hpri_cc_measure(p, p, p, 7, 1, 2, 2, p, 4, p, null), "truth_kind")
    # hpri_cc_clean(pred, kind, thr, is_logits, N, h, w, connectivity, min_area, max_hole, out, out_logits, logit, stats, workspace, ws_ints, stream)
    rejected(lib.hpri_cc_clean(null, 0, 0.5, 1, 1, 2, 2, 8, 0, 0, p, null, 16.0, p, p, ws, null), "null")
    rejected(lib.hpri_cc_clean(p, 0, 0.5, 1, 1, 2, 2, 8, 0, 0, null, null, 16.0, p, p, ws, null), "null")
    rejected(lib.hpri_cc_clean(p, 0, 0.5, 1, 1, 2, 2, 8, 0, 0, p, null, 16.0, null, p, ws, null), "null")
    rejected(lib.hpri_cc_clean(p, 0, 0.5, 1, 1, 2, 2, 8, 0, 0, p, null, 16.0, p, null, ws, null), "null")
    rejected(lib.hpri_cc_clean(p, 0, 0.5, 1, 1, 2, 2, 6, 0, 0, p, null, 16.0, p, p, ws, null), "connectivity")
    rejected(lib.hpri_cc_clean(p, 0, 0.5, 1, 1, 2, 2, 8, -1, 0, p, null, 16.0, p, p, ws, null), "negative")
    rejected(lib.hpri_cc_clean(p, 0, 0.5, 1, 1, 2, 2, 8, 0, -1, p, null, 16.0, p, p, ws, null), "negative")
    rejected(lib.hpri_cc_clean(p, 0, 0.5, 1, 0, 2, 2, 8, 0, 0, p, null, 16.0, p, p, ws, null), "sizes")
    with pytest.raises(RuntimeError, match="cc_clean"):
        _lib.call("hpri_cc_clean", p, 0, 0.5, 1, 1, 2, 2, 8, 0, -1, p, null, 16.0, p, p, ws, null)
    del keep


def test_cpu_tensors_fail_loudly():
    import hyperpri_amd as H
    x = torch.zeros(2, 4, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.label_components(x, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.label_components(x.to(torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.clean_mask(x, 0.5, min_area=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.component_table(torch.zeros(2, 4, 5, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    pred = H.SplitPrediction(torch.zeros(40), torch.zeros(40), [0, 20, 40], [(4, 5), (4, 5)], ["a", "b"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.clean_prediction(pred, 0.5, min_area=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.object_metrics(pred, 0.5)


def test_python_argument_checks():
    import hyperpri_amd as H
    pred = H.SplitPrediction(torch.zeros(40), torch.zeros(40), [0, 20, 40], [(4, 5), (4, 5)], ["a", "b"])
    with pytest.raises(ValueError, match="connectivity"):
        H.label_components(torch.zeros(2, 4, 5), 0.5, connectivity=6)
    with pytest.raises(ValueError, match="negative"):
        H.clean_mask(torch.zeros(2, 4, 5), 0.5, min_area=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.clean_prediction(pred, 0.5, min_area=-1)
    from hyperpri_amd.evaluate import _size_groups
    mixed = H.SplitPrediction(torch.zeros(52), torch.zeros(52), [0, 20, 40, 46, 52], [(4, 5), (4, 5), (2, 3), (3, 2)], list("abcd"))
    assert _size_groups(mixed) == [(0, 2), (2, 3), (3, 4)]
