"""Connected components on the device (hyperpri_amd/components.py, csrc/components.hip) against the numpy restatements of the
contract (``components_reference``, ``table_reference``, ``clean_reference``; tests/test_components_cpu.py holds those against
scipy).  Labels, counts, areas, boxes, overlaps, masks and counters are integers: every comparison is EXACT, there is no tolerance.

Wherever logits are thresholded they are built so that every fp32 sigmoid stays at least 1e-5 away from the threshold
(``_logits_clear_of`` / ``_logits_for``): the one or two ulp between the device's and the host's expf cannot change a decision.
Needs a real MI355X."""
import os

import numpy as np
import pytest
import torch

import _components_patterns as P
from hyperpri_amd import components as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TABLE_SHAPES = [(9, 13), (C.TILE_H + 5, 2 * C.TILE_W - 7), (76, 121)]


def _logits_clear_of(seed, shape, thr):
    """Logits in (-3, 3) whose fp32 sigmoid stays 1e-5 away from ``thr``: any that come closer are moved."""
    x = torch.from_numpy(np.random.RandomState(seed).rand(*shape).astype(np.float32)) * 6 - 3
    near = (torch.sigmoid(x) - thr).abs() < 1e-5
    x[near] += 0.01
    assert not bool(((torch.sigmoid(x) - thr).abs() < 1e-5).any())
    return x


def _logits_for(a, seed, thr):
    """Logits whose decision ``sigmoid(x) > thr`` is the boolean map ``a``, every sigmoid at least 1e-5 away from ``thr``."""
    u = torch.from_numpy(np.random.RandomState(seed).rand(*a.shape).astype(np.float32))
    centre = float(np.log(thr / (1 - thr)))
    x = centre + torch.where(torch.from_numpy(np.array(a)), 0.1 + 3 * u, -(0.1 + 3 * u))
    s = torch.sigmoid(x)
    assert not bool(((s - thr).abs() < 1e-5).any()) and np.array_equal((s > thr).numpy(), a)
    return x


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint8)).to(DEV)


def _assert_raster_order(labels, counts):
    """Labels 1..count appear in raster order of their first pixel (checked without the oracle)."""
    for n in range(labels.shape[0]):
        flat = labels[n].reshape(-1)
        vals, first = np.unique(flat[flat > 0], return_index=True)
        assert vals.tolist() == list(range(1, int(counts[n]) + 1)), n
        assert np.all(np.diff(first) > 0), n


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", P.SHAPES)
def test_labels_match_the_reference(shape, conn):
    import hyperpri_amd as H
    side = torch.cuda.Stream(device=DEV)
    for k, (name, a) in enumerate(P.all_patterns(shape)):
        want_l, want_c = P.reference(name, shape, conn)
        dev = _u8(a)
        labels, counts = H.label_components(dev, connectivity=conn)
        assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and labels.is_cuda
        got_l, got_c = labels.cpu().numpy(), counts.cpu().numpy()
        assert np.array_equal(got_c, want_c), (name, got_c, want_c)
        assert np.array_equal(got_l, want_l), name
        _assert_raster_order(got_l, got_c)
        again = H.label_components(dev, connectivity=conn)                       # a second run: bit-identical
        assert torch.equal(again[0], labels) and torch.equal(again[1], counts), name
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                                            # a non-default stream: bit-identical
            other = H.label_components(dev, connectivity=conn)
        side.synchronize()
        assert torch.equal(other[0], labels) and torch.equal(other[1], counts), name
        # the fp32 / threshold forms of the same decision, bool input and invert
        thr = (0.5, 0.3, 0.77)[k % 3]
        x = _logits_for(a, 17 + k, thr).to(DEV)
        for form in (H.label_components(x, thr, connectivity=conn),
                     H.label_components(torch.sigmoid(x), thr, is_logits=False, connectivity=conn),
                     H.label_components(torch.from_numpy(np.array(a)).to(DEV), connectivity=conn),
                     H.label_components(_u8(~a), connectivity=conn, invert=True),
                     H.label_components(-x, 1 - thr, connectivity=conn, invert=True) if thr == 0.5 else None):
            if form is not None:
                assert torch.equal(form[0], labels) and torch.equal(form[1], counts), name
        if name == "checkerboard":
            assert got_c.tolist() == [int(a[n].sum()) for n in range(P.N)] if conn == 4 or min(shape) == 1 else got_c.tolist() == [1, 1, 1]


def test_images_never_merge():
    import hyperpri_amd as H
    a = np.zeros((3, 5, 70), dtype=bool)
    a[0, -1, :] = True
    a[1, 0, :] = True
    for conn in (4, 8):
        labels, counts = H.label_components(_u8(a), connectivity=conn)
        assert counts.tolist() == [1, 1, 0]
        assert np.array_equal(labels.cpu().numpy(), a.astype(np.int32))
    single, c1 = H.label_components(_u8(a[0]), connectivity=8)                   # a (h, w) map is one image
    assert tuple(single.shape) == (1, 5, 70) and c1.tolist() == [1]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", TABLE_SHAPES)
def test_component_table_matches_numpy(shape, conn):
    import hyperpri_amd as H
    for k, d in enumerate(P.DENSITIES):
        name = f"noise_{d}"
        a = P.pattern(name, shape)
        want_l, want_c = P.reference(name, shape, conn)
        truth = np.random.RandomState(50 + k).rand(*a.shape) < 0.3
        labels, counts = H.label_components(_u8(a), connectivity=conn)
        want = C.table_reference(want_l, want_c, truth)
        for tr in (torch.from_numpy(truth.astype(np.float32) * (k + 1)).to(DEV), _u8(truth), torch.from_numpy(truth).to(DEV)):
            got = H.component_table(labels, counts, truth=tr)
            assert sorted(got) == sorted(want)
            for key in want:
                assert isinstance(got[key], np.ndarray) and np.array_equal(got[key], want[key]), (name, key)
        bare = H.component_table(labels, counts)
        assert "overlap" not in bare and np.array_equal(bare["area"], want["area"])
        # fractions truncate toward zero like every mask of the tail: int(0.5) == 0 is no overlap
        half = H.component_table(labels, counts, truth=torch.full(a.shape, 0.5, device=DEV))
        assert not half["overlap"].any()
    empty = H.component_table(*H.label_components(_u8(np.zeros((2, 4, 5), dtype=bool))))
    assert all(len(v) == 0 for v in empty.values())


def _clean_both(a, min_area, max_hole, conn):
    import hyperpri_amd as H
    mask, stats = H.clean_mask(_u8(a), None, min_area=min_area, max_hole=max_hole, connectivity=conn)
    assert mask.dtype == torch.uint8 and mask.is_cuda
    want, want_stats = C.clean_reference(a, min_area, max_hole, conn)
    got = mask.cpu().numpy().reshape(want.shape)
    assert np.array_equal(got, want), (min_area, max_hole, conn)
    assert stats == want_stats, (stats, want_stats)
    return got, stats


def test_min_area_boundary():
    a = np.zeros((2, 12, 70), dtype=bool)
    a[0, 2, 3:8] = True             # 5 pixels: stays at min_area = 5
    a[0, 6, 3:7] = True             # 4 pixels: goes
    a[1, 1:3, 62:66] = True         # 8 pixels astride a tile edge: stays
    a[1, 8, 63:67] = True           # 4 pixels astride a tile edge: goes
    a[1, 10, 0] = True              # 1 pixel: goes
    for conn in (4, 8):
        got, stats = _clean_both(a, 5, 0, conn)
        assert got[0, 2, 3:8].all() and not got[0, 6].any() and got[1, 1:3, 62:66].all() and not got[1, 8].any() and not got[1, 10].any()
        assert stats == {"components_removed": 3, "pixels_removed": 9, "holes_filled": 0, "pixels_filled": 0}


def test_max_hole_boundary_and_frame_edge():
    a = np.zeros((1, 40, 80), dtype=bool)
    a[0, 2:9, 2:9] = True
    a[0, 4, 4:7] = False            # a hole of 3 pixels: filled at max_hole = 3
    a[0, 28:36, 58:70] = True       # (astride both tile edges)
    a[0, 31:33, 63:65] = False      # a hole of 4 pixels: not filled
    a[0, 0:4, 20:25] = True
    a[0, 0:2, 22] = False           # 2 background pixels closed in by foreground and the frame's top edge: never a hole
    a[0, 20:25, 76:80] = True
    a[0, 22, 78:80] = False         # the same at the right edge
    for conn in (4, 8):
        got, stats = _clean_both(a, 0, 3, conn)
        assert got[0, 4, 4:7].all() and not got[0, 31:33, 63:65].any() and not got[0, 0:2, 22].any() and not got[0, 22, 78:80].any()
        assert stats == {"components_removed": 0, "pixels_removed": 0, "holes_filled": 1, "pixels_filled": 3}
        got, stats = _clean_both(a, 0, 40 * 80, conn)                            # unbounded: the frame-edge pockets still stay
        assert got[0, 31:33, 63:65].all() and not got[0, 0:2, 22].any() and not got[0, 22, 78:80].any()
        assert stats["holes_filled"] == 2 and stats["pixels_filled"] == 7


def test_diagonal_leak_is_a_hole_only_for_foreground_8():
    a = np.zeros((1, 8, 9), dtype=bool)
    a[0, 2:5, 3:6] = True
    a[0, 3, 4] = False              # the centre of a 3 x 3 block ...
    a[0, 4, 5] = False              # ... and its lower right corner: the centre touches the outside only diagonally
    got, stats = _clean_both(a, 0, 5, 8)        # foreground 8, background 4: the centre is closed in
    assert got[0, 3, 4] == 1 and got[0, 4, 5] == 0 and stats["holes_filled"] == 1
    got, stats = _clean_both(a, 0, 5, 4)        # foreground 4, background 8: it leaks out through the corner
    assert got[0, 3, 4] == 0 and stats["holes_filled"] == 0


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", TABLE_SHAPES)
def test_clean_matches_the_reference(shape, conn):
    import hyperpri_amd as H
    h, w = shape
    for k, name in enumerate(("noise_0.3", "noise_0.5", "noise_0.593", "noise_0.8", "spiral", "stripes_both", "checkerboard", "full", "empty")):
        a = P.pattern(name, shape)
        for min_area, max_hole in ((4, 3), (0, 0), (0, h * w), (h * w + 1, 1)):
            got, _ = _clean_both(a, min_area, max_hole, conn)
            if (min_area, max_hole) == (0, 0):
                assert np.array_equal(got, a.astype(np.uint8))                    # the neutral settings change nothing
            if (min_area, max_hole) == (0, h * w) and conn == 8:
                try:
                    from scipy import ndimage
                except ImportError:
                    continue
                for n in range(P.N):
                    assert np.array_equal(got[n].astype(bool), ndimage.binary_fill_holes(a[n])), (name, n)
        # the fp32 / threshold form takes the same decision; a second run is bit-identical; the counters accumulate
        thr = (0.5, 0.25)[k % 2]
        x = _logits_for(a, 90 + k, thr).to(DEV)
        m1, s1 = H.clean_mask(x, thr, min_area=4, max_hole=3, connectivity=conn)
        m2, s2 = H.clean_mask(_u8(a), None, min_area=4, max_hole=3, connectivity=conn)
        assert torch.equal(m1, m2) and s1 == s2


def _split(thr):
    """A synthetic stored split of two sizes (three batches) with its images: no network."""
    import hyperpri_amd as H
    sizes = [(37, 70)] * 3 + [(20, 33)] * 2
    names = [f"img{i}" for i in range(len(sizes))]
    offsets = [0]
    for h, w in sizes:
        offsets.append(offsets[-1] + h * w)
    logits = _logits_clear_of(5, (offsets[-1],), thr)
    masks = torch.from_numpy((np.random.RandomState(6).rand(offsets[-1]) < 0.45).astype(np.float32))
    for i, (h, w) in enumerate(sizes):          # truth in blobs rather than salt and pepper: 3 x 3 blocks
        m = np.kron(np.random.RandomState(60 + i).rand((h + 2) // 3, (w + 2) // 3) < 0.3, np.ones((3, 3)))[:h, :w]
        masks[offsets[i]:offsets[i + 1]] = torch.from_numpy(m.astype(np.float32).reshape(-1))
    pred = H.SplitPrediction(logits.to(DEV), masks.to(DEV), offsets, sizes, names)
    rng = np.random.RandomState(8)
    batches = []
    for lo, hi in ((0, 2), (2, 3), (3, 5)):
        h, w = sizes[lo]
        batches.append({"image": torch.from_numpy(rng.rand(hi - lo, 3, h, w).astype(np.float32)).to(DEV),
                        "mask": masks[offsets[lo]:offsets[hi]].reshape(hi - lo, 1, h, w).to(DEV), "index": names[lo:hi]})
    return pred, batches


def _host_decisions(pred, thr):
    x, m = pred.logits.cpu(), pred.masks.cpu()
    out = []
    for i, (h, w) in enumerate(pred.sizes):
        a, b = pred.offsets[i], pred.offsets[i + 1]
        out.append(((torch.sigmoid(x[a:b]) > thr).numpy().reshape(h, w), (m[a:b].to(torch.int32) != 0).numpy().reshape(h, w)))
    return out


def _host_counts(decisions):
    tp = sum(int((s & g).sum()) for s, g in decisions)
    fp = sum(int((s & ~g).sum()) for s, g in decisions)
    fn = sum(int((~s & g).sum()) for s, g in decisions)
    tn = sum(int((~s & ~g).sum()) for s, g in decisions)
    return {"tp": tp, "fp": fp, "fn": fn, "tn": tn}


def test_clean_prediction_end_to_end(tmp_path):
    import hyperpri_amd as H
    thr = 0.6
    pred, batches = _split(thr)
    raw = _host_decisions(pred, thr)
    assert H.test_net(pred, thr)["counts"] == _host_counts(raw)
    # neutral settings: the decisions of the raw prediction
    neutral, stats = H.clean_prediction(pred, thr)
    assert not any(stats.values())
    assert neutral.offsets == pred.offsets and neutral.sizes == pred.sizes and neutral.names == pred.names and neutral.masks is pred.masks
    assert set(np.unique(neutral.logits.cpu().numpy()).tolist()) == {-H.CLEAN_LOGIT, H.CLEAN_LOGIT}
    assert H.test_net(neutral, thr)["counts"] == H.test_net(pred, thr)["counts"]
    assert torch.equal(neutral.logits > 0, torch.sigmoid(pred.logits) > thr)
    # min_area = 4, max_hole = 3 against clean_reference on the host, for both connectivities
    for conn in (8, 4):
        cleaned, stats = H.clean_prediction(pred, thr, min_area=4, max_hole=3, connectivity=conn)
        want, want_stats = [], dict.fromkeys(C.STAT_NAMES, 0)
        for s, g in raw:
            m, st = C.clean_reference(s, 4, 3, conn)
            want.append((m.astype(bool), g))
            for key in st:
                want_stats[key] += st[key]
        assert stats == want_stats and stats["components_removed"] > 0 and stats["holes_filled"] > 0
        for t in (thr, 1e-6, 0.5, 1 - 1e-6):                                      # any threshold reproduces the cleaned decision
            assert H.test_net(cleaned, t)["counts"] == _host_counts(want), t
        counts = H.SegCounts(0.9)
        counts.update(cleaned.logits, cleaned.masks)
        got = counts.compute()
        assert {k: int(got[k]) for k in ("tp", "fp", "fn", "tn")} == _host_counts(want)
    # (conn == 4 from here on) the class maps and the pictures of the cleaned prediction
    i = 0
    for batch in batches:
        n = int(batch["image"].shape[0])
        a, b = cleaned.offsets[i], cleaned.offsets[i + n]
        rgb, classes = H.color_segmaps(batch["image"], cleaned.logits[a:b], cleaned.masks[a:b], thr, return_classes=True)
        for j in range(n):
            s, g = want[i + j]
            assert np.array_equal(classes[j].cpu().numpy(), s.astype(np.uint8) + 2 * g.astype(np.uint8)), i + j
        batch["rgb"] = rgb.cpu().numpy()
        i += n
    paths = H.write_segmaps(str(tmp_path / "maps"), cleaned, [{k: v for k, v in b.items() if k != "rgb"} for b in batches], thr)
    assert [os.path.basename(p).split("_seg")[0] for p in paths] == cleaned.names
    pictures = np.concatenate([b["rgb"].reshape(-1, 3) for b in batches])
    for i, p in enumerate(paths):
        if p.endswith(".npy"):
            pic = np.load(p)
        else:
            from PIL import Image
            pic = np.asarray(Image.open(p).convert("RGB"))
        a, b = cleaned.offsets[i], cleaned.offsets[i + 1]
        assert np.array_equal(pic.reshape(-1, 3), pictures[a:b]), p


def _host_object_metrics(decisions, conn):
    tot = {"pred_objects": 0, "pred_objects_hit": 0, "truth_objects": 0, "truth_objects_hit": 0}
    pred_areas, truth_areas = [], []
    for s, g in decisions:
        ls, cs = C.components_reference(s, conn)
        lg, cg = C.components_reference(g, conn)
        ts, tg = C.table_reference(ls, cs, g), C.table_reference(lg, cg, s)
        tot["pred_objects"] += int(cs[0]); tot["pred_objects_hit"] += int((ts["overlap"] > 0).sum())
        tot["truth_objects"] += int(cg[0]); tot["truth_objects_hit"] += int((tg["overlap"] > 0).sum())
        pred_areas.append(ts["area"].tolist()); truth_areas.append(tg["area"].tolist())
    return tot, pred_areas, truth_areas


@pytest.mark.parametrize("conn,min_area", [(8, 0), (4, 0), (8, 5)])
def test_object_metrics_match_a_host_count(conn, min_area):
    import hyperpri_amd as H
    thr = 0.6
    pred, _ = _split(thr)
    decisions = _host_decisions(pred, thr)
    if min_area:
        decisions = [(C.clean_reference(s, min_area, 0, conn)[0].astype(bool), g) for s, g in decisions]
    tot, pred_areas, truth_areas = _host_object_metrics(decisions, conn)
    got = H.object_metrics(pred, thr, connectivity=conn, min_area=min_area)
    for key, v in tot.items():
        assert got[key] == v, (key, got[key], v)
    assert got["pred_areas"] == pred_areas and got["truth_areas"] == truth_areas
    p, r = tot["pred_objects_hit"] / tot["pred_objects"], tot["truth_objects_hit"] / tot["truth_objects"]
    assert got["object_precision"] == p and got["object_recall"] == r and got["object_f1"] == 2 * p * r / (p + r)
    assert 0 < tot["pred_objects_hit"] < tot["pred_objects"] and 0 < tot["truth_objects_hit"] <= tot["truth_objects"]
    # nothing predicted: zero denominators are NaN, as the pixel metrics
    nothing = H.SplitPrediction(torch.full_like(pred.logits, -5.0), pred.masks, pred.offsets, pred.sizes, pred.names)
    got = H.object_metrics(nothing, thr, connectivity=conn)
    assert got["pred_objects"] == 0 and got["truth_objects_hit"] == 0 and np.isnan(got["object_precision"]) and got["object_recall"] == 0.0
    assert np.isnan(got["object_f1"])
