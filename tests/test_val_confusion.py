"""Device-resident confusion matrix and native-space predictions (csrc/metrics.hip: et_val_confusion, et_val_predn;
efficientteacher_amd/val.py: ConfusionMatrix, native_predictions, coco_json_rows, run(confusion_matrix=, jdict=)).

* the numpy helper tests/val_confusion_ref.py is pinned on tests/golden/val_confusion.npz, which tools/make_val_confusion_golden.py
  made from the live reference (scale_coords, ConfusionMatrix.process_batch, save_one_json);
* the kernels against the golden and, for inputs the golden does not hold, against the helper: zero tolerance everywhere -- the
  decisions are fp32 comparisons, the counts integers, predn / xywh_tl a handful of fp32 operations in the reference's order.
"""
import inspect

import numpy as np
import pytest
import torch

from oracle import ref_loader
from tests import val_confusion_ref as cr
from tests import val_metrics_ref as vr
from tests.conftest import golden


def _gold():
    g = golden("val_confusion")
    nc, max_det, nh, nw = (int(v) for v in g["meta"])
    batches = [(g[f"dets{b}"], g[f"counts{b}"], g[f"targets{b}"], g[f"rows{b}"]) for b in range(int(g["nbatches"]))]
    return g, batches, nc, max_det, (nh, nw)


def _gold_jdict(g):
    ids = [int(i) if is_int else str(i) for i, is_int in zip(g["jd_image_id"], g["jd_id_is_int"])]
    return [{'image_id': i, 'category_id': int(c), 'bbox': [float(x) for x in b], 'score': float(s)}
            for i, c, b, s in zip(ids, g["jd_category_id"], g["jd_bbox"], g["jd_score"])]


def _feed(hip, batches, nc, net_hw, single_cls=False, **kw):
    from efficientteacher_amd.val import ConfusionMatrix
    cm = ConfusionMatrix(nc, device=hip.device, **kw)
    for dets, counts, targets, rows in batches:
        assert cm.update(hip.t(dets), hip.t(counts), hip.t(targets), hip.t(rows), net_hw, single_cls=single_cls) is None
    return cm


def _check(hip, batches, nc, net_hw, single_cls=False, **kw):
    """device matrix array_equal to the helper's"""
    cm = _feed(hip, batches, nc, net_hw, single_cls, **kw)
    want = cr.confusion_batches(batches, net_hw, nc, single_cls=single_cls, **kw)
    got = cm.matrix
    assert got.dtype == np.float64 and got.shape == (nc + 1, nc + 1)
    assert cm.matrix_device().dtype == torch.int32
    assert np.array_equal(got, want), (got, want)
    return cm, want


# ---- the helper is the reference ---------------------------------------------------------------------------------------
def test_helper_equals_golden():
    g, batches, nc, max_det, net_hw = _gold()
    conf, iou = (float(v) for v in g["thresholds"])
    m = cr.confusion_batches(batches, net_hw, nc, conf, iou)
    assert np.array_equal(m, g["matrix"])
    # every kind of cell is populated: diagonal, off-diagonal, background row (unmatched labels), background column
    assert np.trace(m[:nc, :nc]) > 0 and (m[:nc, :nc].sum() - np.trace(m[:nc, :nc])) > 0 and m[nc, :nc].sum() > 0 and m[:nc, nc].sum() > 0
    rows = []
    for b, (dets, counts, targets, shp) in enumerate(batches):
        predn, tl = cr.predn_batch(dets, counts, shp)
        assert predn.tobytes() == g[f"predn{b}"].tobytes() and tl.tobytes() == g[f"xywh_tl{b}"].tobytes()
        rows += cr.json_rows(predn, tl, counts, [_id(p) for p in g[f"paths{b}"]])
    assert rows == _gold_jdict(g)


def _id(path):
    from efficientteacher_amd.val import image_id_of_path
    return image_id_of_path(str(path))


# ---- kernels against the golden --------------------------------------------------------------------------------------------
def test_confusion_equals_golden(hip):
    g, batches, nc, max_det, net_hw = _gold()
    cm = _feed(hip, batches, nc, net_hw)
    assert np.array_equal(cm.matrix, g["matrix"])
    assert cm.matrix.dtype == np.float64
    again = _feed(hip, batches, nc, net_hw)
    assert torch.equal(cm.matrix_device(), again.matrix_device())
    # accumulated into, not cleared; reset clears
    for dets, counts, targets, rows in batches:
        cm.update(hip.t(dets), hip.t(counts), hip.t(targets), hip.t(rows), net_hw)
    assert np.array_equal(cm.matrix, 2 * g["matrix"])
    cm.reset()
    assert not cm.matrix.any()


def test_predn_and_json_equal_golden(hip):
    from efficientteacher_amd.val import coco_json_rows, native_predictions
    g, batches, nc, max_det, net_hw = _gold()
    jdict = []
    for b, (dets, counts, targets, rows) in enumerate(batches):
        predn, tl = native_predictions(hip.t(dets), hip.t(counts), hip.t(rows), net_hw)
        assert predn.shape == (dets.shape[0], max_det, 6) and tl.shape == (dets.shape[0], max_det, 4)
        assert predn.cpu().numpy().tobytes() == g[f"predn{b}"].tobytes()
        assert tl.cpu().numpy().tobytes() == g[f"xywh_tl{b}"].tobytes()
        jdict += coco_json_rows(predn, tl, hip.t(counts), [_id(p) for p in g[f"paths{b}"]], class_map=list(range(1000)))
    want = _gold_jdict(g)
    assert jdict == want
    assert any(isinstance(r["image_id"], int) for r in jdict) and any(isinstance(r["image_id"], str) for r in jdict)
    # a class map that is not the identity, and single_cls: class column zero
    dets, counts, targets, rows = batches[0]
    predn, tl = native_predictions(hip.t(dets), hip.t(counts), hip.t(rows), net_hw, single_cls=True)
    wp, wt = cr.predn_batch(dets, counts, rows, single_cls=True)
    assert predn.cpu().numpy().tobytes() == wp.tobytes() and tl.cpu().numpy().tobytes() == wt.tobytes()
    cmap = [90 - i for i in range(10)]
    predn, tl = native_predictions(hip.t(dets), hip.t(counts), hip.t(rows), net_hw)
    got = coco_json_rows(predn, tl, hip.t(counts), list(range(dets.shape[0])), class_map=cmap)
    assert [r["category_id"] for r in got] == [cmap[r["category_id"]] for r in want[:len(got)]]
    # the loader's python list of shapes gives the same rows as the device tensor
    ls = [((float(r[3]), float(r[4])), ((float(r[0]), float(r[0])), (float(r[1]), float(r[2])))) for r in rows]
    p2, t2 = native_predictions(hip.t(dets), hip.t(counts), ls, net_hw)
    assert torch.equal(p2, predn) and torch.equal(t2, tl)


# ---- edge cases against the helper -----------------------------------------------------------------------------------------
def test_empty_batch(hip):
    from efficientteacher_amd.val import coco_json_rows, native_predictions
    _, batches, nc, max_det, net_hw = _gold()
    empty = [(np.zeros((0, max_det, 6), np.float32), np.zeros(0, np.int32), np.zeros((0, 6), np.float32), np.zeros((0, 5), np.float32))]
    cm, _ = _check(hip, empty, nc, net_hw)
    assert not cm.matrix.any()
    d, c, t, r = empty[0]
    predn, tl = native_predictions(hip.t(d), hip.t(c), hip.t(r), net_hw)
    assert predn.shape == (0, max_det, 6) and tl.shape == (0, max_det, 4)
    assert coco_json_rows(predn, tl, hip.t(c), []) == []


def test_no_labels_anywhere(hip):
    _, batches, nc, max_det, net_hw = _gold()
    cm, _ = _check(hip, [(d, c, np.zeros((0, 6), np.float32), r) for d, c, t, r in batches], nc, net_hw)
    assert not cm.matrix.any()


def test_no_detections_anywhere(hip):
    """images without an NMS detection contribute nothing, not even their labels (val.py:347-350)"""
    _, batches, nc, max_det, net_hw = _gold()
    cm, _ = _check(hip, [(d, np.zeros_like(c), t, r) for d, c, t, r in batches], nc, net_hw)
    assert not cm.matrix.any()


def test_single_cls(hip):
    data = vr.synth(5, 12, 4, 1, 60, (384, 640))
    cm, want = _check(hip, data, 1, (384, 640), single_cls=True)
    assert want[0, 0] > 0
    # detections of other classes count as class 0 (val.py:353-354) when the labels are class 0
    data = vr.synth(6, 6, 3, 4, 60, (384, 640))
    data = [(d, c, np.concatenate((t[:, :1], np.zeros_like(t[:, 1:2]), t[:, 2:]), 1), r) for d, c, t, r in data]
    cm, want = _check(hip, data, 1, (384, 640), single_cls=True)
    assert want[0, 0] > 0


def test_classes_outside_the_matrix_are_not_counted(hip):
    data = vr.synth(16, 6, 3, 5, 60)
    _, want5 = _check(hip, data, 5, (512, 640))
    _, want3 = _check(hip, data, 3, (512, 640))                    # classes 3 and 4 fall outside
    assert want3.sum() < want5.sum() and want3.sum() > 0


def test_other_thresholds(hip):
    data = vr.synth(12, 10, 5, 4, 80)
    _, base = _check(hip, data, 4, (512, 640))
    _, a = _check(hip, data, 4, (512, 640), conf=0.6, iou_thres=0.7)
    _, b = _check(hip, data, 4, (512, 640), conf=0.001, iou_thres=0.2)
    assert not np.array_equal(a, base) and not np.array_equal(b, base)


def _one_pair(conf):
    """one image (identity letterbox), one label and one detection on the very same box, given confidence"""
    dets = np.zeros((1, 4, 6), np.float32)
    dets[0, 0] = [64, 32, 192, 160, conf, 1]                      # centre (128, 96), 128 x 128: exact in fp32 both ways
    targets = np.array([[0, 1, 128 / 256, 96 / 256, 128 / 256, 128 / 256]], np.float32)
    rows = np.array([[1, 0, 0, 256, 256]], np.float32)
    return [(dets, np.array([1], np.int32), targets, rows)]


def test_thresholds_are_strict(hip):
    nc, hw = 3, (256, 256)
    # IoU exactly 1.0: qualifies below 1.0, not at iou_thres = 1.0
    _, m = _check(hip, _one_pair(0.9), nc, hw, conf=0.25, iou_thres=0.999)
    assert m[1, 1] == 1 and m.sum() == 1
    _, m = _check(hip, _one_pair(0.9), nc, hw, conf=0.25, iou_thres=1.0)
    assert m[nc, 1] == 1 and m.sum() == 1                          # unmatched label; no match in the image: column nc stays empty
    # confidence exactly at the filter: dropped
    _, m = _check(hip, _one_pair(0.5), nc, hw, conf=0.5, iou_thres=0.45)
    assert m[nc, 1] == 1 and m.sum() == 1
    _, m = _check(hip, _one_pair(np.nextafter(np.float32(0.5), np.float32(1))), nc, hw, conf=0.5, iou_thres=0.45)
    assert m[1, 1] == 1 and m.sum() == 1


def test_tie_rules(hip):
    """equal IoU: a detection takes the lower label index, a label the lower detection index"""
    nc, hw = 4, (256, 256)
    rows = np.array([[1, 0, 0, 256, 256]], np.float32)
    box = [128 / 256, 96 / 256, 128 / 256, 128 / 256]
    # two identical labels (classes 2 and 3, in this order), one detection: label 0 is matched, label 1 is background
    dets = np.zeros((1, 4, 6), np.float32)
    dets[0, 0] = [64, 32, 192, 160, 0.9, 1]
    t = np.array([[0, 2, *box], [0, 3, *box]], np.float32)
    _, m = _check(hip, [(dets, np.array([1], np.int32), t, rows)], nc, hw)
    assert m[1, 2] == 1 and m[nc, 3] == 1 and m.sum() == 2
    # two identical detections (classes 0 and 1), one label: detection 0 wins, detection 1 is a background prediction
    dets[0, 0] = [64, 32, 192, 160, 0.9, 0]
    dets[0, 1] = [64, 32, 192, 160, 0.8, 1]
    t = np.array([[0, 2, *box]], np.float32)
    _, m = _check(hip, [(dets, np.array([2], np.int32), t, rows)], nc, hw)
    assert m[0, 2] == 1 and m[1, nc] == 1 and m.sum() == 2


def _exactly(targets, n):
    """the generator draws the label count: cut the rows of a one-image batch to n, or repeat them, shifted a little, up to n"""
    k = 0
    while targets.shape[0] < n:
        k += 1
        extra = targets.copy()
        extra[:, 2:4] += np.float32(0.013 * k)
        targets = np.concatenate((targets, extra), 0)
    assert targets[:n].shape[0] == n
    return targets[:n]


@pytest.mark.parametrize("nlab", [255, 256, 257])
def test_label_tile_edge(hip, nlab):
    """255, 256 and 257 labels in one image: the edge of the LDS tile of 256 target rows"""
    dets, counts, targets, rows = vr.synth(20 + nlab, 1, 1, 3, 200, max_labels=400, max_fp=30)[0]
    targets = _exactly(targets, nlab)
    _, want = _check(hip, [(dets, counts, targets, rows)], 3, (512, 640))
    assert want[:3, :3].sum() > 0 and want[3].sum() > 0


def test_max_det_1024_all_slots_used(hip):
    data = vr.synth(9, 2, 2, 3, 1024, max_labels=300, max_fp=900)
    dets, counts, targets, rows = data[0]
    big = int(np.argmax(counts))
    assert counts[big] > 768
    n = int(counts[big])                                         # fill the rest of that image's slots with copies shifted by a pixel
    for j in range(n, 1024):
        dets[big, j] = dets[big, j - n]
        dets[big, j, :4] += 1.0
        dets[big, j, 4] = dets[big, j - n, 4] * 0.5
    counts = counts.copy()
    counts[big] = 1024
    _, want = _check(hip, [(dets, counts, targets, rows)], 3, (512, 640))
    assert want[:3, 3].sum() > 0


def test_one_update_of_8_equals_8_updates_of_one(hip):
    _, batches, nc, max_det, net_hw = _gold()
    d, c, t, r = batches[0]
    assert d.shape[0] == 8
    split = []
    for k in range(8):
        tk = t[t[:, 0] == k].copy()
        tk[:, 0] = 0
        split.append((d[k:k + 1], c[k:k + 1], tk, r[k:k + 1]))
    one = _feed(hip, [batches[0]], nc, net_hw)
    eight = _feed(hip, split, nc, net_hw)
    assert one.matrix.any() and torch.equal(one.matrix_device(), eight.matrix_device())


def test_process_batch_equals_update(hip):
    """the reference's signature on native-space rows (as val.py:373 holds them) against update on the same images"""
    from efficientteacher_amd.val import ConfusionMatrix
    _, batches, nc, max_det, net_hw = _gold()
    a = _feed(hip, batches, nc, net_hw)
    b = ConfusionMatrix(nc, device=hip.device)
    for dets, counts, targets, rows in batches:
        for si in range(dets.shape[0]):
            n = int(counts[si])
            lab = targets[targets[:, 0] == si, 1:]
            if n == 0 or lab.shape[0] == 0:                       # val.py never reaches process_batch for these
                continue
            predn = np.concatenate((vr.to_native(dets[si, :n, :4], rows[si]), dets[si, :n, 4:6]), 1)
            labelsn = np.concatenate((lab[:, :1], cr.native_labels(lab, rows[si], net_hw)), 1)
            assert b.process_batch(hip.t(predn), hip.t(labelsn)) is None
    assert np.array_equal(a.matrix, b.matrix)
    # called directly with no detections, the reference counts every label as background
    c = ConfusionMatrix(nc, device=hip.device)
    c.process_batch(torch.zeros((0, 6)), hip.t(np.array([[2, 10, 10, 50, 50], [4, 20, 20, 60, 90]], np.float32)))
    assert c.matrix[nc, 2] == 1 and c.matrix[nc, 4] == 1 and c.matrix.sum() == 2


def test_detection_metrics_with_confusion_is_unchanged(hip):
    from efficientteacher_amd.val import ConfusionMatrix, DetectionMetrics
    g, batches, nc, max_det, net_hw = _gold()
    cm = ConfusionMatrix(nc, device=hip.device)
    plain = DetectionMetrics(nc, max_det=max_det, device=hip.device)
    both = DetectionMetrics(nc, max_det=max_det, device=hip.device, confusion=cm)
    assert plain.confusion is None
    for dets, counts, targets, rows in batches:
        args = (hip.t(dets), hip.t(counts), hip.t(targets), hip.t(rows), net_hw)
        plain.update(*args)
        both.update(*args)
    for x, y in zip(plain.rows() + (plain.nt,), both.rows() + (both.nt,)):
        assert torch.equal(x, y)
    ra, rb = plain.compute(), both.compute()
    for k in ("p", "r", "f1", "ap", "ap_class", "nt", "maps"):
        assert np.array_equal(getattr(ra, k), getattr(rb, k)), k
    assert (ra.mp, ra.mr, ra.map50, ra.map, ra.cls_thr) == (rb.mp, rb.mr, rb.map50, rb.map, rb.cls_thr)
    assert np.array_equal(cm.matrix, g["matrix"])


def test_print_and_plot_carry_on(hip, capsys, tmp_path):
    _, batches, nc, max_det, net_hw = _gold()
    cm = _feed(hip, batches[:1], nc, net_hw)
    cm.print()
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == nc + 1 and out[0] == ' '.join(map(str, cm.matrix[0]))
    cm.plot(save_dir=str(tmp_path), names=[str(i) for i in range(nc)])   # a picture, or the reference's warning: never an exception


def test_update_has_no_host_transfer_in_its_source():
    """companion of the GPU sync-debug test below: update() and the wrappers never ask for a value on the host"""
    from efficientteacher_amd import ops, val
    for fn in (val.ConfusionMatrix.update, val._device_shapes, val.native_predictions, ops.val_confusion, ops.val_predn,
               ops._val_batch_operands):
        src = inspect.getsource(fn)
        for word in (".item(", ".cpu(", ".tolist(", ".numpy(", "synchronize"):
            assert word not in src, (fn.__name__, word)
    assert inspect.getsource(val.coco_json_rows).count(".tolist(") == 1


def test_run_keywords_default_off_and_flags_still_raise():
    from efficientteacher_amd import val
    sig = inspect.signature(val.run).parameters
    assert sig["confusion_matrix"].default is None and sig["jdict"].default is None and sig["image_id_of"].default is None
    for kw in ("save_txt", "save_json", "plots"):
        with pytest.raises(NotImplementedError, match="val.py"):
            val.run(None, [], confusion_matrix=object(), jdict=[], **{kw: 1})


# ---- on the GPU --------------------------------------------------------------------------------------------------------
def _gpu():
    from efficientteacher_amd import _lib
    from tests.conftest import _Mode
    _lib._use_library_for_tests(None, False)
    _lib.load()
    return _Mode("cuda:0", False)


@pytest.mark.gpu
@pytest.mark.parametrize("single_cls", [False, True])
def test_64_images_max_det_300(single_cls):
    """64 images x up to 300 detections, 80 classes (single_cls: 1), two batches of 32.  Twice: bit-identical."""
    hip = _gpu()
    nc = 1 if single_cls else 80
    data = vr.synth(31, 64, 32, nc, 300, (640, 640), max_labels=14, max_fp=600)
    assert max(int(c.max()) for _, c, _, _ in data) == 300
    cm, want = _check(hip, data, nc, (640, 640), single_cls=single_cls)
    assert np.trace(want[:nc, :nc]) >= 64 and want[:nc, nc].sum() > 0 and want[nc, :nc].sum() > 0
    again = _feed(hip, data, nc, (640, 640), single_cls=single_cls)
    assert torch.equal(cm.matrix_device(), again.matrix_device())


@pytest.mark.gpu
def test_600_labels_max_det_1024():
    hip = _gpu()
    dets, counts, targets, rows = vr.synth(32, 1, 1, 3, 1024, max_labels=600, max_fp=900)[0]
    targets = _exactly(targets, 600)
    _, want = _check(hip, [(dets, counts, targets, rows)], 3, (512, 640))
    assert want[:3, :3].sum() > 0


@pytest.mark.gpu
def test_update_and_native_predictions_do_not_synchronise():
    from efficientteacher_amd.val import ConfusionMatrix, native_predictions
    _gpu()
    g, batches, nc, max_det, net_hw = _gold()
    dev = torch.device("cuda:0")
    fed = [tuple(torch.as_tensor(x).to(dev) for x in b) for b in batches]
    loader_shapes = [[((float(r[3]), float(r[4])), ((float(r[0]), float(r[0])), (float(r[1]), float(r[2])))) for r in b[3]] for b in batches]
    m, m2 = ConfusionMatrix(nc, device=dev), ConfusionMatrix(nc, device=dev)
    preds = []
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                        # torch must honour the mode here, or the test shows nothing
            fed[0][1].sum().item()
        for (d, c, t, r), ls in zip(fed, loader_shapes):
            assert m.update(d, c, t, r, net_hw) is None        # shapes as a device tensor
            assert m2.update(d, c, t, ls, net_hw) is None      # shapes as the loader's python list
            preds.append(native_predictions(d, c, ls, net_hw))
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert np.array_equal(m.matrix, g["matrix"]) and np.array_equal(m2.matrix, g["matrix"])
    for b, (predn, tl) in enumerate(preds):
        assert predn.cpu().numpy().tobytes() == g[f"predn{b}"].tobytes() and tl.cpu().numpy().tobytes() == g[f"xywh_tl{b}"].tobytes()


# ---- run(confusion_matrix=, jdict=) against the reference's two functions -------------------------------------------------
if ref_loader.available():
    from tests.test_adapters import ref_callbacks  # noqa: F401  (fixture)


@pytest.mark.skipif(not ref_loader.available(), reason="reference tree not present (build container only)")
def test_run_collects_what_the_reference_functions_give(emu, ref_callbacks, monkeypatch):  # noqa: F811
    """val.run(..., confusion_matrix=cm, jdict=[]) over the tiny hot-path model and loader of
    tests/test_val_metrics.py::test_run_equals_reference_val_run.  This run's own padded NMS output, as DetectionMetrics.update
    received it, is fed image by image through the reference's scale_coords, ConfusionMatrix.process_batch and save_one_json as
    val.py:340-382 strings them together; the matrix and the rows must equal what run accumulated.  The third leg, the reference's
    own val.run(plots=True, save_json=True), was NOT done: it needs seaborn, cv2 and pycocotools, which the build container lacks
    (and its check_requirements would try to install the last), so the comparison with the reference's two functions stands alone;
    that the two val.run agree on the detections themselves is test_run_equals_reference_val_run's business."""
    import tempfile
    from copy import deepcopy
    from pathlib import Path
    import val as ref_val
    from utils.general import non_max_suppression as ref_nms, scale_coords, xywh2xyxy, xyxy2xywh
    from utils.metrics import ConfusionMatrix as RefConfusionMatrix, box_iou
    from efficientteacher_amd import val as our_val
    from efficientteacher_amd.trainer.adapters import hot_path_trainers
    from tests.test_adapters import _cfg, _mk
    _, SSODTrainer = hot_path_trainers()
    rng = np.random.default_rng(8)
    nc, CONF = 80, 0.01                                          # this model's confidences lie far below the default filter of 0.25
    with tempfile.TemporaryDirectory() as d:
        cfg = _cfg(d, True)
        t = _mk(SSODTrainer, rng, True)(cfg, torch.device("cpu"), ref_callbacks, -1, -1, 1)
        with torch.no_grad():
            for mi in t.model.head.m:
                mi.weight.mul_(1e5)
                b = mi.bias.view(t.model.head.na, -1)
                b[:, 4] += 4.0
                b[:, 2:4] -= 2.0                                  # boxes of a few pixels: unscaled they cover the whole 64-pixel image
                b[:, 5:] -= 6.0                                   # one likely class per anchor, so that no two detections above the
                for a, c in enumerate((4, 45, 7)):                # filter share a box (multi_label would repeat it per class)
                    b[a, 5 + c] += 8.0
        t.model.flat_state().mark_weights_changed()
        model = deepcopy(t.model).eval()
        loader = []
        for bi in range(2):
            imgs = torch.from_numpy(rng.integers(0, 256, (2, 3, 64, 64), dtype=np.uint8))
            with torch.no_grad():
                z = model(imgs.float() / 255.0)[0][0]
            rows = []
            for i, det in enumerate(ref_nms(z, 0.005, 0.45, max_det=3)):
                for *xyxy, conf, c in det.tolist():
                    rows.append([i, c, *(xyxy2xywh(torch.tensor([xyxy])) / 64.0)[0].tolist()])
            shapes = [((100, 120), ((64 / 120, 64 / 120), (0.0, (64 - 100 * 64 / 120) / 2)))] * 2
            loader.append((imgs, torch.tensor(rows, dtype=torch.float32).reshape(-1, 6), [f"{7 + bi:06d}.jpg", f"b{bi}.jpg"], shapes))
        fed = []
        update = our_val.DetectionMetrics.update
        monkeypatch.setattr(our_val.DetectionMetrics, "update",
                            lambda self, dets, counts, targets, shapes, net_hw, single_cls=False:
                            (fed.append((dets.clone(), counts.clone(), targets.clone(), tuple(net_hw))),
                             update(self, dets, counts, targets, shapes, net_hw, single_cls=single_cls))[1])
        cm = our_val.ConfusionMatrix(nc, conf=CONF, device="cpu")
        jdict = []
        plain = our_val.run(deepcopy(t.model), [(a.clone(), b.clone(), c, s) for a, b, c, s in loader], conf_thres=0.001, half=False,
                            nc=nc, val_ssod=True)
        n_plain = len(fed)
        ours = our_val.run(deepcopy(t.model), [(a.clone(), b.clone(), c, s) for a, b, c, s in loader], conf_thres=0.001, half=False,
                           nc=nc, val_ssod=True, confusion_matrix=cm, jdict=jdict)
    assert ours[0] == plain[0] and np.array_equal(ours[1], plain[1]) and list(ours[3]) == list(plain[3])   # the keywords change nothing else
    ref_cm, ref_jdict, class_map = RefConfusionMatrix(nc, conf=CONF), [], list(range(1000))
    for (dets, counts, targets, net_hw), (_, _, paths, shapes) in zip(fed[n_plain:], loader):
        tg = targets.clone()
        tg[:, 2:6] *= torch.Tensor([net_hw[1], net_hw[0]] * 2)                       # val.py:328
        for si in range(dets.shape[0]):
            pred = dets[si, :int(counts[si]), :6].clone()
            labels = tg[tg[:, 0] == si, 1:]
            if len(pred) == 0:
                continue
            predn = pred.clone()
            scale_coords(net_hw, predn[:, :4], shapes[si][0], shapes[si][1])
            if len(labels):
                tbox = xywh2xyxy(labels[:, 1:5])
                scale_coords(net_hw, tbox, shapes[si][0], shapes[si][1])
                ref_cm.process_batch(predn, torch.cat((labels[:, 0:1], tbox), 1))
                # outside the yardstick: equal IoUs above the filter, which the reference leaves to an unstable argsort
                iou = box_iou(tbox, predn[predn[:, 4] > CONF, :4])
                val = torch.where(iou > 0.45, iou, torch.full_like(iou, -1.0))
                top = torch.topk(val, min(2, val.shape[0]), 0).values
                assert top.shape[0] < 2 or not ((top[0] == top[1]) & (top[0] > 0)).any(), "one detection, two labels of equal IoU"
                best, lstar = val.max(0)
                for l in range(val.shape[0]):
                    b = best[(lstar == l) & (best > 0)]
                    assert b.unique().numel() == b.numel(), "one label, two detections of equal IoU"
            ref_val.save_one_json(predn, ref_jdict, Path(paths[si]), class_map)
    print("matrix sum", ref_cm.matrix.sum(), "diagonal", np.trace(ref_cm.matrix), "json rows", len(ref_jdict))
    assert np.trace(ref_cm.matrix) >= 2 and len(ref_jdict) >= 8
    assert np.array_equal(cm.matrix, ref_cm.matrix)
    assert jdict == ref_jdict
    assert {type(r["image_id"]) for r in jdict} == {int, str}
