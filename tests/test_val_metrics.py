"""On-device validation metrics (csrc/metrics.hip, efficientteacher_amd/val.py: DetectionMetrics, run).

* the numpy helper tests/val_metrics_ref.py is pinned on tests/golden/val_metrics.npz, which tools/make_val_golden.py made from the
  live reference (scale_coords, process_batch, ap_per_class, fitness);
* et_val_match: correct / conf / cls / valid / nt array_equal to the golden -- zero tolerance, the decisions are fp32 comparisons;
* et_val_ap: ap, p, r, f1 within 1e-12 absolute.  Every value on the way (recall, precision, envelope, one interpolation, one
  trapezoid) lies in [0, 1] and comes from fewer than 10 fp64 roundings, so a curve point is within ~1e-15 of numpy's and an AP
  (100 trapezoids of width 0.01 over such points) is too, whatever the summation order; one wrong index moves a value by at
  least 1/N of a count (> 1e-7 at 1.5 M rows).  ap_class, cls_thr and the arg-max index: equal.
"""
import inspect

import numpy as np
import pytest
import torch

from oracle import ref_loader
from tests import val_metrics_ref as vr
from tests.conftest import golden

TOL = 1e-12
IOUV = torch.linspace(0.5, 0.95, 10).numpy()


def _gold():
    g = golden("val_metrics")
    nc, max_det, nh, nw = (int(v) for v in g["meta"])
    batches = [(g[f"dets{b}"], g[f"counts{b}"], g[f"targets{b}"], g[f"rows{b}"]) for b in range(int(g["nbatches"]))]
    return g, batches, nc, max_det, (nh, nw)


def _bits(correct_bool):
    return (correct_bool * (1 << np.arange(correct_bool.shape[1]))).sum(1).astype(np.int32)


def _feed(hip, batches, nc, max_det, net_hw, iouv=None, single_cls=False):
    from efficientteacher_amd.val import DetectionMetrics
    m = DetectionMetrics(nc, iouv=None if iouv is None else torch.as_tensor(iouv), max_det=max_det, device=hip.device)
    for dets, counts, targets, rows in batches:
        assert m.update(hip.t(dets), hip.t(counts), hip.t(targets), hip.t(rows), net_hw, single_cls=single_cls) is None
    return m


def _helper_arena(batches, net_hw, iouv, nc, single_cls=False):
    parts = [vr.match_batch(d, c, t, r, net_hw, iouv, nc, single_cls) for d, c, t, r in batches]
    if not parts:
        z = np.zeros(0, dtype=np.int32)
        return z, z.astype(np.float32), z, z, np.zeros(nc, dtype=np.int32)
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4)) + (sum(p[4] for p in parts),)


def _helper_curves(arena, niou):
    correct, conf, cls, valid, nt = arena
    v = valid > 0
    tp = ((correct[v, None] >> np.arange(niou)) & 1).astype(bool)
    return vr.ap_per_class(tp, conf[v], cls[v].astype(np.int64), nt)


def _check(hip, batches, nc, max_det, net_hw, iouv=IOUV, single_cls=False):
    """device arena array_equal to the helper's; curves and summary within TOL / equal"""
    m = _feed(hip, batches, nc, max_det, net_hw, iouv, single_cls)
    want = _helper_arena(batches, net_hw, iouv, nc, single_cls)
    got = [t.cpu().numpy() for t in m.rows()] + [m.nt.cpu().numpy()]
    for name, a, b in zip(("correct", "conf", "cls", "valid", "nt"), got, want):
        assert np.array_equal(a, b), name
    hc = _helper_curves(want, len(iouv))
    dc = [t.cpu().numpy() for t in m.curves()]
    for name, a, b in zip(("ap", "p", "r", "f1"), dc, hc):
        err = np.abs(a - b).max() if a.size else 0.0
        print(f"{name}: max abs err {err:.3e}")
        assert err <= TOL, name
    res = m.compute()
    s = vr.summarize(*hc, want[4], any_correct=bool(want[0].any()))
    assert np.array_equal(res.ap_class, s["ap_class"])
    assert np.array_equal(res.nt, want[4])
    for k in ("mp", "mr", "map50", "map"):
        assert abs(getattr(res, k) - s[k]) <= TOL, k
    assert np.abs(res.maps - s["maps"]).max() <= TOL
    if len(s["ap_class"]):
        assert res.f1_index == s["index"] and res.cls_thr == s["cls_thr"]
        for k in ("p", "r", "f1", "ap"):
            assert np.abs(getattr(res, k) - s[k]).max() <= TOL, k
    return m, res


# ---- the helper is the reference ---------------------------------------------------------------------------------------
def test_helper_equals_golden():
    g, batches, nc, max_det, net_hw = _gold()
    arena = _helper_arena(batches, net_hw, g["iouv"], nc)
    assert np.array_equal(arena[0], _bits(g["correct"]))
    assert np.array_equal(arena[4], g["nt"])
    ap, p, r, f1 = _helper_curves(arena, 10)
    s = vr.summarize(ap, p, r, f1, arena[4])
    assert np.array_equal(s["ap_class"], g["ap_class"])
    for k in ("p", "r", "ap", "f1"):
        err = np.abs(s[k] - g[k]).max()
        print(f"{k}: helper vs reference max abs err {err:.3e}")
        assert err <= TOL, k
    assert s["cls_thr"] == list(g["cls_thr"])
    res = np.array([[s["mp"], s["mr"], s["map50"], s["map"]]])
    assert np.abs(res - g["results"]).max() <= TOL
    from efficientteacher_amd.val import fitness
    assert abs(fitness(res)[0] - g["fitness"][0]) <= TOL


# ---- kernels against the golden --------------------------------------------------------------------------------------------
def test_val_match_equals_golden(hip):
    from efficientteacher_amd import ops
    g, batches, nc, max_det, net_hw = _gold()
    rows = sum(b[0].shape[0] for b in batches) * max_det
    dev = hip.device
    correct, cls, valid = (torch.full((rows,), -7, dtype=torch.int32, device=dev) for _ in range(3))
    conf = torch.full((rows,), -7.0, device=dev)
    nt = torch.zeros(nc, dtype=torch.int32, device=dev)
    iouv = hip.t(g["iouv"])
    at = 0
    for dets, counts, targets, shp in batches:
        ops.val_match(hip.t(dets), hip.t(counts), hip.t(targets), hip.t(shp), net_hw, iouv, nc, correct, conf, cls, valid, nt,
                      row_offset=at)
        at += dets.shape[0] * max_det
    want = _helper_arena(batches, net_hw, g["iouv"], nc)          # conf / cls / valid layout; correct and nt from the golden itself
    assert np.array_equal(correct.cpu().numpy(), _bits(g["correct"]))
    assert np.array_equal(nt.cpu().numpy(), g["nt"])
    assert np.array_equal(conf.cpu().numpy(), want[1])
    assert np.array_equal(cls.cpu().numpy(), want[2])
    assert np.array_equal(valid.cpu().numpy(), want[3])


def test_val_ap_equals_golden(hip):
    g, batches, nc, max_det, net_hw = _gold()
    m = _feed(hip, batches, nc, max_det, net_hw)
    res = m.compute()
    assert np.array_equal(res.ap_class, g["ap_class"]) and res.ap_class.dtype == np.int32
    for k in ("ap", "p", "r", "f1"):
        err = np.abs(getattr(res, k) - g[k]).max()
        print(f"{k}: device vs reference max abs err {err:.3e}")
        assert err <= TOL, k
    assert res.cls_thr == list(g["cls_thr"])
    assert np.abs(np.array([res.mp, res.mr, res.map50, res.map]) - g["results"][0]).max() <= TOL
    assert abs(res.fitness() - g["fitness"][0]) <= TOL
    assert np.array_equal(res.nt, g["nt"])
    # the classes the golden was built to hold: labels without predictions (4, a zero row) and predictions without labels (5, absent)
    assert 4 in res.ap_class and 5 not in res.ap_class and res.ap[list(res.ap_class).index(4)].max() == 0.0
    m.reset()
    assert m.rows()[0].numel() == 0 and int(m.nt.sum()) == 0


# ---- edge cases against the helper -----------------------------------------------------------------------------------------
def test_empty_batch_and_no_detections(hip):
    g, batches, nc, max_det, net_hw = _gold()
    from efficientteacher_amd.val import DetectionMetrics
    m = DetectionMetrics(nc, max_det=max_det, device=hip.device)
    res = m.compute()                                            # nothing fed at all
    assert res.mp == res.map == 0.0 and len(res.ap_class) == 0 and res.cls_thr == [] and not res.maps.any()
    m.update(hip.t(np.zeros((0, max_det, 6), np.float32)), hip.t(np.zeros(0, np.int32)), hip.t(np.zeros((0, 6), np.float32)),
             hip.t(np.zeros((0, 5), np.float32)), net_hw)
    assert m.rows()[0].numel() == 0
    zero = [(d, np.zeros_like(c), t, r) for d, c, t, r in batches]     # counts == 0 everywhere: labels counted, nothing correct
    m, res = _check(hip, zero, nc, max_det, net_hw)
    assert res.map == 0.0 and len(res.ap_class) == 0 and np.array_equal(res.nt, g["nt"])


def test_no_labels_at_all(hip):
    _, batches, nc, max_det, net_hw = _gold()
    nolab = [(d, c, np.zeros((0, 6), np.float32), r) for d, c, t, r in batches]
    m, res = _check(hip, nolab, nc, max_det, net_hw)
    assert res.map == 0.0 and not res.nt.any() and int(m.rows()[3].sum()) == sum(int(b[1].sum()) for b in batches)


def test_single_cls(hip):
    data = vr.synth(5, 12, 4, 1, 60, (384, 640))
    _, res = _check(hip, data, 1, 60, (384, 640), single_cls=True)
    assert list(res.ap_class) == [0] and res.map50 > 0.1
    # detections of other classes count as class 0 (val.py:353-354) when the labels are class 0
    data = vr.synth(6, 6, 3, 4, 60, (384, 640))
    data = [(d, c, np.concatenate((t[:, :1], np.zeros_like(t[:, 1:2]), t[:, 2:]), 1), r) for d, c, t, r in data]
    _check(hip, data, 1, 60, (384, 640), single_cls=True)


def test_one_threshold(hip):
    data = vr.synth(7, 8, 4, 5, 50)
    _check(hip, data, 5, 50, (512, 640), iouv=np.array([0.5], dtype=np.float32))


def test_many_labels_in_one_image(hip):
    """more labels in one image than one LDS tile holds (256 target rows), and images whose labels straddle tile borders"""
    data = vr.synth(8, 3, 3, 3, 200, max_labels=700, max_fp=40)
    per_image = np.bincount(data[0][2][:, 0].astype(int), minlength=3)
    assert per_image.max() > 256 and data[0][2].shape[0] > 512
    m, res = _check(hip, data, 3, 200, (512, 640))
    assert res.map50 > 0.1


def test_max_det_1024(hip):
    data = vr.synth(9, 2, 2, 3, 1024, max_labels=300, max_fp=900)
    assert data[0][1].max() > 768
    _check(hip, data, 3, 1024, (512, 640))


def test_split_update_equals_one_batch(hip):
    """the same images fed as one batch and as two (arena offsets): identical arena, bit-identical results"""
    _, batches, nc, max_det, net_hw = _gold()
    d, c, t, r = batches[0]
    k = 3
    t2 = t[t[:, 0] >= k].copy()
    t2[:, 0] -= k
    split = [(d[:k], c[:k], t[t[:, 0] < k], r[:k]), (d[k:], c[k:], t2, r[k:])]
    one = _feed(hip, [batches[0]], nc, max_det, net_hw)
    two = _feed(hip, split, nc, max_det, net_hw)
    for a, b in zip(one.rows(), two.rows()):
        assert torch.equal(a, b)
    assert torch.equal(one.nt, two.nt)
    for a, b in zip(one.curves(), two.curves()):
        assert torch.equal(a, b)


def test_arena_growth_keeps_rows(hip):
    data = vr.synth(10, 70, 1, 4, 300, max_fp=20)                # 70 updates of one image: the arena grows past its first size
    _check(hip, data, 4, 300, (512, 640))


def test_unsupported_legs_name_the_reference():
    from efficientteacher_amd import val
    for kw in ("save_txt", "save_json", "save_hybrid", "plots", "num_points"):
        with pytest.raises(NotImplementedError, match="val.py"):
            val.run(None, [], **{kw: 1})


def test_adapter_switch_routes_val_run(monkeypatch):
    """adapters.DeviceVal: calls with a model and a loader go to this package's val.run; plots / save_json calls and everything
    else of the module stay the reference's"""
    import types
    from efficientteacher_amd import val as our_val
    from efficientteacher_amd.trainer.adapters import DeviceVal, _HotPath
    calls = []
    ref = types.SimpleNamespace(run=lambda data, **kw: calls.append(("ref", kw)) or "ref", process_batch="pb")
    monkeypatch.setattr(our_val, "run", lambda model, loader, **kw: calls.append(("ours", kw)) or "ours")
    model = torch.nn.Linear(1, 1)
    v = DeviceVal(ref)
    assert v.run({"nc": 3, "names": ["a", "b", "c"]}, model=model, dataloader=[1], plots=False, val_ssod=True, batch_size=4) == "ours"
    assert calls[-1][1]["nc"] == 3 and calls[-1][1]["val_ssod"] is True and calls[-1][1]["half"] is False
    assert v.run({"nc": 3}, model=model, dataloader=[1], plots=True) == "ref" and calls[-1][0] == "ref"
    assert v.run({"nc": 3}, model=model, dataloader=[1], plots=False, save_json=True) == "ref"
    assert v.process_batch == "pb"
    assert _HotPath.ET_DEVICE_VAL is False and _HotPath()._et_val(ref) is ref            # the default changes nothing
    on = type("T", (_HotPath,), {"ET_DEVICE_VAL": True})()
    assert isinstance(on._et_val(ref), DeviceVal) and on._et_val(None) is None


def test_update_has_no_host_transfer_in_its_source():
    """companion of the GPU sync-debug test below: update() and the wrapper it calls never ask for a value on the host"""
    from efficientteacher_amd import ops
    from efficientteacher_amd.val import DetectionMetrics
    for fn in (DetectionMetrics.update, DetectionMetrics._reserve, ops.val_match):
        src = inspect.getsource(fn)
        for word in (".item(", ".cpu(", ".tolist(", ".numpy(", "synchronize"):
            assert word not in src, (fn.__name__, word)


# ---- full size, on the GPU ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("single_cls", [False, True])
def test_full_size(single_cls):
    """5000 images x up to 300 detections, 80 classes, batches of 32; single_cls: one segment of all rows.  Twice: bit-identical."""
    from efficientteacher_amd import _lib
    from tests.conftest import _Mode
    _lib._use_library_for_tests(None, False)
    _lib.load()
    hip = _Mode("cuda:0", False)
    nc = 1 if single_cls else 80
    data = vr.synth(11, 5000, 32, nc, 300, (640, 640), max_labels=14, max_fp=600)
    assert max(int(c.max()) for _, c, _, _ in data) == 300
    m, res = _check(hip, data, nc, 300, (640, 640), single_cls=single_cls)
    print(f"rows {m.rows()[0].numel()} valid {int(m.rows()[3].sum())} mAP@.5 {res.map50:.4f} mAP {res.map:.4f}")
    # not a degenerate set: the generator jitters ~1.5 detections around each of ~7.5 labels per image by 8 % of the box size, so
    # one true positive at IoU 0.5 per image on average is a loose lower bound
    assert int((m.rows()[0] & 1).sum()) >= 5000 and res.map50 > 0.0
    again = _feed(hip, data, nc, 300, (640, 640), single_cls=single_cls)
    for a, b in zip(m.rows() + m.curves(), again.rows() + again.curves()):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_update_does_not_synchronise():
    from efficientteacher_amd import _lib
    from efficientteacher_amd.val import DetectionMetrics
    _lib._use_library_for_tests(None, False)
    _lib.load()
    _, batches, nc, max_det, net_hw = _gold()
    dev = torch.device("cuda:0")
    fed = [tuple(torch.as_tensor(x).to(dev) for x in b) for b in batches]
    loader_shapes = [[((float(r[3]), float(r[4])), ((float(r[0]), float(r[0])), (float(r[1]), float(r[2])))) for r in b[3]] for b in batches]
    m = DetectionMetrics(nc, max_det=max_det, device=dev)
    m2 = DetectionMetrics(nc, max_det=max_det, device=dev)
    torch.cuda.synchronize()
    # torch must honour the mode here, or the test shows nothing
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            fed[0][1].sum().item()
        for (d, c, t, r), ls in zip(fed, loader_shapes):
            assert m.update(d, c, t, r, net_hw) is None            # shapes as a device tensor
            assert m2.update(d, c, t, ls, net_hw) is None          # shapes as the loader's python list
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    g = golden("val_metrics")
    assert np.array_equal(m.rows()[0].cpu().numpy(), _bits(g["correct"]))
    assert np.array_equal(m2.rows()[0].cpu().numpy(), _bits(g["correct"]))


# ---- end to end against the reference's val.run ------------------------------------------------------------------------
if ref_loader.available():
    from tests.test_adapters import ref_callbacks  # noqa: F401  (fixture)


@pytest.mark.skipif(not ref_loader.available(), reason="reference tree not present (build container only)")
def test_run_equals_reference_val_run(emu, ref_callbacks, monkeypatch):  # noqa: F811
    """this package's val.run and the reference's val.run over the same hot-path model and the same loader (set up as
    tests/test_adapters.py::test_reference_val_run_over_the_hot_path_model does).  The head weights are scaled up: with the plain
    random initialisation the head's input is ~1e-6, every cell answers with the bias alone, 1200 detections share 132 confidence
    values and the reference's AP hangs on its unstable np.argsort(-conf).  The test asserts that no group of equal (class,
    confidence) mixes true and false positives, which is the condition under which that sort order does not matter."""
    import tempfile
    from copy import deepcopy
    from pathlib import Path
    import val as ref_val
    from utils.general import non_max_suppression as ref_nms, xyxy2xywh
    from efficientteacher_amd import val as our_val
    from efficientteacher_amd.trainer.adapters import hot_path_trainers
    from tests.test_adapters import _cfg, _mk
    _, SSODTrainer = hot_path_trainers()
    rng = np.random.default_rng(8)
    with tempfile.TemporaryDirectory() as d:
        cfg = _cfg(d, True)
        t = _mk(SSODTrainer, rng, True)(cfg, torch.device("cpu"), ref_callbacks, -1, -1, 1)
        with torch.no_grad():
            for mi in t.model.head.m:
                mi.weight.mul_(1e5)
                b = mi.bias.view(t.model.head.na, -1)
                b[:, 4] += 4.0
                b[:, 5:] += 2.0
        t.model.flat_state().mark_weights_changed()
        model = deepcopy(t.model).eval()
        seen = {}
        compute = our_val.DetectionMetrics.compute
        monkeypatch.setattr(our_val.DetectionMetrics, "compute", lambda self: (seen.setdefault("m", self), compute(self))[1])
        loader = []
        for bi in range(2):
            imgs = torch.from_numpy(rng.integers(0, 256, (2, 3, 64, 64), dtype=np.uint8))
            with torch.no_grad():
                z = model(imgs.float() / 255.0)[0][0]
            rows = []
            for i, det in enumerate(ref_nms(z, 0.005, 0.45, max_det=3)):
                for *xyxy, conf, c in det.tolist():
                    rows.append([i, c, *(xyxy2xywh(torch.tensor([xyxy])) / 64.0)[0].tolist()])
            # a letterbox with a real gain and pad, the same for both sides
            shapes = [((100, 120), ((64 / 120, 64 / 120), (0.0, (64 - 100 * 64 / 120) / 2)))] * 2
            loader.append((imgs, torch.tensor(rows, dtype=torch.float32).reshape(-1, 6), [f"a{bi}.jpg", f"b{bi}.jpg"], shapes))
        assert sum(x[1].shape[0] for x in loader) >= 4
        data = {'nc': 80, 'names': cfg.Dataset.names, 'val': 'x'}
        fresh = lambda: [(a.clone(), b.clone(), c, s) for a, b, c, s in loader]  # noqa: E731
        ref = ref_val.run(data, batch_size=2, imgsz=64, model=deepcopy(t.model), conf_thres=0.001, single_cls=False, dataloader=fresh(),
                          save_dir=Path(d), plots=False, callbacks=ref_callbacks, compute_loss=None, num_points=0, val_ssod=True,
                          val_kp=False)
        ours = our_val.run(deepcopy(t.model), fresh(), conf_thres=0.001, half=False, nc=80, val_ssod=True)
    correct, conf, cls, valid = (x.numpy() for x in seen["m"].rows())
    groups = {}
    for k, c in zip(zip(cls[valid > 0].tolist(), conf[valid > 0].tolist()), correct[valid > 0].tolist()):
        groups.setdefault(k, set()).add(c)
    assert all(len(v) == 1 for v in groups.values()), "a tie in (class, confidence) mixes TP and FP: outside the yardstick"
    assert ref[0][2] > 0.2, ref[0]
    print("reference", ref[0][:4], "ours", ours[0][:4])
    assert np.abs(np.array(ours[0][:4]) - np.array(ref[0][:4])).max() <= TOL
    assert np.abs(ours[1] - ref[1]).max() <= TOL
    assert list(ours[3]) == list(ref[3])
    assert len(ours[0]) == len(ref[0]) == 7 and len(ours) == len(ref) == 4
