"""LabelMatch's end-of-epoch thresholds on the device (csrc/labelmatch.hip, ops.labelmatch_thresholds, LabelMatch(device_thresholds=True))
against the reference-run golden tests/golden/labelmatch_thresholds.npz (tools/make_labelmatch_thr_golden.py) and the numpy
restatement tests/labelmatch_thr_ref.py.

Tolerances: thresholds, counts and n_iter are compared for EQUALITY (each threshold is one of the logged fp32 values or a config
constant).  The six mixture parameters per class are compared within 100 x ``self_dev``, the worst relative change the generator
saw in them when it moved every exp by up to 4 units in the last place and permuted the scores (1.8e-14 for the committed fixture)."""
import sys

import numpy as np
import pytest
import torch

from tests import labelmatch_thr_ref as lr
from tests.conftest import golden

OUT_KEYS = ("thr_high", "thr_low", "n_per_class", "cls_num_total", "n_iter", "status", "gmm")


@pytest.fixture(scope="module")
def fx():
    g = golden("labelmatch_thresholds")
    nc = int(g["nc"])
    conf_thres, lo, hi, pct = (float(v) for v in g["cfg"])
    logs = [(g[f"conf{e}"], g[f"cls{e}"]) for e in (0, 1)]
    want, total = [], np.zeros(nc, np.int64)
    for e, (conf, cls) in enumerate(logs):                      # the helper's numbers, computed once
        w = lr.thresholds(conf, cls, nc, e, lo, hi, pct, total)
        total = w["cls_num_total"]
        for v in w.values():
            v.setflags(write=False)
        want.append(w)
    return dict(g=g, nc=nc, conf_thres=conf_thres, lo=lo, hi=hi, pct=pct, logs=logs, want=want, tol=100.0 * float(g["self_dev"]))


def _close(got, want, tol):
    fit = np.abs(want).sum(-1) > 0
    assert np.array_equal(np.abs(got).sum(-1) > 0, fit)
    return not fit.any() or float(np.abs(got[fit] / want[fit] - 1).max()) <= tol


def _run(hip, conf, cls, nc, epoch, lo, hi, pct, total, cap=None, count=None, want_sorted=False):
    """the op on a log of capacity cap (default: exactly full) -> (host dict, result object)"""
    from efficientteacher_amd import ops
    n = conf.shape[0]
    cap = n if cap is None else cap
    conf_log, cls_log = np.full(cap, 7.5, np.float32), np.full(cap, 3, np.int32)     # live-looking values behind the count
    conf_log[:n], cls_log[:n] = conf, cls
    n_log = hip.t(np.array([n if count is None else count], np.int64))
    res = ops.labelmatch_thresholds(hip.t(conf_log), hip.t(cls_log), n_log, nc, epoch, lo, hi, pct, hip.t(np.asarray(total, np.int64)),
                                    want_sorted=want_sorted)
    h = res.host()
    assert int(h["log_count"][0]) == (n if count is None else count)
    return h, res


def test_helper_equals_the_reference(fx):
    """pins tests/labelmatch_thr_ref.py on the live reference and sklearn (no kernel involved)"""
    g = fx["g"]
    assert fx["tol"] < 1e-9 and fx["tol"] > 0
    for e in (0, 1):
        w = fx["want"][e]
        assert np.array_equal(w["thr_high"], g[f"thr_high{e}"]) and np.array_equal(w["thr_low"], g[f"thr_low{e}"])
        assert np.array_equal(w["n_iter"], g[f"n_iter{e}"]) and not w["status"].any()
        assert _close(w["gmm"], g[f"gmm{e}"], fx["tol"])
    highs = np.concatenate([g["thr_high0"], g["thr_high1"]])
    assert (highs > 0).any() and (highs == 0).any() and int(max(g["n_iter0"].max(), g["n_iter1"].max())) < lr.MAX_ITER


def test_op_equals_the_reference_over_two_epochs(hip, fx):
    g, nc = fx["g"], fx["nc"]
    total = np.zeros(nc, np.int64)
    for e, (conf, cls) in enumerate(fx["logs"]):
        h, _ = _run(hip, conf, cls, nc, e, fx["lo"], fx["hi"], fx["pct"], total, cap=conf.shape[0] + 1000)
        w = fx["want"][e]
        print(f"epoch {e}: n_iter {h['n_iter'].tolist()} high {h['thr_high'].tolist()} gmm dev "
              f"{np.abs(h['gmm'][w['n_iter'] > 0] / g[f'gmm{e}'][w['n_iter'] > 0] - 1).max():.3e} (tol {fx['tol']:.3e})")
        assert np.array_equal(h["thr_high"], g[f"thr_high{e}"]), (e, h["thr_high"], g[f"thr_high{e}"])
        assert np.array_equal(h["thr_low"], g[f"thr_low{e}"]), (e, h["thr_low"], g[f"thr_low{e}"])
        assert np.array_equal(h["n_iter"], g[f"n_iter{e}"]), (e, h["n_iter"], g[f"n_iter{e}"])
        assert np.array_equal(h["n_per_class"], w["n_per_class"]) and np.array_equal(h["cls_num_total"], w["cls_num_total"])
        assert not h["status"].any()
        assert _close(h["gmm"], g[f"gmm{e}"], fx["tol"])
        total = h["cls_num_total"]


def test_outputs_do_not_depend_on_the_append_order(hip, fx):
    nc = fx["nc"]
    conf, cls = fx["logs"][0]
    first = None
    for seed in (None, 1, 2):
        p = np.arange(conf.shape[0]) if seed is None else np.random.default_rng(seed).permutation(conf.shape[0])
        h, _ = _run(hip, conf[p], cls[p], nc, 0, fx["lo"], fx["hi"], fx["pct"], np.zeros(nc, np.int64), want_sorted=True)
        first = first or h
        for k in OUT_KEYS:
            assert h[k].tobytes() == first[k].tobytes(), (seed, k)
    # a second call on the same device buffers
    from efficientteacher_amd import ops
    logs = hip.t(conf), hip.t(cls), hip.t(np.array([conf.shape[0]], np.int64))
    tot = hip.t(np.zeros(nc, np.int64))
    for _ in range(2):
        h = ops.labelmatch_thresholds(*logs, nc, 0, fx["lo"], fx["hi"], fx["pct"], tot).host()
        for k in OUT_KEYS:
            assert h[k].tobytes() == first[k].tobytes(), k
    assert np.array_equal(logs[0].cpu().numpy(), conf) and np.array_equal(logs[1].cpu().numpy(), cls)      # the log is read only


def test_sorted_segments_equal_the_helper(hip, fx):
    nc = fx["nc"]
    for e, (conf, cls) in enumerate(fx["logs"]):
        cap = conf.shape[0] + 333
        _, res = _run(hip, conf, cls, nc, e, fx["lo"], fx["hi"], fx["pct"], np.zeros(nc, np.int64), cap=cap, want_sorted=True)
        w = fx["want"][e]
        seg, s = res.seg_offset.cpu().numpy(), res.sorted_conf.cpu().numpy()
        assert np.array_equal(seg, w["seg_offset"])
        assert s.shape == (cap,) and np.array_equal(s[:seg[-1]], w["sorted_conf"]) and not s[seg[-1]:].any()


def test_empty_and_full_logs(hip, fx):
    nc = fx["nc"]
    conf, cls = fx["logs"][0]
    h, res = _run(hip, conf, cls, nc, 0, fx["lo"], fx["hi"], fx["pct"], np.arange(nc), cap=8192, count=0, want_sorted=True)
    assert np.array_equal(h["thr_high"], np.full(nc, fx["hi"])) and np.array_equal(h["thr_low"], np.full(nc, fx["lo"]))
    assert not h["n_per_class"].any() and np.array_equal(h["cls_num_total"], np.arange(nc)) and not h["n_iter"].any()
    assert not res.seg_offset.cpu().numpy().any() and not res.sorted_conf.cpu().numpy().any() and not h["status"].any()
    # exactly full: log_count == cap
    h, _ = _run(hip, conf, cls, nc, 0, fx["lo"], fx["hi"], fx["pct"], np.zeros(nc, np.int64))
    w = fx["want"][0]
    for k in ("thr_high", "thr_low", "n_per_class", "n_iter"):
        assert np.array_equal(h[k], w[k]), k
    # the counter ran past the capacity: the kernel reads `cap` pairs and no more, the raw counter comes back
    n = 3000
    h, _ = _run(hip, conf[:n], cls[:n], nc, 0, fx["lo"], fx["hi"], fx["pct"], np.zeros(nc, np.int64), count=n + 12345)
    w = lr.thresholds(conf[:n], cls[:n], nc, 0, fx["lo"], fx["hi"], fx["pct"], np.zeros(nc, np.int64))
    for k in ("thr_high", "thr_low", "n_per_class", "n_iter"):
        assert np.array_equal(h[k], w[k]), k


def _cfg(nc, pct, conf_thres=None):
    import os
    from efficientteacher_amd.configs import get_cfg
    from tests.conftest import ROOT
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "efficientteacher_amd/configs/ssod/coco-standard/yolov5l_coco_ssod_10_percent.yaml"))
    cfg.merge_from_list(["Dataset.nc", nc, "SSOD.pseudo_label_type", "LabelMatch", "SSOD.resample_low_percent", float(pct),
                         "Dataset.names", [str(i) for i in range(nc)]])
    return cfg


def _fill(lm, hip, conf, cls, count=None):
    conf_log, cls_log, n_log = lm._ensure_log(hip.device)
    n = min(conf.shape[0], lm.capacity)
    conf_log[:n] = hip.t(conf[:n])
    cls_log[:n] = hip.t(cls[:n])
    n_log.fill_(conf.shape[0] if count is None else count)


def test_labelmatch_device_path_errors(hip, fx, monkeypatch):
    from efficientteacher_amd.utils.labelmatch import LabelMatch
    monkeypatch.setitem(sys.modules, "sklearn.mixture", None)
    nc = fx["nc"]
    conf, cls = fx["logs"][0]
    cfg = _cfg(nc, fx["pct"])
    assert [cfg.SSOD.nms_conf_thres, cfg.SSOD.ignore_thres_low, cfg.SSOD.ignore_thres_high] == [fx["conf_thres"], fx["lo"], fx["hi"]]
    # the log overflew: the host path's RuntimeError
    lm = LabelMatch(cfg, 1, 5, cls_ratio_gt=np.full(nc, 1.0 / nc), score_log_capacity=1024, device_thresholds=True)
    _fill(lm, hip, conf, cls)
    with pytest.raises(RuntimeError, match=f"overflow: {conf.shape[0]} detections this epoch, capacity 1024"):
        lm.update_epoch_cls_thr(0)
    # resample_low_percent = 1.0 on a first epoch: pos_loc_low == len(scores), the reference's IndexError; nothing is read there
    lm = LabelMatch(_cfg(nc, 1.0), 1, 5, cls_ratio_gt=np.full(nc, 1.0 / nc), score_log_capacity=conf.shape[0], device_thresholds=True)
    _fill(lm, hip, conf, cls)
    with pytest.raises(IndexError):
        lm.update_epoch_cls_thr(0)
    from efficientteacher_amd import ops
    h, _ = _run(hip, conf, cls, nc, 0, fx["lo"], fx["hi"], 1.0, np.zeros(nc, np.int64))
    n = fx["want"][0]["n_per_class"]
    assert np.array_equal(h["status"], np.where(n > 0, ops.LM_RANK_OUT_OF_SEGMENT, ops.LM_OK))
    assert np.array_equal(h["thr_low"], np.full(nc, fx["lo"])) and np.array_equal(h["thr_high"], fx["want"][0]["thr_high"])
    # the fixture itself through the class: lists of python floats, the helper's numbers, the running totals on the host
    lm = LabelMatch(cfg, 1, 5, cls_ratio_gt=np.full(nc, 1.0 / nc), score_log_capacity=8192, device_thresholds=True)
    for e, (c, k) in enumerate(fx["logs"]):
        _fill(lm, hip, c, k)
        lm.count = 5
        lm.update_epoch_cls_thr(e)
        w = fx["want"][e]
        assert lm.cls_thr_high == w["thr_high"].tolist() and lm.cls_thr_low == w["thr_low"].tolist()
        assert all(type(v) is float for v in lm.cls_thr_high + lm.cls_thr_low)
        assert np.array_equal(lm.cls_num_total, w["cls_num_total"].astype(np.float64)) and lm.cls_num_total.dtype == np.float64
        assert lm.count == 0 and int(lm._log[2].item()) == 0
        served = lm.closed_epoch_scores()
        assert all(served[q] == w["sorted_conf"][w["seg_offset"][q]:w["seg_offset"][q + 1]].astype(np.float64).tolist() for q in range(nc))


def test_labelmatch_device_path_equals_the_host_golden(hip, monkeypatch, caplog):
    """the batches of tests/golden/labelmatch.npz (tests/test_labelmatch.py runs them through the host path) with
    device_thresholds=True and sklearn.mixture unimportable: the same thresholds, the same log lines"""
    import logging
    from efficientteacher_amd.utils import labelmatch as lm_mod
    from oracle.make_golden import labelmatch_pred
    from tests.test_labelmatch import _cfg as host_cfg
    monkeypatch.setitem(sys.modules, "sklearn.mixture", None)
    with pytest.raises(ImportError):
        lm_mod.LabelMatch.gmm_policy(np.linspace(0.1, 0.9, 8), 0.0)             # the host path could not run here
    g = golden("labelmatch")
    nc = int(g["nc"])
    B, A = (int(v) for v in g["BA"])
    H, W = (int(v) for v in g["hw"])
    rng = np.random.default_rng(int(g["seed"]))
    lm = lm_mod.LabelMatch(host_cfg(g), 100, 5, cls_ratio_gt=np.full(nc, 1.0 / nc), device_thresholds=True)
    M_s = hip.t(g["M_s"])
    total = 0
    for epoch, nb in enumerate((3, 2)):
        for _ in range(nb):
            lm.create_pseudo_label_padded(hip.t(labelmatch_pred(rng, B, A, nc)), M_s, W, H)
            lm.update(hip.t(np.array([[0, 1, .5, .5, .1, .1]], np.float32)), 1, B)
        n_logged = int(lm._log[2].item())
        total += n_logged
        with caplog.at_level(logging.INFO, logger=lm_mod.LOGGER.name):
            caplog.clear()
            lm.update_epoch_cls_thr(epoch)
        assert np.array_equal(np.array(lm.cls_thr_high), g[f"thr_high{epoch}"]), (epoch, lm.cls_thr_high)
        assert np.array_equal(np.array(lm.cls_thr_low), g[f"thr_low{epoch}"]), (epoch, lm.cls_thr_low)
        assert lm.count == 0 and lm.pse_count == 0 and int(lm._log[2].item()) == 0 and lm._cls_hist is None
        assert lm.cls_num_total.sum() == total
        lines = [r.getMessage() for r in caplog.records]
        assert len(lines) == nc and all(ln.endswith(f":{lm.cls_thr_low[c]}") for c, ln in enumerate(lines))
        assert sum(int(ln.split()[0]) for ln in lines) == n_logged


def test_trainer_hands_the_device_thresholds_to_the_loss(hip, fx):
    """SSODTrainer(device_labelmatch=True).after_epoch (ssod_trainer.py:319-323): the loss's thresholds are the creator's lists and the
    log is empty again; hot_path_trainers passes the same flag on"""
    import os
    from efficientteacher_amd.configs import get_cfg
    from efficientteacher_amd.trainer import SSODTrainer
    from efficientteacher_amd.trainer.adapters import hot_path_trainers
    from tests.conftest import ROOT
    from tests.test_ssod_step import YAML
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, YAML))
    cfg.merge_from_list(["Model.width_multiple", 0.125, "Model.depth_multiple", 0.33, "SSOD.pseudo_label_type", "LabelMatch",
                         "SSOD.resample_low_percent", fx["pct"]])
    cfg.freeze()
    nc = cfg.Dataset.nc
    kw = dict(nb=1000, target_data_len=8, label_num_per_image=3, cls_ratio_gt=np.full(nc, 1.0 / nc))
    assert SSODTrainer(cfg, hip.device, **kw).pseudo_label_creator.device_thresholds is False       # off by default
    t = SSODTrainer(cfg, hip.device, device_labelmatch=True, **kw)
    lm = t.pseudo_label_creator
    assert lm.device_thresholds is True
    conf, cls = fx["logs"][0]
    _fill(lm, hip, conf, cls)
    lo0 = list(t.compute_un_sup_loss.ignore_thres_low)
    t.after_epoch(0)
    assert t.compute_un_sup_loss.ignore_thres_low is lm.cls_thr_low and t.compute_un_sup_loss.ignore_thres_high is lm.cls_thr_high
    w = lr.thresholds(conf, cls, nc, 0, cfg.SSOD.ignore_thres_low, cfg.SSOD.ignore_thres_high, fx["pct"], np.zeros(nc, np.int64))
    assert lm.cls_thr_low == w["thr_low"].tolist() and lm.cls_thr_high == w["thr_high"].tolist() and lm.cls_thr_low != lo0
    assert int(lm._log[2].item()) == 0 and lm.cls_num_total.sum() == (cls >= 0).sum()

    class Ref:
        pass
    for flag in (False, True):
        hot, ssod = hot_path_trainers(Ref, Ref, device_labelmatch=flag)
        assert ssod.ET_DEVICE_LABELMATCH is flag
    assert hot_path_trainers(Ref, Ref)[1].ET_DEVICE_LABELMATCH is False
