"""Time LabelMatch's end-of-epoch thresholds: the device call against the host path it can replace, on one GPU in one process.

    python tools/labelmatch_thr_bench.py [--pairs 2000000] [--classes 80] [--reps 5] [--out profiles/labelmatch_thresholds_mi355x.txt]

The log is synthetic and COCO-like: `pairs` (class, confidence) pairs over `classes` classes whose sizes fall off like 1 / rank^1.1
(the largest class holds about a quarter of them, as `person` does); every other class by size, the largest included, has skewed
confidences (beta-like, most of them just above nms_conf_thres: the slow case of the mixture fit), the rest bimodal ones; shuffled.
Legs:
  (host)   LabelMatch.update_epoch_cls_thr as it is by default: the log copied to the host, a numpy sort per class, one
           sklearn.mixture.GaussianMixture fit per class.  Run once: it takes tens of seconds.
  (device) LabelMatch(device_thresholds=True).update_epoch_cls_thr: et_labelmatch_thresholds on the log where it lies plus the one
           small read.  `reps` runs, median and spread; the launches alone (ops.labelmatch_thresholds between two device
           synchronisations, no read) are timed the same way, and once more on an almost empty log (one tile).
Both legs see the same log; their thresholds are compared before any time is reported."""
import argparse
import logging
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientteacher_amd import ops  # noqa: E402
from efficientteacher_amd.configs import get_cfg  # noqa: E402
from efficientteacher_amd.utils.labelmatch import LabelMatch  # noqa: E402
from tools.val_metrics_bench import clocks  # noqa: E402


def synth_log(rng, pairs, nc, conf_thres):
    share = 1.0 / np.arange(1, nc + 1) ** 1.1
    sizes = np.floor(share / share.sum() * pairs).astype(np.int64)
    cls = np.repeat(rng.permutation(nc), sizes).astype(np.int32)
    skewed = np.repeat(np.arange(nc) % 2 == 0, sizes)                           # by size rank: the largest class is a skewed one
    n = cls.shape[0]
    top = rng.random(n) < 0.35
    conf = np.where(top, rng.normal(0.78, 0.09, n), conf_thres + rng.gamma(1.5, 0.09, n))
    conf = np.where(skewed, conf_thres + (1.0 - conf_thres) * rng.beta(1.2, 4.0, n), conf)
    conf = np.clip(conf, conf_thres + 1e-4, 0.999).astype(np.float32)
    p = rng.permutation(n)
    return conf[p], cls[p], np.sort(sizes)[::-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    logging.getLogger("efficientteacher_amd.utils.labelmatch").setLevel(logging.WARNING)
    nc = a.classes
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "efficientteacher_amd/configs/ssod/coco-standard/yolov5l_coco_ssod_10_percent.yaml"))
    cfg.merge_from_list(["Dataset.nc", nc, "SSOD.pseudo_label_type", "LabelMatch", "Dataset.names", [str(i) for i in range(nc)]])
    conf, cls, sizes = synth_log(np.random.default_rng(20261019), a.pairs, nc, cfg.SSOD.nms_conf_thres)
    n = conf.shape[0]
    cap = max(1 << 16, 1 << (n - 1).bit_length())
    conf_d, cls_d = torch.from_numpy(conf).to(dev), torch.from_numpy(cls).to(dev)

    def creator(device_thresholds):
        lm = LabelMatch(cfg, 1, 5, cls_ratio_gt=np.full(nc, 1.0 / nc), score_log_capacity=cap, device_thresholds=device_thresholds)
        return lm

    def fill(lm, count=n):
        conf_log, cls_log, n_log = lm._ensure_log(dev)
        conf_log[:n] = conf_d
        cls_log[:n] = cls_d
        n_log.fill_(count)
        lm.cls_num_total[:] = 0
        torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    lm_dev = creator(True)
    fill(lm_dev)
    timed(lambda: lm_dev.update_epoch_cls_thr(0))                               # warm-up: allocator, code objects
    whole, launches, small = [], [], []
    for _ in range(a.reps):
        fill(lm_dev)
        whole.append(timed(lambda: lm_dev.update_epoch_cls_thr(0))[0])
    zero = torch.zeros(nc, dtype=torch.int64, device=dev)
    for _ in range(a.reps):
        fill(lm_dev)
        launches.append(timed(lambda: ops.labelmatch_thresholds(*lm_dev._log, nc, 0, lm_dev.ignore_thres_low, lm_dev.ignore_thres_high,
                                                                lm_dev.resample_low_percent, zero))[0])
    for _ in range(a.reps):
        fill(lm_dev, count=2048)
        small.append(timed(lambda: ops.labelmatch_thresholds(*lm_dev._log, nc, 0, lm_dev.ignore_thres_low, lm_dev.ignore_thres_high,
                                                             lm_dev.resample_low_percent, zero))[0])
    fill(lm_dev)
    res = ops.labelmatch_thresholds(*lm_dev._log, nc, 0, lm_dev.ignore_thres_low, lm_dev.ignore_thres_high, lm_dev.resample_low_percent, zero)
    h = res.host()

    host_ms, same = None, "not run"
    if not a.skip_host:
        try:
            import sklearn
            lm_host = creator(False)
            fill(lm_host)
            host_ms, _ = timed(lambda: lm_host.update_epoch_cls_thr(0))
            assert lm_host.cls_thr_high == h["thr_high"].tolist(), (lm_host.cls_thr_high, h["thr_high"].tolist())
            assert lm_host.cls_thr_low == h["thr_low"].tolist(), (lm_host.cls_thr_low, h["thr_low"].tolist())
            same = f"equal on all {nc} classes (sklearn {sklearn.__version__})"
        except ImportError as e:
            same = f"host leg not run: {e}"

    def fmt(v):
        return f"median {statistics.median(v):9.3f} ms   all {[round(x, 3) for x in v]}"

    lines = [
        f"device {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
        f"log: {n} pairs over {nc} classes, capacity {cap}; class sizes {sizes[:4].tolist()} ... {sizes[-3:].tolist()}",
        f"EM iterations per class: min {int(h['n_iter'].min())} median {int(np.median(h['n_iter']))} max {int(h['n_iter'].max())}; "
        f"classes with thr_high > 0: {int((h['thr_high'] > 0).sum())}",
        f"thresholds, device vs host path: {same}",
        f"  (host)   update_epoch_cls_thr, default path, once        {'%9.1f ms' % host_ms if host_ms is not None else '      n/a'}",
        f"  (device) update_epoch_cls_thr, device_thresholds=True    {fmt(whole)}",
        f"  (device) launches only, no read                          {fmt(launches)}",
        f"  (device) launches only, 2048 pairs in the same log       {fmt(small)}",
    ]
    if host_ms is not None:
        lines.append(f"host / device = {host_ms / statistics.median(whole):.1f}x")
    lines += ["clocks (read only):", clocks()]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
