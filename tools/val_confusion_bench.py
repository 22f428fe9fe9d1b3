"""Time the on-device confusion matrix against the host loop it replaces, on one GPU in one process.

    python tools/val_confusion_bench.py [--images 5000] [--batch 32] [--out profiles/val_confusion_mi355x.txt]

The method of tools/val_metrics_bench.py: a synthetic set (tests/val_metrics_ref.synth: 80 classes, up to 300 detections per image),
every region between two device synchronisations, median of several repeats after a warm-up:
  (A) the per-image host loop: each image's detections and labels fetched with .cpu(), the confusion matrix worked out in numpy
      (tests/val_confusion_ref.confusion_batches -- the helper, not the code under test), which is what the reference does;
  (B) DetectionMetrics.update once per batch without and with confusion=, the latter followed by one read of ``matrix``.
Both see the same device tensors; the matrices are compared before the times are reported."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientteacher_amd.val import ConfusionMatrix, DetectionMetrics  # noqa: E402
from tests import val_confusion_ref as cr  # noqa: E402
from tests import val_metrics_ref as vr  # noqa: E402
from tools.val_metrics_bench import clocks  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats-host", type=int, default=3)
    ap.add_argument("--repeats-device", type=int, default=11)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nc, max_det, net_hw = 80, 300, (640, 640)
    data = vr.synth(11, a.images, a.batch, nc, max_det, net_hw, max_labels=14, max_fp=600)
    fed = [tuple(torch.as_tensor(x).to(dev) for x in b) for b in data]
    ndet = sum(int(b[1].sum()) for b in data)

    def host():
        return cr.confusion_batches(fed, net_hw, nc, to_host=lambda t: t.cpu().numpy())

    def device(confusion):
        cm = ConfusionMatrix(nc, device=dev) if confusion else None
        m = DetectionMetrics(nc, max_det=max_det, device=dev, confusion=cm)
        for d, c, t, r in fed:
            m.update(d, c, t, r, net_hw)
        return cm.matrix if confusion else None

    def alone():
        cm = ConfusionMatrix(nc, device=dev)
        for d, c, t, r in fed:
            cm.update(d, c, t, r, net_hw)
        return cm.matrix

    def timed(fn, warm, reps):
        for _ in range(warm):
            out = fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return out, ts

    _, t0 = timed(lambda: device(False), 2, a.repeats_device)
    got, t1 = timed(lambda: device(True), 2, a.repeats_device)
    got2, t2 = timed(alone, 2, a.repeats_device)
    want, ta = timed(host, 1, a.repeats_host)
    assert np.array_equal(got, want) and np.array_equal(got2, want), "device matrix differs from the host helper's"
    ma, m0, m1, m2 = (statistics.median(t) for t in (ta, t0, t1, t2))
    ms = lambda ts: [round(t * 1e3, 2) for t in ts]  # noqa: E731
    lines = [
        f"device {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
        f"set: {a.images} images, {len(fed)} batches of {a.batch}, {ndet} detections, max_det {max_det}, {nc} classes",
        f"matrix: sum {int(want.sum())} diagonal {int(np.trace(want[:nc, :nc]))} background row {int(want[nc].sum())} "
        f"background column {int(want[:, nc].sum())} (device == host helper, array_equal)",
        f"(A)  host loop, .cpu() per image + numpy           : median {ma * 1e3:10.2f} ms   all {ms(ta)}",
        f"(B0) update x {len(fed)}, confusion=None               : median {m0 * 1e3:10.2f} ms   all {ms(t0)}",
        f"(B1) update x {len(fed)}, confusion=cm + matrix read   : median {m1 * 1e3:10.2f} ms   all {ms(t1)}",
        f"(B2) ConfusionMatrix.update x {len(fed)} + matrix read : median {m2 * 1e3:10.2f} ms   all {ms(t2)}",
        f"added per evaluation (B1 - B0) = {(m1 - m0) * 1e3:.2f} ms;  ratio B2 / A = {m2 / ma:.5f}  (A / B2 = {ma / m2:.1f}x);"
        f"  (B1 - B0) / A = {(m1 - m0) / ma:.5f}",
        "clocks (read only):", clocks(),
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
