"""Time the on-device validation metrics against the host path they replace, on one GPU in one process.

    python tools/val_metrics_bench.py [--images 5000] [--batch 32] [--out profiles/val_metrics_mi355x.txt]

For a synthetic set (tests/val_metrics_ref.synth: 80 classes, up to 300 detections per image), every region between two device
synchronisations, median of several repeats after a warm-up:
  (A) the per-image host loop: each image's detections and labels fetched with .cpu(), matched in numpy, then numpy ap_per_class
      (tests/val_metrics_ref.host_path -- the helper, not the code under test);
  (B) DetectionMetrics.update once per batch + compute().
Both see the same device tensors; the results are compared before the times are reported."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientteacher_amd.val import DetectionMetrics  # noqa: E402
from tests import val_metrics_ref as vr  # noqa: E402


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return "\n".join(l for l in out.splitlines() if "clk" in l.lower()) or "(rocm-smi printed no clocks)"
    except Exception as e:  # reading only; never fatal
        return f"(clocks not readable: {e})"


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
    iouv = torch.linspace(0.5, 0.95, 10).numpy()
    data = vr.synth(11, a.images, a.batch, nc, max_det, net_hw, max_labels=14, max_fp=600)
    fed = [tuple(torch.as_tensor(x).to(dev) for x in b) for b in data]
    ndet = sum(int(b[1].sum()) for b in data)

    def host():
        h = vr.host_path(fed, net_hw, iouv, nc, to_host=lambda t: t.cpu().numpy())
        return vr.summarize(*h[:4], h[4])

    def device():
        m = DetectionMetrics(nc, max_det=max_det, device=dev)
        for d, c, t, r in fed:
            m.update(d, c, t, r, net_hw)
        return m.compute()

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

    res, tb = timed(device, 2, a.repeats_device)
    ref, ta = timed(host, 1, a.repeats_host)
    assert abs(res.map - ref["map"]) <= 1e-12 and abs(res.map50 - ref["map50"]) <= 1e-12, (res.map, ref["map"])
    ma, mb = statistics.median(ta), statistics.median(tb)
    lines = [
        f"device {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
        f"set: {a.images} images, {len(fed)} batches of {a.batch}, {ndet} detections, max_det {max_det}, {nc} classes, 10 thresholds",
        f"mAP@.5 {res.map50:.6f} mAP@.5:.95 {res.map:.6f} (device == host helper within 1e-12)",
        f"(A) host loop + numpy ap_per_class : median {ma * 1e3:10.2f} ms   all {[round(t * 1e3, 2) for t in ta]}",
        f"(B) update x {len(fed)} + compute()      : median {mb * 1e3:10.2f} ms   all {[round(t * 1e3, 2) for t in tb]}",
        f"ratio B / A = {mb / ma:.5f}  (A / B = {ma / mb:.1f}x)",
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
