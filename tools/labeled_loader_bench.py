"""Time the labeled batch generator (utils/augment.py LabeledBatchGenerator) on one GPU and hold it to its budget.

    python bench.py --gpus 1 --steps 40 --warmup 5 > bench.json          # the step the generator shares the GPU with, same session
    python tools/labeled_loader_bench.py --bench-json bench.json [--out profiles/labeled_loader_mi355x.txt]

Measured in one process, with HIP events around the launches, median of `--reps` after a warm-up:
  (1) et_labeled_mosaic_u8 for one batch of B = 32 images at S = 640 with a mixup partner on EVERY image (eight source images and two
      warps per output pixel: the most the recipe asks of the kernel), HSV LUTs and flips on;
  (2) et_labeled_mosaic_targets for the same batch (COCO density: about 7 labels per source image);
  (3) the whole generator call -- host recipe, table building, the small host->device copies, both kernels -- between two events;
  (4) et_strong_view_u8 at the same B and S (the unlabeled stream's kernel: one image, one warp per pixel);
and, with the host clock, the Python time of sample() for the 32 images of a batch.
GATE: the generator shares the GPU with the training step, so its device time per batch, (1) + (2), must stay under 10 % of the step
time bench.py measured in the same session (its `ms_per_step`; the labeled batch of that step is the 32 images this batch feeds).
The tool exits non-zero when the gate fails."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientteacher_amd import ops  # noqa: E402
from efficientteacher_amd.utils.augment import LabeledBatchGenerator, StrongViewGenerator  # noqa: E402


def event_ms(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--bench-json", default="", help="file holding bench.py's JSON line of this session")
    ap.add_argument("--step-ms", type=float, default=0.0, help="the step time, when no --bench-json is given")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    step_ms = a.step_ms
    if a.bench_json:
        with open(a.bench_json) as f:
            line = [ln for ln in f.read().splitlines() if ln.startswith("{")][-1]
        step_ms = float(json.loads(line)["ms_per_step"])
    if step_ms <= 0:
        raise SystemExit("need --bench-json or --step-ms: the gate is relative to the measured step")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, S = a.batch, a.size
    rng = np.random.default_rng(0)
    # load_image's output: the longest side is S, the other one as COCO's aspect ratios have it
    shapes = [(S, int(rng.integers(S * 2 // 3, S + 1))) if rng.random() < 0.3 else (int(rng.integers(S * 2 // 3, S + 1)), S)
              for _ in range(a.images)]
    images = [torch.from_numpy(rng.integers(0, 256, (3, h, w), dtype=np.uint8)).to(dev) for h, w in shapes]
    labels = []
    for _ in shapes:
        n = int(rng.poisson(7.0))
        xy = rng.uniform(0.1, 0.9, (n, 2))
        wh = np.minimum(np.exp(rng.uniform(np.log(0.02), np.log(0.6), (n, 2))), 2 * np.minimum(xy, 1 - xy))
        labels.append(np.concatenate((rng.integers(0, 80, (n, 1)), xy, wh), 1).astype(np.float32))
    hyp = types.SimpleNamespace(mosaic=1.0, mixup=1.0, copy_paste=0.0, degrees=0.0, translate=0.1, scale=0.9, shear=0.0, perspective=0.0,
                                hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, flipud=0.0, fliplr=0.5, cutout=0.0)
    cfg = types.SimpleNamespace(hyp=hyp, Dataset=types.SimpleNamespace(img_size=S, np=0, num_ids=0))
    gen = LabeledBatchGenerator(cfg, n=a.images, seed=0)
    idx = [int(i) for i in rng.integers(0, a.images, B)]

    # capture the arguments of one generator call so that the two kernels can be timed alone
    cap = {}
    real_px, real_lb = ops.labeled_mosaic_u8, ops.labeled_mosaic_targets
    ops.labeled_mosaic_u8 = lambda *x: cap.setdefault("px", x) and real_px(*x)
    ops.labeled_mosaic_targets = lambda *x: cap.setdefault("lb", x) and real_lb(*x)
    try:
        imgs, targets, _, _ = gen(images, labels, idx)
    finally:
        ops.labeled_mosaic_u8, ops.labeled_mosaic_targets = real_px, real_lb
    tiles, layouts, minv, mix, lut, flags, _ = cap["px"]
    table = torch.from_numpy(ops.labeled_tile_table(tiles, layouts, S)).to(dev)
    out = torch.empty((B, 3, S, S), dtype=torch.uint8, device=dev)
    from efficientteacher_amd import _lib
    lib = _lib.load()

    def pixels():
        _lib.check(lib.et_labeled_mosaic_u8(_lib.ptr(table), _lib.ptr(minv), _lib.ptr(mix), _lib.ptr(lut), _lib.ptr(flags), _lib.ptr(out),
                                            B, S, 114, _lib.stream(out)), "et_labeled_mosaic_u8")
    pixels()
    assert torch.equal(out, imgs)                              # the bare launch reproduces the generator's batch
    t_px = event_ms(pixels, a.reps)
    t_lb = event_ms(lambda: real_lb(*cap["lb"]), a.reps)
    t_all = event_ms(lambda: gen(images, labels, idx), a.reps)
    sv = StrongViewGenerator(hyp, seed=0)
    weak = torch.from_numpy(rng.integers(0, 256, (B, 3, S, S), dtype=np.uint8)).to(dev)
    s_minv, s_lut, s_cuts, s_flags, _ = sv.sample(B, S, S)
    t = lambda x: torch.from_numpy(x).to(dev)
    s_args = (weak, t(s_minv), t(s_lut), t(s_cuts), t(s_flags))
    t_sv = event_ms(lambda: ops.strong_view_u8(*s_args), a.reps)
    host = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for i in idx:
            gen.sample(i)
        host.append((time.perf_counter() - t0) * 1e3)

    med = statistics.median
    px, lb, al, svm, hs = med(t_px), med(t_lb), med(t_all), med(t_sv), med(host)
    device_ms = px + lb
    share = device_ms / step_ms
    gate = share < 0.10
    lines = [
        f"device {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
        f"batch: {B} labeled images at {S}, mixup partner on every image (8 source images of {a.images}, 2 warps per pixel), HSV LUTs, fliplr 0.5; "
        f"{int(cap['lb'][0].shape[0])} source labels -> {int(targets.shape[0])} target rows",
        f"HIP events, median of {a.reps} (min .. max):",
        f"  (1) et_labeled_mosaic_u8          {px:8.3f} ms   ({min(t_px):.3f} .. {max(t_px):.3f})",
        f"  (2) et_labeled_mosaic_targets     {lb:8.3f} ms   ({min(t_lb):.3f} .. {max(t_lb):.3f})   two launches + scratch allocation",
        f"  (3) generator call, whole         {al:8.3f} ms   ({min(t_all):.3f} .. {max(t_all):.3f})   host recipe + tables + copies + kernels + read of n",
        f"  (4) et_strong_view_u8, same B, S  {svm:8.3f} ms   ({min(t_sv):.3f} .. {max(t_sv):.3f})",
        f"host clock: sample() for the {B} images of a batch {hs:8.3f} ms   ({min(host):.3f} .. {max(host):.3f})",
        f"ratio (1) / (4): {px / svm:.2f} x   (expected about 2 x: twice the taps, plus the tile lookup per tap)",
        f"step of the default workload (bench.py --gpus 1, this session): {step_ms:.3f} ms",
        f"device time of the generator per batch, (1) + (2): {device_ms:.3f} ms = {100 * share:.2f} % of the step",
        f"GATE (< 10 % of the step): {'holds' if gate else 'FAILS'}",
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not gate:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
