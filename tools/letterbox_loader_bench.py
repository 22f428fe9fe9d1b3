"""Time the letterbox batch generator (utils/augment.py LetterboxBatchGenerator) on one GPU and hold both of its forms to their budget.

    python bench.py --gpus 1 --steps 40 --warmup 5 > bench.json          # the step the augment form shares the GPU with, same session
    python tools/letterbox_loader_bench.py --bench-json bench.json [--out profiles/letterbox_loader_mi355x.txt]

Measured in one process, with HIP events around the launches, median of `--reps` after a warm-up:
  VAL FORM (augment = False): one rect batch of B = 32 images letterboxed to 512 x 672 from sources whose long side is 640 -- 16 of
      480 x 640 (r == 1: a pad) and 16 of 640 x 640 (r = 0.8: the on-the-fly INTER_LINEAR resize)
    (1) et_letterbox_u8      (2) et_letterbox_targets      (3) the whole generator call
    (4) val.infer_batch (YOLOv5l of the default workload, bf16, padded NMS) on the batch (1) produced: what the val form feeds
  AUGMENT FORM (the closed mosaic): B = 32 images at 640 x 640 (sources 480 x 640 and 640 x 480), warp + HSV LUTs + flips
    (5) et_letterbox_u8      (6) et_letterbox_targets      (7) the whole generator call
  (8) et_strong_view_u8 at the same B and size, for scale (one resident image, one warp per pixel).
GATES: device time under 10 % of what it feeds -- (1) + (2) against (4); (5) + (6) against the step bench.py measured in the same
session (its `ms_per_step`).  The tool exits non-zero when a gate fails.
NOT measured: the reference's cv2 loader (cv2 is not installed), any real dataset, the generator running beside a live step."""
import argparse
import json
import os
import statistics
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientteacher_amd import ops  # noqa: E402
from efficientteacher_amd.utils.augment import LetterboxBatchGenerator, StrongViewGenerator  # noqa: E402


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


def coco_labels(rng, count):
    labels = []
    for _ in range(count):
        n = int(rng.poisson(7.0))
        xy = rng.uniform(0.1, 0.9, (n, 2))
        wh = np.minimum(np.exp(rng.uniform(np.log(0.02), np.log(0.6), (n, 2))), 2 * np.minimum(xy, 1 - xy))
        labels.append(np.concatenate((rng.integers(0, 80, (n, 1)), xy, wh), 1).astype(np.float32))
    return labels


def time_form(gen, images, labels, idx, reps):
    """-> (pixels ms list, labels ms list, whole-call ms list, the batch)"""
    cap = {}
    real_px, real_lb = ops.letterbox_u8, ops.letterbox_targets
    ops.letterbox_u8 = lambda *x: cap.setdefault("px", x) and real_px(*x)
    ops.letterbox_targets = lambda *x: cap.setdefault("lb", x) and real_lb(*x)
    state = gen.py_rng.getstate(), gen.np_rng.get_state()
    try:
        batch = gen(images, labels, idx)
    finally:
        ops.letterbox_u8, ops.letterbox_targets = real_px, real_lb
    assert torch.equal(real_px(*cap["px"]), batch[0])          # the bare launch reproduces the generator's batch
    t_px = event_ms(lambda: real_px(*cap["px"]), reps)
    t_lb = event_ms(lambda: real_lb(*cap["lb"]), reps)
    t_all = event_ms(lambda: gen(images, labels, idx), reps)
    gen.py_rng.setstate(state[0]); gen.np_rng.set_state(state[1])
    return t_px, t_lb, t_all, batch, int(cap["lb"][0].shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
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
        raise SystemExit("need --bench-json or --step-ms: the augment form's gate is relative to the measured step")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, S = a.batch, 640
    rng = np.random.default_rng(0)
    hyp = types.SimpleNamespace(mosaic=1.0, mixup=0.1, copy_paste=0.0, degrees=0.0, translate=0.1, scale=0.9, shear=0.0, perspective=0.0,
                                hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, flipud=0.0, fliplr=0.5, cutout=0.0)
    cfg = types.SimpleNamespace(hyp=hyp, Dataset=types.SimpleNamespace(img_size=S, np=0, num_ids=0))
    up = lambda h, w: torch.from_numpy(rng.integers(0, 256, (3, h, w), dtype=np.uint8)).to(dev)
    idx = list(range(B))
    labels = coco_labels(rng, B)

    # ---- val form: one rect batch, the shape of 4:3 landscape images (ceil(0.75 * 640 / 32 + 0.5) * 32 = 512, ceil(20.5) * 32 = 672)
    v_images = [up(480, 640) if k % 2 == 0 else up(640, 640) for k in range(B)]
    val_gen = LetterboxBatchGenerator(cfg, B, augment=False, rect=True, batch_size=B, stride=32, pad=0.5, shapes_wh=[(640, 480)] * B)
    assert val_gen.batch_shapes.tolist() == [[512, 672]]
    val_gen.order = np.arange(B)                               # every aspect ratio is equal: keep the images where they are
    v_px, v_lb, v_all, v_batch, v_rows = time_form(val_gen, v_images, labels, idx, a.reps)

    from efficientteacher_amd import val
    from efficientteacher_amd.configs import get_cfg
    from efficientteacher_amd.models.detector.yolo_ssod import Model
    mcfg = get_cfg()
    mcfg.merge_from_file(os.path.join(ROOT, "efficientteacher_amd", "configs", "ssod", "coco-standard", "yolov5l_coco_ssod_10_percent.yaml"))
    torch.manual_seed(0)
    model = Model(mcfg).to(dev).eval()
    with torch.no_grad():
        t_inf = event_ms(lambda: val.infer_batch(model, v_batch[0], half=True, padded=True), max(a.reps // 3, 5), warm=3)

    # ---- augment form: the closed mosaic
    a_images = [up(480, 640) if k % 2 == 0 else up(640, 480) for k in range(B)]
    aug_gen = LetterboxBatchGenerator(cfg, B, seed=0, augment=True)
    a_px, a_lb, a_all, a_batch, a_rows = time_form(aug_gen, a_images, labels, idx, a.reps)

    sv = StrongViewGenerator(hyp, seed=0)
    weak = torch.from_numpy(rng.integers(0, 256, (B, 3, S, S), dtype=np.uint8)).to(dev)
    s_minv, s_lut, s_cuts, s_flags, _ = sv.sample(B, S, S)
    t = lambda x: torch.from_numpy(x).to(dev)
    s_args = (weak, t(s_minv), t(s_lut), t(s_cuts), t(s_flags))
    t_sv = event_ms(lambda: ops.strong_view_u8(*s_args), a.reps)

    med = statistics.median
    row = lambda name, ts, note="": f"  {name:<38s}{med(ts):8.3f} ms   ({min(ts):.3f} .. {max(ts):.3f})   {note}".rstrip()
    v_dev, a_dev, inf = med(v_px) + med(v_lb), med(a_px) + med(a_lb), med(t_inf)
    v_share, a_share = v_dev / inf, a_dev / step_ms
    lines = [
        f"device {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
        f"HIP events, median of {a.reps} (min .. max); (4): median of {len(t_inf)}",
        f"VAL FORM: {B} images -> {tuple(v_batch[0].shape)}, 16 of 480 x 640 (pad only) + 16 of 640 x 640 (resize by 0.8); {v_rows} label rows",
        row("(1) et_letterbox_u8", v_px),
        row("(2) et_letterbox_targets", v_lb, "two launches + scratch allocation"),
        row("(3) generator call, whole", v_all, "geometry + tables + copies + kernels + read of n"),
        row("(4) val.infer_batch, YOLOv5l bf16", t_inf, "forward + padded NMS on the batch of (1)"),
        f"  device time of the val form per batch, (1) + (2): {v_dev:.3f} ms = {100 * v_share:.2f} % of (4)",
        f"  GATE (< 10 % of val.infer_batch): {'holds' if v_share < 0.10 else 'FAILS'}",
        f"AUGMENT FORM (closed mosaic): {B} images -> {tuple(a_batch[0].shape)}, warp + HSV LUTs + fliplr 0.5; {a_rows} label rows -> "
        f"{int(a_batch[1].shape[0])} target rows",
        row("(5) et_letterbox_u8", a_px),
        row("(6) et_letterbox_targets", a_lb),
        row("(7) generator call, whole", a_all, "host recipe + tables + copies + kernels + read of n"),
        row("(8) et_strong_view_u8, same B, 640 x 640", t_sv),
        f"  ratio (5) / (8): {med(a_px) / med(t_sv):.2f} x",
        f"  step of the default workload (bench.py --gpus 1, this session): {step_ms:.3f} ms",
        f"  device time of the augment form per batch, (5) + (6): {a_dev:.3f} ms = {100 * a_share:.2f} % of the step",
        f"  GATE (< 10 % of the step): {'holds' if a_share < 0.10 else 'FAILS'}",
        "NOT measured: the reference's cv2 loader, any real dataset, the generator beside a live step.",
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not (v_share < 0.10 and a_share < 0.10):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
