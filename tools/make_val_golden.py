"""Write tests/golden/val_metrics.npz: seeded synthetic validation batches and what the LIVE reference computes for them.

The reference is imported through oracle/ref_loader.py (nothing of it is copied): its ``scale_coords``, ``xywh2xyxy``,
``process_batch`` (val.py:123), ``ap_per_class`` and ``fitness`` (utils/metrics.py) run exactly as val.py:340-403 strings them
together, on CPU tensors.  Needs the reference tree, so it runs in the build container only:

    python tools/make_val_golden.py

The generator ASSERTS the conditions outside which the reference's result hangs on an unstable sort and is no yardstick:
(a) no detection has two class-matching labels of equal IoU >= 0.5; (b) all confidences are distinct; (c) the two largest values
of f1.mean(0), and of every class's f1 row, differ by more than 1e-9."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import val_metrics_ref as vr  # noqa: E402

NC, MAX_DET, NET_HW, SEED = 6, 100, (512, 640), 20261016


def batches():
    # class 4 has labels and never a prediction, class 5 has predictions and never a label; image 3 has no labels, image 5 no detections
    return vr.synth(SEED, 20, 8, NC, MAX_DET, NET_HW, label_classes=[0, 1, 2, 3, 4], det_fp_classes=[0, 1, 2, 3, 5], drop_det_class=4,
                    empty_label_image=3, empty_det_image=5)


def main():
    ref_loader.load()
    import val as ref_val
    from utils.general import scale_coords, xywh2xyxy
    from utils.metrics import ap_per_class, box_iou, fitness
    iouv = torch.linspace(0.5, 0.95, 10)
    data = batches()
    out, stats, correct_rows = {}, [], []
    all_conf = []
    for bi, (dets, counts, targets, rows) in enumerate(data):
        for k, v in (("dets", dets), ("counts", counts), ("targets", targets), ("rows", rows)):
            out[f"{k}{bi}"] = v
        tg = torch.from_numpy(targets.copy())
        tg[:, 2:6] *= torch.Tensor([NET_HW[1], NET_HW[0]] * 2)                       # val.py:328
        arena = np.zeros((dets.shape[0] * MAX_DET, 10), dtype=bool)
        for si in range(dets.shape[0]):
            pred = torch.from_numpy(dets[si, :counts[si]].copy())
            labels = tg[tg[:, 0] == si, 1:]
            gain, padx, pady, h0, w0 = (float(v) for v in rows[si])
            shape, ratio_pad = (int(h0), int(w0)), ((gain, gain), (padx, pady))
            all_conf.append(pred[:, 4].numpy())
            if len(pred) == 0:
                if len(labels):
                    stats.append((torch.zeros(0, 10, dtype=torch.bool), torch.Tensor(), torch.Tensor(), labels[:, 0].tolist()))
                continue
            predn = pred.clone()
            scale_coords(NET_HW, predn[:, :4], shape, ratio_pad)
            if len(labels):
                tbox = xywh2xyxy(labels[:, 1:5])
                scale_coords(NET_HW, tbox, shape, ratio_pad)
                labelsn = torch.cat((labels[:, 0:1], tbox), 1)
                correct = ref_val.process_batch(predn, labelsn, iouv)
                # (a): no equal-IoU pair of class-matching labels at or above the first threshold
                iou = box_iou(labelsn[:, 1:], predn[:, :4])
                iou = torch.where(labelsn[:, 0:1] == predn[:, 5], iou, torch.full_like(iou, -1.0))
                top2 = torch.topk(iou, min(2, iou.shape[0]), 0).values
                if top2.shape[0] == 2:
                    assert not ((top2[0] == top2[1]) & (top2[0] >= 0.5)).any(), "equal-IoU label pair: pick another seed"
            else:
                correct = torch.zeros(pred.shape[0], 10, dtype=torch.bool)
            arena[si * MAX_DET:si * MAX_DET + len(pred)] = correct.numpy()
            stats.append((correct.cpu(), pred[:, 4].cpu(), pred[:, 5].cpu(), labels[:, 0].tolist()))
        correct_rows.append(arena)
    conf = np.concatenate(all_conf)
    assert np.unique(conf).size == conf.size, "(b) confidences collide"
    stats = [np.concatenate(x, 0) for x in zip(*stats)]
    assert stats[0].any()
    p, r, ap, f1, ap_class, cls_thr = ap_per_class(*stats, plot=False, names={})
    # (c) on the full curves, which ap_per_class does not return: recompute them with the helper (pinned on the returned values by
    # tests/test_val_metrics.py) and check the arg-max gaps there
    nt = np.bincount(stats[3].astype(np.int64), minlength=NC)
    hap, hp, hr, hf1 = vr.ap_per_class(stats[0], stats[1], stats[2].astype(np.int64), nt)
    cl = np.nonzero(nt > 0)[0]
    for row in [hf1[cl].mean(0)] + [hf1[c] for c in cl if hf1[c].any()]:
        top = np.sort(row)[-2:]
        assert top[1] - top[0] > 1e-9, "(c) F1 arg-max is a near tie: pick another seed"
    ap50, apm = ap[:, 0], ap.mean(1)
    res = np.array([[p.mean(), r.mean(), ap50.mean(), apm.mean()]])
    out.update(correct=np.concatenate(correct_rows, 0), iouv=iouv.numpy(), nt=nt, p=p, r=r, ap=ap, f1=f1, ap_class=ap_class,
               cls_thr=np.array(cls_thr), results=res, fitness=fitness(res), nbatches=np.array(len(data)),
               meta=np.array([NC, MAX_DET, NET_HW[0], NET_HW[1]]))
    path = os.path.join(ROOT, "tests", "golden", "val_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; images", sum(d[0].shape[0] for d in data), "detections", conf.size, "labels", int(nt.sum()),
          "mAP@.5", res[0, 2], "mAP", res[0, 3])


if __name__ == "__main__":
    main()
