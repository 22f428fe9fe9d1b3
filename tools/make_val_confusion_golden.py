"""Write tests/golden/val_confusion.npz: seeded synthetic validation batches and what the LIVE reference computes for them.

The reference is imported through oracle/ref_loader.py (nothing of it is copied): its ``scale_coords``, ``xywh2xyxy``,
``ConfusionMatrix(nc).process_batch`` (utils/metrics.py:137) and ``save_one_json`` (val.py:67) run exactly as val.py:340-382 strings
them together, on CPU tensors.  Needs the reference tree, so it runs in the build container only:

    python tools/make_val_confusion_golden.py

The batches are tests.val_metrics_ref.synth's, post-processed so that every case of the closed form occurs (an image whose detections
all lie at or below the confidence filter, an image whose labels overlap nothing, a label doubled with a small shift so that
detections qualify for two labels).  The generator ASSERTS that they all occur, and that neither tie the reference leaves to an
unstable sort does: no detection has two qualifying labels of equal IoU, no label two candidate detections of equal IoU."""
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import val_metrics_ref as vr  # noqa: E402

NC, MAX_DET, NET_HW, SEED = 6, 100, (512, 640), 20261018
CONF, IOU = 0.25, 0.45
LOW_CONF_IMAGE, NO_MATCH_IMAGE, DOUBLED_IMAGE = 1, 9, 12          # global image indices; 3 has no labels, 5 no detections


def batches():
    data = vr.synth(SEED, 20, 8, NC, MAX_DET, NET_HW, empty_label_image=3, empty_det_image=5)
    out = []
    for bi, (dets, counts, targets, rows) in enumerate(data):
        dets, targets = dets.copy(), targets.copy()
        for si in range(dets.shape[0]):
            g = bi * 8 + si
            mine = targets[:, 0] == si
            if g == LOW_CONF_IMAGE:                                  # order kept, every confidence at or below the filter
                dets[si, :, 4] *= np.float32(0.25)
            if g == NO_MATCH_IMAGE:                                  # labels shrunk to specks: no pair reaches the IoU filter
                targets[mine, 4:6] = np.float32(0.004)
            if g == DOUBLED_IMAGE:                                   # every label once more, shifted by 6 % of its width
                twin = targets[mine].copy()
                twin[:, 2] += np.float32(0.06) * twin[:, 4]
                targets = np.concatenate((targets, twin), 0)
        out.append((dets, counts, targets[np.argsort(targets[:, 0], kind="stable")], rows))
    return out


def paths_of(bi, B):
    # numeric stems become int image ids, the others stay strings (val.py:69)
    return [f"{bi * 8 + si:012d}.jpg" if (bi + si) % 2 == 0 else f"val/img_b{bi}_{si}.png" for si in range(B)]


def main():
    ref_loader.load()
    import val as ref_val
    from utils.general import scale_coords, xywh2xyxy, xyxy2xywh
    from utils.metrics import ConfusionMatrix, box_iou
    data = batches()
    cm = ConfusionMatrix(NC)
    assert cm.conf == CONF and cm.iou_thres == IOU
    class_map = list(range(1000))                                    # val.py:241 for a set that is not COCO
    jdict, out = [], {}
    seen = dict.fromkeys(("diag", "offdiag", "unmatched_label", "unmatched_det", "no_match", "no_labels", "no_dets", "all_low",
                          "shared_label", "two_labels"), 0)
    for bi, (dets, counts, targets, rows) in enumerate(data):
        B = dets.shape[0]
        paths = paths_of(bi, B)
        for k, v in (("dets", dets), ("counts", counts), ("targets", targets), ("rows", rows), ("paths", np.array(paths))):
            out[f"{k}{bi}"] = v
        tg = torch.from_numpy(targets.copy())
        tg[:, 2:6] *= torch.Tensor([NET_HW[1], NET_HW[0]] * 2)                       # val.py:328
        predn_all = np.zeros((B, MAX_DET, 6), dtype=np.float32)
        tl_all = np.zeros((B, MAX_DET, 4), dtype=np.float32)
        for si in range(B):
            pred = torch.from_numpy(dets[si, :counts[si]].copy())
            labels = tg[tg[:, 0] == si, 1:]
            gain, padx, pady, h0, w0 = (float(v) for v in rows[si])
            shape, ratio_pad = (int(h0), int(w0)), ((gain, gain), (padx, pady))
            if len(pred) == 0:                                                       # val.py:347-350
                seen["no_dets"] += len(labels) > 0
                continue
            predn = pred.clone()
            scale_coords(NET_HW, predn[:, :4], shape, ratio_pad)                     # val.py:356
            if len(labels):
                tbox = xywh2xyxy(labels[:, 1:5])
                scale_coords(NET_HW, tbox, shape, ratio_pad)
                labelsn = torch.cat((labels[:, 0:1], tbox), 1)
                cm.process_batch(predn, labelsn)                                     # val.py:373
                census(seen, predn, labelsn, box_iou)
            else:
                seen["no_labels"] += 1
            n0 = len(jdict)
            ref_val.save_one_json(predn, jdict, Path(paths[si]), class_map)         # val.py:382
            assert len(jdict) - n0 == len(pred)
            box = xyxy2xywh(predn[:, :4])
            box[:, :2] -= box[:, 2:] / 2
            predn_all[si, :len(pred)], tl_all[si, :len(pred)] = predn.numpy(), box.numpy()
        out[f"predn{bi}"], out[f"xywh_tl{bi}"] = predn_all, tl_all
    missing = [k for k, v in seen.items() if not v]
    assert not missing, f"cases the golden must hold do not occur: {missing} (pick another seed)"
    assert cm.matrix.sum() > 0 and np.array_equal(cm.matrix, np.round(cm.matrix))
    ids = [d["image_id"] for d in jdict]
    out.update(matrix=cm.matrix.astype(np.int64), nbatches=np.array(len(data)), meta=np.array([NC, MAX_DET, NET_HW[0], NET_HW[1]]),
               thresholds=np.array([CONF, IOU]), jd_image_id=np.array([str(i) for i in ids]),
               jd_id_is_int=np.array([isinstance(i, int) for i in ids]), jd_category_id=np.array([d["category_id"] for d in jdict]),
               jd_bbox=np.array([d["bbox"] for d in jdict], dtype=np.float64), jd_score=np.array([d["score"] for d in jdict]))
    path = os.path.join(ROOT, "tests", "golden", "val_confusion.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; json rows", len(jdict), "cases", seen)
    print(cm.matrix.astype(np.int64))


def census(seen, predn, labelsn, box_iou):
    """which cases of the closed form this image holds, worked out from the reference's own box_iou; asserts the absence of ties"""
    det = predn[predn[:, 4] > CONF]
    if len(det) == 0:
        seen["all_low"] += 1
        seen["unmatched_label"] += 1
        return
    iou = box_iou(labelsn[:, 1:], det[:, :4])
    q = iou > IOU
    val = torch.where(q, iou, torch.full_like(iou, -1.0))
    for d in range(val.shape[1]):                                    # tie of the first kind
        col = val[:, d][q[:, d]]
        assert col.unique().numel() == col.numel(), "two qualifying labels of equal IoU for one detection: pick another seed"
    seen["two_labels"] += int((q.sum(0) >= 2).any())
    has = q.any(0)
    lstar, best = val.argmax(0), val.max(0).values
    matched = 0
    winners = set()
    for l in range(val.shape[0]):
        ds = torch.nonzero(has & (lstar == l)).flatten()
        if len(ds) == 0:
            seen["unmatched_label"] += 1
            continue
        b = best[ds]
        assert b.unique().numel() == b.numel(), "two detections of equal IoU for one label: pick another seed"
        seen["shared_label"] += len(ds) >= 2
        d = int(ds[b.argmax()])
        winners.add(d)
        matched += 1
        same = int(det[d, 5]) == int(labelsn[l, 0])
        seen["diag" if same else "offdiag"] += 1
    if matched:
        seen["unmatched_det"] += len(winners) < len(det)
    else:
        seen["no_match"] += 1


if __name__ == "__main__":
    main()
