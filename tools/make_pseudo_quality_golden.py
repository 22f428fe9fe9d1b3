"""Write tests/golden/pseudo_quality.npz: seeded synthetic pseudo-label tables with ground truth and what the LIVE reference computes
for them.

The reference is imported through oracle/ref_loader.py (nothing of it is copied): its ``check_pseudo_label_with_gt`` and
``check_pseudo_label`` (utils/self_supervised_utils.py:481-609) run on the compacted rows as trainer/ssod_trainer.py:655-672 calls
them, zeros when no pseudo label exists (:658-660).  They get clones: the reference scales ``labels`` in place.  Needs the reference
tree, so it runs in the build container only:

    python tools/make_pseudo_quality_golden.py

The cases are tests.pseudo_quality_ref.synth's (A mixed, B wide, C crowded, D0 / D1 / D2 degenerate).  For each the generator
ASSERTS the conditions outside which the reference is no yardstick and moves on to the next seed until they hold:
  (a) within a category no pseudo row has two qualifying labels of equal IoU (the reference leaves that to an unstable argsort);
  (b) every same-image IoU differs from 0.5 and from 0.01 by more than 1e-5;
  (c) in case A every category counts at least 3, and in at least one category two rows pick the same label, so that
      "distinct labels" differs from "rows"; the confidences sit on both thresholds; image 1 has no label, image 2 no pseudo row."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import pseudo_quality_ref as pr  # noqa: E402

SEED0 = 20261019


class Unfit(Exception):
    pass


def need(ok, why):
    if not ok:
        raise Unfit(why)


def reference_numbers(case, fns):
    check_with_gt, check_without, box_iou, xywh2xyxy = fns
    t9, valid, gt, lo, hi, bs = (case[k] for k in ("t9", "valid", "gt", "lo", "hi", "bs"))
    rows = torch.from_numpy(t9[valid.astype(bool)].copy())                       # (n, 9) fp64, as the reference's trainer holds them
    labels = torch.from_numpy(gt.copy())
    if rows.shape[0] == 0:                                                       # ssod_trainer.py:658-660
        return np.zeros(5), np.zeros(5), dict(counts=(0, 0, 0), shared=False)
    tp, fp_cls, fp_loc, pse, gtn = check_with_gt(rows.clone(), labels.clone(), ignore_thres_low=lo.tolist(),
                                                 ignore_thres_high=hi.tolist(), batch_size=bs)
    assert torch.equal(labels, torch.from_numpy(gt))                            # the clone took the in-place scaling
    want1 = np.array([float(np.asarray(v).reshape(-1)[0]) for v in (tp, fp_cls, fp_loc)] + [float(pse), float(gtn)])
    prec, rec, both, rel = check_without(rows.clone(), ignore_thres_low=lo.tolist(), ignore_thres_high=hi.tolist(), batch_size=bs)
    want0 = np.array([float(prec), 0.0, float(rec), float(both), float(rel)])   # ssod_trainer.py:667-671
    # the conditions, from the reference's own box arithmetic
    _, unc = pr.split_rows(t9, valid, lo, hi)
    u = torch.from_numpy(t9[unc].astype(np.float32))
    info = dict(counts=(0, 0, 0), shared=False)
    if u.shape[0] and labels.shape[0]:
        s = torch.tensor([640, 640] * 2)
        g = xywh2xyxy(labels[:, 2:6] * s) + labels[:, 0:1] * s
        p = xywh2xyxy(u[:, 2:6] * s) + u[:, 0:1] * s
        iou = box_iou(g, p)
        same_img = labels[:, 0:1] == u[:, 0]
        same_cls = labels[:, 1:2] == u[:, 1]
        near = same_img & (((iou - 0.5).abs() <= 1e-5) | ((iou - 0.01).abs() <= 1e-5))
        need(not near.any(), "(b) an IoU within 1e-5 of a threshold")
        cats = [(iou >= 0.5) & same_cls & same_img, (iou >= 0.5) & ~same_cls & same_img, (iou < 0.5) & (iou > 0.01) & same_img]
        counts, shared = [], False
        for q in cats:
            picked = []
            for d in range(q.shape[1]):
                col = iou[:, d][q[:, d]]
                need(col.unique().numel() == col.numel(), "(a) two qualifying labels of equal IoU")
                if col.numel():
                    picked.append(int(torch.where(q[:, d], iou[:, d], torch.full_like(iou[:, d], -1.0)).argmax()))
            counts.append(len(set(picked)))
            shared |= len(set(picked)) < len(picked)
        info = dict(counts=tuple(counts), shared=shared)
        n = int(unc.sum())
        assert np.array_equal(want1[:3], np.array(counts, np.float64) / n), (want1, counts, n)   # distinct labels IS what it yields
    return want1, want0, info


def fit(name, case, info):
    t9, valid, gt, lo, hi = (case[k] for k in ("t9", "valid", "gt", "lo", "hi"))
    rel, unc = pr.split_rows(t9, valid, lo, hi)
    v = valid.astype(bool)
    c = t9[:, 1].astype(np.int64)
    if name == "A":
        need(min(info["counts"]) >= 3, f"(c) counts {info['counts']}")
        need(info["shared"], "(c) no label is picked twice")
        need((v & (t9[:, 6] == hi[c])).any() and (v & (t9[:, 6] == lo[c])).any(), "no confidence on a threshold")
        need(set(lo) == {0.125, 0.25} and set(hi) == {0.5, 0.75}, "thresholds")
        need(not (gt[:, 0] == 1).any() and not (v & (t9[:, 0] == 2)).any() and (unc & (t9[:, 0] == 1)).any(), "empty images")
        need(35 <= gt.shape[0] <= 45 and not np.array_equal(gt[:, 0], np.sort(gt[:, 0])), "labels")
    elif name == "B":
        need(sum(info["counts"]) >= 6 and (unc & (t9[:, 0] == 31)).any() and (gt[:, 0] >= 24).any(), "wide: nothing far out")
    elif name == "C":
        need((gt[:, 0] == 0).sum() == 150 and (v & (t9[:, 0] == 0)).sum() == 60 and min(info["counts"][0::2]) >= 3, "crowded")
    elif name == "D0":
        need(gt.shape[0] == 0 and unc.any(), "D0")
    elif name == "D1":
        need(not v.any() and gt.shape[0] > 0, "D1")
    elif name == "D2":
        need(v.any() and not unc.any() and rel.any() and gt.shape[0] > 0, "D2")


def main():
    ref_loader.load()
    from utils.general import xywh2xyxy
    from utils.metrics import box_iou
    from utils.self_supervised_utils import check_pseudo_label, check_pseudo_label_with_gt
    fns = (check_pseudo_label_with_gt, check_pseudo_label, box_iou, xywh2xyxy)
    out = {}
    for name in pr.CASES:
        for seed in range(SEED0, SEED0 + 200):
            case = pr.synth(name, seed)
            try:
                want1, want0, info = reference_numbers(case, fns)
                fit(name, case, info)
            except Unfit as e:
                print(f"case {name} seed {seed}: {e}")
                continue
            break
        else:
            raise SystemExit(f"case {name}: no seed fits")
        for k, val in case.items():
            out[f"{name}_{k}"] = np.asarray(val)
        out[f"{name}_with_gt"], out[f"{name}_without_gt"], out[f"{name}_seed"] = want1, want0, np.array(seed)
        print(f"case {name} seed {seed}: M {case['gt'].shape[0]} valid {int(case['valid'].sum())} distinct labels {info['counts']} "
              f"shared {info['shared']}\n   with_gt {want1.tolist()}\n   without {want0.tolist()}")
    path = os.path.join(ROOT, "tests", "golden", "pseudo_quality.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
