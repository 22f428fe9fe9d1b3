"""Plain-numpy statement of the pseudo-label hit rate (helper, like tests/val_confusion_ref.py): what et_pseudo_quality computes,
written from the closed form and independently of the kernel.  tests/test_pseudo_quality.py pins it on
tests/golden/pseudo_quality.npz (made from the live reference by tools/make_pseudo_quality_golden.py); tools/pseudo_quality_bench.py
uses it as the host path the device path is timed against.

with_gt (the reference's check_pseudo_label_with_gt, iouv = [0.5]):
  1. a row of the padded table takes part only if it is valid and UNCERTAIN: thr_low[cls] <= conf < thr_high[cls], in fp64;
  2. from there on fp32: box = xywh * 640, xywh2xyxy, + img * 640 on all four coordinates (640 is the reference's literal);
     IoU = inter / (area_label + area_pseudo - inter);
  3. pairs (label, pseudo) of the same image:  tp: iou >= 0.5, same class;  fp_cls: iou >= 0.5, other class;
     fp_loc: 0.01 < iou < 0.5, any class;
  4. per category every pseudo row picks its qualifying label of largest IoU (equal IoU: the lower label index); the count is the
     number of DISTINCT labels picked;
  5. [tp / n_unc, fp_cls / n_unc, fp_loc / n_unc (0 if n_unc == 0), n_unc / batch_size, M / batch_size]; five zeros if no row is valid.
without gt (check_pseudo_label as the trainer logs it): reliable = #(conf >= thr_high[cls]) / bs, uncertain = n_unc / bs ->
  [reliable / (reliable + uncertain), 0, (reliable + uncertain) * bs / n_valid, reliable + uncertain, reliable]."""
import numpy as np

F = np.float32
REF_SIZE = F(640)
MAX_DET = 300
CASES = ("A", "B", "C", "D0", "D1", "D2")


def split_rows(t9, valid, lo, hi):
    """(reliable, uncertain) boolean masks over the padded rows; the class index is clamped like et_select_targets does"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.asarray(valid).astype(bool)
    c = np.clip(np.trunc(t9[:, 1]).astype(np.int64), 0, len(lo) - 1)
    conf = t9[:, 6]
    return v & (conf >= hi[c]), v & (conf < hi[c]) & (conf >= lo[c])


def boxes(img, xywh):
    """img (k) fp32, xywh (k, 4) fp32 normalised -> (k, 4) fp32 corners in the reference's 640-pixel tiles"""
    img, s = np.asarray(img, F), np.asarray(xywh, F) * REF_SIZE
    hw, hh = s[:, 2] / F(2), s[:, 3] / F(2)
    xyxy = np.stack((s[:, 0] - hw, s[:, 1] - hh, s[:, 0] + hw, s[:, 1] + hh), 1)
    return xyxy + (img * REF_SIZE)[:, None]


def iou_matrix(lb, pb):
    """(M, 4), (n, 4) fp32 -> (M, n) fp32, box_iou's operation order with the labels as box1"""
    la = (lb[:, 2] - lb[:, 0]) * (lb[:, 3] - lb[:, 1])
    pa = (pb[:, 2] - pb[:, 0]) * (pb[:, 3] - pb[:, 1])
    w = np.maximum(np.minimum(lb[:, None, 2], pb[None, :, 2]) - np.maximum(lb[:, None, 0], pb[None, :, 0]), F(0))
    h = np.maximum(np.minimum(lb[:, None, 3], pb[None, :, 3]) - np.maximum(lb[:, None, 1], pb[None, :, 1]), F(0))
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (la[:, None] + pa[None, :] - inter)


def categories(rows, gt):
    """rows (n, 9) fp32 uncertain pseudo labels, gt (M, 6) fp32 -> (iou (M, n), [tp, fp_cls, fp_loc] boolean (M, n))"""
    rows, gt = np.asarray(rows, F), np.asarray(gt, F)
    iou = iou_matrix(boxes(gt[:, 0], gt[:, 2:6]), boxes(rows[:, 0], rows[:, 2:6]))
    same_img = gt[:, 0:1] == rows[None, :, 0]
    same_cls = gt[:, 1:2] == rows[None, :, 1]
    hit = iou >= F(0.5)
    return iou, [hit & same_cls & same_img, hit & ~same_cls & same_img, (iou < F(0.5)) & (iou > F(0.01)) & same_img]


def distinct_labels(iou, q):
    """every pseudo row (column) with a qualifying label picks the one of largest IoU (first maximum = lower index)"""
    if q.shape[0] == 0 or q.shape[1] == 0:
        return 0, np.zeros(0, np.int64)
    cols = np.nonzero(q.any(0))[0]
    picked = np.where(q, iou, F(-1))[:, cols].argmax(0)
    return len(np.unique(picked)), picked


def match_counts(rows, gt):
    """(tp, fp_cls, fp_loc) distinct-label counts of compacted uncertain rows (n, 9) against gt (M, 6)"""
    iou, cats = categories(rows, gt)
    return tuple(distinct_labels(iou, q)[0] for q in cats)


def hit_rate(t9, valid, gt, lo, hi, batch_size, with_gt=True):
    """-> (5,) fp64 [tp, fp_cls, fp_loc, pse_num, gt_num]"""
    t9 = np.asarray(t9, np.float64)
    rel, unc = split_rows(t9, valid, lo, hi)
    n_valid, n_rel, n_unc = int(np.asarray(valid).astype(bool).sum()), int(rel.sum()), int(unc.sum())
    bs = float(batch_size)
    out = np.zeros(5, np.float64)
    if with_gt:
        gt = np.asarray(gt, F).reshape(-1, 6)
        if n_valid == 0:
            return out
        if n_unc:
            out[:3] = np.array(match_counts(t9[unc].astype(F), gt), np.float64) / float(n_unc)
        out[3], out[4] = n_unc / bs, gt.shape[0] / bs
        return out
    # the torch-op chain of the trainer adapter before the kernel existed, in numpy fp64
    reliable, uncertain = n_rel / bs, n_unc / bs
    both = reliable + uncertain
    out[0] = reliable / both if both > 0 else 0.0
    out[2] = both * bs / float(n_valid) if n_valid > 0 else 0.0
    out[3], out[4] = both, reliable
    return out


# ---- seeded synthetic cases (the generator of the golden draws from here; the tests read the npz) --------------------------------
def _f32(a):
    return np.asarray(a, np.float64).astype(F).astype(np.float64)


def _label_boxes(rng, k, wh):
    return np.concatenate((rng.uniform(0.15, 0.85, (k, 2)), rng.uniform(wh[0], wh[1], (k, 2))), 1)


def _jitter(rng, box, kind):
    """a pseudo box made from a label box: 'hit' overlaps it well, 'loc' poorly, 'far' not at all"""
    x, y, w, h = box
    if kind == "hit":
        return [x + rng.uniform(-0.06, 0.06) * w, y + rng.uniform(-0.06, 0.06) * h, w * rng.uniform(0.9, 1.1), h * rng.uniform(0.9, 1.1)]
    if kind == "loc":
        return [x + rng.choice([-1, 1]) * rng.uniform(0.45, 0.7) * w, y + rng.uniform(-0.1, 0.1) * h, w * rng.uniform(0.9, 1.1), h * rng.uniform(0.9, 1.1)]
    return [(x + 0.5) % 1.0, (y + 0.5) % 1.0, w * 0.5, h * 0.5]


def _conf(rng, kind, lo, hi):
    if kind == "unc":
        return rng.uniform(lo + 0.01, hi - 0.01)
    if kind == "unc_edge":
        return lo                                               # conf == thr_low: uncertain (>=)
    if kind == "rel_edge":
        return hi                                               # conf == thr_high: reliable (<), takes no part
    if kind == "rel":
        return rng.uniform(hi + 0.01, 0.99)
    return rng.uniform(0.01, lo - 0.01)                         # "low": below thr_low


def synth(case, seed):
    """-> dict(t9 (B*300, 9) fp64, valid uint8, gt (M, 6) fp32, lo, hi (nc) fp64, bs).  Every value of the table is an fp32 number.
    A: mixed (B 4, nc 5, 40 labels shuffled, image 1 without labels, image 2 without pseudo rows, a twin label in another image,
    confidences on both thresholds);  B: wide (B 32);  C: crowded (150 labels and 60 pseudo rows in one image);
    D0 / D1 / D2: no label, no valid row, no uncertain row."""
    rng = np.random.default_rng(seed)
    base = case[0]
    B, nc, wh = {"A": (4, 5, (0.08, 0.3)), "B": (32, 3, (0.08, 0.3)), "C": (2, 4, (0.03, 0.1)), "D": (3, 3, (0.08, 0.3))}[base]
    lo = rng.choice([0.125, 0.25], nc)
    hi = rng.choice([0.5, 0.75], nc)
    if base == "A":
        lo[:2], hi[:2] = [0.125, 0.25], [0.5, 0.75]                # both values of each list occur
    labels, pseudo = [], []                                      # rows [img, cls, x, y, w, h] / [img, cls, x, y, w, h, conf]
    for b in range(B):
        if base == "A":
            nl = 0 if b == 1 else 13 + (b == 3)
        elif base == "B":
            nl = int(rng.integers(0, 5))
        elif base == "C":
            nl = 150 if b == 0 else 5
        else:
            nl = 4
        lb = _label_boxes(rng, nl, wh)
        lc = rng.integers(0, nc, nl)
        labels += [[b, lc[i], *lb[i]] for i in range(nl)]
        if base == "A" and b == 2:
            continue
        if base == "B":
            npse = int(rng.integers(1, 4))
        elif base == "C":
            npse = 60 if b == 0 else 4
        else:
            npse = 14
        for k in range(npse):
            if nl:
                # two consecutive rows share a label now and then, so that "distinct labels" differs from "rows"
                i = int(rng.integers(0, nl)) if (k % 3 or not pseudo or pseudo[-1][0] != b) else pseudo[-1][-1]
                geo = rng.choice(["hit", "hit", "loc", "loc", "far"])
                c = int(lc[i]) if rng.random() < 0.5 else int((lc[i] + 1 + rng.integers(0, nc - 1)) % nc)
                box = _jitter(rng, lb[i], geo)
            else:
                i, c, box = -1, int(rng.integers(0, nc)), _label_boxes(rng, 1, wh)[0]
            kind = rng.choice(["unc", "unc", "unc", "unc", "unc_edge", "rel_edge", "rel", "low"])
            if case == "D2":
                kind = rng.choice(["rel_edge", "rel", "low"])
            pseudo.append([b, c, *box, _conf(rng, kind, lo[c], hi[c]), i])
    if base == "A":
        # a same-class label of image 0 at identical normalised coordinates, as an uncertain pseudo row of image 1
        twin = labels[3]
        pseudo.append([1, int(twin[1]), *twin[2:6], _conf(rng, "unc", lo[int(twin[1])], hi[int(twin[1])]), -1])
    pseudo.sort(key=lambda r: r[0])
    gt = np.array(labels, np.float64).reshape(-1, 6).astype(F)
    gt = gt[rng.permutation(gt.shape[0])]                        # any row order
    if case == "D0":
        gt = gt[:0]
    t9 = np.zeros((B * MAX_DET, 9), np.float64)
    valid = np.zeros(B * MAX_DET, np.uint8)
    t9[:, 0] = np.repeat(np.arange(B), MAX_DET)
    fill = np.zeros(B, np.int64)
    for r in pseudo:
        b = int(r[0])
        row = b * MAX_DET + fill[b]
        fill[b] += 1
        t9[row, :7] = _f32(r[:7])
        t9[row, 7], t9[row, 8] = _f32(min(1.0, r[6] + 0.02)), _f32(min(1.0, r[6] + 0.01))
        valid[row] = 1
    # padding rows that WOULD count if the valid mask were ignored: copies of live rows behind each image's last one
    for b in range(B):
        if fill[b]:
            t9[b * MAX_DET + fill[b] + 1] = t9[b * MAX_DET]
    if case == "D1":
        valid[:] = 0
    return dict(t9=t9, valid=valid, gt=gt, lo=lo.astype(np.float64), hi=hi.astype(np.float64), bs=B)
