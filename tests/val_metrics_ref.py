"""Plain-numpy statement of the validation metrics (helper, like tests/exact_ref.py): what csrc/metrics.hip computes,
written independently of it.  tests/test_val_metrics.py pins it on tests/golden/val_metrics.npz (made from the live reference
by tools/make_val_golden.py) and then uses it as the yardstick for inputs the golden does not hold; tools/val_metrics_bench.py
uses it as the host path the device path is timed against.

Matching (reference val.py:123-145 in closed form, DESIGN.md "Validation metrics"): per detection d the class-matching label of
largest IoU l*(d) (equal IoU: lower label index), and correct[d, i] = iou(d, l*(d)) >= iouv[i] and d is the lowest detection index
among those that chose l*(d) with IoU >= iouv[i].  AP (utils/metrics.py:22-126): per class, rows by confidence descending
(equal confidence: input order), cumulative TP / FP, recall, precision, envelope, 101-point interpolation, trapezoid rule."""
import numpy as np

F = np.float32


def shape_row(h0, w0, net_hw):
    """letterbox of an (h0, w0) image into net_hw -> (python doubles) gain, pad_x, pad_y"""
    gain = min(net_hw[0] / h0, net_hw[1] / w0)
    return gain, (net_hw[1] - w0 * gain) / 2, (net_hw[0] - h0 * gain) / 2


def to_native(xyxy, row):
    """fp32: subtract pad, divide by gain, clamp to the native image; row = [gain, pad_x, pad_y, h0, w0] fp32"""
    b = np.array(xyxy, dtype=F).reshape(-1, 4)
    gain, px, py, h0, w0 = (F(v) for v in row)
    b[:, [0, 2]] = (b[:, [0, 2]] - px) / gain
    b[:, [1, 3]] = (b[:, [1, 3]] - py) / gain
    b[:, [0, 2]] = np.minimum(np.maximum(b[:, [0, 2]], F(0)), w0)
    b[:, [1, 3]] = np.minimum(np.maximum(b[:, [1, 3]], F(0)), h0)
    return b


def iou_matrix(lab, det):
    """(M, 4), (N, 4) fp32 xyxy -> (M, N) fp32, in the order inter / (area_l + area_d - inter)"""
    la = (lab[:, 2] - lab[:, 0]) * (lab[:, 3] - lab[:, 1])
    da = (det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1])
    w = np.maximum(np.minimum(lab[:, None, 2], det[None, :, 2]) - np.maximum(lab[:, None, 0], det[None, :, 0]), F(0))
    h = np.maximum(np.minimum(lab[:, None, 3], det[None, :, 3]) - np.maximum(lab[:, None, 1], det[None, :, 1]), F(0))
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (la[:, None] + da[None, :] - inter)


def match_image(det, labels, row, net_hw, iouv, single_cls=False):
    """det (n, 6) fp32 [xyxy letterbox pixels, conf, cls]; labels (m, 5) fp32 [cls, xywh normalised] -> correct (n, niou) bool"""
    iouv = np.asarray(iouv, dtype=F)
    n, m = det.shape[0], labels.shape[0]
    correct = np.zeros((n, iouv.size), dtype=bool)
    if n == 0 or m == 0:
        return correct
    scale = np.array([net_hw[1], net_hw[0], net_hw[1], net_hw[0]], dtype=F)
    xywh = labels[:, 1:5].astype(F) * scale
    half_w, half_h = xywh[:, 2] / F(2), xywh[:, 3] / F(2)
    lab = to_native(np.stack((xywh[:, 0] - half_w, xywh[:, 1] - half_h, xywh[:, 0] + half_w, xywh[:, 1] + half_h), 1), row)
    dn = to_native(det[:, :4], row)
    dcls = np.zeros(n, dtype=F) if single_cls else det[:, 5].astype(F)
    iou = iou_matrix(lab, dn)
    iou = np.where(labels[:, 0:1].astype(F) == dcls[None, :], iou, F(-1))
    iou = np.where(np.isnan(iou), F(-1), iou)
    best_l = iou.argmax(0)                                  # first maximum = lower label index
    best = iou[best_l, np.arange(n)]
    has = best >= 0
    for i, thr in enumerate(iouv):
        d = np.nonzero(has & (best >= thr))[0]             # ascending detection index
        first = np.unique(best_l[d], return_index=True)[1]  # per chosen label: its first (lowest) detection
        correct[d[first], i] = True
    return correct


def match_batch(dets, counts, targets, rows, net_hw, iouv, nc, single_cls=False):
    """the padded arena of one batch: correct (B*max_det) int32 bit masks, conf fp32, cls int32 (-1 padding), valid int32, nt (nc)"""
    B, max_det = dets.shape[0], dets.shape[1]
    correct = np.zeros(B * max_det, dtype=np.int32)
    conf = np.zeros(B * max_det, dtype=F)
    cls = np.full(B * max_det, -1, dtype=np.int32)
    valid = np.zeros(B * max_det, dtype=np.int32)
    nt = np.zeros(nc, dtype=np.int32)
    targets = np.asarray(targets, dtype=F).reshape(-1, 6)
    bits = (1 << np.arange(len(iouv))).astype(np.int32)
    for si in range(B):
        n = int(counts[si])
        lab = targets[targets[:, 0] == si, 1:]
        nt += np.bincount(lab[:, 0].astype(np.int64), minlength=nc)[:nc].astype(np.int32)
        c = match_image(dets[si, :n, :6], lab, rows[si], net_hw, iouv, single_cls)
        s = slice(si * max_det, si * max_det + n)
        correct[s] = (c * bits).sum(1)
        conf[s] = dets[si, :n, 4]
        cls[s] = 0 if single_cls else dets[si, :n, 5].astype(np.int32)
        valid[s] = 1
    return correct, conf, cls, valid, nt


def _interp_rightmost(x, xp, fp, left, right):
    """np.interp spelled out: for x equal to a repeated xp value the right-most such index is taken"""
    return np.interp(x, xp, fp, left=left, right=right)


def ap_per_class(tp, conf, pred_cls, nt):
    """tp (n, niou) bool, conf (n), pred_cls (n) int, nt (nc) labels per class ->
    ap (nc, niou), p, r, f1 (nc, 1000) fp64 indexed by CLASS (zero rows where a class has no labels or no predictions)"""
    nc, niou = len(nt), tp.shape[1]
    order = np.argsort(-conf.astype(np.float64), kind="stable")
    tp, conf, pred_cls = tp[order], conf[order], pred_cls[order]
    px = np.linspace(0, 1, 1000)
    x101 = np.linspace(0, 1, 101)
    ap = np.zeros((nc, niou))
    p, r = np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for c in range(nc):
        sel = pred_cls == c
        if nt[c] == 0 or not sel.any():
            continue
        tpc = tp[sel].cumsum(0).astype(np.float64)
        fpc = (~tp[sel]).cumsum(0).astype(np.float64)
        recall = tpc / (nt[c] + 1e-16)
        precision = tpc / (tpc + fpc)
        xc = -conf[sel].astype(np.float64)
        r[c] = _interp_rightmost(-px, xc, recall[:, 0], 0.0, None)
        p[c] = _interp_rightmost(-px, xc, precision[:, 0], 1.0, None)
        for j in range(niou):
            mrec = np.concatenate(([0.0], recall[:, j], [1.0]))
            mpre = np.concatenate(([1.0], precision[:, j], [0.0]))
            mpre = np.maximum.accumulate(mpre[::-1])[::-1]
            y = np.interp(x101, mrec, mpre)
            ap[c, j] = ((x101[1:] - x101[:-1]) * (y[1:] + y[:-1]) / 2.0).sum()
    f1 = 2 * p * r / (p + r + 1e-16)
    return ap, p, r, f1


def summarize(ap, p, r, f1, nt, any_correct=True):
    """the reference's reductions: ap_class, the F1-optimal index, p / r / f1 at it, cls_thr, mp, mr, map50, map, maps"""
    nc = len(nt)
    cl = np.nonzero(np.asarray(nt) > 0)[0]
    out = dict(ap_class=cl.astype(np.int32), maps=np.zeros(nc), mp=0.0, mr=0.0, map50=0.0, map=0.0, cls_thr=[], index=0)
    if not any_correct or cl.size == 0:
        out["ap_class"] = cl[:0].astype(np.int32)
        return out
    px = np.linspace(0, 1, 1000)
    i = int(f1[cl].mean(0).argmax())
    out.update(index=i, p=p[cl, i], r=r[cl, i], f1=f1[cl, i], ap=ap[cl], cls_thr=[px[k] for k in f1[cl].argmax(1)])
    apm = ap[cl].mean(1)
    out.update(mp=p[cl, i].mean(), mr=r[cl, i].mean(), map50=ap[cl, 0].mean(), map=apm.mean())
    out["maps"] = np.zeros(nc) + out["map"]
    out["maps"][cl] = apm
    return out


def host_path(batches, net_hw, iouv, nc, single_cls=False, to_host=np.asarray):
    """the per-image loop the device path replaces: every image's detections and labels fetched to the host (to_host), matched
    there, then ap_per_class over the concatenated statistics.  batches: iterable of (dets, counts, targets, rows)."""
    tps, confs, clss = [], [], []
    nt = np.zeros(nc, dtype=np.int64)
    for dets, counts, targets, rows in batches:
        B = dets.shape[0]
        for si in range(B):
            n = int(to_host(counts[si]))
            tg = to_host(targets).reshape(-1, 6)
            lab = tg[tg[:, 0] == si, 1:]
            nt += np.bincount(lab[:, 0].astype(np.int64), minlength=nc)[:nc]
            d = to_host(dets[si, :n])
            tps.append(match_image(d, lab, to_host(rows[si]), net_hw, iouv, single_cls))
            confs.append(d[:, 4])
            clss.append(np.zeros(n, dtype=np.int64) if single_cls else d[:, 5].astype(np.int64))
    tp, conf, cls = np.concatenate(tps, 0), np.concatenate(confs), np.concatenate(clss)
    return ap_per_class(tp, conf, cls, nt) + (nt,)


def synth(seed, n_images, batch, nc, max_det, net_hw=(512, 640), max_labels=24, label_classes=None, det_fp_classes=None,
          drop_det_class=None, empty_label_image=None, empty_det_image=None, max_fp=12):
    """Seeded synthetic validation set: detections jittered around labels (some class flips, some pure false positives), letterbox
    shapes with non-trivial gain and pad, globally distinct confidences (a permutation), rows sorted by confidence inside an image
    as NMS leaves them.  Returns a list of batches (dets (B, max_det, 6) fp32, counts int32, targets (NT, 6) fp32, rows (B, 5) fp32)."""
    rng = np.random.default_rng(seed)
    label_classes = np.arange(nc) if label_classes is None else np.asarray(label_classes)
    det_fp_classes = np.arange(nc) if det_fp_classes is None else np.asarray(det_fp_classes)
    per_image = []
    total = 0
    for g in range(n_images):
        h0, w0 = int(rng.integers(200, 900)), int(rng.integers(200, 900))
        gain, padx, pady = shape_row(h0, w0, net_hw)
        m = 0 if g == empty_label_image else int(rng.integers(1, max_labels + 1))
        cx, cy = rng.uniform(0.1, 0.9, m) * w0, rng.uniform(0.1, 0.9, m) * h0
        bw, bh = rng.uniform(0.05, 0.4, m) * w0, rng.uniform(0.05, 0.4, m) * h0
        lcls = rng.choice(label_classes, m)
        # labels in letterbox space, normalised xywh
        lab = np.stack((lcls, (cx * gain + padx) / net_hw[1], (cy * gain + pady) / net_hw[0], bw * gain / net_hw[1],
                        bh * gain / net_hw[0]), 1).reshape(-1, 5)
        boxes, dcls = [], []
        for k in range(m):
            for _ in range(int(rng.integers(0, 4))):
                j = rng.normal(0, 0.08, 4) * np.array([bw[k], bh[k], bw[k], bh[k]])
                x, y, w, h = cx[k] + j[0], cy[k] + j[1], bw[k] * np.exp(j[2] / bw[k]), bh[k] * np.exp(j[3] / bh[k])
                boxes.append([(x - w / 2) * gain + padx, (y - h / 2) * gain + pady, (x + w / 2) * gain + padx, (y + h / 2) * gain + pady])
                dcls.append(rng.choice(det_fp_classes) if rng.random() < 0.1 else lcls[k])
        nfp = int(rng.integers(0, max_fp + 1))
        x, y = rng.uniform(0, net_hw[1], nfp), rng.uniform(0, net_hw[0], nfp)
        w, h = rng.uniform(10, 200, nfp), rng.uniform(10, 200, nfp)
        fp = np.stack((x - w / 2, y - h / 2, x + w / 2, y + h / 2), 1)
        boxes = np.concatenate((np.array(boxes, dtype=np.float64).reshape(-1, 4), fp), 0)
        dcls = np.concatenate((np.array(dcls, dtype=np.float64), rng.choice(det_fp_classes, nfp).astype(np.float64)))
        keep = rng.permutation(boxes.shape[0])               # which rows survive the max_det cut is random
        boxes, dcls = boxes[keep], dcls[keep]
        if drop_det_class is not None:
            boxes, dcls = boxes[dcls != drop_det_class], dcls[dcls != drop_det_class]
        if g == empty_det_image:
            boxes, dcls = boxes[:0], dcls[:0]
        boxes, dcls = boxes[:max_det], dcls[:max_det]
        per_image.append((lab, boxes, dcls, (gain, padx, pady, h0, w0)))
        total += boxes.shape[0]
    ranks = rng.permutation(total)
    out, at = [], 0
    for b0 in range(0, n_images, batch):
        chunk = per_image[b0:b0 + batch]
        B = len(chunk)
        dets = np.zeros((B, max_det, 6), dtype=F)
        counts = np.zeros(B, dtype=np.int32)
        tg, rows = [], np.zeros((B, 5), dtype=F)
        for si, (lab, boxes, dcls, row) in enumerate(chunk):
            n = boxes.shape[0]
            conf = (ranks[at:at + n] + 1.0) / (total + 1.0)
            at += n
            o = np.argsort(-conf)
            dets[si, :n, :4], dets[si, :n, 4], dets[si, :n, 5] = boxes[o], conf[o], dcls[o]
            counts[si] = n
            rows[si] = row
            tg.append(np.concatenate((np.full((lab.shape[0], 1), si), lab), 1))
        out.append((dets, counts, np.concatenate(tg, 0).astype(F).reshape(-1, 6), rows))
    return out
