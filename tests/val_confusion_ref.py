"""Plain-numpy statement of the confusion matrix and of the native-space predictions (helper, like tests/val_metrics_ref.py): what
et_val_confusion / et_val_predn compute, written from the closed form and independently of the kernels.
tests/test_val_confusion.py pins it on tests/golden/val_confusion.npz (made from the live reference by
tools/make_val_confusion_golden.py) and then uses it as the yardstick for inputs the golden does not hold;
tools/val_confusion_bench.py uses it as the host path the device path is timed against.

One image with at least one label and at least one NMS detection (any other image adds nothing):
  1. the detections with conf > conf_thres (strict) take part;
  2. class-agnostic IoU in native space; a pair qualifies if iou > iou_thres (strict);
  3. l*(d): the qualifying label of largest IoU of detection d (equal IoU: the lower label index);
  4. d*(l): the detection of largest IoU among those with l*(d) = l (equal IoU: the lower detection index);
  5. matrix[cls(d*(l)), cls(l)] += 1 per matched label, matrix[nc, cls(l)] += 1 per unmatched label, and, only if the image has a
     match, matrix[cls(d), nc] += 1 per filtered detection that is no d*(l);
  6. classes truncated to int, single_cls: detections are class 0; counts whose class lies outside [0, nc) are not made."""
import numpy as np

from tests import val_metrics_ref as vr

F = np.float32


def _cls(c, nc):
    c = np.trunc(np.asarray(c, dtype=np.float64)).astype(np.int64)
    return np.where((c >= 0) & (c < nc), c, -1)


def native_labels(labels, row, net_hw):
    """labels (m, 5) fp32 [cls, xywh normalised to the network input] -> (m, 4) fp32 xyxy in the native image"""
    scale = np.array([net_hw[1], net_hw[0], net_hw[1], net_hw[0]], dtype=F)
    xywh = labels[:, 1:5].astype(F) * scale
    hw, hh = xywh[:, 2] / F(2), xywh[:, 3] / F(2)
    return vr.to_native(np.stack((xywh[:, 0] - hw, xywh[:, 1] - hh, xywh[:, 0] + hw, xywh[:, 1] + hh), 1), row)


def confusion_native(matrix, dn, dconf, dcls, ln, lcls, nc, conf=0.25, iou_thres=0.45):
    """one image in native space: dn (n, 4), dconf (n), dcls (n); ln (m, 4), lcls (m); matrix (nc+1, nc+1) int64 is added to.
    Called only for an image that has a label and an NMS detection."""
    keep = dconf > F(conf)
    dn, dc = dn[keep], _cls(dcls[keep], nc)
    lc = _cls(lcls, nc)
    m, n = ln.shape[0], dn.shape[0]
    iou = vr.iou_matrix(ln, dn) if n else np.zeros((m, 0), dtype=F)
    q = iou > F(iou_thres)                                    # NaN compares false
    val = np.where(q, iou, F(-1))
    lstar = np.where(q.any(0), val.argmax(0), -1) if n else np.zeros(0, dtype=np.int64)   # first maximum: lower label index
    best = val.max(0) if n else np.zeros(0, dtype=F)
    winner = np.zeros(n, dtype=bool)
    matched = np.zeros(m, dtype=bool)
    for l in range(m):
        ds = np.nonzero(lstar == l)[0]
        if ds.size:
            d = ds[np.argmax(best[ds])]                        # first maximum: lower detection index
            winner[d] = matched[l] = True
            if lc[l] >= 0 and dc[d] >= 0:
                matrix[dc[d], lc[l]] += 1
        elif lc[l] >= 0:
            matrix[nc, lc[l]] += 1
    if matched.any():
        for d in np.nonzero(~winner)[0]:
            if dc[d] >= 0:
                matrix[dc[d], nc] += 1


def confusion_image(matrix, det, labels, row, net_hw, nc, conf=0.25, iou_thres=0.45, single_cls=False):
    """det (n, >=6) fp32 letterbox pixels, labels (m, 5) fp32 [cls, xywh normalised], row [gain, pad_x, pad_y, h0, w0]"""
    if det.shape[0] == 0 or labels.shape[0] == 0:
        return
    dcls = np.zeros(det.shape[0], dtype=F) if single_cls else det[:, 5]
    confusion_native(matrix, vr.to_native(det[:, :4], row), det[:, 4].astype(F), dcls, native_labels(labels, row, net_hw),
                     labels[:, 0], nc, conf, iou_thres)


def confusion_batches(batches, net_hw, nc, conf=0.25, iou_thres=0.45, single_cls=False, to_host=np.asarray):
    """batches of (dets, counts, targets, rows) -> (nc+1, nc+1) int64; the per-image loop with its fetches (to_host), which is
    what the reference does"""
    matrix = np.zeros((nc + 1, nc + 1), dtype=np.int64)
    for dets, counts, targets, rows in batches:
        for si in range(dets.shape[0]):
            n = int(to_host(counts[si]))
            tg = to_host(targets).reshape(-1, 6)
            confusion_image(matrix, to_host(dets[si, :n]), tg[tg[:, 0] == si, 1:], to_host(rows[si]), net_hw, nc, conf, iou_thres,
                            single_cls)
    return matrix


def predn_batch(dets, counts, rows, single_cls=False):
    """-> predn (B, max_det, 6), xywh_tl (B, max_det, 4) fp32, padding rows zero"""
    B, max_det = dets.shape[0], dets.shape[1]
    predn = np.zeros((B, max_det, 6), dtype=F)
    tl = np.zeros((B, max_det, 4), dtype=F)
    for si in range(B):
        n = int(counts[si])
        b = vr.to_native(dets[si, :n, :4], rows[si])
        predn[si, :n, :4], predn[si, :n, 4] = b, dets[si, :n, 4]
        predn[si, :n, 5] = 0 if single_cls else dets[si, :n, 5]
        w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        tl[si, :n] = np.stack(((b[:, 0] + b[:, 2]) / F(2) - w / F(2), (b[:, 1] + b[:, 3]) / F(2) - h / F(2), w, h), 1)
    return predn, tl


def json_rows(predn, tl, counts, image_ids, class_map=None):
    out = []
    for si, image_id in enumerate(image_ids):
        for p, b in zip(predn[si, :int(counts[si])].tolist(), tl[si, :int(counts[si])].tolist()):
            c = int(p[5])
            out.append({'image_id': image_id, 'category_id': c if class_map is None else class_map[c],
                        'bbox': [round(x, 3) for x in b], 'score': round(p[4], 5)})
    return out
