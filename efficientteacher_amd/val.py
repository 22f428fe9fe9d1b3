"""Validation on the device (reference val.py:149-465).

Inference half, ``infer_batch`` (val.py:277-338):

    img uint8 -> (half | float) / 255 -> model(img) in eval mode (BatchNorm folded into the conv epilogues)
              -> non_max_suppression(out, conf_thres=0.001, iou_thres=0.6, multi_label=True, agnostic=single_cls)

the uint8 batch is normalised inside the input pack kernel, the EMA / student detector runs its folded-BN inference convs
(bf16 when ``half``: the reference's fp16 switch maps to this package's bf16 compute mode), the decoded (B, A, 5+nc) tensor
goes through et_nms (multi-label candidates, exact max_nms cut, class-offset NMS) and comes back as the reference's
``list[Tensor(n, 6)]`` or, with ``padded=True``, as the device tensors ``(dets (B, max_det, 6), counts (B))`` et_nms wrote.

Metric half, ``DetectionMetrics`` (val.py:339-403 + utils/metrics.py:16-126): ``update`` is one et_val_match launch per batch
-- scale_coords, box_iou and process_batch for every image of the batch, results appended to a device arena at fixed row
positions, no device->host transfer and no synchronisation -- and ``compute`` is one stable sort, one et_val_ap launch and one
copy of a few KB to the host: P, R, AP per class and threshold, F1, the per-class F1-optimal confidence thresholds
(``cls_thr``, which SSOD validation hands back to the trainer) and ``fitness``.

``ConfusionMatrix`` (utils/metrics.py:129-204) is the same on the device: ``update`` is one et_val_confusion launch per batch into
an int32 (nc+1, nc+1) matrix, reading ``matrix`` is the one transfer.  ``native_predictions`` / ``coco_json_rows`` are the ``predn``
of val.py:355-356 and the rows ``save_one_json`` (val.py:67-76) appends, from one et_val_predn launch and one transfer per batch.

``run`` is the reference's ``val.run`` over these for a model and a loader that already exist (its ``training`` branch).  Its
``confusion_matrix=`` / ``jdict=`` keywords collect the two above; the plots, save_txt / save_json / pycocotools legs behind the
reference's own flags and the keypoint (num_points) variants are host code of the reference and stay there.
"""
import torch

import time
from pathlib import Path

import numpy as np

from . import ops
from .utils.general import nms_padded, non_max_suppression


@torch.no_grad()
def infer_batch(model, img, conf_thres=0.001, iou_thres=0.6, half=True, augment=False, single_cls=False, multi_label=True,
                max_det=300, labels=(), padded=False):
    """One batch of val.run: returns (detections list[Tensor(n,6)] [x1,y1,x2,y2,conf,cls], train_out) -- train_out are the raw
    head outputs the reference feeds to compute_loss (val.py:312-314).  padded=True: the detections stay the device tensors
    (dets (B, max_det, 6) zero padded, counts (B,) int32) of et_nms, nothing is unpacked and the host is not synchronised --
    the form ``DetectionMetrics.update`` takes."""
    if labels:
        raise NotImplementedError("save_hybrid autolabelling (labels=lb) stays on the reference's host path")
    was_training = model.training
    dtype = torch.bfloat16 if half else torch.float32
    inner = model.module if hasattr(model, "module") else model
    if inner._compute_dtype != dtype:
        inner.set_compute_dtype(dtype)
    model.eval()
    if img.dtype != torch.uint8:                      # already normalised by the caller (val.py:283-289 did img /= 255)
        img = img.float()
    outputs = model(img, augment=augment)
    # val.py:300-318 "ugly solution": SSOD detectors return ((z, train_out), feats), plain ones (z, train_out)
    out = outputs
    train_out = None
    while isinstance(out, (tuple, list)):
        if len(out) == 2 and torch.is_tensor(out[0]) and out[0].dim() == 3:
            out, train_out = out[0], out[1]
            break
        out = out[0]
    if padded:
        dets = nms_padded(out, conf_thres, iou_thres, agnostic=single_cls, multi_label=multi_label, max_det=max_det)[:2]
    else:
        dets = non_max_suppression(out, conf_thres, iou_thres, multi_label=multi_label, agnostic=single_cls, max_det=max_det)
    if was_training:
        model.train()
    return dets, train_out


def fitness(x):
    """utils/metrics.py:16-19: rows [P, R, mAP@.5, mAP@.5:.95, ...] -> 0.1 * mAP@.5 + 0.9 * mAP@.5:.95"""
    w = [0.0, 0.0, 0.1, 0.9]
    return (np.atleast_2d(np.asarray(x, dtype=np.float64))[:, :4] * w).sum(1)


class DetectionResults:
    """what ``ap_per_class`` returns (p, r, ap, f1, ap_class, cls_thr: utils/metrics.py:98) and what val.run derives from it
    (val.py:401-403, :459-461): ap50, mp, mr, map50, map, nt, maps."""

    def __init__(self, nc, niou):
        self.p = self.r = self.f1 = np.zeros(0)
        self.ap = np.zeros((0, niou))
        self.ap50 = np.zeros(0)
        self.ap_class = np.zeros(0, dtype=np.int32)
        self.cls_thr = []
        self.f1_index = 0
        self.mp = self.mr = self.map50 = self.map = 0.0
        self.nt = np.zeros(nc, dtype=np.int64)
        self.maps = np.zeros(nc)

    def fitness(self):
        return float(fitness(np.array([[self.mp, self.mr, self.map50, self.map]]))[0])


def shape_rows(shapes, net_hw):
    """the loader's ``shapes`` (val.py:344,356: shapes[si] = ((h0, w0), ((gain_h, gain_w), (pad_x, pad_y))), or ((h0, w0), None) for
    scale_coords to work the letterbox out itself, utils/general.py:704-706) -> (B, 5) fp32 rows [gain, pad_x, pad_y, h0, w0]"""
    rows = []
    for s in shapes:
        (h0, w0), rp = s[0], (s[1] if len(s) > 1 else None)
        if rp is None:
            gain = min(net_hw[0] / h0, net_hw[1] / w0)
            pad = (net_hw[1] - w0 * gain) / 2, (net_hw[0] - h0 * gain) / 2
        else:
            gain, pad = rp[0][0], rp[1]
        rows.append([gain, pad[0], pad[1], h0, w0])
    return torch.tensor(rows, dtype=torch.float32).reshape(-1, 5)


def _device_shapes(shapes, net_hw, device):
    """``shapes`` of one batch as the (B, 5) fp32 device rows the kernels take: a tensor as it is, the loader's list through
    ``shape_rows`` and one stream-ordered copy"""
    if not torch.is_tensor(shapes):
        shapes = shape_rows(shapes, net_hw)
        if device.type == "cuda":
            shapes = shapes.pin_memory()
    return shapes.to(device, torch.float32, non_blocking=True).contiguous()


class ConfusionMatrix:
    """The reference's ConfusionMatrix (utils/metrics.py:129-204), device resident: ``matrix[predicted, true]`` with row / column nc
    as background, accumulated by et_val_confusion (the closed form: include/et_hip.h) in int32.

    Where the reference leaves the outcome to an unstable argsort: of two qualifying labels of exactly equal IoU a detection takes
    the lower label index; of two detections of exactly equal IoU a label takes the lower detection index."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45, device=None):
        self.nc, self.conf, self.iou_thres = int(nc), float(conf), float(iou_thres)
        self.device = torch.device(device if device is not None else "cuda")
        self.reset()

    def reset(self):
        self._m = torch.zeros((self.nc + 1, self.nc + 1), dtype=torch.int32, device=self.device)

    def update(self, dets, counts, targets, shapes, net_hw, single_cls=False):
        """one batch, the arguments of ``DetectionMetrics.update``: one launch, no transfer, no synchronisation"""
        assert 1 <= dets.shape[1] <= 1024, dets.shape
        shapes = _device_shapes(shapes, net_hw, self.device)
        ops.val_confusion(dets, counts, targets, shapes, net_hw, self.nc, self._m, self.conf, self.iou_thres, single_cls)

    def process_batch(self, detections, labels):
        """the reference's signature: one image, detections (N, 6) [x1,y1,x2,y2,conf,cls] and labels (M, 5) [cls,x1,y1,x2,y2] in
        native space, coordinates >= 0 as scale_coords leaves them.  The same kernel over corner-form label rows and an identity shape
        row (gain 1, pad 0, no upper clip), so the counts equal ``update``'s on the same image."""
        dev = self.device
        det = torch.as_tensor(detections, dtype=torch.float32).to(dev).reshape(-1, 6)
        lab = torch.as_tensor(labels, dtype=torch.float32).to(dev).reshape(-1, 5)
        if det.shape[0] == 0:                                        # no row passes the conf filter; the labels still count (:165-170)
            det = torch.tensor([[0.0, 0.0, 0.0, 0.0, float("-inf"), 0.0]], device=dev)
        n = det.shape[0]
        if n > 1024:
            raise ValueError(f"process_batch takes at most 1024 detections of one image, got {n}")
        targets = torch.cat((torch.zeros_like(lab[:, :1]), lab), 1)
        row = torch.tensor([[1.0, 0.0, 0.0, float("inf"), float("inf")]], device=dev)
        counts = torch.full((1,), n, dtype=torch.int32, device=dev)
        ops.val_confusion(det.reshape(1, n, 6).contiguous(), counts, targets, row, (0, 0), self.nc, self._m, self.conf,
                          self.iou_thres, False)

    def matrix_device(self):
        """the (nc+1, nc+1) int32 device tensor the kernel accumulates into"""
        return self._m

    @property
    def matrix(self):
        """(nc+1, nc+1) float64 numpy array, as the reference holds it: the one transfer"""
        return self._m.cpu().numpy().astype(np.float64)

    def print(self):
        for row in self.matrix:
            print(' '.join(map(str, row)))

    def plot(self, normalize=True, save_dir='', names=()):
        """confusion_matrix.png in save_dir: columns normalised to sum 1 (normalize), cells below 0.005 left blank, class names on the
        ticks when there are nc of them (fewer than 99).  Host code; a missing seaborn / matplotlib is a warning, not an error."""
        try:
            import warnings
            import matplotlib.pyplot as plt
            import seaborn as sn
            m = self.matrix
            if normalize:
                m = m / (m.sum(0, keepdims=True) + 1E-6)
            m[m < 0.005] = np.nan
            names = list(names)
            named = 0 < len(names) < 99 and len(names) == self.nc
            fig = plt.figure(figsize=(12, 9), tight_layout=True)
            sn.set(font_scale=0.8 if self.nc >= 50 else 1.0)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')                      # an all-NaN matrix
                ax = sn.heatmap(m, annot=self.nc < 30, annot_kws={"size": 8}, cmap='Blues', fmt='.2f', square=True,
                                xticklabels=names + ['background FP'] if named else "auto",
                                yticklabels=names + ['background FN'] if named else "auto")
            ax.set_facecolor((1, 1, 1))
            ax.set_xlabel('True')
            ax.set_ylabel('Predicted')
            fig.savefig(Path(save_dir) / 'confusion_matrix.png', dpi=250)
            plt.close(fig)
        except Exception as e:
            print(f'WARNING: ConfusionMatrix plot failure: {e}')


def native_predictions(dets, counts, shapes, net_hw, single_cls=False):
    """``predn`` of val.py:355-356 for a padded batch (``infer_batch(padded=True)``): -> predn (B, max_det, 6) [x1,y1,x2,y2 in the
    native image, conf, cls] and xywh_tl (B, max_det, 4), the top-left xywh box save_one_json writes -- device tensors, padding rows
    zero, one launch, no transfer.  shapes as ``DetectionMetrics.update`` takes them."""
    return ops.val_predn(dets, counts, _device_shapes(shapes, net_hw, dets.device), net_hw, single_cls=single_cls)


def image_id_of_path(path):
    """save_one_json's image id (val.py:69): the file stem, as an int when it is numeric"""
    stem = Path(path).stem
    return int(stem) if stem.isnumeric() else stem


def coco_json_rows(predn, xywh_tl, counts, image_ids, class_map=None):
    """the dicts save_one_json (val.py:67-76) appends for a batch, from ``native_predictions``' tensors: one transfer (a single
    list conversion), then the reference's round(x, 3) / round(score, 5) on the host.  class_map: category id by class index (the
    reference's coco80_to_91_class() list); None = the class index itself."""
    B, max_det = predn.shape[0], predn.shape[1]
    assert len(image_ids) == B and xywh_tl.shape[:2] == (B, max_det)
    if B == 0:
        return []
    n = counts.to(torch.float32).reshape(B, 1, 1).expand(B, max_det, 1)
    host = torch.cat((predn, xywh_tl, n), 2).tolist()
    rows = []
    for image_id, img in zip(image_ids, host):
        for r in img[:min(max(int(img[0][10]), 0), max_det)]:
            c = int(r[5])
            rows.append({'image_id': image_id, 'category_id': c if class_map is None else class_map[c],
                         'bbox': [round(x, 3) for x in r[6:10]], 'score': round(r[4], 5)})
    return rows


class DetectionMetrics:
    """Device-resident P / R / mAP accumulator (see the module docstring).  ``confusion``: a ``ConfusionMatrix`` that ``update`` feeds
    with the same batch (one more launch); None: nothing else runs.

    Order rules the reference leaves to unstable sorts: a detection with two class-matching labels of exactly equal IoU takes the
    lower label index; detections of equal confidence are ranked in arena order (image, then NMS rank)."""

    def __init__(self, nc, iouv=None, max_det=300, device=None, confusion=None):
        self.nc, self.max_det = int(nc), int(max_det)
        self.confusion = confusion
        self.device = torch.device(device if device is not None else "cuda")
        iouv = torch.linspace(0.5, 0.95, 10) if iouv is None else torch.as_tensor(iouv)          # val.py:244
        self.iouv = iouv.detach().to("cpu", torch.float32).contiguous().to(self.device)
        self.niou = self.iouv.numel()
        assert 1 <= self.niou <= 16 and 1 <= self.max_det <= 1024
        self.reset()

    def reset(self):
        self._rows = 0
        self._arena = None
        self.nt = torch.zeros(self.nc, dtype=torch.int32, device=self.device)
        self.seen = 0

    def _reserve(self, rows):
        cap = 0 if self._arena is None else self._arena[0].numel()
        if rows <= cap and self._arena is not None:
            return
        cap = max(rows, 2 * cap, 64 * self.max_det)
        new = [torch.empty(cap, dtype=dt, device=self.device) for dt in (torch.int32, torch.float32, torch.int32, torch.int32)]
        if self._arena is not None:
            for a, b in zip(new, self._arena):
                a[:self._rows].copy_(b[:self._rows])                 # device to device, stream ordered
        self._arena = new

    def update(self, dets, counts, targets, shapes, net_hw, single_cls=False):
        """one batch: dets (B, max_det, >=6) + counts (B) from ``infer_batch(padded=True)``, targets (NT, 6) [img, cls, xywh
        normalised] on the device, shapes: (B, 5) fp32 device rows [gain, pad_x, pad_y, h0, w0] or the loader's list
        (``shape_rows``), net_hw: (height, width) of the network input."""
        B = dets.shape[0]
        assert dets.shape[1] == self.max_det, (dets.shape, self.max_det)
        if not torch.is_tensor(shapes):
            shapes = shape_rows(shapes, net_hw)
            if self.device.type == "cuda":
                shapes = shapes.pin_memory()
        shapes = shapes.to(self.device, torch.float32, non_blocking=True).contiguous()
        self._reserve(self._rows + B * self.max_det)
        correct, conf, cls, valid = self._arena
        ops.val_match(dets, counts, targets, shapes, net_hw, self.iouv, self.nc, correct, conf, cls, valid, self.nt,
                      row_offset=self._rows, single_cls=single_cls)
        self._rows += B * self.max_det
        self.seen += B
        if self.confusion is not None:
            self.confusion.update(dets, counts, targets, shapes, net_hw, single_cls=single_cls)

    def rows(self):
        """the arena so far: correct (bit i = true positive at iouv[i]), conf, cls, valid -- device tensors, one row per
        (image, NMS slot)"""
        if self._arena is None:
            z = torch.zeros(0, dtype=torch.int32, device=self.device)
            return z, z.float(), z, z
        return tuple(a[:self._rows] for a in self._arena)

    def sorted_rows(self):
        """the rows ordered by (class, conf descending, arena row): one stable sort of a packed 64-bit key"""
        correct, conf, cls, valid = self.rows()
        kc = torch.where((valid > 0) & (cls >= 0) & (cls < self.nc), cls, torch.full_like(cls, self.nc)).to(torch.int64)
        key = (kc << 32) | ((~conf.view(torch.int32)).to(torch.int64) & 0xFFFFFFFF)   # conf >= 0: fp32 bits are monotone
        order = torch.sort(key, stable=True).indices
        return kc[order].to(torch.int32), correct[order].contiguous(), conf[order].contiguous()

    def curves(self):
        """ap (nc, niou), p, r, f1 (nc, 1000) fp64 on the device, indexed by class (utils/metrics.py:46-74)"""
        cls_s, correct_s, conf_s = self.sorted_rows()
        return ops.val_ap(cls_s, correct_s, conf_s, self.nt, self.niou)

    def compute(self):
        nc, niou = self.nc, self.niou
        ap, p, r, f1 = self.curves()
        correct = self.rows()[0]
        # utils/metrics.py:83 f1.mean(0).argmax(): the rows of classes without labels are zero, so the sum over all classes has
        # the same arg-max as the mean over the classes that have labels
        i = f1.sum(0).argmax()
        pack = torch.cat((ap.reshape(-1), p[:, i], r[:, i], f1[:, i], f1.argmax(1).double(), self.nt.double(),
                          i.double().reshape(1), (correct != 0).any().double().reshape(1)))
        h = pack.cpu().numpy()                                        # the one transfer
        res = DetectionResults(nc, niou)
        o = nc * niou
        res.nt = h[o + 4 * nc:o + 5 * nc].astype(np.int64)
        res.maps = np.zeros(nc)
        if h[-1] == 0.0:                                              # val.py:399: nothing correct at any threshold -> zeros
            return res
        cl = np.nonzero(res.nt > 0)[0]                                # np.unique(target_cls), :41
        px = np.linspace(0, 1, 1000)
        res.ap_class = cl.astype(np.int32)
        res.ap = h[:o].reshape(nc, niou)[cl]
        res.p, res.r, res.f1 = h[o:o + nc][cl], h[o + nc:o + 2 * nc][cl], h[o + 2 * nc:o + 3 * nc][cl]
        res.cls_thr = [px[int(k)] for k in h[o + 3 * nc:o + 4 * nc][cl]]
        res.f1_index = int(h[-2])
        res.ap50, apm = res.ap[:, 0], res.ap.mean(1)                  # val.py:401-402
        res.mp, res.mr, res.map50, res.map = res.p.mean(), res.r.mean(), res.ap50.mean(), apm.mean()
        res.maps = np.zeros(nc) + res.map                             # val.py:459-461
        res.maps[cl] = apm
        return res

    def fitness(self):
        return self.compute().fitness()


@torch.no_grad()
def run(model, dataloader, *, conf_thres=0.001, iou_thres=0.6, half=True, single_cls=False, augment=False, compute_loss=None,
        val_ssod=False, nc=80, names=None, eval_num=-1, verbose=False, max_det=300, save_txt=False, save_json=False,
        save_hybrid=False, plots=False, num_points=0, confusion_matrix=None, jdict=None, image_id_of=None, class_map=None):
    """The reference's val.run (val.py:149-465) for a model and a loader that exist (its ``training`` branch):
    returns ((mp, mr, map50, map, *loss), maps, t) and, with val_ssod, cls_thr as a fourth element; prints its table.
    The three loss entries are zeros as in the reference, whose compute_loss call is unreachable (val.py:307 is always true);
    ``compute_loss`` is accepted for call compatibility.  t = (pre-process, inference + NMS + matching, 0) ms per image: the stages
    are not separated by device synchronisations here.
    confusion_matrix: a ``ConfusionMatrix`` to accumulate over the loop (val.py:372-373).  jdict: a list that receives the rows
    save_one_json would append (val.py:381-382), ``image_id_of(path)`` (default: the reference's stem rule) and ``class_map`` as in
    ``coco_json_rows``.  Both default to off and change nothing else; plots / save_json / save_txt themselves keep raising."""
    for flag, what in ((save_txt, "save_txt (val.py:379)"), (save_json, "save_json / pycocotools (val.py:381, :428-452)"),
                       (save_hybrid, "save_hybrid autolabelling (val.py:330)"), (plots, "plots / ConfusionMatrix (val.py:372, :386, :423)"),
                       (num_points, "num_points keypoint validation (val.py:332, :357-364)")):
        if flag:
            raise NotImplementedError(f"{what} stays on the reference's host path")
    device = next(model.parameters()).device
    nc = 1 if single_cls else int(nc)                                # val.py:243
    if names is None:
        inner = model.module if hasattr(model, "module") else model
        names = getattr(inner, "names", None) or {}
    if isinstance(names, (list, tuple)):
        names = dict(enumerate(names))
    if confusion_matrix is not None:
        assert confusion_matrix.nc == nc, (confusion_matrix.nc, nc)
    metrics = DetectionMetrics(nc, max_det=max_det, device=device, confusion=confusion_matrix)
    if jdict is not None and image_id_of is None:
        image_id_of = image_id_of_path
    s = ('%20s' + '%11s' * 6) % ('Class', 'Images', 'Labels', 'P', 'R', 'mAP@.5', 'mAP@.5:.95')
    dt = [0.0, 0.0, 0.0]
    nbatches = 0
    for batch_i, (img, targets, paths, shapes) in enumerate(dataloader):
        if batch_i == eval_num:                                      # val.py:277
            break
        t1 = time.perf_counter()
        img = img.to(device, non_blocking=True)
        targets = targets.to(device, non_blocking=True)
        t2 = time.perf_counter()
        (dets, counts), _ = infer_batch(model, img, conf_thres, iou_thres, half=half, augment=augment, single_cls=single_cls,
                                        max_det=max_det, padded=True)
        if jdict is not None:
            shapes = _device_shapes(shapes, img.shape[2:], device)
            predn, xywh_tl = native_predictions(dets, counts, shapes, img.shape[2:], single_cls=single_cls)
        metrics.update(dets, counts, targets, shapes, img.shape[2:], single_cls=single_cls)
        if jdict is not None:                                        # after the launches: the transfer waits for all of them at once
            jdict.extend(coco_json_rows(predn, xywh_tl, counts, [image_id_of(p) for p in paths], class_map))
        dt[0] += t2 - t1
        dt[1] += time.perf_counter() - t2
        nbatches += 1
    t2 = time.perf_counter()
    res = metrics.compute()
    dt[1] += time.perf_counter() - t2
    seen = metrics.seen
    pf = '%20s' + '%11i' * 2 + '%11.3g' * 4
    print(s)
    print(pf % ('all', seen, res.nt.sum(), res.mp, res.mr, res.map50, res.map))
    if verbose and nc > 1:                                           # val.py:412
        for i, c in enumerate(res.ap_class):
            print(pf % (names.get(int(c), str(int(c))), seen, res.nt[c], res.p[i], res.r[i], res.ap50[i], res.ap[i].mean()))
    t = tuple(x / max(seen, 1) * 1E3 for x in dt)
    out = (res.mp, res.mr, res.map50, res.map, 0.0, 0.0, 0.0), res.maps, t
    return out + (res.cls_thr,) if val_ssod else out
