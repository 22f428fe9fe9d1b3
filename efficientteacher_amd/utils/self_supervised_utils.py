"""Host-side mirror of the reference's ``utils/self_supervised_utils.py`` for the hot path:
``FairPseudoLabel`` (:54) turns the EMA teacher's decoded predictions into pseudo labels.

``create_pseudo_label_online_with_gt`` keeps the reference signature / return value (a compacted
(N,9) float64 tensor and ``invalid_target_shape``), which costs one host synchronisation;
``create_pseudo_label_padded`` is the device-resident form the trainer uses (no synchronisation).
``pseudo_label_hit_rate`` gives the progress-bar statistics of the step (:481-609) from that padded form, on the device;
``check_pseudo_label_with_gt`` keeps the reference's signature over the same kernel.
"""
import torch

from .. import ops
from .general import nms_ssod_padded

HIT_RATE_KEYS = ("tp", "fp_cls", "fp_loc", "pse_num", "gt_num")


def pseudo_label_hit_rate(t9, valid, gt, thr_low, thr_high, batch_size, with_gt):
    """the progress-bar statistics of the reference's ssod_trainer.py:655-672 as a dict of five 0-dim fp64 DEVICE tensors
    (tp, fp_cls, fp_loc, pse_num, gt_num), from the padded pseudo-label table (t9 (N,9) fp64, valid (N) uint8) of
    ``create_pseudo_label_padded``.  with_gt: how many of the uncertain pseudo labels hit a ground-truth row of gt (M,6)
    [img, cls, x, y, w, h] (check_pseudo_label_with_gt, :481-585); otherwise the reliable / uncertain counts of check_pseudo_label
    (:587-609), gt is not looked at.  thr_low / thr_high: (nc) fp64 device tensors (the loss's ``refresh_thresholds``).
    One call of ``ops.pseudo_label_quality``: stream-ordered, no synchronisation; whoever formats the numbers reads them back."""
    out = ops.pseudo_label_quality(t9, valid, gt, thr_low, thr_high, batch_size, with_gt=bool(with_gt))
    return dict(zip(HIT_RATE_KEYS, out.unbind(0)))


def check_pseudo_label_with_gt(detections, labels, iouv=torch.tensor([0.5]), ignore_thres_low=None, ignore_thres_high=None,
                               batch_size=1):
    """the reference's signature (utils/self_supervised_utils.py:481) over the device statistic: detections (n,9) COMPACTED
    pseudo labels [img, cls, x, y, w, h, conf, obj_conf, cls_conf], labels (M,6) [img, cls, x, y, w, h]
    -> (tp_rate, fp_cls_rate, fp_loc_rate, pseudo_label_num, gt_label_num), the rates arrays of one element per IoU threshold (the
    integer 0 when no pseudo label takes part), as the reference returns them.  Only iouv = [0.5] exists, the one value any caller
    passes.  Without thresholds every row takes part (:509-513).  Reading the result back is this API's host synchronisation;
    ``labels`` is NOT scaled in place (the reference multiplies the caller's tensor by 640, :515)."""
    thr = [float(v) for v in torch.as_tensor(iouv).reshape(-1).tolist()]
    if thr != [0.5]:
        raise NotImplementedError(f"check_pseudo_label_with_gt: iouv {thr}; only [0.5] is built (csrc/pseudo_quality.hip)")
    if (ignore_thres_low is None) != (ignore_thres_high is None):
        raise ValueError("ignore_thres_low and ignore_thres_high go together")
    n, M = detections.shape[0], labels.shape[0]
    if n == 0:                                                      # :567-570
        return 0, 0, 0, 0 / batch_size, M / batch_size
    dev = detections.device
    if ignore_thres_low is None:                                    # every row lies inside (-inf, +inf): all take part
        lo, hi = [float("-inf")], [float("inf")]
    else:
        lo, hi = [float(v) for v in ignore_thres_low], [float(v) for v in ignore_thres_high]
    t9 = detections.to(torch.float64).contiguous()
    out = ops.pseudo_label_quality(t9, torch.ones(n, dtype=torch.uint8, device=dev), labels,
                                   torch.tensor(lo, dtype=torch.float64).to(dev), torch.tensor(hi, dtype=torch.float64).to(dev),
                                   batch_size, with_gt=True)
    tp, fp_cls, fp_loc, pse, gt = out.tolist()
    if pse == 0:
        return 0, 0, 0, pse, gt
    import numpy as np
    return np.array([tp]), np.array([fp_cls]), np.array([fp_loc]), pse, gt


class FairPseudoLabel:
    def __init__(self, cfg):
        self.nms_conf_thres = cfg.SSOD.nms_conf_thres
        self.nms_iou_thres = cfg.SSOD.nms_iou_thres
        self.debug = cfg.SSOD.debug
        self.multi_label = cfg.SSOD.multi_label
        self.names = cfg.Dataset.names
        self.num_points = cfg.Dataset.np
        if self.multi_label or self.num_points:
            raise NotImplementedError("multi_label / keypoint pseudo labels are outside the hot path")

    def create_pseudo_label_padded(self, out, M_s, width, height, max_det=300):
        """out (B, A, 5+nc) teacher predictions -> (targets9 (B*max_det, 9) fp64, valid (B*max_det) uint8)."""
        dets, counts, _, _ = nms_ssod_padded(out, self.nms_conf_thres, self.nms_iou_thres, max_det=max_det)
        return ops.pseudo_label_transform(dets, counts, M_s, width, height)

    def create_pseudo_label_online_with_gt(self, out, target_imgs, M_s, target_imgs_ori, gt=None, RANK=-2):
        n_img, _, height, width = target_imgs.shape
        t9, valid = self.create_pseudo_label_padded(out, M_s, width, height)
        targets = t9[valid.bool()]                  # compaction: the one host sync of this API
        invalid_target_shape = targets.shape[0] == 0
        return targets, invalid_target_shape
