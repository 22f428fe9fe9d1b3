"""Strong-view generation for the unlabeled stream on the device (reference utils/datasets_ssod.py:520-570).

The reference's data-loader workers produce BOTH views with cv2 on the host.  ``StrongViewGenerator`` keeps their random
recipe on the host -- a few numbers per image -- and does the per-pixel work in one kernel (csrc/augment.hip):

    M = T @ S @ R @ C            random_perspective_with_M   (datasets_ssod.py:902-945; perspective = 0 in every recipe)
    hue / sat / val gains        augment_hsv                 (augmentations.py:48-61)
    cutout rectangles + colours  cutout                      (augmentations.py:382-398; label filtering stays with the labels)
    flipud / fliplr                                          (datasets_ssod.py:552-563)

and returns the strong batch together with the ``M_s`` rows ``[i, M(9), s, ud, lr]`` the pseudo-label transform consumes
(utils/self_supervised_utils.py).  PARITY UNPINNED for the pixels (cv2 is not installed here; see csrc/augment.hip): the
matrices, LUTs and rectangles follow the reference's formulas exactly, given the same random numbers.
"""
import math
import random

import numpy as np
import torch

from .. import ops

MAX_CUT = 32


def affine_matrix(h, w, degrees, translate, scale, shear, rng=random, out_hw=None):
    """(M (3,3), s): datasets_ssod.py:909-938 with perspective = 0.  (h, w) is the size of the image that is warped: C centres it.
    out_hw = (height, width) of the OUTPUT when a border changes it (random_perspective_keypoints, augmentations.py:130-159: the
    mosaic's 2s x 2s canvas comes out s x s) -- T translates by the output size; None = no border, the same size"""
    oh, ow = (h, w) if out_hw is None else out_hw
    C = np.eye(3)
    C[0, 2] = -w / 2
    C[1, 2] = -h / 2
    rng.uniform(0, 0); rng.uniform(0, 0)                       # the two perspective draws of the reference's stream
    a = rng.uniform(-degrees, degrees)
    s = rng.uniform(1 - scale, 1 + scale)
    R = np.eye(3)
    ar = math.radians(a)                                       # cv2.getRotationMatrix2D(angle=a, center=(0,0), scale=s)
    al, be = s * math.cos(ar), s * math.sin(ar)
    R[:2] = [[al, be, 0.0], [-be, al, 0.0]]
    S = np.eye(3)
    S[0, 1] = math.tan(rng.uniform(-shear, shear) * math.pi / 180)
    S[1, 0] = math.tan(rng.uniform(-shear, shear) * math.pi / 180)
    T = np.eye(3)
    T[0, 2] = rng.uniform(0.5 - translate, 0.5 + translate) * ow
    T[1, 2] = rng.uniform(0.5 - translate, 0.5 + translate) * oh
    return T @ S @ R @ C, s


def invert_affine(M):
    """cv2.warpAffine's inversion of the 2x3 forward map (imgwarp.cpp: invertAffineTransform semantics), fp64"""
    m0, m1, m2, m3, m4, m5 = (float(M[0, 0]), float(M[0, 1]), float(M[0, 2]), float(M[1, 0]), float(M[1, 1]), float(M[1, 2]))
    D = m0 * m4 - m1 * m3
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m4 * D, m0 * D
    i0, i1, i3, i4 = A11, m1 * -D, m3 * -D, A22
    return [i0, i1, -i0 * m2 - i1 * m5, i3, i4, -i3 * m2 - i4 * m5]


def hsv_luts(hgain, sgain, vgain, rng=np.random):
    """augmentations.py:51-58"""
    r = rng.uniform(-1, 1, 3) * [hgain, sgain, vgain] + 1
    x = np.arange(0, 256, dtype=r.dtype)
    return np.stack((((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8),
                     np.clip(x * r[2], 0, 255).astype(np.uint8)))


def cutout_rects(h, w, rng=random):
    """augmentations.py:386-398 -> rows (x0, y0, x1, y1, r, g, b); the reference assigns [c0, c1, c2] to a BGR image"""
    rows = []
    for s in [0.5] * 1 + [0.25] * 2 + [0.125] * 4 + [0.0625] * 8 + [0.03125] * 16:
        mask_h = rng.randint(1, int(h * s))
        mask_w = rng.randint(1, int(w * s))
        xmin = max(0, rng.randint(0, w) - mask_w // 2)
        ymin = max(0, rng.randint(0, h) - mask_h // 2)
        xmax, ymax = min(w, xmin + mask_w), min(h, ymin + mask_h)
        c = [rng.randint(64, 191) for _ in range(3)]
        rows.append([xmin, ymin, xmax, ymax, c[2], c[1], c[0]])
    return rows[:MAX_CUT]


class StrongViewGenerator:
    def __init__(self, hyp, seed=None):
        """hyp: the reference's cfg.hyp node (degrees, translate, scale, shear, hsv_h, hsv_s, hsv_v, cutout, flipud, fliplr)"""
        self.hyp = hyp
        self.py_rng = random.Random(seed)
        self.np_rng = np.random.RandomState(seed)

    def sample(self, B, H, W):
        """host side: (minv (B,6) f64, lut (B,3,256) u8, cutouts (B,32,7) i32, flags (B,3) i32, M_s (B,13) f64)"""
        hyp = self.hyp
        minv = np.zeros((B, 6)); lut = np.zeros((B, 3, 256), np.uint8)
        cuts = np.zeros((B, MAX_CUT, 7), np.int32); flags = np.zeros((B, 3), np.int32); M_s = np.zeros((B, 13))
        for i in range(B):
            M, s = affine_matrix(H, W, hyp.degrees, hyp.translate, hyp.scale, hyp.shear, self.py_rng)
            minv[i] = invert_affine(M)
            lut[i] = hsv_luts(hyp.hsv_h, hyp.hsv_s, hyp.hsv_v, self.np_rng)
            if self.py_rng.random() < float(getattr(hyp, "cutout", 0.0)) and self.py_rng.random() < 0.5:     # :540, :384
                rows = cutout_rects(H, W, self.py_rng)
                cuts[i, :len(rows)] = rows
                flags[i, 0] = len(rows)
            flags[i, 1] = int(self.py_rng.random() < hyp.flipud)
            flags[i, 2] = int(self.py_rng.random() < hyp.fliplr)
            M_s[i] = [i, *M.reshape(-1), s, flags[i, 1], flags[i, 2]]
        return minv, lut, cuts, flags, M_s

    def __call__(self, weak_u8):
        """weak (B,3,H,W) uint8 on the device -> (strong (B,3,H,W) uint8, M_s (B,13) fp64 on the device)"""
        B, _, H, W = weak_u8.shape
        minv, lut, cuts, flags, M_s = self.sample(B, H, W)
        dev = weak_u8.device
        t = lambda a: torch.from_numpy(a).to(dev, non_blocking=True)
        strong = ops.strong_view_u8(weak_u8.contiguous(), t(minv), t(lut), t(cuts), t(flags))
        return strong, t(M_s)


# ---- 4-image mosaic (load_mosaic_with_M, utils/datasets_ssod.py:732-792) ---------------------------------------------------
def mosaic_layout(s, yc, xc, shapes):
    """Placement of the four tiles around the centre (xc, yc) of the 2s x 2s canvas (datasets_ssod.py:746-762).
    shapes: [(h, w)] * 4 in tile order (top left, top right, bottom left, bottom right).
    -> rows (x1a, y1a, x2a, y2a, x1b, y1b, padw, padh): canvas rectangle, its origin inside the image, label offsets"""
    rows = []
    for i, (h, w) in enumerate(shapes):
        if i == 0:
            x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
            x1b, y1b = w - (x2a - x1a), h - (y2a - y1a)
        elif i == 1:
            x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
            x1b, y1b = 0, h - (y2a - y1a)
        elif i == 2:
            x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
            x1b, y1b = w - (x2a - x1a), 0
        else:
            x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
            x1b, y1b = 0, 0
        rows.append((x1a, y1a, x2a, y2a, x1b, y1b, x1a - x1b, y1a - y1b))
    return rows


def mosaic_labels(s, layout, shapes, labels):
    """labels: four (n, 5) arrays [cls, x, y, w, h] normalised to their image -> (N, 5) [cls, x1, y1, x2, y2] in the frame of the
    s x s mosaic: xywhn2xyxy with w / 2, h / 2, padw / 2, padh / 2 (datasets_ssod.py:768: the canvas is halved by the resize that
    follows), then the reference's clip to [0, 2s] (:775-776 -- it clips to the CANVAS size although the coordinates are already
    halved: kept as it is)"""
    out = []
    for (x1a, y1a, x2a, y2a, x1b, y1b, padw, padh), (h, w), lb in zip(layout, shapes, labels):
        lb = np.asarray(lb, dtype=np.float64).reshape(-1, 5).copy()
        if lb.size:
            x = lb[:, 1:].copy()
            lb[:, 1] = (w / 2) * (x[:, 0] - x[:, 2] / 2) + padw / 2
            lb[:, 2] = (h / 2) * (x[:, 1] - x[:, 3] / 2) + padh / 2
            lb[:, 3] = (w / 2) * (x[:, 0] + x[:, 2] / 2) + padw / 2
            lb[:, 4] = (h / 2) * (x[:, 1] + x[:, 3] / 2) + padh / 2
        out.append(lb)
    out = np.concatenate(out, 0)
    np.clip(out[:, 1:], 0, 2 * s, out=out[:, 1:])
    return out


class MosaicGenerator:
    """The 4-image mosaic of the reference's SSOD loader (load_mosaic_with_M) with the per-pixel work on the device: the host draws
    the centre and the three partner images exactly as the reference does (same calls on the same `random` stream: two
    `random.uniform` for (yc, xc), `random.choices(indices, k=3)`, `random.shuffle`) and lays the tiles out; ONE kernel
    (et_mosaic4_u8, csrc/augment.hip) then writes the s x s mosaic -- the 2s x 2s canvas of border value 114 is never materialised:
    every output pixel averages its 2 x 2 canvas pixels, which is what cv2.resize(img4, (s, s)) computes at this exact 2:1 ratio
    (OpenCV switches INTER_LINEAR to its fast INTER_AREA path there: (a + b + c + d + 2) >> 2).  The result is the WEAK view
    (`img4_ori`); the strong view and M_s come from StrongViewGenerator on it, as random_perspective_with_M follows in the reference.
    PARITY: placement, label arithmetic and the consumption of the random stream are pinned on the live reference
    (tests/golden/mosaic.npz); the 2:1 resampling restates OpenCV's published algorithm and is unpinned (no cv2 here)."""

    def __init__(self, img_size, seed=None):
        self.s = int(img_size)
        self.border = [-self.s // 2, -self.s // 2]             # datasets_ssod.py:260
        self.rng = random.Random(seed)

    def sample(self, index, indices):
        """-> (yc, xc, the four image indices in tile order)"""
        s = self.s
        yc, xc = [int(self.rng.uniform(-x, 2 * s + x)) for x in self.border]
        four = [index] + self.rng.choices(indices, k=3)
        self.rng.shuffle(four)
        return yc, xc, four

    def __call__(self, images, labels, index, indices=None):
        """images: dict / list index -> uint8 device tensor (3, h, w) with max(h, w) <= img_size (what load_image returns, as RGB
        planes); labels: index -> (n, 5) normalised [cls, x, y, w, h].  -> (mosaic (3, s, s) uint8 on the device, labels (N, 5) xyxy)"""
        indices = list(range(len(images))) if indices is None else list(indices)
        yc, xc, four = self.sample(index, indices)
        tiles = [images[i] for i in four]
        shapes = [(int(t.shape[1]), int(t.shape[2])) for t in tiles]
        layout = mosaic_layout(self.s, yc, xc, shapes)
        out = ops.mosaic4_u8([tiles], [layout], self.s)[0]
        return out, mosaic_labels(self.s, layout, shapes, [labels[i] for i in four])


# ---- the labeled batch (LoadImagesAndLabels.__getitem__'s mosaic branch, utils/datasets.py:889-1043) -----------------------------------
class PendingLabeledBatch:
    """A labeled batch whose kernels have been launched.  `event` (None for the emulator's CPU tensors) is recorded behind them and behind the
    copy of the row count n to pinned memory; result() waits for it on the HOST -- the one host read of n -- narrows the targets to
    (n, 6) and makes the consumer's current stream wait for the event"""

    def __init__(self, imgs, out, n_dev, n_host, paths, event, stream):
        self.imgs, self.out, self.n_dev, self.n_host, self.paths, self.event, self.stream = imgs, out, n_dev, n_host, paths, event, stream

    def result(self):
        if self.n_host is None:                                # emulator / CPU tensors
            n = int(self.n_dev[0])
        else:
            self.event.synchronize()
            n = int(self.n_host[0])
            if self.stream is not None:
                cur = torch.cuda.current_stream(self.imgs.device)
                cur.wait_event(self.event)
                self.imgs.record_stream(cur)
                self.out.record_stream(cur)
        return self.imgs, self.out[:n], self.paths, (None,) * self.imgs.shape[0]


class LabeledBatchGenerator:
    """The labeled stream's batches on the device.  The host keeps the reference's random recipe -- sample() consumes `random` and
    `np.random` exactly as __getitem__'s mosaic branch does: the mosaic gate, load_mosaic (centre, three partners, shuffle,
    random_perspective_keypoints' eight draws with C from the 2s canvas and T from the s output), the mixup gate and, behind it,
    randint, a second mosaic and np.random.beta(32, 32), the HSV gains, the two flips -- and two kernels do the work
    (csrc/augment.hip): et_labeled_mosaic_u8 the pixels, et_labeled_mosaic_targets the labels.
    PARITY: recipe, random streams, canvas, matrices, ratio, LUTs and labels are pinned on the live reference
    (tests/golden/labeled_mosaic.npz); the warp sampling and the HSV round trip restate OpenCV's published algorithms (no cv2).
    cfg: the reference's config node (cfg.hyp, cfg.Dataset.img_size / np / num_ids); n: the number of images of the dataset.
    What the kernels do not cover raises NotImplementedError here, and the caller keeps the reference's loader for it."""

    def __init__(self, cfg, n, seed=None, stream=None, rect=False, image_weights=False):
        hyp, ds = cfg.hyp, cfg.Dataset
        g = lambda node, k, d=0: (node.get(k, d) if hasattr(node, "get") else getattr(node, k, d))
        if float(g(hyp, "perspective", 0.0)) != 0:
            raise NotImplementedError("LabeledBatchGenerator: hyp.perspective != 0 needs cv2.warpPerspective's projective sampling; "
                                      "the kernel implements the affine warp of every shipped recipe")
        if float(g(hyp, "copy_paste", 0.0)) > 0:
            raise NotImplementedError("LabeledBatchGenerator: hyp.copy_paste > 0 needs segment masks, which the device path does not hold")
        if int(g(ds, "np", 0)) > 0:
            raise NotImplementedError("LabeledBatchGenerator: Dataset.np > 0 (keypoint labels) is not transformed on the device")
        if int(g(ds, "num_ids", 0)) > 0:
            raise NotImplementedError("LabeledBatchGenerator: Dataset.num_ids > 0 (with_id: a tracking id per label) is not carried on the device")
        if rect:
            raise NotImplementedError("LabeledBatchGenerator: rect batches take the letterbox branch, which stays with the reference's loader")
        if image_weights:
            raise NotImplementedError("LabeledBatchGenerator: image_weights re-draws the index list per epoch on the host; not supported")
        if float(g(hyp, "mosaic", 1.0)) < 1:
            raise NotImplementedError("LabeledBatchGenerator: hyp.mosaic < 1 sends some images through the letterbox branch, which stays "
                                      "with the reference's loader")
        self.hyp, self.s, self.n = hyp, int(ds.img_size), int(n)
        self._g = g
        self.indices = range(self.n)
        self.border = [-self.s // 2, -self.s // 2]                # datasets.py:651
        self.mosaic = True                                       # the trainer sets dataset.mosaic = False for the last no_aug_epochs
        self.py_rng = random.Random(seed)
        self.np_rng = np.random.RandomState(seed)
        self.stream = stream

    def _mosaic(self, index):
        """load_mosaic's draws (datasets.py:1223-1225, augmentations.py:140-159) -> (yc, xc, four, M, s)"""
        s, hyp, g = self.s, self.hyp, self._g
        yc, xc = [int(self.py_rng.uniform(-x, 2 * s + x)) for x in self.border]
        four = [index] + self.py_rng.choices(self.indices, k=3)
        self.py_rng.shuffle(four)
        M, sc = affine_matrix(2 * s, 2 * s, g(hyp, "degrees"), g(hyp, "translate"), g(hyp, "scale"), g(hyp, "shear"), self.py_rng,
                              out_hw=(2 * s + 2 * self.border[0], 2 * s + 2 * self.border[1]))
        return yc, xc, four, M, sc

    def sample(self, index):
        """host side of one image: {'mosaics': [(yc, xc, four, M, s)] * (1 or 2), 'r': mixup ratio or None, 'lut': (3,256) u8 or None,
        'flipud', 'fliplr'}"""
        hyp, g = self.hyp, self._g
        if not self.mosaic:
            raise NotImplementedError("LabeledBatchGenerator: the mosaic is closed (no_aug_epochs): the letterbox branch stays with the "
                                      "reference's loader")
        index = self.indices[index]
        self.py_rng.random()                                     # the mosaic gate (hyp.mosaic = 1: always taken)
        mosaics = [self._mosaic(index)]
        r = None
        if self.py_rng.random() < g(hyp, "mixup", 0.0):
            mosaics.append(self._mosaic(self.py_rng.randint(0, self.n - 1)))
            r = float(self.np_rng.beta(32.0, 32.0))
        hs = (g(hyp, "hsv_h", 0.0), g(hyp, "hsv_s", 0.0), g(hyp, "hsv_v", 0.0))
        lut = hsv_luts(*hs, self.np_rng) if any(hs) else None
        ud = self.py_rng.random() < g(hyp, "flipud", 0.0)
        lr = self.py_rng.random() < g(hyp, "fliplr", 0.0)
        return dict(mosaics=mosaics, r=r, lut=lut, flipud=bool(ud), fliplr=bool(lr))

    def launch(self, images, labels, indices, paths=None):
        """sample every image of the batch and launch the two kernels (on self.stream when given) -> PendingLabeledBatch"""
        from .. import ops
        s, B = self.s, len(indices)
        samples = [self.sample(int(i)) for i in indices]
        use_lut = any(sm["lut"] is not None for sm in samples)
        f64 = np.zeros(B * 33)                                   # one staging array: minv (B,2,6) | M (B,2,9) | s (B,2) | mix (B,)
        minv, M, sc, mix = (f64[:B * 12].reshape(B, 2, 6), f64[B * 12:B * 30].reshape(B, 2, 9), f64[B * 30:B * 32].reshape(B, 2),
                            f64[B * 32:])
        minv[:] = [1, 0, 0, 0, 1, 0]; M[:] = np.eye(3).reshape(9); sc[:] = 1.0; mix[:] = 1.0
        flags = np.zeros((B, 3), np.int32)
        lut = np.tile(np.arange(256, dtype=np.uint8), (B, 3, 1)) if use_lut else None
        ltab = np.zeros((B, 2, 4, 6), np.int32)
        tiles, layouts, rows, row = [], [], [], 0
        for b, sm in enumerate(samples):
            tb, lb = [None, None], [None, None]
            for m in range(2):
                if m < len(sm["mosaics"]):
                    yc, xc, four, Mm, sm_s = sm["mosaics"][m]
                    tb[m] = [images[i] for i in four]
                    shapes = [(int(t.shape[1]), int(t.shape[2])) for t in tb[m]]
                    lb[m] = mosaic_layout(s, yc, xc, shapes)
                    minv[b, m], M[b, m], sc[b, m] = invert_affine(Mm), Mm.reshape(-1), sm_s
                    for k, (i, (h, w), lay) in enumerate(zip(four, shapes, lb[m])):
                        lab = np.asarray(labels[i], dtype=np.float32).reshape(-1, 5)
                        ltab[b, m, k] = (row, row + lab.shape[0], h, w, lay[6], lay[7])
                        rows.append(lab)
                        row += lab.shape[0]
                else:
                    ltab[b, m, :, :2] = row
            tiles.append(tb); layouts.append(lb)
            flags[b] = (len(sm["mosaics"]) == 2, sm["flipud"], sm["fliplr"])
            if sm["r"] is not None:
                mix[b] = sm["r"]
            if sm["lut"] is not None:
                lut[b] = sm["lut"]
        lab_all = np.concatenate(rows, 0) if rows else np.zeros((0, 5), np.float32)
        dev = tiles[0][0][0].device
        cuda = dev.type == "cuda"
        side = self.stream if cuda else None
        import contextlib
        if side is not None:
            side.wait_stream(torch.cuda.current_stream(dev))     # the source images were written on the caller's stream
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            t = lambda a: torch.from_numpy(a).to(dev, non_blocking=True)
            d64 = t(f64)
            dflags = t(flags)
            imgs = ops.labeled_mosaic_u8(tiles, layouts, d64[:B * 12].view(B, 2, 6), d64[B * 32:], t(lut) if use_lut else None, dflags, s)
            out, n_dev = ops.labeled_mosaic_targets(t(lab_all), ltab, d64[B * 12:B * 30].view(B, 2, 9), d64[B * 30:B * 32].view(B, 2),
                                                    dflags, s)
            n_host = event = None
            if cuda:
                n_host = torch.empty(1, dtype=torch.int32).pin_memory()
                n_host.copy_(n_dev, non_blocking=True)
                event = torch.cuda.Event()
                event.record(torch.cuda.current_stream(dev))
        return PendingLabeledBatch(imgs, out, n_dev, n_host, tuple(indices) if paths is None else tuple(paths[i] for i in indices),
                                   event, side)

    def __call__(self, images, labels, indices, paths=None):
        """images: index -> (3, h, w) uint8 device tensor with max(h, w) <= img_size (what load_image returns, as RGB planes); labels:
        index -> (n, 5) float32 [cls, x, y, w, h] normalised; indices: the dataset indices of this batch.  -> the reference's batch tuple
        (imgs (B,3,s,s) uint8, targets (n,6) float32 [img, cls, x, y, w, h], paths, shapes = (None,) * B), tensors on the device"""
        return self.launch(images, labels, indices, paths).result()

    def batches(self, images, labels, index_batches, paths=None):
        """the `labeled` iterable of Trainer / SSODTrainer.train_with_unlabeled: batch k + 1 is launched before batch k is handed out, so
        with stream= its kernels run beside the step that consumes batch k"""
        pending = None
        for idx in index_batches:
            nxt = self.launch(images, labels, list(idx), paths)
            if pending is not None:
                yield pending.result()
            pending = nxt
        if pending is not None:
            yield pending.result()


# ---- the letterbox branch (LoadImagesAndLabels.__getitem__, utils/datasets.py:904-953): val / rect batches and the closed mosaic ----------
def letterbox_geometry(h, w, new_shape, scaleup):
    """letterbox(im (h, w), new_shape, auto=False, scaleFill=False, scaleup) without the pixels (utils/augmentations.py:92-123) ->
    (ratio (rw, rh), (dw, dh), new_unpad (nw, nh), top, left); bottom = new_shape[0] - nh - top and right = new_shape[1] - nw - left
    (round(d - 0.1) + round(d + 0.1) == 2 d for every d = k / 2).  Written with the reference's own operations so that the TYPES flow as
    they do there: with an int new_shape everything is a Python number, with a row of rect_batch_shapes (numpy ints) r, dw and dh are
    numpy float64 -- except the Python 1.0 that min(r, 1.0) returns for r > 1 (LetterboxBatchGenerator reads the label dtype off that)"""
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    r = min(new_shape[0] / h, new_shape[1] / w)
    if not scaleup:
        r = min(r, 1.0)
    nw, nh = int(round(w * r)), int(round(h * r))
    dw, dh = new_shape[1] - nw, new_shape[0] - nh
    dw /= 2
    dh /= 2
    top, left = int(round(dh - 0.1)), int(round(dw - 0.1))
    return (r, r), (dw, dh), (nw, nh), top, left


def rect_batch_shapes(shapes_wh, batch_size, img_size, stride=32, pad=0.0):
    """Rectangular batches (utils/datasets.py:747-749, 772-795).  shapes_wh: (n, 2) the ORIGINAL (w, h) of every image.  ->
    (order (n,): the dataset is re-ordered by aspect ratio h / w, position i holds image order[i]; batch_index (n,): the batch of
    position i; batch_shapes (nb, 2) int: the (H, W) every image of the batch is letterboxed to)"""
    s = np.array(shapes_wh, dtype=np.float64).reshape(-1, 2)
    n = s.shape[0]
    bi = np.floor(np.arange(n) / batch_size).astype(int)
    nb = bi[-1] + 1
    ar = s[:, 1] / s[:, 0]
    irect = ar.argsort()
    ar = ar[irect]
    shapes = [[1, 1]] * nb
    for i in range(nb):
        ari = ar[bi == i]
        mini, maxi = ari.min(), ari.max()
        if maxi < 1:
            shapes[i] = [maxi, 1]
        elif mini > 1:
            shapes[i] = [1, 1 / mini]
    return irect, bi, np.ceil(np.array(shapes) * img_size / stride + pad).astype(int) * stride


class PendingLetterboxBatch(PendingLabeledBatch):
    """PendingLabeledBatch whose result() carries the letterbox branch's `shapes`"""

    def __init__(self, shapes, *a):
        super().__init__(*a)
        self.shapes = shapes

    def result(self):
        imgs, targets, paths, _ = super().result()
        return imgs, targets, paths, self.shapes


class LetterboxBatchGenerator:
    """The letterbox branch of the labeled loader on the device, in its two uses: augment=False -- every VALIDATION batch (the reference
    builds that loader with rect=True, pad=0.5; scaleup = False, no random draw at all) -- and augment=True -- the labeled batches of the
    CLOSED MOSAIC (the trainer sets dataset.mosaic = False for the last no_aug_epochs; scaleup = True).  The host keeps the recipe --
    letterbox_geometry, rect_batch_shapes and, for augment, sample()'s draws in the reference's order: the mosaic gate `random.random()`
    only when self.mosaic is set (`self.mosaic and ...` short-circuits; the default here is the closed mosaic, False),
    random_perspective_keypoints' eight draws with C and T from the letterboxed H x W, `np.random.uniform(-1, 1, 3)` when an HSV gain is
    non-zero, the two flip draws -- and two kernels do the work (csrc/augment.hip): et_letterbox_u8 the pixels, et_letterbox_targets the
    labels.  With rect the dataset is re-ordered as the reference re-orders it: an index is a POSITION of that order and the image
    behind it is self.order[index]; self.rect_batches lists the positions of every batch.
    PARITY: geometry, shapes, random streams, matrices, LUTs, flips and labels are pinned on the live reference
    (tests/golden/letterbox.npz); the 8-bit INTER_LINEAR resize, the warp sampling and the HSV round trip restate OpenCV's published
    algorithms (no cv2) -- the r == 1 case needs no resize and is a pad, exact by construction.
    cfg: the reference's config node (cfg.hyp, cfg.Dataset.img_size / np / num_ids); n: the number of images; shapes_wh: their original
    (w, h), needed with rect.  What the kernels do not cover raises NotImplementedError here."""

    def __init__(self, cfg, n, seed=None, stream=None, augment=False, rect=False, batch_size=None, stride=32, pad=0.0, shapes_wh=None,
                 image_weights=False, albumentations=False):
        hyp, ds = cfg.hyp, cfg.Dataset
        g = lambda node, k, d=0: (node.get(k, d) if hasattr(node, "get") else getattr(node, k, d))
        if float(g(hyp, "perspective", 0.0)) != 0:
            raise NotImplementedError("LetterboxBatchGenerator: hyp.perspective != 0 needs cv2.warpPerspective's projective sampling; "
                                      "the kernel implements the affine warp of every shipped recipe")
        if int(g(ds, "np", 0)) > 0:
            raise NotImplementedError("LetterboxBatchGenerator: Dataset.np > 0 (keypoint labels) is not transformed on the device")
        if int(g(ds, "num_ids", 0)) > 0:
            raise NotImplementedError("LetterboxBatchGenerator: Dataset.num_ids > 0 (with_id: a tracking id per label) is not carried on the device")
        if image_weights:
            raise NotImplementedError("LetterboxBatchGenerator: image_weights re-draws the index list per epoch on the host; not supported")
        if albumentations:
            raise NotImplementedError("LetterboxBatchGenerator: the albumentations pipeline runs on host arrays; not supported")
        self.hyp, self.s, self.n = hyp, int(ds.img_size), int(n)
        self._g = g
        self.augment, self.rect = bool(augment), bool(rect)
        self.mosaic = False                                      # the closed mosaic; True draws the gate and needs hyp.mosaic == 0
        self.order = np.arange(self.n)
        if self.rect:
            if batch_size is None or shapes_wh is None or len(shapes_wh) != self.n:
                raise ValueError("LetterboxBatchGenerator: rect needs batch_size and the original (w, h) of every image")
            self.order, self.batch, self.batch_shapes = rect_batch_shapes(shapes_wh, int(batch_size), self.s, stride, pad)
            self.rect_batches = [np.flatnonzero(self.batch == b).tolist() for b in range(int(self.batch[-1]) + 1)]
        self.py_rng = random.Random(seed)
        self.np_rng = np.random.RandomState(seed)
        self.stream = stream

    def new_shape(self, index):
        """the final letterboxed shape of position `index` (datasets.py:909): a batch_shapes row (numpy ints) with rect, else img_size"""
        return self.batch_shapes[self.batch[index]] if self.rect else self.s

    def sample(self, index):
        """host side of one image: {'shape': (H, W), 'M': (3,3) or None, 's', 'lut': (3,256) u8 or None, 'flipud', 'fliplr'}; without
        augment nothing is drawn"""
        hyp, g = self.hyp, self._g
        shape = self.new_shape(index)
        H, W = (shape, shape) if isinstance(shape, int) else (int(shape[0]), int(shape[1]))
        if self.mosaic and self.py_rng.random() < g(hyp, "mosaic", 1.0):
            raise NotImplementedError("LetterboxBatchGenerator: this image takes the mosaic branch (LabeledBatchGenerator); a batch that "
                                      "mixes both branches is not supported")
        if not self.augment:
            return dict(shape=(H, W), M=None, s=1.0, lut=None, flipud=False, fliplr=False)
        M, sc = affine_matrix(H, W, g(hyp, "degrees"), g(hyp, "translate"), g(hyp, "scale"), g(hyp, "shear"), self.py_rng)
        hs = (g(hyp, "hsv_h", 0.0), g(hyp, "hsv_s", 0.0), g(hyp, "hsv_v", 0.0))
        lut = hsv_luts(*hs, self.np_rng) if any(hs) else None
        ud = self.py_rng.random() < g(hyp, "flipud", 0.0)
        lr = self.py_rng.random() < g(hyp, "fliplr", 0.0)
        return dict(shape=(H, W), M=M, s=sc, lut=lut, flipud=bool(ud), fliplr=bool(lr))

    @staticmethod
    def label_dtype_mode(scale, pad):
        """how THIS numpy evaluates xywhn2xyxy's `w * (x - x / 2) + padw` on float32 labels (utils/general.py:640): 0 float32 throughout
        (Python floats are weak), 1 float32 product and float64 sum, 2 float64 throughout (numpy float64 scalars are not weak)"""
        x = np.zeros(1, np.float32)
        p = scale * x
        return 2 if p.dtype == np.float64 else int((p + pad).dtype == np.float64)

    def launch(self, images, labels, indices, hw0=None, paths=None):
        """sample every image of the batch and launch the two kernels (on self.stream when given) -> PendingLetterboxBatch"""
        from .. import ops
        B = len(indices)
        samples = [self.sample(int(i)) for i in indices]
        H, W = samples[0]["shape"]
        if any(sm["shape"] != (H, W) for sm in samples):
            raise ValueError("LetterboxBatchGenerator: the images of one batch must share their letterboxed shape (with rect: one of rect_batches)")
        use_lut = any(sm["lut"] is not None for sm in samples)
        f64 = np.zeros(B * 20)                                   # one staging array: minv (B,6) | M (B,9) | s (B,) | geom (B,4)
        minv, M, sc, geom = f64[:B * 6].reshape(B, 6), f64[B * 6:B * 15].reshape(B, 9), f64[B * 15:B * 16], f64[B * 16:].reshape(B, 4)
        minv[:] = [1, 0, 0, 0, 1, 0]; M[:] = np.eye(3).reshape(9); sc[:] = 1.0
        i32 = np.zeros(B * 4, np.int32)                          # flags (B,3) | wide (B,)
        flags, wide = i32[:B * 3].reshape(B, 3), i32[B * 3:]
        lut = np.tile(np.arange(256, dtype=np.uint8), (B, 3, 1)) if use_lut else None
        rows = np.zeros((B, 2), np.int32)
        ims, geo, labs, shapes, row = [], [], [], [], 0
        for b, (i, sm) in enumerate(zip(indices, samples)):
            src = int(self.order[int(i)])
            im = images[src]
            h, w = int(im.shape[1]), int(im.shape[2])
            ratio, (dw, dh), (nw, nh), top, left = letterbox_geometry(h, w, self.new_shape(int(i)), scaleup=self.augment)
            ims.append(im); geo.append((nw, nh, left, top))
            h0, w0 = (h, w) if hw0 is None else hw0[src]
            shapes.append(((h0, w0), ((h / h0, w / w0), (dw, dh))))
            lab = np.asarray(labels[src], dtype=np.float32).reshape(-1, 5)
            rows[b] = (row, row + lab.shape[0])
            labs.append(lab); row += lab.shape[0]
            geom[b] = (ratio[0] * w, ratio[1] * h, dw, dh)
            wide[b] = self.label_dtype_mode(ratio[0] * w, dw)
            flags[b] = (self.augment, sm["flipud"], sm["fliplr"])
            if sm["M"] is not None:
                minv[b], M[b], sc[b] = invert_affine(sm["M"]), sm["M"].reshape(-1), sm["s"]
            if sm["lut"] is not None:
                lut[b] = sm["lut"]
        lab_all = np.concatenate(labs, 0) if labs else np.zeros((0, 5), np.float32)
        dev = ims[0].device
        cuda = dev.type == "cuda"
        side = self.stream if cuda else None
        import contextlib
        if side is not None:
            side.wait_stream(torch.cuda.current_stream(dev))     # the source images were written on the caller's stream
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            t = lambda a: torch.from_numpy(a).to(dev, non_blocking=True)
            d64, d32 = t(f64), t(i32)
            dflags = d32[:B * 3].view(B, 3)
            imgs = ops.letterbox_u8(ims, geo, d64[:B * 6].view(B, 6), t(lut) if use_lut else None, dflags, H, W)
            out, n_dev = ops.letterbox_targets(t(lab_all), rows, d64[B * 16:].view(B, 4), d32[B * 3:], d64[B * 6:B * 15].view(B, 9),
                                               d64[B * 15:B * 16], dflags, H, W)
            n_host = event = None
            if cuda:
                n_host = torch.empty(1, dtype=torch.int32).pin_memory()
                n_host.copy_(n_dev, non_blocking=True)
                event = torch.cuda.Event()
                event.record(torch.cuda.current_stream(dev))
        srcs = [int(self.order[int(i)]) for i in indices]
        return PendingLetterboxBatch(tuple(shapes), imgs, out, n_dev, n_host, tuple(srcs) if paths is None else tuple(paths[i] for i in srcs),
                                     event, side)

    def __call__(self, images, labels, indices, hw0=None, paths=None):
        """images: image -> (3, h, w) uint8 device tensor (what load_image returns, as RGB planes); labels: image -> (n, 5) float32
        [cls, x, y, w, h] normalised; hw0: image -> (h0, w0) as load_image returns it (None: the images were not resized); indices:
        the dataset positions of this batch.  -> the reference's batch tuple (imgs (B,3,H,W) uint8, targets (n,6) float32 [img, cls, x, y,
        w, h], paths, shapes) with shapes[i] = ((h0, w0), ((h / h0, w / w0), (dw, dh))), tensors on the device"""
        return self.launch(images, labels, indices, hw0, paths).result()

    def batches(self, images, labels, index_batches=None, hw0=None, paths=None):
        """the dataloader iterable of val.run / Trainer: batch k + 1 is launched before batch k is handed out.  index_batches None:
        self.rect_batches"""
        pending = None
        for idx in (self.rect_batches if index_batches is None else index_batches):
            nxt = self.launch(images, labels, list(idx), hw0, paths)
            if pending is not None:
                yield pending.result()
            pending = nxt
        if pending is not None:
            yield pending.result()
