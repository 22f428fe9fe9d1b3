"""Numpy restatements for the letterbox-batch tests (tests/test_letterbox.py) and the golden tool (tools/make_letterbox_golden.py).

TEST INFRASTRUCTURE, independent of the package's code: cv2.resize's 8-bit INTER_LINEAR (resize.cpp: per-axis float offsets, 11-bit
coefficients as shorts, int32 horizontal pass, the vertical pass's two shifted products), copyMakeBorder, and the label arithmetic of
the letterbox branch in numpy with the reference's dtypes.  The warp and the HSV round trip come from tests/labeled_mosaic_ref.py.  The
OpenCV parts restate the published algorithms (cv2 is not installed): they pin the kernel to this reading of them, not to cv2."""
import numpy as np

from tests import labeled_mosaic_ref as lr


def resize_axis(dst, src):
    """one axis of cv2.resize INTER_LINEAR, 8 bit -> (s0 (dst,), s1 (dst,), c0 (dst,), c1 (dst,)): source indices and short coefficients"""
    scale = 1.0 / (float(dst) / float(src))
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    lo, hi = s < 0, s >= src - 1
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, src - 1), c0, c1


def resize(img, nw, nh):
    """cv2.resize(img, (nw, nh), interpolation=INTER_LINEAR) on (C, h, w) uint8"""
    C, h, w = img.shape
    sx, sx1, a0, a1 = resize_axis(nw, w)
    sy, sy1, b0, b1 = resize_axis(nh, h)
    p = img.astype(np.int64)
    S = a0 * p[:, :, sx] + a1 * p[:, :, sx1]                      # (C, h, nw) int32 in OpenCV: at most 2048 * 255
    S0, S1 = S[:, sy], S[:, sy1]
    out = (((b0[:, None] * (S0 >> 4)) >> 16) + ((b1[:, None] * (S1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def letterboxed(img, nw, nh, left, top, H, W, border=114):
    """letterbox's pixels (utils/augmentations.py:117-122) on (3, h, w) uint8 -> the (3, H, W) canvas"""
    if (img.shape[2], img.shape[1]) != (nw, nh):
        img = resize(img, nw, nh)
    canvas = np.full((3, H, W), border, np.uint8)
    canvas[:, top:top + nh, left:left + nw] = img
    return canvas


def letterbox_image(img, geo, H, W, minv, lut, flipud, fliplr, border=114):
    """geo = (nw, nh, left, top); minv (6,) or None (no warp); lut (3, 256) or None -> the (3, H, W) uint8 image of the letterbox branch"""
    im = letterboxed(img, *geo, H, W, border)
    if minv is not None:
        im = lr.warp(im, minv, H, W, border)
    if lut is not None:
        im = lr.hsv_lut(im, lut)
    if flipud:
        im = im[:, ::-1]
    if fliplr:
        im = im[:, :, ::-1]
    return np.ascontiguousarray(im)


def labels_of_image(lb, rw, rh, padw, padh, H, W, M, sc, flipud, fliplr):
    """The label arithmetic of the letterbox branch in numpy, in the reference's expression order (utils/general.py:640-658,
    utils/augmentations.py:176-265,417-422, utils/datasets.py:913-1027).  lb (n, 5) float32; rw = ratio_w * w, rh, padw, padh: scalars
    of WHATEVER type the caller holds (Python float or numpy float64: numpy's promotion then decides the dtype of the expression, as it
    does in the reference); M (3,3) fp64 or None (no random_perspective_keypoints) -> (n', 5) float32 [cls, x, y, w, h]"""
    t = np.array(lb, np.float32).reshape(-1, 5).copy()
    if t.size:
        x = t[:, 1:5]
        y = np.copy(x)
        y[:, 0] = rw * (x[:, 0] - x[:, 2] / 2) + padw
        y[:, 1] = rh * (x[:, 1] - x[:, 3] / 2) + padh
        y[:, 2] = rw * (x[:, 0] + x[:, 2] / 2) + padw
        y[:, 3] = rh * (x[:, 1] + x[:, 3] / 2) + padh
        t[:, 1:5] = y
    n = len(t)
    if n and M is not None:
        xy = np.ones((n * 4, 3))
        xy[:, :2] = t[:, [1, 2, 3, 4, 1, 4, 3, 2]].reshape(n * 4, 2)
        xy = (xy @ M.T)[:, :2].reshape(n, 8)
        x, y = xy[:, [0, 2, 4, 6]], xy[:, [1, 3, 5, 7]]
        new = np.concatenate((x.min(1), y.min(1), x.max(1), y.max(1))).reshape(4, n).T
        new[:, [0, 2]] = new[:, [0, 2]].clip(0, W)
        new[:, [1, 3]] = new[:, [1, 3]].clip(0, H)
        box1, box2, eps = t[:, 1:5].T * sc, new.T, 1e-16
        w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
        w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
        ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
        i = (w2 > 2) & (h2 > 2) & (w2 * h2 / (w1 * h1 + eps) > 0.1) & (ar < 20)
        t = t[i]
        t[:, 1:5] = new[i]
    if len(t):
        x = t[:, 1:5]
        x[:, [0, 2]] = x[:, [0, 2]].clip(0, W - 1e-3)
        x[:, [1, 3]] = x[:, [1, 3]].clip(0, H - 1e-3)
        y = np.copy(x)
        y[:, 0] = ((x[:, 0] + x[:, 2]) / 2) / W
        y[:, 1] = ((x[:, 1] + x[:, 3]) / 2) / H
        y[:, 2] = (x[:, 2] - x[:, 0]) / W
        y[:, 3] = (x[:, 3] - x[:, 1]) / H
        t[:, 1:5] = y
        if flipud:
            t[:, 2] = 1 - t[:, 2]
        if fliplr:
            t[:, 1] = 1 - t[:, 1]
        t[:, 1:] = t[:, 1:].clip(0, 1.0)
    assert t.dtype == np.float32
    return t
