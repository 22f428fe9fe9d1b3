"""Numpy restatements for the labeled-batch tests (tests/test_labeled_mosaic.py) and the golden tool (tools/make_labeled_golden.py).

TEST INFRASTRUCTURE, independent of the package's code: the canvas paste of load_mosaic, cv2.warpAffine's fixed-point bilinear sampling
with SEPARATE source and destination sizes, the fp64 mixup with truncation, cvtColor's 8-bit RGB <-> HSV round trip around three LUTs,
and the label arithmetic of the mosaic branch in numpy with the reference's dtypes.  The OpenCV parts restate the published
algorithms (cv2 is not installed): they pin the kernel to this reading of them, not to cv2."""
import numpy as np

F = np.float32


def paste_canvas(s, tiles, layout, border=114):
    """tiles: four (3, h, w) uint8; layout: rows (x1a, y1a, x2a, y2a, x1b, y1b, ...) -> the (3, 2s, 2s) canvas of load_mosaic"""
    canvas = np.full((3, 2 * s, 2 * s), border, np.uint8)
    for (x1a, y1a, x2a, y2a, x1b, y1b, *_), im in zip(layout, tiles):
        canvas[:, y1a:y2a, x1a:x2a] = im[:, y1b:y1b + (y2a - y1a), x1b:x1b + (x2a - x1a)]
    return canvas


def invert_affine(M):
    """cv2.invertAffineTransform of the 2 x 3 forward map, as warpAffine applies it (fp64)"""
    M = np.asarray(M, np.float64)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    a11, a22, a12, a21 = M[1, 1] * D, M[0, 0] * D, M[0, 1] * -D, M[1, 0] * -D
    return np.array([a11, a12, -a11 * M[0, 2] - a12 * M[1, 2], a21, a22, -a21 * M[0, 2] - a22 * M[1, 2]])


def warp(img, minv, out_h, out_w, border=114):
    """cv2.warpAffine(img, M[:2], dsize=(out_w, out_h), borderValue=border), INTER_LINEAR, on (C, H, W) uint8: AB_BITS 10, INTER_BITS 5,
    weights * 2^15, constant border per tap.  minv: the inverted matrix (6,)"""
    C, H, W = img.shape
    ys, xs = np.mgrid[0:out_h, 0:out_w]
    rnd = lambda v: np.rint(v).astype(np.int64)
    X0 = rnd((minv[1] * ys + minv[2]) * 1024.0) + 16
    Y0 = rnd((minv[4] * ys + minv[5]) * 1024.0) + 16
    X = (X0 + rnd(minv[0] * xs * 1024.0)) >> 5
    Y = (Y0 + rnd(minv[3] * xs * 1024.0)) >> 5
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    out = np.zeros((C, out_h, out_w), np.uint8)

    def at(c, yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return np.where(ok, img[c][np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64), border)
    for c in range(C):
        v = ((32 - fx) * (32 - fy) * 32 * at(c, sy, sx) + fx * (32 - fy) * 32 * at(c, sy, sx + 1)
             + (32 - fx) * fy * 32 * at(c, sy + 1, sx) + fx * fy * 32 * at(c, sy + 1, sx + 1))
        out[c] = ((v + (1 << 14)) >> 15).astype(np.uint8)
    return out


def mixup(a, b, r):
    """augmentations.py:412 on uint8 arrays: fp64 products and sum, truncation"""
    return (a * r + b * (1 - r)).astype(np.uint8)


def rgb_to_hsv(r, g, b):
    """cvtColor(..., COLOR_RGB2HSV) on uint8 planes: the integer form with hsv_shift = 12 division tables, H in [0, 180)"""
    r, g, b = (x.astype(np.int64) for x in (r, g, b))
    i = np.arange(1, 256, dtype=np.float64)
    sdiv = np.concatenate(([0], np.rint((255 << 12) / i).astype(np.int64)))
    hdiv = np.concatenate(([0], np.rint((180 << 12) / (6.0 * i)).astype(np.int64)))
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    vr = np.where(v == r, -1, 0)
    vg = np.where(v == g, -1, 0)
    s = (diff * sdiv[v] + (1 << 11)) >> 12
    h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + (~vg & (r - g + 4 * diff))))
    h = (h * hdiv[diff] + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    return h.astype(np.uint8), s.astype(np.uint8), v.astype(np.uint8)


def hsv_to_rgb(h, s, v):
    """cvtColor(..., COLOR_HSV2RGB) on uint8 planes: float32 sector arithmetic, cvRound, saturation"""
    fs, fv = s.astype(F) * (F(1) / F(255)), v.astype(F) * (F(1) / F(255))
    hh = h.astype(F) * (F(6) / F(180))
    sector = np.floor(hh).astype(np.int64)
    hh = hh - sector.astype(F)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    hh = np.where(bad, F(0), hh).astype(F)
    one = F(1)
    tab = np.stack((fv, fv * (one - fs), fv * (one - fs * hh), fv * (one - fs * (one - hh))))
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])          # b, g, r
    pick = lambda k: np.take_along_axis(tab, sd[sector, k][None], 0)[0]
    fb, fg, fr = pick(0), pick(1), pick(2)
    grey = s == 0
    fr, fg, fb = (np.where(grey, fv, x).astype(F) for x in (fr, fg, fb))
    q = lambda x: np.clip(np.rint(x * F(255)), 0, 255).astype(np.uint8)
    return q(fr), q(fg), q(fb)


def hsv_lut(img, lut):
    """augment_hsv on a (3, H, W) uint8 RGB image with the three LUTs (3, 256)"""
    h, s, v = rgb_to_hsv(img[0], img[1], img[2])
    return np.stack(hsv_to_rgb(lut[0][h], lut[1][s], lut[2][v]))


def labeled_image(s, mosaics, r, lut, flipud, fliplr, border=114):
    """mosaics: [(tiles, layout, minv)] * (1 or 2) -> the (3, s, s) uint8 image of the mosaic branch"""
    ims = [warp(paste_canvas(s, t, lay, border), minv, s, s, border) for t, lay, minv in mosaics]
    im = ims[0] if len(ims) == 1 else mixup(ims[0], ims[1], r)
    if lut is not None:
        im = hsv_lut(im, lut)
    if flipud:
        im = im[:, ::-1]
    if fliplr:
        im = im[:, :, ::-1]
    return np.ascontiguousarray(im)


def labels_of_image(S, mosaics, flipud, fliplr):
    """The label arithmetic of the mosaic branch in numpy, in the reference's dtypes and expression order (utils/general.py:640-658,
    utils/augmentations.py:176-265,417-422, utils/datasets.py:962-1027).  mosaics: [(labels [4 x (n,5) float32], shapes [(h, w)] * 4,
    layout rows, M (3,3) fp64, s float)] -> (n, 5) float32 [cls, x, y, w, h]"""
    parts = []
    for labels, shapes, layout, M, sc in mosaics:
        l4 = []
        for lb, (h, w), row in zip(labels, shapes, layout):
            lb = np.array(lb, np.float32).reshape(-1, 5).copy()
            padw, padh = int(row[6]), int(row[7])
            if lb.size:
                x = lb[:, 1:5]
                y = np.copy(x)
                y[:, 0] = w * (x[:, 0] - x[:, 2] / 2) + padw
                y[:, 1] = h * (x[:, 1] - x[:, 3] / 2) + padh
                y[:, 2] = w * (x[:, 0] + x[:, 2] / 2) + padw
                y[:, 3] = h * (x[:, 1] + x[:, 3] / 2) + padh
                lb[:, 1:5] = y
            l4.append(lb)
        t = np.concatenate(l4, 0)
        n = len(t)
        if n:
            xy = np.ones((n * 4, 3))
            xy[:, :2] = t[:, [1, 2, 3, 4, 1, 4, 3, 2]].reshape(n * 4, 2)
            xy = (xy @ M.T)[:, :2].reshape(n, 8)
            x, y = xy[:, [0, 2, 4, 6]], xy[:, [1, 3, 5, 7]]
            new = np.concatenate((x.min(1), y.min(1), x.max(1), y.max(1))).reshape(4, n).T
            new[:, [0, 2]] = new[:, [0, 2]].clip(0, S)
            new[:, [1, 3]] = new[:, [1, 3]].clip(0, S)
            box1, box2, eps = t[:, 1:5].T * sc, new.T, 1e-16
            w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
            w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
            ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
            i = (w2 > 2) & (h2 > 2) & (w2 * h2 / (w1 * h1 + eps) > 0.1) & (ar < 20)
            t = t[i]
            t[:, 1:5] = new[i]
        parts.append(t)
    lab = np.concatenate(parts, 0)
    if len(lab):
        x = lab[:, 1:5]
        x[:, [0, 2]] = x[:, [0, 2]].clip(0, S - 1e-3)
        x[:, [1, 3]] = x[:, [1, 3]].clip(0, S - 1e-3)
        y = np.copy(x)
        y[:, 0] = ((x[:, 0] + x[:, 2]) / 2) / S
        y[:, 1] = ((x[:, 1] + x[:, 3]) / 2) / S
        y[:, 2] = (x[:, 2] - x[:, 0]) / S
        y[:, 3] = (x[:, 3] - x[:, 1]) / S
        lab[:, 1:5] = y
        if flipud:
            lab[:, 2] = 1 - lab[:, 2]
        if fliplr:
            lab[:, 1] = 1 - lab[:, 1]
        lab[:, 1:] = lab[:, 1:].clip(0, 1.0)
    assert lab.dtype == np.float32
    return lab
