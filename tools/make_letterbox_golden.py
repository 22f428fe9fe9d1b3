"""Write tests/golden/letterbox.npz: the LIVE reference's labeled loader with the mosaic closed, on a seven-image in-memory dataset.

The reference is imported through oracle/ref_loader.py (nothing of it is copied): its own ``LoadImagesAndLabels.__getitem__`` runs
unbound on a dataset namespace with ``mosaic = False`` (the letterbox branch, utils/datasets.py:904-953), and its ``collate_fn`` collates
every batch.  Needs the reference tree, so it runs in the build container only:

    python tools/make_letterbox_golden.py

Three groups of samples from ONE seeded pair of random streams:
  A   augment, img_size 32, not rect: six samples letterboxed to 32 x 32 (one of them a 12 x 9 image that scaleup enlarges)
  B   augment, rect: three samples letterboxed to 32 x 64 (H != W; numpy-typed shapes)
  V   augment = False, rect (the validation form): three batches of two, 32 x 64, 64 x 32 and 32 x 32, one image needing the resize
cv2 is not installed, so its calls are RECORDERS that pass pixels through the numpy restatements of tests/letterbox_ref.py and
tests/labeled_mosaic_ref.py:
  resize                records new_unpad, returns the restated 8-bit INTER_LINEAR resize
  copyMakeBorder        records (top, bottom, left, right), returns the padded image
  getRotationMatrix2D   the closed form (records the scale s)
  warpAffine            records M, returns the restated fixed-point bilinear warp
  cvtColor / split / merge / LUT    record the three LUTs, pass pixels through the restated 8-bit RGB <-> HSV round trip
letterbox is wrapped to record its (ratio, pad) and the TYPES of ratio and pad (they decide the dtype numpy gives xywhn2xyxy's
expression); np.flipud and np.fliplr record the flips.  What the file therefore pins on the reference: the geometry, `shapes`, the
consumption of both random streams, M, s, the LUTs, the flips and ALL label arithmetic (labels_out, the collated batches).  The PIXELS
of ``out*`` are ORACLE-DERIVED: the reference's control flow around this repository's restatement of OpenCV, not cv2's output.

The tool REFUSES a seed (and moves on to the next) when any box_candidates or clip decision of any row lies within 1e-6 (relative) of
its threshold, so that tests may demand survivorship exactly; and when the samples do not cover what the tests need: a label dropped by
box_candidates, a label clipped at each of the four canvas edges, an image without labels, both values of both flips."""
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import labeled_mosaic_ref as lr  # noqa: E402
from tests import letterbox_ref as lt  # noqa: E402

S = 32
SHAPES = [(32, 24), (20, 32), (32, 32), (12, 9), (48, 36), (32, 13), (16, 32)]     # (h, w) of the in-memory images
HW0 = [(64, 48), (41, 65), (32, 32), (12, 9), (97, 72), (70, 29), (33, 64)]        # what load_image would report as the original size
GROUP_A = (0, 3, 6, 1, 2, 5)
BATCH_SHAPES = np.array([[32, 64], [64, 32], [32, 32]])                             # (H, W) rows, numpy ints as datasets.py:795 leaves them
GROUP_B = (1, 6, 3)                                                                # all in batch 0
GROUP_V = ((1, 6), (0, 5), (4, 2))                                                 # batches 0, 1, 2
BATCH_OF = np.array([1, 0, 2, 0, 2, 1, 0])                                         # image -> row of BATCH_SHAPES
SEED0 = 20261020
REL = 1e-6


class Unfit(Exception):
    pass


class Hyp(dict):
    __getattr__ = dict.__getitem__


def dataset(rng):
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]     # BGR, HWC: what load_image returns
    labels = []
    for k in range(len(SHAPES)):
        n = 0 if k == 6 else int(rng.integers(4, 9))                                # image 6 has no label
        lb = np.zeros((n, 5), np.float32)
        if n:
            lb[:, 0] = rng.integers(0, 80, n)
            lb[:, 1:3] = rng.uniform(0.2, 0.8, (n, 2))
            lb[:, 3:5] = np.minimum(rng.uniform(0.2, 0.7, (n, 2)), 2 * np.minimum(lb[:, 1:3], 1 - lb[:, 1:3]))
            lb[0, 1:] = (0.12, 0.5, 0.24, 0.6)                                      # touches the left border
            lb[1, 1:] = (0.6, 0.9, 0.5, 0.2)                                        # touches the bottom border
            lb[2, 3:5] = rng.uniform(0.02, 0.06, 2)                                 # tiny
            lb[3, 1:] = (0.85, 0.15, 0.3, 0.3)                                      # touches the top and the right border
        labels.append(lb)
    return imgs, labels


def near(v, thr, scale=None):
    v = np.asarray(v, np.float64)
    return bool((np.abs(v - thr) <= REL * (abs(thr) if scale is None else scale)).any())


def type_code(v):
    """0 a Python number (weak in numpy's promotion), 1 a numpy scalar"""
    return int(isinstance(v, np.generic))


def run(seed):
    import utils.augmentations as A
    import utils.datasets as D
    cv2 = sys.modules["cv2"]
    rng = np.random.default_rng(seed)
    imgs, labels = dataset(rng)
    hyp = Hyp(mosaic=1.0, mixup=0.5, copy_paste=0.0, degrees=10.0, translate=0.1, scale=0.5, shear=2.0, perspective=0.0,
              hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, flipud=0.5, fliplr=0.5)
    n = len(SHAPES)
    ds = types.SimpleNamespace(indices=range(n), n=n, hyp=hyp, mosaic=False, num_points=0, with_id=False, img_size=S,
                               imgs=imgs, img_hw0=HW0, img_hw=SHAPES, labels=labels, segments=[[] for _ in SHAPES], augment=True,
                               rect=False, batch_shapes=BATCH_SHAPES, batch=BATCH_OF, albumentations=A.Albumentations(), debug=False,
                               img_files=[f"img{k}" for k in range(n)])
    rec = {}
    stats = dict(dropped=0, kept=0, left=0, right=0, top=0, bottom=0)
    cur = {}

    def rotation(angle, center, scale):
        assert tuple(center) == (0, 0)
        rec["s"] = float(scale)
        a = np.radians(angle)
        al, be = scale * np.cos(a), scale * np.sin(a)
        return np.array([[al, be, 0.0], [-be, al, 0.0]])

    def resize(im, dsize, interpolation=None):
        assert interpolation == cv2.INTER_LINEAR
        rec["resize"] = tuple(int(v) for v in dsize)
        out = lt.resize(np.ascontiguousarray(im.transpose(2, 0, 1)), int(dsize[0]), int(dsize[1]))
        return np.ascontiguousarray(out.transpose(1, 2, 0))

    def make_border(im, top, bottom, left, right, kind, value=None):
        assert kind == cv2.BORDER_CONSTANT and tuple(value) == (114, 114, 114)
        rec["border"] = (top, bottom, left, right)
        out = np.full((im.shape[0] + top + bottom, im.shape[1] + left + right, 3), 114, np.uint8)
        out[top:top + im.shape[0], left:left + im.shape[1]] = im
        return out

    def warp_affine(img, M, dsize, borderValue=(0, 0, 0)):
        H, W = img.shape[:2]
        assert tuple(dsize) == (W, H) and tuple(borderValue) == (114, 114, 114)
        rec["M"] = np.array(M, np.float64).copy()
        cur["HW"] = (H, W)
        out = lr.warp(np.ascontiguousarray(img.transpose(2, 0, 1)), lr.invert_affine(M), H, W, 114)
        return np.ascontiguousarray(out.transpose(1, 2, 0))

    def cvt_color(im, code, dst=None):
        if code == cv2.COLOR_BGR2HSV:
            return np.stack(lr.rgb_to_hsv(im[..., 2], im[..., 1], im[..., 0]), -1)
        assert code == cv2.COLOR_HSV2BGR and dst is not None
        r, g, b = lr.hsv_to_rgb(im[..., 0], im[..., 1], im[..., 2])
        dst[...] = np.stack((b, g, r), -1)
        return dst

    def lut(ch, table):
        rec.setdefault("lut", []).append(np.array(table).copy())
        return table[ch]

    orig_bc, orig_ud, orig_lr, orig_lb = A.box_candidates, np.flipud, np.fliplr, D.letterbox

    def letterbox(im, new_shape, **k):
        assert k.get("auto") is False and not k.get("scaleFill", False)
        out, ratio, pad = orig_lb(im, new_shape, **k)
        rec["ratio"], rec["pad"] = (float(ratio[0]), float(ratio[1])), (float(pad[0]), float(pad[1]))
        rec["types"] = (type_code(ratio[0]), type_code(pad[0]))
        rec["canvas"] = out.copy()
        return out, ratio, pad

    def box_candidates(box1, box2, **k):
        fr = sys._getframe(1).f_locals                          # random_perspective_keypoints' corners BEFORE its clip
        H, W = fr["height"], fr["width"]
        x, y = fr["x"], fr["y"]
        for v, ext in ((x, W), (y, H)):
            if near(v.min(1), 0.0, ext) or near(v.min(1), ext, ext) or near(v.max(1), 0.0, ext) or near(v.max(1), ext, ext):
                raise Unfit("a corner within 1e-6 of the clip to the canvas")
        stats["left"] += int((x.min(1) < 0).sum()); stats["right"] += int((x.max(1) > W).sum())
        stats["top"] += int((y.min(1) < 0).sum()); stats["bottom"] += int((y.max(1) > H).sum())
        w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
        w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
        ar = np.maximum(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16))
        if near(w2, 2.0) or near(h2, 2.0) or near(w2 * h2 / (w1 * h1 + 1e-16), 0.1) or near(ar, 20.0):
            raise Unfit("a box_candidates term within 1e-6 of its threshold")
        if near(box2[[0, 2]], W - 1e-3, W) or near(box2[[1, 3]], H - 1e-3, H):
            raise Unfit("a coordinate within 1e-6 of xyxy2xywhn's clip to the size - eps")
        i = orig_bc(box1, box2, **k)
        stats["dropped"] += int((~i).sum())
        stats["kept"] += int(i.sum())
        return i

    names = ("getRotationMatrix2D", "warpAffine", "cvtColor", "split", "merge", "LUT", "resize", "copyMakeBorder")
    keep = {k: cv2.__dict__.get(k) for k in names}
    cv2.getRotationMatrix2D, cv2.warpAffine, cv2.cvtColor, cv2.LUT = rotation, warp_affine, cvt_color, lut
    cv2.resize, cv2.copyMakeBorder = resize, make_border
    cv2.split = lambda im: tuple(im[..., k] for k in range(im.shape[-1]))
    cv2.merge = lambda chans: np.stack(chans, -1)
    A.box_candidates, D.letterbox = box_candidates, letterbox
    np.flipud = lambda a: (rec.__setitem__("ud", 1), orig_ud(a))[1]
    np.fliplr = lambda a: (rec.__setitem__("lr", 1), orig_lr(a))[1]
    out = {}

    def sample(tag, index):
        rec.clear()
        img, labels_out, path, shapes = D.LoadImagesAndLabels.__getitem__(ds, index)
        (h0, w0), ((rh, rw), (dw, dh)) = shapes
        out[f"shapes{tag}"] = np.array([h0, w0, rh, rw, dw, dh], np.float64)
        out[f"ratio{tag}"] = np.array(rec["ratio"]); out[f"pad{tag}"] = np.array(rec["pad"])
        out[f"types{tag}"] = np.array(rec["types"])
        out[f"unpad{tag}"] = np.array(rec.get("resize", SHAPES[index][::-1]))       # no resize: new_unpad is the image's (w, h)
        out[f"resized{tag}"] = np.array([int("resize" in rec)])
        out[f"border{tag}"] = np.array(rec["border"])
        out[f"canvas{tag}"] = rec["canvas"]
        out[f"HW{tag}"] = np.array(img.shape[1:])
        if ds.augment:
            assert len(rec["lut"]) == 3
            out[f"M{tag}"] = rec["M"]; out[f"s{tag}"] = np.array([rec["s"]]); out[f"lut{tag}"] = np.stack(rec["lut"]).astype(np.uint8)
        else:
            assert "M" not in rec and "lut" not in rec
        out[f"flips{tag}"] = np.array([rec.get("ud", 0), rec.get("lr", 0)])
        out[f"out{tag}"] = img.numpy().copy()                                       # ORACLE-DERIVED pixels (RGB planes)
        out[f"labels_out{tag}"] = labels_out.numpy().copy()
        return img, labels_out, path, shapes
    try:
        random.seed(seed)
        np.random.seed(seed)
        batch = [sample(f"A{j}", i) for j, i in enumerate(GROUP_A)]
        out["targetsA"] = D.LoadImagesAndLabels.collate_fn(batch)[1].numpy().copy()
        ds.rect = True
        batch = [sample(f"B{j}", i) for j, i in enumerate(GROUP_B)]
        out["targetsB"] = D.LoadImagesAndLabels.collate_fn(batch)[1].numpy().copy()
        state, np_state = random.getstate(), np.random.get_state()
        ds.augment = False
        for k, idx in enumerate(GROUP_V):
            batch = [sample(f"V{k}_{j}", i) for j, i in enumerate(idx)]
            out[f"targetsV{k}"] = D.LoadImagesAndLabels.collate_fn(batch)[1].numpy().copy()
        assert random.getstate() == state and all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), np_state))
        out["next_random"] = np.array([random.random()])
        out["next_np_random"] = np.array([np.random.random()])
    finally:
        for k, v in keep.items():
            if v is None:
                delattr(cv2, k)
            else:
                setattr(cv2, k, v)
        A.box_candidates, np.flipud, np.fliplr, D.letterbox = orig_bc, orig_ud, orig_lr, orig_lb
    fl = np.stack([out[f"flips{t}"] for t in [f"A{j}" for j in range(len(GROUP_A))] + [f"B{j}" for j in range(len(GROUP_B))]])
    if not (set(fl[:, 0]) == {0, 1} and set(fl[:, 1]) == {0, 1}):
        raise Unfit("a flip never (or always) happens")
    if stats["dropped"] < 1 or stats["kept"] < 10 or min(stats[k] for k in ("left", "right", "top", "bottom")) < 1:
        raise Unfit(f"coverage {stats}")
    for k, im in enumerate(imgs):
        out[f"img{k}"] = im
        out[f"lab{k}"] = labels[k]
    out["shapes_hw"] = np.array(SHAPES); out["hw0"] = np.array(HW0)
    out["groupA"] = np.array(GROUP_A); out["groupB"] = np.array(GROUP_B); out["groupV"] = np.array(GROUP_V)
    out["batch_shapes"] = BATCH_SHAPES; out["batch_of"] = BATCH_OF
    out["S"] = np.array([S])
    out["seed"] = np.array([seed])
    return out, stats


def main():
    ref_loader.load()
    for seed in range(SEED0, SEED0 + 400):
        try:
            out, stats = run(seed)
        except Unfit as e:
            print(f"seed {seed}: {e}")
            continue
        break
    else:
        raise SystemExit("no seed fits")
    path = os.path.join(ROOT, "tests", "golden", "letterbox.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"seed {seed}: {stats}, collated targets A {out['targetsA'].shape} B {out['targetsB'].shape}")
    print(path, size, "bytes")
    if size > 200 * 1024:
        os.remove(path)
        raise SystemExit("the golden exceeds 200 KB")


if __name__ == "__main__":
    main()
