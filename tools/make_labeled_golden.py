"""Write tests/golden/labeled_mosaic.npz: the LIVE reference's labeled loader on a six-image in-memory dataset.

The reference is imported through oracle/ref_loader.py (nothing of it is copied): its own ``LoadImagesAndLabels.__getitem__`` runs
unbound on a dataset namespace (the technique of oracle/make_golden.py::case_mosaic) with img_size 32, and its ``collate_fn`` collates
the samples.  Needs the reference tree, so it runs in the build container only:

    python tools/make_labeled_golden.py

cv2 is not installed, so its calls are RECORDERS that pass pixels through the numpy restatements of tests/labeled_mosaic_ref.py:
  getRotationMatrix2D   the closed form (records the scale s)
  warpAffine            records (canvas, M, dsize), returns the restated fixed-point bilinear warp
  cvtColor / split / merge / LUT    record the three LUTs, pass pixels through the restated 8-bit RGB <-> HSV round trip
np.random.beta, np.flipud and np.fliplr are wrapped to record the mixup ratio and the flips.  What the file therefore pins on the
reference: the consumption of both random streams, tile choice and placement (the canvases), M, s, r, the LUTs, the flips and ALL label
arithmetic (labels_out, the collated batch).  The PIXELS of ``out{j}`` are ORACLE-DERIVED: the reference's control flow around this
repository's restatement of OpenCV, not cv2's output.

The tool REFUSES a seed (and moves on to the next) when any box_candidates or clip decision of any row lies within 1e-6 (relative) of
its threshold, so that tests may demand survivorship exactly; and when the samples do not cover what the tests need (at least two
mixup samples and one without, both values of both flips, rows dropped and rows kept by box_candidates)."""
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import labeled_mosaic_ref as lr  # noqa: E402

S = 32
SHAPES = [(32, 24), (21, 32), (32, 32), (17, 32), (32, 13), (27, 32)]              # load_image: the longest side = img_size
ORDER = (0, 3, 5, 2, 1, 4)
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
        n = int(rng.integers(3, 9))
        lb = np.zeros((n, 5), np.float32)
        lb[:, 0] = rng.integers(0, 80, n)
        lb[:, 1:3] = rng.uniform(0.2, 0.8, (n, 2))
        lb[:, 3:5] = np.minimum(rng.uniform(0.2, 0.7, (n, 2)), 2 * np.minimum(lb[:, 1:3], 1 - lb[:, 1:3]))
        lb[0, 1:] = (0.12, 0.5, 0.24, 0.6)                                          # touches the left border
        lb[1, 1:] = (0.6, 0.9, 0.5, 0.2)                                            # touches the bottom border
        lb[2, 3:5] = rng.uniform(0.02, 0.06, 2)                                     # tiny
        labels.append(lb)
    return imgs, labels


def near(v, thr, scale=None):
    v = np.asarray(v, np.float64)
    return bool((np.abs(v - thr) <= REL * (abs(thr) if scale is None else scale)).any())


def run(seed):
    import utils.augmentations as A
    import utils.datasets as D
    cv2 = sys.modules["cv2"]
    rng = np.random.default_rng(seed)
    imgs, labels = dataset(rng)
    hyp = Hyp(mosaic=1.0, mixup=0.5, copy_paste=0.0, degrees=10.0, translate=0.1, scale=0.9, shear=2.0, perspective=0.0,
              hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, flipud=0.5, fliplr=0.5)
    n = len(SHAPES)
    ds = types.SimpleNamespace(indices=range(n), n=n, hyp=hyp, mosaic=True, num_points=0, with_id=False, img_size=S, mosaic_border=[-S // 2, -S // 2],
             imgs=imgs, img_hw0=SHAPES, img_hw=SHAPES, labels=labels, segments=[[] for _ in SHAPES], augment=True, rect=False,
             albumentations=A.Albumentations(), debug=False, img_files=[f"img{k}" for k in range(n)])
    rec = {}
    stats = dict(dropped=0, kept=0)

    def rotation(angle, center, scale):
        assert tuple(center) == (0, 0)
        rec.setdefault("s", []).append(float(scale))
        a = np.radians(angle)
        al, be = scale * np.cos(a), scale * np.sin(a)
        return np.array([[al, be, 0.0], [-be, al, 0.0]])

    def warp_affine(img, M, dsize, borderValue=(0, 0, 0)):
        assert tuple(dsize) == (S, S) and tuple(borderValue) == (114, 114, 114) and img.shape == (2 * S, 2 * S, 3)
        rec.setdefault("canvas", []).append(img.copy())
        rec.setdefault("M", []).append(np.array(M, np.float64).copy())
        out = lr.warp(np.ascontiguousarray(img.transpose(2, 0, 1)), lr.invert_affine(M), S, S, 114)
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

    orig_bc, orig_beta, orig_ud, orig_lr = A.box_candidates, np.random.beta, np.flipud, np.fliplr

    def box_candidates(box1, box2, **k):
        fr = sys._getframe(1).f_locals                          # random_perspective_keypoints' corners BEFORE its clip
        for v in (fr["x"], fr["y"]):
            if near(v.min(1), 0.0, S) or near(v.min(1), S, S) or near(v.max(1), 0.0, S) or near(v.max(1), S, S):
                raise Unfit("a corner within 1e-6 of the clip to [0, S]")
        w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
        w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
        ar = np.maximum(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16))
        if near(w2, 2.0) or near(h2, 2.0) or near(w2 * h2 / (w1 * h1 + 1e-16), 0.1) or near(ar, 20.0):
            raise Unfit("a box_candidates term within 1e-6 of its threshold")
        if near(box2, S - 1e-3, S):
            raise Unfit("a coordinate within 1e-6 of xyxy2xywhn's clip to S - eps")
        i = orig_bc(box1, box2, **k)
        stats["dropped"] += int((~i).sum())
        stats["kept"] += int(i.sum())
        return i

    def beta(a, b):
        r = orig_beta(a, b)
        rec.setdefault("r", []).append(float(r))
        return r
    names = ("getRotationMatrix2D", "warpAffine", "cvtColor", "split", "merge", "LUT")
    keep = {k: cv2.__dict__.get(k) for k in names}
    cv2.getRotationMatrix2D, cv2.warpAffine, cv2.cvtColor, cv2.LUT = rotation, warp_affine, cvt_color, lut
    cv2.split = lambda im: tuple(im[..., k] for k in range(im.shape[-1]))
    cv2.merge = lambda chans: np.stack(chans, -1)
    A.box_candidates = box_candidates
    np.random.beta = beta
    np.flipud = lambda a: (rec.setdefault("ud", []).append(1), orig_ud(a))[1]
    np.fliplr = lambda a: (rec.setdefault("lr", []).append(1), orig_lr(a))[1]
    out = {}
    batch = []
    try:
        random.seed(seed)
        np.random.seed(seed)
        for j, index in enumerate(ORDER):
            rec.clear()
            img, labels_out, path, shapes = D.LoadImagesAndLabels.__getitem__(ds, index)
            assert shapes is None and img.shape == (3, S, S)
            batch.append((img, labels_out, path, shapes))
            nm = len(rec["canvas"])
            assert nm in (1, 2) and len(rec["M"]) == nm and len(rec["s"]) == nm and len(rec.get("r", [])) == nm - 1
            assert len(rec["lut"]) == 3
            for m in range(nm):
                out[f"canvas{j}_{m}"] = rec["canvas"][m]
            out[f"M{j}"] = np.stack(rec["M"])                                   # (nm, 2, 3)
            out[f"s{j}"] = np.array(rec["s"])
            out[f"r{j}"] = np.array(rec.get("r", []))
            out[f"lut{j}"] = np.stack(rec["lut"]).astype(np.uint8)
            out[f"flips{j}"] = np.array([len(rec.get("ud", [])), len(rec.get("lr", []))])
            out[f"out{j}"] = img.numpy().copy()                                 # ORACLE-DERIVED pixels (RGB planes)
            out[f"labels_out{j}"] = labels_out.numpy().copy()
        out["next_random"] = np.array([random.random()])
        out["next_np_random"] = np.array([np.random.random()])
        _, targets, _, _ = D.LoadImagesAndLabels.collate_fn(batch)
        out["targets"] = targets.numpy().copy()
    finally:
        for k, v in keep.items():
            if v is None:
                delattr(cv2, k)
            else:
                setattr(cv2, k, v)
        A.box_candidates, np.random.beta, np.flipud, np.fliplr = orig_bc, orig_beta, orig_ud, orig_lr
    nmix = sum(out[f"r{j}"].size for j in range(len(ORDER)))
    fl = np.stack([out[f"flips{j}"] for j in range(len(ORDER))])
    if not (2 <= nmix < len(ORDER)):
        raise Unfit(f"{nmix} mixup samples")
    if not (set(fl[:, 0]) == {0, 1} and set(fl[:, 1]) == {0, 1}):
        raise Unfit("a flip never (or always) happens")
    if stats["dropped"] < 3 or stats["kept"] < 10:
        raise Unfit(f"box_candidates {stats}")
    for k, im in enumerate(imgs):
        out[f"img{k}"] = im
        out[f"lab{k}"] = labels[k]
    out["index"] = np.array(ORDER)
    out["S"] = np.array([S])
    out["seed"] = np.array([seed])
    return out, stats, nmix


def main():
    ref_loader.load()
    for seed in range(SEED0, SEED0 + 200):
        try:
            out, stats, nmix = run(seed)
        except Unfit as e:
            print(f"seed {seed}: {e}")
            continue
        break
    else:
        raise SystemExit("no seed fits")
    path = os.path.join(ROOT, "tests", "golden", "labeled_mosaic.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"seed {seed}: {nmix} mixup samples, box_candidates {stats}, collated targets {out['targets'].shape}")
    print(path, size, "bytes")
    if size > 200 * 1024:
        os.remove(path)
        raise SystemExit("the golden exceeds 200 KB")


if __name__ == "__main__":
    main()
