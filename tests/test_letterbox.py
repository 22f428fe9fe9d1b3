"""Letterbox batches on the device (csrc/augment.hip et_letterbox_u8 / et_letterbox_targets, utils/augment.py LetterboxBatchGenerator;
reference utils/datasets.py:904-953 LoadImagesAndLabels.__getitem__, letterbox branch: validation / rect batches and the closed mosaic).

tests/golden/letterbox.npz comes from the LIVE reference (tools/make_letterbox_golden.py): its own __getitem__ with mosaic = False and
its collate_fn on a seven-image in-memory dataset -- six augment samples at 32 x 32, three augment + rect samples at 32 x 64, three
validation batches (32 x 64, 64 x 32, 32 x 32) -- from one seeded pair of random streams.  PINNED on it: the letterbox geometry,
`shapes`, the consumption of `random` and `np.random`, M, s, the LUTs, the flips and all label arithmetic.  cv2 is not installed, so the
golden's PIXELS (`out*`) are ORACLE-DERIVED: the reference's control flow around the numpy restatement of OpenCV's published 8-bit
INTER_LINEAR resize (tests/letterbox_ref.py), fixed-point warp and HSV round trip (tests/labeled_mosaic_ref.py); the kernel is held to
that restatement, to the existing kernels and to invariants, not to cv2."""
import random
import types

import numpy as np
import pytest
import torch

from tests import labeled_mosaic_ref as lr
from tests import letterbox_ref as lt
from tests.conftest import golden

HYP = dict(mosaic=1.0, mixup=0.5, copy_paste=0.0, degrees=10.0, translate=0.1, scale=0.5, shear=2.0, perspective=0.0,
           hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, flipud=0.5, fliplr=0.5)
XYWH_TOL = 2 * 2.0 ** -23


def _cfg(S=32, dataset=None, **hyp):
    return types.SimpleNamespace(hyp=types.SimpleNamespace(**{**HYP, **hyp}),
                                 Dataset=types.SimpleNamespace(**{**dict(img_size=S, np=0, num_ids=0), **(dataset or {})}))


def _golden_dataset(g):
    imgs = [np.ascontiguousarray(g[f"img{k}"][:, :, ::-1].transpose(2, 0, 1)) for k in range(len(g["shapes_hw"]))]   # BGR HWC -> RGB planes
    return imgs, [g[f"lab{k}"] for k in range(len(imgs))], [tuple(int(v) for v in r) for r in g["hw0"]]


def _generators(g):
    """(A, B, V): the augment generator at img_size, the augment + rect one and the validation one.  B continues A's random streams, as the
    golden's samples were drawn; the rect generators take the golden's hand-made batch shapes in place of rect_batch_shapes' own"""
    from efficientteacher_amd.utils.augment import LetterboxBatchGenerator
    n, S, seed = len(g["shapes_hw"]), int(g["S"][0]), int(g["seed"][0])
    wh0 = [(w, h) for h, w in g["hw0"]]
    A = LetterboxBatchGenerator(_cfg(S), n, seed=seed, augment=True)
    B = LetterboxBatchGenerator(_cfg(S), n, seed=seed, augment=True, rect=True, batch_size=3, shapes_wh=wh0)
    V = LetterboxBatchGenerator(_cfg(S), n, seed=seed, augment=False, rect=True, batch_size=3, shapes_wh=wh0)
    B.py_rng, B.np_rng = A.py_rng, A.np_rng
    for gen in (B, V):
        gen.order, gen.batch, gen.batch_shapes = np.arange(n), g["batch_of"], g["batch_shapes"]
    return A, B, V


def _samples(g):
    """(generator key, tag, image index) of every golden sample in the order they were drawn"""
    out = [("A", f"A{j}", int(i)) for j, i in enumerate(g["groupA"])] + [("B", f"B{j}", int(i)) for j, i in enumerate(g["groupB"])]
    return out + [("V", f"V{k}_{j}", int(i)) for k, idx in enumerate(g["groupV"]) for j, i in enumerate(idx)]


# ---- 1. geometry and recipe against the live reference (host only) ------------------------------------------------------------------------
def test_geometry_and_recipe_equal_the_reference():
    from efficientteacher_amd.utils.augment import letterbox_geometry
    g = golden("letterbox")
    gens = dict(zip("ABV", _generators(g)))
    hw, hw0 = g["shapes_hw"], g["hw0"]
    seen_hw, modes = set(), set()
    for key, tag, i in _samples(g):
        gen = gens[key]
        h, w = (int(v) for v in hw[i])
        ratio, (dw, dh), (nw, nh), top, left = letterbox_geometry(h, w, gen.new_shape(i), scaleup=gen.augment)
        H, W = (int(v) for v in g[f"HW{tag}"])
        assert tuple(ratio) == tuple(g[f"ratio{tag}"]) and (dw, dh) == tuple(g[f"pad{tag}"]), tag
        assert (nw, nh) == tuple(g[f"unpad{tag}"]) and ((nw, nh) != (w, h)) == bool(g[f"resized{tag}"][0]), tag
        assert (top, H - nh - top, left, W - nw - left) == tuple(g[f"border{tag}"]), tag
        # the dtype numpy gives xywhn2xyxy's expression follows from the TYPES the reference held (numpy >= 2: a numpy float64 scalar is
        # not weak): ratio numpy -> 2 (float64 throughout), only pad numpy -> 1 (float64 sum), both Python -> 0 (float32)
        r_np, p_np = (int(v) for v in g[f"types{tag}"])
        mode = gen.label_dtype_mode(ratio[0] * w, dw)
        assert mode == (2 if r_np else p_np), (tag, mode, r_np, p_np)
        modes.add(mode)
        sm = gen.sample(i)
        assert sm["shape"] == (H, W), tag
        seen_hw.add((H, W))
        if gen.augment:
            assert np.allclose(sm["M"][:2], g[f"M{tag}"], rtol=1e-12, atol=0) and np.array_equal(sm["M"][2], [0, 0, 1]), tag
            assert sm["s"] == g[f"s{tag}"][0] and np.array_equal(sm["lut"], g[f"lut{tag}"]), tag
        else:
            assert sm["M"] is None and sm["lut"] is None
        assert [int(sm["flipud"]), int(sm["fliplr"])] == g[f"flips{tag}"].tolist(), tag
        want = g[f"shapes{tag}"]                                                              # h0, w0, h / h0, w / w0, dw, dh
        h0, w0 = (int(v) for v in hw0[i])
        assert [h0, w0, h / h0, w / w0, dw, dh] == want.tolist(), tag
    assert modes == {0, 1, 2} and any(H != W for H, W in seen_hw)
    A, B, V = gens["A"], gens["B"], gens["V"]
    assert A.py_rng is B.py_rng
    assert A.py_rng.random() == float(g["next_random"][0])                                   # both streams are where the reference
    assert A.np_rng.random_sample() == float(g["next_np_random"][0])                         # left them
    fresh = _generators(g)[2]                                                                # augment=False draws nothing
    assert V.py_rng.getstate() == fresh.py_rng.getstate()
    assert all(np.array_equal(a, b) for a, b in zip(V.np_rng.get_state(), fresh.np_rng.get_state()))


# ---- 2. labels against the live reference -----------------------------------------------------------------------------------------------
def _golden_batches(hip, g):
    """every golden batch through the generators -> [(name, tags, (imgs, targets, paths, shapes))]"""
    imgs, labels, hw0 = _golden_dataset(g)
    dimgs = [hip.t(im) for im in imgs]
    A, B, V = _generators(g)
    out = [("A", [f"A{j}" for j in range(len(g["groupA"]))], A(dimgs, labels, [int(i) for i in g["groupA"]], hw0)),
           ("B", [f"B{j}" for j in range(len(g["groupB"]))], B(dimgs, labels, [int(i) for i in g["groupB"]], hw0))]
    for k, idx in enumerate(g["groupV"]):
        out.append((f"V{k}", [f"V{k}_{j}" for j in range(len(idx))], V(dimgs, labels, [int(i) for i in idx], hw0)))
    return out


def test_labels_equal_the_reference(hip):
    """The kernel's collated (n, 6) of the augment batches (A at 32 x 32, B at 32 x 64) and of the three validation batches against the
    reference's collate_fn output.  Survivorship and order are demanded exactly (the golden tool refuses thresholds closer than 1e-6).
    For xywh the bound that can be argued is 2 * 2^-23 (tests/test_labeled_mosaic.py: numpy's BLAS may contract the 3-term fp64 dot
    products of xy @ M.T, which can flip one fp32 rounding of a pixel coordinate).  Measured maximum over the 38 augment and 31 validation
    rows: 0 in the emulator and 0 on an MI355X, so the test demands equality."""
    g = golden("letterbox")
    worst = 0.0
    for name, tags, (imgs, targets, paths, shapes) in _golden_batches(hip, g):
        got, want = targets.cpu().numpy(), g[f"targets{name}"]
        assert got.dtype == np.float32 and got.shape == want.shape, (name, got.shape, want.shape)
        assert np.array_equal(got[:, :2], want[:, :2]), name                                  # img, cls, row order
        d = np.abs(got[:, 2:].astype(np.float64) - want[:, 2:]).max() if len(got) else 0.0
        print(f"labels vs reference, batch {name}: max |xywh difference| = {d:.3e} over {got.shape[0]} rows")
        worst = max(worst, d)
        assert d <= XYWH_TOL, (name, d)
        k = 0                                                                                # and per sample: labels_out, shapes
        for j, tag in enumerate(tags):
            lo = g[f"labels_out{tag}"]
            assert np.array_equal(got[k:k + len(lo), 1:2], lo[:, 1:2]), tag
            k += len(lo)
            (h0, w0), ((rh, rw), (dw, dh)) = shapes[j]
            assert [h0, w0, rh, rw, dw, dh] == g[f"shapes{tag}"].tolist(), tag
        assert k == got.shape[0] and len(paths) == len(tags)
        if name.startswith("V"):                                                             # without has_warp every row survives
            assert got.shape[0] == sum(len(g[f"lab{int(i)}"]) for i in g["groupV"][int(name[1])])
    assert len(g["lab6"]) == 0 and 6 in g["groupA"] and 6 in g["groupB"]                      # an image without labels inside a batch
    assert worst == 0.0, worst                                                              # tightened: see the docstring


def test_an_image_without_labels_and_a_long_image(hip):
    """against the numpy restatement: an image with more rows than one pass of the workgroup (300: the scan carries over) that loses
    rows in both passes, an image without a label between two that have some, every dtype mode, and a batch with no label at all"""
    from efficientteacher_amd import ops
    from efficientteacher_amd.utils.augment import affine_matrix
    H, W = 32, 64
    rng = np.random.default_rng(7)
    pr = random.Random(7)
    n_rows = (300, 0, 40)
    geoms = [(24.0, 32.0, 20.0, 0.0), (np.float64(32.0), np.float64(20.0), np.float64(16.0), np.float64(6.0)),
             (13.0, 32.0, np.float64(25.5), np.float64(0.0))]
    wide = np.array([0, 2, 1], np.int32)
    flags = np.array([[1, 0, 1], [1, 1, 0], [1, 1, 1]], np.int32)
    M = np.zeros((3, 9)); sc = np.zeros(3); rows = np.zeros((3, 2), np.int32)
    labs, want, row = [], [], 0
    for b, n in enumerate(n_rows):
        lb = np.zeros((n, 5), np.float32)
        lb[:, 0] = rng.integers(0, 80, n)
        lb[:, 1:3] = rng.uniform(0.1, 0.9, (n, 2))
        lb[:, 3:5] = rng.uniform(0.02, 0.6, (n, 2))
        Mm, s = affine_matrix(H, W, 10.0, 0.1, 0.5, 2.0, pr)
        M[b], sc[b] = Mm.reshape(-1), s
        rows[b] = (row, row + n); row += n
        labs.append(lb)
        t = lt.labels_of_image(lb, *geoms[b], H, W, Mm, s, flags[b, 1], flags[b, 2])
        want.append(np.concatenate((np.full((len(t), 1), b, np.float32), t), 1))
    want = np.concatenate(want, 0)
    assert 100 < (want[:, 0] == 0).sum() < 256 and (want[:, 0] == 2).any()
    geom = np.array([[float(v) for v in gm] for gm in geoms])
    out, n = ops.letterbox_targets(hip.t(np.concatenate(labs, 0)), rows, hip.t(geom), hip.t(wide), hip.t(M), hip.t(sc), hip.t(flags), H, W)
    n = int(n[0])
    got = out[:n].cpu().numpy()
    assert n == want.shape[0] and np.array_equal(got[:, :2], want[:, :2])
    assert np.abs(got[:, 2:].astype(np.float64) - want[:, 2:]).max() <= XYWH_TOL
    # no warp: every row survives, in order
    flags0 = flags.copy(); flags0[:, 0] = 0
    out, n = ops.letterbox_targets(hip.t(np.concatenate(labs, 0)), rows, hip.t(geom), hip.t(wide), hip.t(M), hip.t(sc), hip.t(flags0), H, W)
    want0 = np.concatenate([np.concatenate((np.full((len(lb), 1), b, np.float32),
                                            lt.labels_of_image(lb, *geoms[b], H, W, None, 1.0, flags[b, 1], flags[b, 2])), 1)
                            for b, lb in enumerate(labs)], 0)
    assert int(n[0]) == row and np.array_equal(out.cpu().numpy(), want0)
    out, n = ops.letterbox_targets(hip.t(np.zeros((0, 5), np.float32)), np.zeros((3, 2), np.int32), hip.t(geom), hip.t(wide), hip.t(M),
                                   hip.t(sc), hip.t(flags), H, W)
    assert out.shape == (0, 6) and int(n[0]) == 0
    with pytest.raises(ValueError):                                                          # overlapping row ranges are refused
        bad = rows.copy(); bad[2, 0] -= 1
        ops.letterbox_targets(hip.t(np.concatenate(labs, 0)), bad, hip.t(geom), hip.t(wide), hip.t(M), hip.t(sc), hip.t(flags), H, W)


# ---- 3. pixels against the numpy restatement -------------------------------------------------------------------------------------------
# name -> (H, W, [(source (h, w), scaleup)] * 3): the smallest sets that reach every path of the kernel
GEOMETRY = {
    # r == 1 everywhere: (32, 24) even pads; (19, 32) top 6 / bottom 7; (32, 13) left 25 / right 26
    "wide_pad": (32, 64, [((32, 24), False), ((19, 32), False), ((32, 13), False)]),
    # (48, 36): r = 0.889, a non-integer ratio and an odd pad; the others r == 1 with top != 0
    "tall": (64, 32, [((32, 24), False), ((20, 32), False), ((48, 36), False)]),
    # r = 2 / 3 (48 x 36 -> 32 x 24); scale-up of a 12 x 9 source by 2.67; the exact 2 : 1
    "square_resize": (32, 32, [((48, 36), False), ((12, 9), True), ((64, 64), False)]),
    # new_unpad one pixel wide, one pixel high, and a source that is itself one pixel wide
    "thin": (32, 32, [((64, 2), False), ((3, 96), False), ((40, 1), False)]),
}


def _pixel_case(name, seed):
    from efficientteacher_amd.utils.augment import affine_matrix, letterbox_geometry
    H, W, srcs = GEOMETRY[name]
    rng = np.random.default_rng(seed)
    pr = random.Random(seed)
    images, geo, minv = [], [], np.zeros((len(srcs), 6))
    for b, ((h, w), scaleup) in enumerate(srcs):
        images.append(rng.integers(0, 256, (3, h, w), dtype=np.uint8))
        _, _, (nw, nh), top, left = letterbox_geometry(h, w, (H, W), scaleup)
        geo.append((nw, nh, left, top))
        M, _ = affine_matrix(H, W, 10.0, 0.1, 0.5, 2.0, pr)                                   # rotation, scale, shear, sub-pixel translation
        minv[b] = lr.invert_affine(M)
    return H, W, images, geo, minv


def _run_pixels(hip, images, geo, minv, lut, flags, H, W):
    from efficientteacher_amd import ops
    return ops.letterbox_u8([hip.t(im) for im in images], geo, hip.t(minv), None if lut is None else hip.t(lut), hip.t(flags), H, W).cpu().numpy()


def _want_pixels(images, geo, minv, lut, flags, H, W):
    return np.stack([lt.letterbox_image(images[b], geo[b], H, W, minv[b] if flags[b, 0] else None, None if lut is None else lut[b],
                                        flags[b, 1], flags[b, 2]) for b in range(len(images))])


def test_the_geometry_sets_reach_every_path():
    from efficientteacher_amd.utils.augment import letterbox_geometry
    seen = set()
    for name, (H, W, srcs) in GEOMETRY.items():
        for (h, w), scaleup in srcs:
            (r, _), _, (nw, nh), top, left = letterbox_geometry(h, w, (H, W), scaleup)
            bottom, right = H - nh - top, W - nw - left
            seen |= {"r1" if (nw, nh) == (w, h) else ("up" if r > 1 else ("half" if (2 * nw, 2 * nh) == (w, h) else "down"))}
            seen |= {"odd_x"} if left != right else set()
            seen |= {"odd_y"} if top != bottom else set()
            seen |= {"nw1"} if nw == 1 and w > 1 else set()
            seen |= {"nh1"} if nh == 1 else set()
            seen |= {"w1"} if w == 1 else set()
    assert seen == {"r1", "up", "half", "down", "odd_x", "odd_y", "nw1", "nh1", "w1"}, seen


@pytest.mark.parametrize("with_lut", [False, True])
@pytest.mark.parametrize("warp", [False, True])
@pytest.mark.parametrize("ud,lr_", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("name", list(GEOMETRY))
def test_pixels_match_the_numpy_restatement(hip, name, ud, lr_, warp, with_lut):
    """B = 3 per geometry set (canvases 32 x 64, 64 x 32, 32 x 32): pads, non-integer down-scaling, scale-up, the exact 2 : 1, one-pixel
    results; the warps rotate, scale and translate by fractions, so taps straddle the image / border seam and leave the canvas"""
    H, W, images, geo, minv = _pixel_case(name, seed=11 + 2 * ud + lr_)
    flags = np.array([[int(warp), ud, lr_]] * 3, np.int32)
    lut = None
    if with_lut:
        from efficientteacher_amd.utils.augment import hsv_luts
        lut = np.stack([hsv_luts(0.015, 0.7, 0.4, np.random.RandomState(s)) for s in (1, 2, 3)])
    got = _run_pixels(hip, images, geo, minv, lut, flags, H, W)
    want = _want_pixels(images, geo, minv, lut, flags, H, W)
    assert got.shape == (3, 3, H, W) and np.array_equal(got, want)
    if not with_lut:
        assert (want == 114).any() and (want != 114).any()


# ---- 4. invariants that need no restatement ----------------------------------------------------------------------------------------------
IDENT = np.tile(np.array([1., 0, 0, 0, 1, 0]), (3, 1))


def test_r_equal_one_is_a_copy_into_the_border(hip):
    H, W, images, geo, _ = _pixel_case("wide_pad", seed=3)
    got = _run_pixels(hip, images, geo, IDENT, None, np.zeros((3, 3), np.int32), H, W)
    for b, (im, (nw, nh, left, top)) in enumerate(zip(images, geo)):
        want = np.full((3, H, W), 114, np.uint8)
        want[:, top:top + im.shape[1], left:left + im.shape[2]] = im
        assert (nw, nh) == (im.shape[2], im.shape[1]) and np.array_equal(got[b], want), b


def test_exact_half_is_the_box_average(hip):
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, (3, 64, 48), dtype=np.uint8), rng.integers(0, 256, (3, 40, 64), dtype=np.uint8),
              rng.integers(0, 256, (3, 64, 64), dtype=np.uint8)]
    geo = [(24, 32, 4, 0), (32, 20, 0, 6), (32, 32, 0, 0)]
    got = _run_pixels(hip, images, geo, IDENT, None, np.zeros((3, 3), np.int32), 32, 32)
    for b, (im, (nw, nh, left, top)) in enumerate(zip(images, geo)):
        p = im.astype(np.int64)
        box = (p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2] + 2) >> 2
        assert np.array_equal(got[b][:, top:top + nh, left:left + nw], box), b
        assert np.array_equal(lt.resize(im, nw, nh), box)                                    # the restatement has the invariant too


@pytest.mark.parametrize("name", ["tall", "square_resize"])
def test_identity_warp_equals_no_warp_and_strong_view_agrees(hip, name):
    """has_warp with the identity map is the no-warp output; and on the canvas the no-warp path materialises, strong_view_u8 (no
    cutouts, same minv / LUT / flips) gives what the warp path samples from the virtual canvas"""
    from efficientteacher_amd import ops
    from efficientteacher_amd.utils.augment import hsv_luts
    H, W, images, geo, minv = _pixel_case(name, seed=21)
    plain = np.zeros((3, 3), np.int32)
    canvas = _run_pixels(hip, images, geo, IDENT, None, plain, H, W)
    ident = plain.copy(); ident[:, 0] = 1
    assert np.array_equal(_run_pixels(hip, images, geo, IDENT, None, ident, H, W), canvas)
    lut = np.stack([hsv_luts(0.015, 0.7, 0.4, np.random.RandomState(s)) for s in (4, 5, 6)])
    flags = np.array([[1, 0, 1], [1, 1, 0], [1, 1, 1]], np.int32)
    got = _run_pixels(hip, images, geo, minv, lut, flags, H, W)
    sflags = flags.copy(); sflags[:, 0] = 0                                                  # strong_view's first flag: the cutout count
    strong = ops.strong_view_u8(hip.t(canvas), hip.t(minv), hip.t(lut), hip.t(np.zeros((3, 32, 7), np.int32)), hip.t(sflags)).cpu().numpy()
    assert np.array_equal(got, strong)


def test_pixels_equal_the_golden_run(hip):
    """ORACLE-DERIVED pixels: the reference's control flow (letterbox, random_perspective_keypoints, augment_hsv, the flips) around the
    numpy restatements"""
    g = golden("letterbox")
    for name, tags, (imgs, _, _, _) in _golden_batches(hip, g):
        out = imgs.cpu().numpy()
        for j, tag in enumerate(tags):
            assert np.array_equal(out[j], g[f"out{tag}"]), tag


# ---- 5. rect shapes (host) ---------------------------------------------------------------------------------------------------------------
def test_rect_batch_shapes():
    """utils/datasets.py:747-749, 772-795 by hand.  (w, h) -> ar = h / w:
        0 (100, 200) 2.0   1 (200, 100) 0.5   2 (100, 100) 1.0   3 (200, 80) 0.4   4 (80, 100) 1.25
        5 (100, 60) 0.6    6 (100, 150) 1.5   7 (200, 150) 0.75  8 (100, 80) 0.8
    ar.argsort(): 0.4, 0.5, 0.6, 0.75 | 0.8, 1.0, 1.25, 1.5 | 2.0 = images 3, 1, 5, 7 | 8, 2, 4, 6 | 0; bi = floor(arange(9) / 4).
    batch 0: every ar < 1, maxi 0.75 -> [0.75, 1]; ceil([0.75, 1] * 64 / 32 + 0.5) = ceil([2.0, 2.5]) = [2, 3] -> (64, 96)
    batch 1: mini 0.8 < 1 < maxi 1.5, mixed -> [1, 1]; ceil(2.5) = 3 -> (96, 96)
    batch 2: every ar > 1, mini 2.0 -> [1, 1 / 2]; ceil([2.5, 1.5]) = [3, 2] -> (96, 64)"""
    from efficientteacher_amd.utils.augment import LetterboxBatchGenerator, rect_batch_shapes
    wh = [(100, 200), (200, 100), (100, 100), (200, 80), (80, 100), (100, 60), (100, 150), (200, 150), (100, 80)]
    order, bi, shapes = rect_batch_shapes(wh, batch_size=4, img_size=64, stride=32, pad=0.5)
    assert order.tolist() == [3, 1, 5, 7, 8, 2, 4, 6, 0]
    assert bi.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2]
    assert shapes.tolist() == [[64, 96], [96, 96], [96, 64]]
    gen = LetterboxBatchGenerator(_cfg(64), 9, rect=True, batch_size=4, stride=32, pad=0.5, shapes_wh=wh)
    assert gen.rect_batches == [[0, 1, 2, 3], [4, 5, 6, 7], [8]] and gen.sample(8)["shape"] == (96, 64)
    assert not isinstance(gen.new_shape(0)[0], int)                                          # numpy ints, as the reference holds them


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_bad_tables_are_refused_before_the_launch(hip, monkeypatch):
    from efficientteacher_amd import _lib, ops
    im = hip.t(np.zeros((3, 8, 8), np.uint8))
    minv, flags = hip.t(IDENT[:1].copy()), hip.t(np.zeros((1, 3), np.int32))
    launched = []
    real = _lib.load

    class Spy:
        def __getattr__(self, k):
            launched.append(k)
            return getattr(real(), k)
    monkeypatch.setattr(_lib, "load", lambda: Spy())
    for geo, H, W in (((8, 8, 10, 0), 16, 16),            # left + nw > W
                      ((8, 8, 0, 9), 16, 16),             # top + nh > H
                      ((8, 8, 0, 0), 16, 18),             # W % 4 != 0
                      ((0, 8, 0, 0), 16, 16),             # nw == 0
                      ((8, 8, -1, 0), 16, 16)):           # a negative border
        with pytest.raises(ValueError):
            ops.letterbox_u8([im], [geo], minv, None, flags, H, W)
    assert launched == []
    assert ops.letterbox_u8([im], [(8, 8, 4, 4)], minv, None, flags, 16, 16).shape == (1, 3, 16, 16) and launched == ["et_letterbox_u8"]


@pytest.mark.parametrize("kw", [dict(hyp=dict(perspective=0.001)), dict(dataset=dict(np=4)), dict(dataset=dict(num_ids=10)),
                                dict(gen=dict(image_weights=True)), dict(gen=dict(albumentations=True))])
def test_unsupported_settings_are_refused(kw):
    from efficientteacher_amd.utils.augment import LetterboxBatchGenerator
    with pytest.raises(NotImplementedError) as e:
        LetterboxBatchGenerator(_cfg(32, kw.get("dataset"), **kw.get("hyp", {})), n=6, seed=0, **kw.get("gen", {}))
    assert "LetterboxBatchGenerator" in str(e.value)


def test_an_open_mosaic_is_refused_after_its_gate_draw():
    """self.mosaic = True draws the gate as the reference does; an image the gate sends to the mosaic branch is not this class's"""
    from efficientteacher_amd.utils.augment import LetterboxBatchGenerator
    gen = LetterboxBatchGenerator(_cfg(32, mosaic=0.0), n=6, seed=0, augment=True)
    gen.mosaic = True
    gen.sample(0)                                                                            # hyp.mosaic = 0: the gate never opens
    twin = random.Random(0)
    for _ in range(11):                                                                      # the gate, eight matrix draws, two flips
        twin.random()
    assert gen.py_rng.random() == twin.random()
    closed = LetterboxBatchGenerator(_cfg(32, mosaic=0.0), n=6, seed=0, augment=True)
    closed.sample(0)                                                                         # closed mosaic: no gate draw (`and` short-circuits)
    twin = random.Random(0)
    for _ in range(10):
        twin.random()
    assert closed.py_rng.random() == twin.random()
    gen.hyp.mosaic = 1.0
    with pytest.raises(NotImplementedError):
        gen.sample(0)


# ---- 7. end to end (gpu only) ------------------------------------------------------------------------------------------------------------
def _val_dataset(S):
    """twelve images of mixed aspect whose long side is S (what load_image leaves), their original sizes and labels"""
    rng = np.random.default_rng(4)
    hw = [(S, 40), (36, S), (S, S), (30, S), (S, 27), (56, S), (S, 52), (24, S), (S, 33), (48, S), (S, 60), (44, S)]
    hw0 = [(2 * h, 2 * w) if k % 2 else (h, w) for k, (h, w) in enumerate(hw)]
    imgs = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in hw]
    labels = []
    for _ in hw:
        n = int(rng.integers(2, 6))
        lb = np.zeros((n, 5), np.float32)
        lb[:, 0] = rng.integers(0, 80, n)
        lb[:, 1:3] = rng.uniform(0.3, 0.7, (n, 2))
        lb[:, 3:5] = rng.uniform(0.2, 0.5, (n, 2))
        labels.append(lb)
    return imgs, labels, hw0


def _trainer(dev):
    import os
    from efficientteacher_amd.configs import get_cfg
    from efficientteacher_amd.trainer import Trainer
    from tests.conftest import ROOT
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "efficientteacher_amd", "configs", "sup", "public", "yolov5s_coco.yaml"))
    cfg.merge_from_list(["Model.width_multiple", 0.125, "Model.depth_multiple", 0.33, "Dataset.batch_size", 2, "Dataset.img_size", 64])
    cfg.freeze()
    torch.manual_seed(0)
    t = Trainer(cfg, dev, nb=1000)
    t.model.set_compute_dtype(torch.float32)
    t.build_optimizer(cfg)
    return t


@pytest.mark.gpu
def test_val_run_over_the_generators_rect_batches():
    """val.run over LetterboxBatchGenerator(...).batches(...) -- twelve images, three rect batches of four -- returns the metrics of
    val.run over the same batches built on the host by tests/letterbox_ref.py and uploaded: pixels and labels are equal, so equality"""
    from copy import deepcopy
    from efficientteacher_amd import _lib, val
    from efficientteacher_amd.utils.augment import LetterboxBatchGenerator, letterbox_geometry
    assert torch.cuda.is_available(), "-m gpu selected but no GPU is visible"
    _lib._use_library_for_tests(None, False)
    dev = torch.device("cuda:0")
    S = 64
    imgs, labels, hw0 = _val_dataset(S)
    gen = LetterboxBatchGenerator(_cfg(S), len(imgs), augment=False, rect=True, batch_size=4, stride=32, pad=0.5,
                                  shapes_wh=[(w, h) for h, w in hw0])
    assert len(gen.rect_batches) == 3 and len({tuple(s) for s in gen.batch_shapes.tolist()}) > 1

    def geometry(pos):
        i = int(gen.order[pos])
        h, w = imgs[i].shape[1:]
        return (i, h, w) + letterbox_geometry(h, w, gen.new_shape(pos), scaleup=False)

    def host_batches(labels):
        out = []
        for idx in gen.rect_batches:
            H, W = (int(v) for v in gen.new_shape(idx[0]))
            ims, rows, shapes = [], [], []
            for j, pos in enumerate(idx):
                i, h, w, ratio, (dw, dh), (nw, nh), top, left = geometry(pos)
                ims.append(lt.letterbox_image(imgs[i], (nw, nh, left, top), H, W, None, None, False, False))
                t = lt.labels_of_image(labels[i], ratio[0] * w, ratio[1] * h, dw, dh, H, W, None, 1.0, False, False)
                rows.append(np.concatenate((np.full((len(t), 1), j, np.float32), t), 1))
                shapes.append((hw0[i], ((h / hw0[i][0], w / hw0[i][1]), (dw, dh))))
            out.append((torch.from_numpy(np.stack(ims)).to(dev), torch.from_numpy(np.concatenate(rows, 0)).to(dev),
                        tuple(int(gen.order[p]) for p in idx), tuple(shapes)))
        return out
    t = _trainer(dev)
    with torch.no_grad():
        for mi in t.model.head.m:                                                             # confidences above val's filter
            mi.bias.view(t.model.head.na, -1)[:, 4] += 4.0
    t.model.flat_state().mark_weights_changed()
    # labels the untrained model can find: its own three most confident detections per image, carried back to the source image's
    # normalised xywh (the inverse of xywhn2xyxy), so that the metrics that must be equal are not all zero
    found = [None] * len(imgs)
    for idx, (x, _, _, _) in zip(gen.rect_batches, host_batches(labels)):
        dets, _ = val.infer_batch(deepcopy(t.model), x, 0.001, 0.6, half=False)
        for j, pos in enumerate(idx):
            i, h, w, ratio, (dw, dh), _, _, _ = geometry(pos)
            d = dets[j][:3].cpu().numpy().astype(np.float64)
            xy = np.stack((((d[:, 0] + d[:, 2]) / 2 - dw) / (ratio[0] * w), ((d[:, 1] + d[:, 3]) / 2 - dh) / (ratio[1] * h),
                           (d[:, 2] - d[:, 0]) / (ratio[0] * w), (d[:, 3] - d[:, 1]) / (ratio[1] * h)), 1)
            found[i] = np.concatenate((d[:, 5:6], np.clip(xy, 0.0, 1.0)), 1).astype(np.float32)
    assert sum(len(f) for f in found) >= 24
    host = host_batches(found)
    ours = list(gen.batches([torch.from_numpy(im).to(dev) for im in imgs], found, hw0=hw0))
    assert len(ours) == 3
    for (a, b, _, sa), (c, d, _, sb) in zip(ours, host):
        assert torch.equal(a, c) and torch.equal(b, d) and sa == sb
    r_dev = val.run(deepcopy(t.model), ours, conf_thres=0.001, half=False, nc=80)
    r_host = val.run(deepcopy(t.model), host, conf_thres=0.001, half=False, nc=80)
    assert r_dev[0][:4] == r_host[0][:4] and np.array_equal(r_dev[1], r_host[1]), (r_dev[0], r_host[0])
    assert all(np.isfinite(v) for v in r_dev[0][:4]) and r_dev[0][2] > 0, r_dev[0]           # map50 > 0: the labels were found


@pytest.mark.gpu
def test_trainer_step_on_the_closed_mosaic_batch():
    """one Trainer step fed by the augment=True form (the closed mosaic of no_aug_epochs) on a side stream: the loss is finite and
    BIT-equal to the same step fed the same batch from host tensors"""
    from efficientteacher_amd import _lib
    from efficientteacher_amd.utils.augment import LetterboxBatchGenerator
    assert torch.cuda.is_available(), "-m gpu selected but no GPU is visible"
    _lib._use_library_for_tests(None, False)
    dev = torch.device("cuda:0")
    S = 64
    imgs, labels, hw0 = _val_dataset(S)
    gen = LetterboxBatchGenerator(_cfg(S), len(imgs), seed=3, stream=torch.cuda.Stream(device=dev), augment=True)
    batches = list(gen.batches([torch.from_numpy(im).to(dev) for im in imgs], labels, [[0, 3], [5, 2]], hw0=hw0))
    assert len(batches) == 2
    x, targets, _, shapes = batches[1]
    assert x.shape == (2, 3, S, S) and targets.shape[0] > 0 and shapes[0][0] == hw0[5]
    a = _trainer(dev).train_step(x, targets, 5)
    b = _trainer(dev).train_step(x.cpu(), targets.cpu(), 5)
    la, lb = float(a["loss"].detach()), float(b["loss"].detach())
    assert np.isfinite(la) and la == lb, (la, lb)
