"""Labeled batches on the device (csrc/augment.hip et_labeled_mosaic_u8 / et_labeled_mosaic_targets, utils/augment.py
LabeledBatchGenerator; reference utils/datasets.py:889-1043 LoadImagesAndLabels.__getitem__, mosaic branch).

tests/golden/labeled_mosaic.npz comes from the LIVE reference (tools/make_labeled_golden.py): its own __getitem__ and collate_fn on a
six-image in-memory dataset, six samples from one seeded pair of random streams.  PINNED on it: the consumption of `random` and
`np.random`, tile choice and placement (the canvases), M, s, the mixup ratio, the LUTs, the flips and all label arithmetic.  cv2 is not
installed, so the golden's PIXELS (`out{j}`) are ORACLE-DERIVED: the reference's control flow around the numpy restatement of OpenCV's
published fixed-point warp and 8-bit HSV round trip (tests/labeled_mosaic_ref.py); the kernel is held to that restatement, to the
existing strong-view kernel and to invariants, not to cv2."""
import random
import types

import numpy as np
import pytest
import torch

from tests import labeled_mosaic_ref as lr
from tests.conftest import golden

HYP = dict(mosaic=1.0, mixup=0.5, copy_paste=0.0, degrees=10.0, translate=0.1, scale=0.9, shear=2.0, perspective=0.0,
           hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, flipud=0.5, fliplr=0.5)
XYWH_TOL = 2 * 2.0 ** -23


def _cfg(S=32, dataset=None, **hyp):
    return types.SimpleNamespace(hyp=types.SimpleNamespace(**{**HYP, **hyp}),
                                 Dataset=types.SimpleNamespace(**{**dict(img_size=S, np=0, num_ids=0), **(dataset or {})}))


def _golden_dataset(g):
    imgs, labels = [], []
    k = 0
    while f"img{k}" in g.files:
        imgs.append(np.ascontiguousarray(g[f"img{k}"][:, :, ::-1].transpose(2, 0, 1)))      # BGR HWC -> RGB planes
        labels.append(g[f"lab{k}"]); k += 1
    return imgs, labels


def _generator(g, **kw):
    from efficientteacher_amd.utils.augment import LabeledBatchGenerator
    return LabeledBatchGenerator(_cfg(int(g["S"][0])), n=len(_golden_dataset(g)[0]), seed=int(g["seed"][0]), **kw)


# ---- 1. the host recipe against the live reference ---------------------------------------------------------------------------------------
def test_recipe_equals_the_reference():
    from efficientteacher_amd.utils.augment import mosaic_layout
    g = golden("labeled_mosaic")
    S = int(g["S"][0])
    imgs, _ = _golden_dataset(g)
    gen = _generator(g)
    n_mix = 0
    for j, index in enumerate(g["index"]):
        sm = gen.sample(int(index))
        assert len(sm["mosaics"]) == g[f"M{j}"].shape[0], j
        n_mix += len(sm["mosaics"]) - 1
        for m, (yc, xc, four, M, s) in enumerate(sm["mosaics"]):
            tiles = [imgs[i] for i in four]
            layout = mosaic_layout(S, yc, xc, [t.shape[1:] for t in tiles])
            want = g[f"canvas{j}_{m}"][:, :, ::-1].transpose(2, 0, 1)                        # the reference's own canvas
            assert np.array_equal(lr.paste_canvas(S, tiles, layout), want), (j, m)
            assert np.allclose(M[:2], g[f"M{j}"][m], rtol=1e-12, atol=0), (j, m)
            assert np.array_equal(M[2], [0, 0, 1]) and s == g[f"s{j}"][m]
        assert (sm["r"] is None) == (g[f"r{j}"].size == 0) and (sm["r"] is None or sm["r"] == g[f"r{j}"][0])
        assert np.array_equal(sm["lut"], g[f"lut{j}"]), j
        assert [int(sm["flipud"]), int(sm["fliplr"])] == g[f"flips{j}"].tolist(), j
    assert n_mix >= 2
    assert gen.py_rng.random() == float(g["next_random"][0])                                 # both streams are where the reference
    assert gen.np_rng.random_sample() == float(g["next_np_random"][0])                       # left them


# ---- 2. labels ---------------------------------------------------------------------------------------------------------------------------
def _golden_batch(hip, g, **kw):
    imgs, labels = _golden_dataset(g)
    gen = _generator(g, **kw)
    return gen([hip.t(im) for im in imgs], labels, [int(i) for i in g["index"]])


def test_labels_equal_the_reference(hip):
    """The kernel's collated (n, 6) against the reference's collate_fn output.  Survivorship and order are demanded exactly (the golden
    tool refuses thresholds closer than 1e-6).  For xywh the bound that can be argued is 2 * 2^-23: numpy's BLAS may contract the
    3-term fp64 dot products of xy @ M.T, which can flip one fp32 rounding of a pixel coordinate <= S -- <= 2^-23 after the division
    by S, doubled for the centre / extent arithmetic behind it.  Measured maximum over the 83 rows: 0 in the emulator and 0 on an
    MI355X, so the test demands equality."""
    g = golden("labeled_mosaic")
    _, targets, paths, shapes = _golden_batch(hip, g)
    got, want = targets.cpu().numpy(), g["targets"]
    assert got.dtype == np.float32 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got[:, :2], want[:, :2])                                           # img, cls, row order
    d = np.abs(got[:, 2:].astype(np.float64) - want[:, 2:]).max()
    print(f"labels vs reference: max |xywh difference| = {d:.3e} over {got.shape[0]} rows")
    assert np.array_equal(got, want), d
    assert shapes == (None,) * len(g["index"]) and len(paths) == len(g["index"])
    k = 0                                                                                    # and per sample: labels_out
    for j in range(len(g["index"])):
        lo = g[f"labels_out{j}"]
        assert np.array_equal(got[k:k + len(lo), 1:], lo[:, 1:]), j
        k += len(lo)
    assert k == got.shape[0]


def _label_case(rng, S, n_rows, scales, mix):
    """B images with hand-made mosaics -> (labels (L,5), table (B,2,4,6), M (B,2,9), s (B,2), flags (B,3), numpy rows [img, cls, xywh])"""
    from efficientteacher_amd.utils.augment import affine_matrix, mosaic_layout
    B = len(n_rows)
    pr = random.Random(int(rng.integers(1 << 30)))
    table = np.zeros((B, 2, 4, 6), np.int32); M = np.tile(np.eye(3).reshape(9), (B, 2, 1)); sc = np.ones((B, 2))
    flags = np.zeros((B, 3), np.int32)
    rows, want, row = [], [], 0
    for b in range(B):
        flags[b] = (mix[b], b % 2, (b // 2) % 2)
        mos = []
        for m in range(2):
            if m == 1 and not mix[b]:
                table[b, m, :, :2] = row
                continue
            shapes = [(int(rng.integers(S // 2, S + 1)), int(rng.integers(S // 2, S + 1))) for _ in range(4)]
            layout = mosaic_layout(S, int(rng.integers(S // 2, 3 * S // 2)), int(rng.integers(S // 2, 3 * S // 2)), shapes)
            Mm, _ = affine_matrix(2 * S, 2 * S, 10.0, 0.1, 0.0, 2.0, pr, out_hw=(S, S))
            s = scales[b]
            Mm = Mm @ np.diag([s, s, 1.0])                                                    # shrink about the canvas origin
            labs = []
            for k in range(4):
                n = n_rows[b] if (m == 0 and k == 1) else int(rng.integers(0, 4))
                lb = np.zeros((n, 5), np.float32)
                lb[:, 0] = rng.integers(0, 80, n)
                lb[:, 1:3] = rng.uniform(0.1, 0.9, (n, 2))
                lb[:, 3:5] = rng.uniform(0.02, 0.6, (n, 2))
                table[b, m, k] = (row, row + n, shapes[k][0], shapes[k][1], layout[k][6], layout[k][7])
                row += n
                labs.append(lb); rows.append(lb)
            M[b, m], sc[b, m] = Mm.reshape(-1), s
            mos.append((labs, shapes, layout, Mm, s))
        lab = lr.labels_of_image(S, mos, flags[b, 1], flags[b, 2])
        want.append(np.concatenate((np.full((len(lab), 1), b, np.float32), lab), 1))
    labels = np.concatenate(rows, 0) if rows else np.zeros((0, 5), np.float32)
    return labels, table, M, sc, flags, np.concatenate(want, 0)


def test_labels_scan_empty_image_and_no_labels(hip):
    """against the numpy restatement of the reference's arithmetic: an image with more rows than one pass of the workgroup (300 in one
    tile: the scan carries over), an image that loses ALL its labels (scale 0.02: every box falls under 2 pixels) between two that keep
    some, and a batch with no label at all (L_in = 0)"""
    from efficientteacher_amd import ops
    S = 64
    rng = np.random.default_rng(7)
    labels, table, M, sc, flags, want = _label_case(rng, S, n_rows=(300, 5, 40), scales=(1.0, 0.02, 0.7), mix=(1, 1, 0))
    assert table[0, 1, 3, 1] - table[0, 0, 0, 0] > 256 and 100 < (want[:, 0] == 0).sum() < 256       # image 0: two passes, rows dropped in both
    assert not (want[:, 0] == 1).any() and (want[:, 0] == 2).any()
    out, n = ops.labeled_mosaic_targets(hip.t(labels), table, hip.t(M), hip.t(sc), hip.t(flags), S)
    n = int(n[0])
    got = out[:n].cpu().numpy()
    assert n == want.shape[0] and np.array_equal(got[:, :2], want[:, :2])
    assert np.abs(got[:, 2:].astype(np.float64) - want[:, 2:]).max() <= XYWH_TOL
    empty = np.zeros((3, 2, 4, 6), np.int32)
    empty[..., 2:4] = 8
    out, n = ops.labeled_mosaic_targets(hip.t(np.zeros((0, 5), np.float32)), empty, hip.t(M), hip.t(sc), hip.t(flags), S)
    assert out.shape == (0, 6) and int(n[0]) == 0
    with pytest.raises(ValueError):                                                          # a table whose ranges overlap is refused
        bad = table.copy(); bad[1, 0, 0, 0] -= 1
        ops.labeled_mosaic_targets(hip.t(labels), bad, hip.t(M), hip.t(sc), hip.t(flags), S)


def test_generator_with_unlabeled_images(hip):
    """a dataset without a single label: the batch tuple still has its (0, 6) targets"""
    g = golden("labeled_mosaic")
    imgs, labels = _golden_dataset(g)
    gen = _generator(g)
    out, targets, _, _ = gen([hip.t(im) for im in imgs], [np.zeros((0, 5), np.float32)] * len(imgs), [1, 4])
    assert out.shape == (2, 3, 32, 32) and targets.shape == (0, 6) and targets.dtype == torch.float32


# ---- 3. pixels against the numpy restatement -------------------------------------------------------------------------------------------
def _pixel_case(S, seed, partner=(True, False, True), centres=((8, 24), (23, 9), (16, 16))):
    from efficientteacher_amd.utils.augment import affine_matrix, mosaic_layout
    rng = np.random.default_rng(seed)
    pr = random.Random(seed)
    tiles, layouts, minv = [], [], np.tile(np.array([1., 0, 0, 0, 1, 0]), (len(centres), 2, 1))
    for b, (yc, xc) in enumerate(centres):
        tb, lb = [None, None], [None, None]
        for m in range(1 + partner[b]):
            shapes = [(int(rng.integers(3, S + 1)), int(rng.integers(3, S + 1))) for _ in range(4)]
            tb[m] = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in shapes]
            lb[m] = mosaic_layout(S, yc * S // 16, xc * S // 16, shapes)
            M, _ = affine_matrix(2 * S, 2 * S, 10.0, 0.1, 0.5, 2.0, pr, out_hw=(S, S))      # rotation, shear, sub-pixel translation
            minv[b, m] = lr.invert_affine(M)
        tiles.append(tb); layouts.append(lb)
    return tiles, layouts, minv


def _run_pixels(hip, tiles, layouts, minv, mix, lut, flags, S):
    from efficientteacher_amd import ops
    dt = [[None if m is None else [hip.t(t) for t in m] for m in tb] for tb in tiles]
    return ops.labeled_mosaic_u8(dt, layouts, hip.t(minv), hip.t(mix), None if lut is None else hip.t(lut), hip.t(flags), S).cpu().numpy()


def _want_pixels(S, tiles, layouts, minv, mix, lut, flags):
    out = []
    for b in range(len(tiles)):
        mos = [(tiles[b][m], layouts[b][m], minv[b, m]) for m in range(1 + int(flags[b, 0]))]
        out.append(lr.labeled_image(S, mos, mix[b], None if lut is None else lut[b], flags[b, 1], flags[b, 2]))
    return np.stack(out)


@pytest.mark.parametrize("with_lut", [False, True])
@pytest.mark.parametrize("ud,lr_", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_pixels_match_the_numpy_restatement(hip, ud, lr_, with_lut):
    """B = 3, S = 16, tiles of 3..16 pixels (odd ones included) around centres that clip them and leave canvas uncovered; taps straddle
    the tile seams and leave the canvas; images 0 and 2 are blended with a partner at r = 0.37, image 1 is not"""
    S = 16
    tiles, layouts, minv = _pixel_case(S, seed=11 + 2 * ud + lr_)
    mix = np.full(3, 0.37)
    flags = np.array([[1, ud, lr_], [0, ud, lr_], [1, ud, lr_]], np.int32)
    lut = None
    if with_lut:
        from efficientteacher_amd.utils.augment import hsv_luts
        lut = np.stack([hsv_luts(0.015, 0.7, 0.4, np.random.RandomState(s)) for s in (1, 2, 3)])
    got = _run_pixels(hip, tiles, layouts, minv, mix, lut, flags, S)
    want = _want_pixels(S, tiles, layouts, minv, mix, lut, flags)
    assert got.shape == (3, 3, S, S) and np.array_equal(got, want)
    assert (want == 114).any() and (want != 114).any()


def test_pixels_when_the_size_is_no_multiple_of_four(hip):
    """S = 18: the last group of a row holds two pixels and the planes are written byte by byte"""
    S = 18
    tiles, layouts, minv = _pixel_case(S, seed=5)
    mix = np.full(3, 0.37)
    flags = np.array([[1, 0, 1], [0, 1, 0], [1, 1, 1]], np.int32)
    got = _run_pixels(hip, tiles, layouts, minv, mix, None, flags, S)
    assert np.array_equal(got, _want_pixels(S, tiles, layouts, minv, mix, None, flags))


def test_a_rectangle_outside_its_tile_is_refused(hip):
    from efficientteacher_amd import ops
    S = 16
    tiles, layouts, minv = _pixel_case(S, seed=5, partner=(False,), centres=((16, 16),))
    row = list(layouts[0][0][3]); row[2] += 40                                                # x2a beyond the tile and the canvas
    layouts[0][0][3] = tuple(row)
    with pytest.raises(ValueError):
        ops.labeled_tile_table([[[hip.t(t) for t in tiles[0][0]], None]], layouts, S)


# ---- 4. invariants that need no restatement ----------------------------------------------------------------------------------------------
def _full_canvas(S, rng):
    """four S x S tiles around the centre (S, S): the canvas is covered completely"""
    from efficientteacher_amd.utils.augment import mosaic_layout
    tiles = [rng.integers(0, 256, (3, S, S), dtype=np.uint8) for _ in range(4)]
    layout = mosaic_layout(S, S, S, [(S, S)] * 4)
    return tiles, layout, lr.paste_canvas(S, tiles, layout)


def test_integer_translation_is_the_canvas_crop_and_mixup_truncates(hip):
    S = 16
    rng = np.random.default_rng(3)
    ta, la, ca = _full_canvas(S, rng)
    tb, lb, cb = _full_canvas(S, rng)
    # forward map x' = x - 5, y' = y - 9 (angle 0, scale 1): the output is canvas[9:9 + S, 5:5 + S], exactly
    minv = np.array([[[1., 0, 5, 0, 1, 9], [1., 0, 11, 0, 1, 2]]])
    flags = np.array([[0, 0, 0]], np.int32)
    got = _run_pixels(hip, [[ta, tb]], [[la, lb]], minv, np.ones(1), None, flags, S)
    assert np.array_equal(got[0], ca[:, 9:9 + S, 5:5 + S])
    # the blend is truncated, not rounded: with r = 0.37 the two differ on many pixels
    r = 0.37
    a, b = ca[:, 9:9 + S, 5:5 + S].astype(np.float64), cb[:, 2:2 + S, 11:11 + S].astype(np.float64)
    trunc, rounded = np.floor(a * r + b * (1 - r)), np.rint(a * r + b * (1 - r))
    assert (trunc != rounded).sum() > 100
    flags[0, 0] = 1
    got = _run_pixels(hip, [[ta, tb]], [[la, lb]], minv, np.full(1, r), None, flags, S)
    assert np.array_equal(got[0], trunc.astype(np.uint8))
    # a translation that leaves the canvas: what it does not cover is the border value
    minv[0, 0] = [1, 0, -3, 0, 1, 2 * S - 4]
    flags[0, 0] = 0
    got = _run_pixels(hip, [[ta, tb]], [[la, lb]], minv, np.ones(1), None, flags, S)
    want = np.full((3, S, S), 114, np.uint8)
    want[:, :4, 3:] = ca[:, 2 * S - 4:, :S - 3]
    assert np.array_equal(got[0], want)


# ---- 5. agreement with the existing kernel -----------------------------------------------------------------------------------------------
def test_agrees_with_strong_view_on_the_materialised_canvas(hip):
    """no mixup, no LUT, no flips: strong_view_u8 warps the 2S x 2S canvas to 2S x 2S; its top-left S x S is the labeled kernel's output"""
    from efficientteacher_amd import ops
    S = 16
    tiles, layouts, minv = _pixel_case(S, seed=21, partner=(False, False, False))
    flags = np.zeros((3, 3), np.int32)
    got = _run_pixels(hip, tiles, layouts, minv, np.ones(3), None, flags, S)
    canvas = np.stack([lr.paste_canvas(S, tiles[b][0], layouts[b][0]) for b in range(3)])
    strong = ops.strong_view_u8(hip.t(canvas), hip.t(np.ascontiguousarray(minv[:, 0])), None, hip.t(np.zeros((3, 32, 7), np.int32)),
                                hip.t(flags)).cpu().numpy()
    assert np.array_equal(got, strong[..., :S, :S])


# ---- 6. the golden's pixels (ORACLE-DERIVED) ---------------------------------------------------------------------------------------------
def test_pixels_equal_the_golden_run(hip):
    g = golden("labeled_mosaic")
    out, _, _, _ = _golden_batch(hip, g)
    out = out.cpu().numpy()
    for j in range(len(g["index"])):
        assert np.array_equal(out[j], g[f"out{j}"]), j


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(hyp=dict(perspective=0.001)), dict(hyp=dict(copy_paste=0.1)), dict(dataset=dict(np=4)),
                                dict(dataset=dict(num_ids=10)), dict(gen=dict(rect=True)), dict(gen=dict(image_weights=True)),
                                dict(hyp=dict(mosaic=0.5))])
def test_unsupported_settings_are_refused(kw):
    from efficientteacher_amd.utils.augment import LabeledBatchGenerator
    with pytest.raises(NotImplementedError) as e:
        LabeledBatchGenerator(_cfg(32, kw.get("dataset"), **kw.get("hyp", {})), n=6, seed=0, **kw.get("gen", {}))
    assert "LabeledBatchGenerator" in str(e.value)


def test_closed_mosaic_is_refused():
    from efficientteacher_amd.utils.augment import LabeledBatchGenerator
    gen = LabeledBatchGenerator(_cfg(32), n=6, seed=0)
    gen.sample(0)
    gen.mosaic = False                                                                       # what the trainer does for no_aug_epochs
    with pytest.raises(NotImplementedError):
        gen.sample(0)


# ---- 8. one training step fed by the generator (gpu only) --------------------------------------------------------------------------------
def _step_dataset(S):
    rng = np.random.default_rng(4)
    shapes = [(S, 48), (40, S), (S, S), (33, S), (S, 27), (56, S)]
    imgs = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for h, w in shapes]
    labels = []
    for _ in shapes:
        n = int(rng.integers(2, 6))
        lb = np.zeros((n, 5), np.float32)
        lb[:, 0] = rng.integers(0, 80, n)
        lb[:, 1:3] = rng.uniform(0.3, 0.7, (n, 2))
        lb[:, 3:5] = rng.uniform(0.3, 0.6, (n, 2))
        labels.append(lb)
    return imgs, labels


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


def _step_losses(dev, side_stream):
    """-> (loss of a step fed the generator's device batch, loss of the same step on an equal trainer fed host copies, targets rows)"""
    from efficientteacher_amd.utils.augment import LabeledBatchGenerator
    S = 64
    imgs, labels = _step_dataset(S)
    stream = torch.cuda.Stream(device=dev) if side_stream else None
    gen = LabeledBatchGenerator(_cfg(S, mixup=1.0), n=len(imgs), seed=3, stream=stream)
    batches = list(gen.batches([torch.from_numpy(im).to(dev) for im in imgs], labels, [[0, 3], [5, 2]]))
    assert len(batches) == 2
    x, targets, _, _ = batches[1]
    if side_stream:
        assert gen.stream is stream
    a = _trainer(dev).train_step(x, targets, 5)
    b = _trainer(dev).train_step(x.cpu(), targets.cpu(), 5)
    return float(a["loss"].detach()), float(b["loss"].detach()), int(targets.shape[0])


@pytest.mark.gpu
@pytest.mark.parametrize("side_stream", [False, True])
def test_trainer_step_on_the_generators_batch(side_stream):
    """Trainer.train_step takes the generator's device batch as it is: the loss is finite and BIT-equal to the same step fed the same
    batch from host tensors; second case: the generator works on a side stream and the batch is handed over through its event"""
    from efficientteacher_amd import _lib
    assert torch.cuda.is_available(), "-m gpu selected but no GPU is visible"
    _lib._use_library_for_tests(None, False)
    la, lb, n = _step_losses(torch.device("cuda:0"), side_stream)
    assert n > 0 and np.isfinite(la) and la == lb, (la, lb, n)
