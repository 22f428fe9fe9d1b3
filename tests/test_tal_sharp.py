"""csrc/tal.hip against tests/tal_ref.py (the derivation of every bound is that module's docstring): the TaskAlignedAssigner with its
decisions exact and its scores per element, ComputeTalLoss with four outputs and both gradients per element, the pseudo-label split /
merge and the padded target table bit for bit.  Each case runs on the emulator and on the GPU; all operands come from fixed seeds.
The worst error / bound per (tier, path, output) and the excluded decisions per case are printed at the end of the module (pytest -s)
and written as JSON to the file ET_TAL_SHARP_REPORT names; NOTEBOOK.md ("TAL per element") holds the tables of both tiers."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import tal_ref

F32 = np.float32
RECORD = {}
EXCLUDED = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    rows = sorted(RECORD.items())
    for (tier, path, out), v in rows:
        print(f"tal_sharp {tier:3s} {path:10s} {out:10s} {v:.3f}")
    for k, v in sorted(EXCLUDED.items()):
        print(f"tal_sharp excluded {k}: {v}")
    dst = os.environ.get("ET_TAL_SHARP_REPORT")
    if dst:
        with open(dst, "w") as fh:
            json.dump({"ratios": [[*k, v] for k, v in rows], "excluded": EXCLUDED}, fh, indent=0)


def _rec(hip, path, out, v):
    k = ("emu" if hip.emulated else "gpu", path, out)
    RECORD[k] = max(RECORD.get(k, 0.0), v)
    return v


def _ratio(got, ref, bound):
    return tal_ref.ratio(got, torch.as_tensor(np.asarray(ref), dtype=torch.float64), torch.as_tensor(np.asarray(bound), dtype=torch.float64))


# ---- assigner --------------------------------------------------------------------------------------------------------------------
def _points(levels):
    """anchor points in PIXELS of (h, w, stride) levels"""
    out = []
    for h, w, s in levels:
        ys, xs = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
        out.append(np.stack((xs.ravel(), ys.ravel()), 1) * s)
    return np.concatenate(out).astype(F32)


def _strides(levels):
    return np.concatenate([np.full(h * w, s, F32) for h, w, s in levels])


PYR = ((8, 8, 8), (4, 4, 16), (2, 2, 32))          # a 64-px image: A = 84, mixed strides
ONE300 = ((15, 20, 8),)                             # A = 300: two trips of the 256-thread scan
ONE9 = ((3, 3, 8),)                                 # A = 9 < topk

#              levels  B  nc  G  (topk, alpha, beta)   valid gts per image   seed
ASSIGN_CASES = {
    "pyr-default":   (PYR, 3, 3, 5, (13, 1.0, 6.0), (5, 0, 3), 11),
    "pyr-alpha":     (PYR, 1, 80, 17, (10, 0.5, 6.0), (12,), 12),
    "pyr-g1":        (PYR, 3, 80, 1, (10, 0.5, 6.0), (1, 1, 0), 13),
    "pyr-allpad":    (PYR, 1, 3, 5, (13, 1.0, 6.0), (0,), 14),
    "a300-default":  (ONE300, 3, 1, 17, (13, 1.0, 6.0), (17, 9, 1), 15),
    "a300-top1":     (ONE300, 1, 3, 1, (1, 1.0, 6.0), (1,), 16),
    "a300-topk>A":   (ONE300, 1, 3, 5, (400, 1.0, 6.0), (5,), 17),
    "a9-topk>A":     (ONE9, 3, 3, 5, (13, 1.0, 6.0), (5, 2, 0), 18),
    "a9-top1":       (ONE9, 1, 1, 5, (1, 1.0, 6.0), (4,), 19),
}


@functools.lru_cache(maxsize=None)
def _assign_random(name):
    levels, B, nc, G, (topk, alpha, beta), valid, seed = ASSIGN_CASES[name]
    rng = np.random.default_rng(seed)
    pts, st = _points(levels), _strides(levels)
    A = pts.shape[0]
    ext = pts.max(0) + st[-1] / 2
    c = pts[None] + rng.normal(0, 0.25, (B, A, 2)) * st[None, :, None]
    wh = (np.abs(rng.normal(3, 1.2, (B, A, 2))) + 0.25) * st[None, :, None]
    pb = np.concatenate((c - wh / 2, c + wh / 2), -1).astype(F32)
    ps = (rng.uniform(0, 1, (B, A, nc)) ** 2).astype(F32)
    gxy = rng.uniform(0, 1, (B, G, 2)) * ext
    gwh = np.abs(rng.normal(0.45, 0.2, (B, G, 2))) * ext + 4
    gb = np.concatenate((gxy - gwh / 2, gxy + gwh / 2), -1).astype(F32)
    gl = rng.integers(0, nc, (B, G)).astype(F32)
    mg = (np.arange(G)[None] < np.asarray(valid)[:, None]).astype(F32)
    gb = gb * mg[..., None]
    gl = np.where(mg > 0, gl, -1).astype(F32)                  # padded rows as tal_targets_pad writes them
    ops_in = (ps, pb, pts, gl[..., None], gb, mg[..., None])
    return ops_in, (topk, alpha, beta), tal_ref.assign(ps, pb, pts, gl, gb, mg, topk, alpha, beta)


def _check_caps(name, ref, directed):
    EXCLUDED[name] = dict(pairs=f"{ref.n_pairs_undecided}/{ref.n_pairs}", multi=f"{ref.n_multi_undecided}/{ref.n_multi}",
                          topk_gap=ref.min_topk_gap, iou_gap=ref.min_iou_gap)
    if directed:
        assert ref.n_pairs_undecided == 0 and ref.n_multi_undecided == 0, name
    assert ref.n_pairs_undecided * 100 <= ref.n_pairs and ref.n_multi_undecided * 100 <= ref.n_multi, name


def _run_assign(hip, name, ops_in, params, ref, directed=False):
    from efficientteacher_amd import ops
    _check_caps(name, ref, directed)                         # before anything is compared
    topk, alpha, beta = params
    tl, tb, ts, fg, idx = ops.tal_assign(*(hip.t(v) for v in ops_in), topk=topk, alpha=alpha, beta=beta, return_idx=True)
    tl, tb, ts, fg, idx = (v.cpu().numpy() for v in (tl, tb, ts, fg, idx))
    keep = ~ref.excluded
    assert np.array_equal(fg[keep], ref.fg[keep]), name
    assert np.array_equal(idx[keep], ref.idx[keep]), name
    assert np.array_equal(tl[keep], ref.tl[keep]) and np.array_equal(tb[keep], ref.tb[keep]), name
    assert ts.dtype == np.float32
    v = _rec(hip, "assign", "ts", _ratio(torch.from_numpy(ts[keep]), ref.ts[keep], ref.b_ts[keep]))
    assert v <= 1.0, (name, v)
    return tl, tb, ts, fg, idx


@pytest.mark.parametrize("name", list(ASSIGN_CASES))
def test_assign_random(hip, name):
    ops_in, params, ref = _assign_random(name)
    tl, tb, ts, fg, idx = _run_assign(hip, name, ops_in, params, ref)
    if name == "pyr-allpad":
        assert not fg.any() and not ts.any()
    else:
        assert ref.fg.any() and (ref.ts > 0).any(), "the case has no positive target"


def test_assign_reference_alone_meets_the_exclusion_caps():
    """CPU only: the caps hold on the reference for every seeded case, and the multi-claim / top-k paths are really reached"""
    multi = pairs = 0
    for name in ASSIGN_CASES:
        ref = _assign_random(name)[2]
        _check_caps(name, ref, False)
        multi, pairs = multi + ref.n_multi, pairs + ref.n_pairs
    assert multi > 50 and pairs > 40


def _grid_case(nc=1, G=1, B=1):
    """8 x 8 cells of 8 px; predictions = anchor +- 10, every score 0.5; gts to be filled in"""
    pts = _points(((8, 8, 8),))
    A = 64
    pb = np.concatenate((pts - 10, pts + 10), -1)[None].repeat(B, 0).astype(F32)
    ps = np.full((B, A, nc), 0.5, F32)
    return pts, pb, ps, np.zeros((B, G), F32), np.zeros((B, G, 4), F32), np.ones((B, G), F32)


def _directed(hip, name, ps, pb, pts, gl, gb, mg, params=(13, 1.0, 6.0)):
    ref = tal_ref.assign(ps, pb, pts, gl, gb, mg, *params)
    out = _run_assign(hip, name, (ps, pb, pts, gl[..., None], gb, mg[..., None]), params, ref, directed=True)
    return ref, out


def test_assign_anchor_on_a_gt_edge_is_outside(hip):
    pts, pb, ps, gl, gb, mg = _grid_case()
    gb[0, 0] = (12, 12, 36, 36)                              # edges at 8k + 4: the anchors at 12 and 36 lie ON them
    ref, (tl, tb, ts, fg, idx) = _directed(hip, "edge", ps, pb, pts, gl, gb, mg)
    inside = (pts[:, 0] > 12) & (pts[:, 0] < 36) & (pts[:, 1] > 12) & (pts[:, 1] < 36)
    assert inside.sum() == 4 and np.array_equal(fg[0], inside)


def test_assign_gt_with_no_anchor_and_with_one(hip):
    pts, pb, ps, gl, gb, mg = _grid_case(G=2)
    gb[0, 0] = (13, 13, 19, 19)                              # between the centres 12 and 20
    gb[0, 1] = (17, 17, 23, 23)                              # (20, 20) alone
    ref, (tl, tb, ts, fg, idx) = _directed(hip, "none-one", ps, pb, pts, gl, gb, mg)
    a = 2 * 8 + 2
    assert fg.sum() == 1 and fg[0, a] and idx[0, a] == 1 and ts[0, a, 0] > 0


def test_assign_predictions_that_miss_the_gt_have_metric_zero(hip):
    """every metric is exactly 0: the 13 picks are the anchors 0..12 (the smaller index wins), six of them inside the gt"""
    pts, pb, ps, gl, gb, mg = _grid_case()
    pb += 200
    gb[0, 0] = (0, 0, 24, 24)                                # holds the anchors {0, 1, 2} + 8 {0, 1, 2}
    ref, (tl, tb, ts, fg, idx) = _directed(hip, "miss", ps, pb, pts, gl, gb, mg)
    assert sorted(np.nonzero(fg[0])[0]) == [0, 1, 2, 8, 9, 10] and not ts.any()


def test_assign_degenerate_predicted_box(hip):
    pts, pb, ps, gl, gb, mg = _grid_case()
    gb[0, 0] = (0, 0, 24, 24)
    a = 1                                                    # metric 0 with the smallest index of all zeros: one of the 13 picks
    pb[0, a] = (22, -6, 2, 14)                               # x2 < x1: its area clamps to 0
    ref, (tl, tb, ts, fg, idx) = _directed(hip, "degenerate", ps, pb, pts, gl, gb, mg)
    assert fg[0, a] and ts[0, a, 0] == 0 and ref.iou[0, 0, a] == 0 and ts[0].max() > 0


def test_assign_padded_rows_do_not_leak_the_last_class(hip):
    nc = 3
    pts, pb, ps, gl, gb, mg = _grid_case(nc=nc, G=3)
    ps[..., nc - 1] = 0.99                                   # what a label of -1 would read after wrapping
    ps[..., 0] = 0.1
    gb[0, 0] = (10, 10, 30, 30)
    gl[0] = (0, -1, -1)
    mg[0] = (1, 0, 0)
    ref, (tl, tb, ts, fg, idx) = _directed(hip, "padded", ps, pb, pts, gl, gb, mg)
    assert fg.sum() == 9 and not ts[..., 1:].any() and (idx[fg] == 0).all() and (tl[fg] == 0).all()


def test_assign_identical_gts_first_one_owns(hip):
    pts, pb, ps, gl, gb, mg = _grid_case(nc=2, G=2)
    ps[..., 1] = 0.25
    gb[0, 0] = gb[0, 1] = (10, 10, 30, 30)
    gl[0] = (1, 0)
    ref, (tl, tb, ts, fg, idx) = _directed(hip, "identical", ps, pb, pts, gl, gb, mg)
    assert fg.sum() == 9 and ref.n_multi == 9 and (ref.cnt[ref.fg] == 2).all()
    assert (idx[fg] == 0).all() and (tl[fg] == 1).all() and not ts[..., 0].any()


def test_assign_anchor_won_on_iou_by_a_gt_without_it_in_topk(hip):
    pts, pb, ps, gl, gb, mg = _grid_case(nc=2, G=3)
    a, a2 = 3 * 8 + 3, 4 * 8 + 4                             # (28, 28) and (36, 36)
    ps[..., 0], ps[..., 1] = 0.01, 0.001
    ps[0, a, 0], ps[0, a2, 1] = 0.9, 0.9
    pb[0, a] = (14, 14, 42, 42)                              # == gt 2
    pb[0, a2] = (20, 20, 50, 50)
    gb[0] = ((10, 10, 40, 40), (16, 18, 46, 44), (14, 14, 42, 42))
    gl[0] = (0, 0, 1)
    ref, (tl, tb, ts, fg, idx) = _directed(hip, "won-on-iou", ps, pb, pts, gl, gb, mg, params=(1, 1.0, 6.0))
    assert ref.pos[0, 0, a] and ref.pos[0, 1, a] and not ref.pos[0, 2, a] and ref.pos[0, 2, a2]
    assert fg[0, a] and idx[0, a] == 2 and tl[0, a] == 1 and idx[0, a2] == 2 and fg.sum() == 2


def test_assign_equal_nonzero_metrics_smaller_index_wins(hip):
    """a gt centred on a grid corner, equal scores and sizes: four bit-equal non-zero metrics, topk = 2 keeps the two smaller indices"""
    pts, pb, ps, gl, gb, mg = _grid_case()
    pb[0] = np.concatenate((pts - 12, pts + 12), -1)
    gb[0, 0] = (20, 20, 44, 44)                              # centre (32, 32): the corner of the cells 27, 28, 35, 36
    ref, (tl, tb, ts, fg, idx) = _directed(hip, "symmetric", ps, pb, pts, gl, gb, mg, params=(2, 1.0, 6.0))
    four = [27, 28, 35, 36]
    assert ref.inbox[0, 0].sum() == 4 and len(set(ref.metric[0, 0, four])) == 1 and ref.metric[0, 0, 27] > 0
    assert sorted(np.nonzero(fg[0])[0]) == [27, 28] and (ts[0, [27, 28], 0] > 0).all()


# ---- loss ------------------------------------------------------------------------------------------------------------------------
W_CLASS, W_IOU, W_DFL = 0.5, 7.5, 1.5


def _loss_operands(seed, B, levels, nc, reg_max, p_fg=0.4):
    rng = np.random.default_rng(seed)
    st = _strides(levels)
    anc = _points(tuple((h, w, 1) for h, w, _ in levels))     # grid units
    A, nb = anc.shape[0], reg_max + 1
    ps = np.clip(rng.normal(0, 9, (B, A, nc)), -30, 30).astype(F32)
    pd = (rng.normal(1.0, 1.5, (B, A, 4 * nb))).astype(F32)
    fg = rng.uniform(size=(B, A)) < p_fg
    cls = rng.integers(0, nc, (B, A))
    ts = np.zeros((B, A, nc), F32)
    np.put_along_axis(ts, cls[..., None], rng.uniform(0.05, 1, (B, A, 1)).astype(F32), -1)
    ts *= fg[..., None]
    td = rng.uniform(0.15, 0.95 * reg_max, (B, A, 4))
    tb = np.concatenate((anc[None] - td[..., :2], anc[None] + td[..., 2:]), -1) * st[None, :, None]
    tb = (tb * fg[..., None]).astype(F32)
    return dict(ps=ps, pd=pd, anc=anc, st=st, tb=tb, ts=ts, fg=fg, reg_max=reg_max, nc=nc)


def _run_loss(hip, name, o, iou_type):
    from efficientteacher_amd import ops
    ref = tal_ref.loss(o["ps"], o["pd"], o["anc"], o["st"], o["tb"], o["ts"], o["fg"], o["reg_max"], iou_type, W_CLASS, W_IOU, W_DFL)
    t = hip.t
    out, gs, gd = ops.tal_loss(t(o["ps"]), t(o["pd"]), t(o["anc"]), t(o["st"]), t(o["tb"]), t(o["ts"]), t(o["fg"]), o["reg_max"], iou_type,
                               W_CLASS, W_IOU, W_DFL)
    assert out.dtype == gs.dtype == gd.dtype == torch.float32
    res = {}
    for i, k in enumerate(("iou", "dfl", "cls", "total")):
        res[k] = _rec(hip, "loss-" + iou_type, k, tal_ref.ratio(out[i:i + 1], ref.out[i:i + 1], ref.b_out[i:i + 1]))
    res["gs"] = _rec(hip, "loss-" + iou_type, "grad_cls", tal_ref.ratio(gs, ref.gs, ref.b_gs))
    res["gd"] = _rec(hip, "loss-" + iou_type, "grad_dfl", tal_ref.ratio(gd, ref.gd, ref.b_gd))
    print(f"tal_sharp loss {name} {iou_type} " + " ".join(f"{k}={v:.3f}" for k, v in res.items()))
    gd_c = gd.cpu().numpy()
    assert not gd_c[~o["fg"]].any(), "rows of non-foreground anchors in grad_distri must be exactly 0"
    assert all(v <= 1.0 for v in res.values()), (name, res)
    return ref, out.cpu().numpy(), gs.cpu().numpy(), gd_c


LOSS_SHAPES = {"A84": (1, PYR), "BA128": (2, ((8, 8, 8),)), "BA336": (4, PYR)}


@pytest.mark.parametrize("iou_type", ["iou", "giou"])
@pytest.mark.parametrize("reg_max,nc,shape", [(1, 3, "A84"), (7, 80, "BA128"), (16, 1, "BA336"), (31, 3, "A84"), (16, 80, "A84")])
def test_loss_random(hip, iou_type, reg_max, nc, shape):
    B, levels = LOSS_SHAPES[shape]
    o = _loss_operands(100 + reg_max + nc, B, levels, nc, reg_max)
    ref, out, gs, gd = _run_loss(hip, f"random-{reg_max}-{nc}-{shape}", o, iou_type)
    assert ref.S > 4.0 and o["fg"].sum() > 8                    # S well above its clamp


@pytest.mark.parametrize("iou_type", ["iou", "giou"])
def test_loss_sum_of_scores_below_one(hip, iou_type):
    o = _loss_operands(201, 1, PYR, 3, 16, p_fg=0.06)
    o["ts"] *= F32(0.125)
    assert 0 < o["ts"].sum() < 0.9 and o["fg"].sum() >= 2
    ref, out, gs, gd = _run_loss(hip, "S<1", o, iou_type)
    assert ref.S == 1.0


def test_loss_no_foreground(hip):
    o = _loss_operands(202, 1, PYR, 3, 16, p_fg=0.0)
    assert not o["fg"].any()
    ref, out, gs, gd = _run_loss(hip, "no-fg", o, "giou")
    assert out[0] == 0 and out[1] == 0 and not gd.any() and out[2] > 0 and out[3] == out[2]


def test_loss_foreground_anchor_with_zero_scores(hip):
    o = _loss_operands(203, 2, ((8, 8, 8),), 3, 7)
    a = np.nonzero(o["fg"][0])[0][:3]
    o["ts"][0, a] = 0
    ref, out, gs, gd = _run_loss(hip, "w=0", o, "giou")
    assert not gd[0, a].any() and (ref.gd[0, a] == 0).all()


@pytest.mark.parametrize("reg_max", [1, 16])
def test_loss_target_distances_outside_the_bins(hip, reg_max):
    """per stride: a target side beyond reg_max - 0.01 (clipped) and an anchor OUTSIDE its target box (negative distance, clipped to 0)"""
    o = _loss_operands(204 + reg_max, 1, PYR, 3, reg_max, p_fg=1.0)
    anc, st = o["anc"], o["st"]
    for first in (0, 64, 80):                                 # the first anchors of each level
        for j, (side, dist) in enumerate(((0, reg_max + 2.5), (3, reg_max - 0.005), (1, -1.75), (2, -0.5))):
            a = first + j
            sgn = -1.0 if side < 2 else 1.0
            o["tb"][0, a, side] = F32((anc[a, side % 2] + sgn * dist) * st[a])
    ref, out, gs, gd = _run_loss(hip, "clip", o, "giou")


@pytest.mark.parametrize("iou_type", ["iou", "giou"])
def test_loss_disjoint_boxes(hip, iou_type):
    o = _loss_operands(206, 1, PYR, 3, 7, p_fg=1.0)
    o["tb"][0, :40] += (o["st"][:40] * 40)[:, None]           # far to the lower right of every prediction
    ref, out, gs, gd = _run_loss(hip, "disjoint", o, iou_type)
    if iou_type == "iou":                                     # no overlap: the plain IoU has no gradient, only the DFL term is left
        assert np.abs(ref.gd[0, :40].numpy()).max() > 0


@pytest.mark.parametrize("iou_type", ["iou", "giou"])
def test_loss_enclosing_and_enclosed_per_side(hip, iou_type):
    """16 anchors: every combination of (predicted side longer / shorter than the target side) -- each arm of the di and dc selections"""
    reg_max, nb = 16, 17
    o = _loss_operands(207, 1, ((4, 4, 8),), 3, reg_max, p_fg=1.0)
    pd = o["pd"].reshape(1, 16, 4, nb)
    pd[:] = 0
    for a in range(16):
        for s in range(4):
            longer = (a >> s) & 1
            pd[0, a, s, 6 if longer else 2] = 9.0 + 0.25 * s     # the expectation sits near bin 6 / bin 2
            dist = 3.25 + 0.125 * s
            sgn = -1.0 if s < 2 else 1.0
            o["tb"][0, a, s] = F32((o["anc"][a, s % 2] + sgn * dist) * 8)
    o["pd"] = pd.reshape(1, 16, 4 * nb)
    ref, out, gs, gd = _run_loss(hip, "enclose", o, iou_type)


def test_loss_saturated_softmax_side(hip):
    o = _loss_operands(208, 1, PYR, 3, 16, p_fg=1.0)
    pd = o["pd"].reshape(1, 84, 4, 17)
    pd[0, :20, 0, 5] = 60.0                                   # p = 1 on one bin
    pd[0, 20:40, 1, 3] = -90.0                                # a bin whose exponential is below the normal range
    pd[0, 40:60, 2, 16] = 45.0                                # the last bin
    ref, out, gs, gd = _run_loss(hip, "saturated", o, "giou")


# ---- pseudo-label split ----------------------------------------------------------------------------------------------------------
def _below(v):
    return float(np.nextafter(v, -np.inf))


def _split_rows():
    lo, hi = np.array([0.2, 0.3, 0.25]), np.array([0.6, 0.7, 0.65])
    rows, valid = [], []
    rng = np.random.default_rng(301)

    def add(cls, conf, oc=0.5, cc=0.5, ok=1):
        rows.append([len(rows) % 2, cls, *rng.uniform(0.2, 0.8, 2), *rng.uniform(0.05, 0.4, 2), conf, oc, cc])
        valid.append(ok)
    for c in range(3):
        for conf in (hi[c], _below(hi[c]), lo[c], _below(lo[c]), 0.01, 0.95):
            add(c, conf)
    add(1, 0.95, ok=0); add(1, 0.5, ok=0)                     # invalid rows
    add(-1.0, 0.61); add(-0.5, 0.59); add(-7, 0.3)            # class below 0 -> 0
    add(3, 0.66); add(9, 0.64); add(2.7, 0.66); add(1.999, 0.65)     # clamped to nc - 1; fractional classes truncate
    for oc in (0.99, _below(0.99), 1.0):
        for cc in (0.99, _below(0.99)):
            add(0, 0.4, oc, cc); add(2, 0.3, oc, cc)
    if len(rows) % 2:
        add(0, 0.0)
    return np.array(rows, dtype=np.float64), np.array(valid, dtype=np.uint8), lo, hi


@pytest.mark.parametrize("flags", range(8))
@pytest.mark.parametrize("use_valid", [True, False])
def test_pseudo_split_bit_exact(hip, flags, use_valid):
    from efficientteacher_amd import ops
    with_obj, with_bbox, with_cls = flags & 1, (flags >> 1) & 1, (flags >> 2) & 1
    t9, valid, lo, hi = _split_rows()
    n, B, nc, img_w, img_h = t9.shape[0], 2, 3, 96.0, 64.0
    ref = tal_ref.pseudo_split(t9, valid if use_valid else None, lo, hi, nc, with_obj, with_bbox, with_cls, img_w, img_h)
    thr = hip.t(np.stack((lo, hi)))
    v = hip.t(valid) if use_valid else None
    (glr, gbr, mr), (glu, gbu, mu), us, uf = ops.tal_pseudo_split(hip.t(t9), v, thr, B, nc, with_obj, with_bbox, with_cls, img_w, img_h)
    got = dict(glabel_r=glr, gbox_r=gbr, glabel_u=glu, gbox_u=gbu, mask_r=mr, mask_u=mu, u_score=us, u_flags=uf)
    for k, r in ref.items():
        g = got[k].cpu().numpy().reshape(r.shape)
        assert g.dtype == r.dtype and np.array_equal(g.view(np.uint8), r.view(np.uint8)), k
    # the rows the case is about, asserted on the kernel's output itself
    mr, mu = got["mask_r"].cpu().numpy().ravel(), got["mask_u"].cpu().numpy().ravel()
    ok = valid.astype(bool) if use_valid else np.ones(n, bool)
    for c in range(3):
        assert list(mr[6 * c:6 * c + 6]) == [1, 0, 0, 0, 0, 1] and list(mu[6 * c:6 * c + 6]) == [0, 1, 1, 0, 0, 0]
    assert (mr[18:20] == (0 if use_valid else 1) * np.array([1, 0])).all() and mu[19] == (0 if use_valid else 1)
    assert list(mr[20:23]) == [1, 0, 0] and list(mu[20:23]) == [0, 1, 1]
    assert list(got["glabel_r"].cpu().numpy().ravel()[23:27]) == [2, -1, 2, -1] and list(got["glabel_u"].cpu().numpy().ravel()[23:27]) == [-1, 2, -1, 1]
    f = got["u_flags"].cpu().numpy().ravel()[27:39].reshape(3, 2, 2)        # (oc, cc, row)
    want = np.zeros((3, 2, 2), np.uint8)
    if with_obj:
        want[[0, 2]] |= np.uint8(with_bbox)
        want[:, 0] |= np.uint8(2 * with_cls)
    assert np.array_equal(f, want) and ok.sum() == (n - 2 if use_valid else n)
    assert (gbr.cpu().numpy()[..., 2] != gbr.cpu().numpy()[..., 3]).any()       # img_w != img_h is visible in the boxes


# ---- merge -----------------------------------------------------------------------------------------------------------------------
def test_merge_pseudo_every_owner_and_flag_combination(hip):
    from efficientteacher_amd import ops
    rng = np.random.default_rng(401)
    B, A, G, nc = 2, 16, 4, 3
    ts_r, ts_u = rng.uniform(0.1, 1, (B, A, nc)).astype(F32), rng.uniform(0.1, 1, (B, A, nc)).astype(F32)
    tb_r, tb_u = rng.uniform(0, 64, (B, A, 4)).astype(F32), rng.uniform(0, 64, (B, A, 4)).astype(F32)
    a = np.arange(A)
    perm = np.stack((a, a[::-1]))
    fg_u, fg_r, flag = (perm & 1) > 0, (perm & 2) > 0, perm >> 2          # (owner u, owner r) x flags {0, 1, 2, 3}
    u_flags = np.stack((np.arange(4), np.arange(4)[::-1])).astype(np.uint8)
    idx_u = np.where(np.arange(B)[:, None] == 0, flag, 3 - flag).astype(np.int32)    # the row whose flags are `flag`
    u_score = rng.uniform(0.3, 0.9, (B, G)).astype(F32)
    r_ts, r_tb, r_fg, r_scale = tal_ref.merge_pseudo(ts_r, tb_r, fg_r, ts_u, tb_u, fg_u, idx_u, u_score, u_flags)
    t = hip.t
    tb, ts, fgb = ops.tal_merge_pseudo((t(tb_r), t(ts_r), t(fg_r)), (t(tb_u), t(ts_u), t(fg_u), t(idx_u)), t(u_score), t(u_flags))
    tb, ts, fgb = tb.cpu().numpy(), ts.cpu().numpy(), fgb.cpu().numpy()
    assert np.array_equal(ts.view(np.uint32), r_ts.view(np.uint32)) and np.array_equal(tb.view(np.uint32), r_tb.view(np.uint32))
    assert np.array_equal(fgb, r_fg)
    for b in range(B):                                        # the rule itself, spelled out per combination
        for i in range(A):
            u, r, f = fg_u[b, i], fg_r[b, i], flag[b, i]
            assert u_flags[b, idx_u[b, i]] == f
            scale = (1.0 if f & 2 else u_score[b, idx_u[b, i]]) if u else (1.0 if r else 0.0)
            src_s, src_b = (ts_u, tb_u) if u else (ts_r, tb_r)
            assert np.array_equal(ts[b, i], src_s[b, i] * F32(scale)) and np.array_equal(tb[b, i], src_b[b, i])
            assert fgb[b, i] == ((f & 1) if u else (1 if r else 0)) and r_scale[b, i] == F32(scale)


# ---- targets_pad -----------------------------------------------------------------------------------------------------------------
def _pad_rows(imgs, seed=501):
    rng = np.random.default_rng(seed)
    n = len(imgs)
    return np.concatenate((np.asarray(imgs, F32)[:, None], rng.integers(0, 80, (n, 1)).astype(F32),
                           rng.uniform(0.2, 0.7, (n, 4)).astype(F32)), 1)


def _check_pad(hip, t, B, G_want, img_w=96.0, img_h=64.0):
    from efficientteacher_amd import ops
    la, ba, ma = ops.tal_targets_pad(hip.t(torch.from_numpy(t).reshape(-1, 6)), B, img_w, img_h)
    assert la.shape == (B, G_want, 1) and ba.shape == (B, G_want, 4) and ma.shape == (B, G_want, 1)
    out, mask = tal_ref.targets_pad(t, B, G_want, img_w, img_h)
    got = torch.cat((la, ba), -1).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), out.view(np.uint32)) and np.array_equal(ma.cpu().numpy()[..., 0], mask)
    return out, mask


def test_targets_pad_bit_exact(hip, monkeypatch):
    from efficientteacher_amd import ops
    out, mask = _check_pad(hip, np.zeros((0, 6), F32), 2, 1)                 # n = 0
    assert not mask.any() and (out[..., 0] == -1).all()
    imgs = [2, 0, 2, 3, 0, 2, -1, 2, 0, 5, 2]                                # image 1 has no rows; -1, 3 and 5 are dropped (B = 3)
    t = _pad_rows(imgs)
    t[2, 2:] = (0.0, 0.0, 0.0, 0.0)                                          # corner sum 0: mask 0
    t[4, 2:] = (-0.5, -0.5, 0.1, 0.1)                                        # corner sum < 0
    out, mask = _check_pad(hip, t, 3, len(imgs))
    assert mask.sum(1).tolist() == [2, 0, 4] and not mask[1].any()
    assert out[2, :5, 0].tolist() == t[[0, 2, 5, 7, 10], 1].tolist() and out[0, :3, 0].tolist() == t[[1, 4, 8], 1].tolist()
    assert mask[2, 1] == 0 and mask[0, 1] == 0 and out[0, 1, 0] == t[4, 1]
    monkeypatch.setattr(ops, "TAL_PAD_SYNC_FREE_ROWS", 2)                    # the crowded path: G = the largest per-image count
    imgs = [2, 0, 2, 1, 0, 2, 2, 0, 2]
    out, mask = _check_pad(hip, _pad_rows(imgs, 502), 3, 5)
    assert mask.sum(1).tolist() == [3, 1, 5]
