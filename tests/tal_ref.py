"""The YOLOv8 target path of csrc/tal.hip -- TaskAlignedAssigner, ComputeTalLoss with its gradients, the pseudo-label split / merge and
the padded target table -- restated from the written spec (oracle/v8.py, the comments of tal.hip), with DERIVED error bounds per output
element.  A plain module: no fixtures, no GPU.  Every operand is an fp32 value held exactly in float64.

Constants.  r = 2^-24 (bn_ref.R): one fp32 operation (add, sub, mul, div -- HIP divides correctly rounded by default) returns its exact
result times (1 + d), |d| <= r.  HO = 1 + 2^-10 (bn_ref.HO) covers the second-order products, FLOOR = 2^-126 (bn_ref.FLOOR) a result
flushed below the normal range.  bn_ref.silu_fwd_error is NOT reused: it describes v_rcp_f32(1 + v_exp_f32(-u log2 e)) of norm.hip,
while et_sigmoid here is 1 / (1 + expf(-x)) -- library expf, IEEE division; its bound is section L2.
tal.hip is compiled with -ffp-contract=off: no operation below is fused.

Library calls.  expf / logf / log1pf / powf are allowed U_EXP / U_LOG / U_LOG1P / U_POW ulp (1 ulp = 2 r relative): twice the larger
measured maximum error, rounded up to a whole ulp.  Measured against float64 on 2^20 uniform arguments over the ranges the cases use,
by a stand-alone program with the expressions below compiled as tal.hip is (NOTEBOOK.md "TAL per element"):
                              host libm (emulator)   device library (MI355X)   allowance
    expf   on [-100, 0]             0.502                   0.862              U_EXP   = 2
    logf   on [1, 32]               0.787                   1.877              U_LOG   = 4
    log1pf on [0, 1]                0.821                   0.567              U_LOG1P = 2
    powf   on (0, 1] ^ {.5, 1, 6}   0.502                   1.267              U_POW   = 3     (the device's powf(x, 1) is 1 ulp off, not exact)
    a / b                           0.500                   0.500              one rounding, r

ASSIGNER (tal_topk / tal_resolve / tal_gtmax / tal_emit)
 A1. IoU of gt g and prediction p.  The four clamped differences and the two products round once each, operands exact:
     ov, a1, a2 carry 3 r relative.  uni = fl(fl(fl(a1 + a2) - ov) + eps):
         d_uni = 3 r (a1 + a2 + ov) + r (|a1 + a2| + |a1 + a2 - ov| + |uni|),   rel(iou) = HO (3 r + d_uni / uni + r).
 A2. metric = fl(powf(sc, alpha) * powf(iou, beta)), sc an exact operand: rel(m) = HO (beta rel(iou) + (4 U_POW + 1) r), + FLOOR
     absolute where m > 0.  m = 0 exactly (sc = 0 or ov = 0 or the anchor outside the box) is 0 in the kernel too.
 A3. Decisions.  (in-box) the kernel compares fl(difference) > eps for the smallest of four differences: undecided where
     |diff - eps| <= r |diff| for one of them; an anchor ON an edge has diff = 0 exactly and is decidedly outside.
     (top-k) for a valid (image, gt) with k = min(topk, A) < A every member x of the k largest masked metrics against every other y:
     decided where m_x - e_x > m_y + e_y, or where x and y are an EXACT TIE -- both exactly 0, or the same score bits and the same
     fp32 (ov, uni) bits (restated in numpy float32: identical operands of the same instructions give identical results, so the kernel
     sees a tie too and the smaller anchor index wins, which is the documented rule).
     (multi-claim) for an anchor claimed by more than one gt the largest IoU over ALL rows of the table against every other row, with
     the errors of A1 and the same tie rule (first row wins).
     An undecided decision excludes its whole IMAGE from the comparison (a superset of what depends on it); assign() reports the
     counts and the smallest margins, the tests assert the caps before they compare anything.
 A4. score = fl(fl(m * pos_ov) / fl(pos_am + eps)): pos_ov / pos_am are maxima of fp32 values, so their relative error is at most
     the largest over the anchors the gt owns:
         rel(score) = HO (rel(m) + max rel(iou) + (max rel(m) pos_am + r (pos_am + eps)) / (pos_am + eps) + 2 r), + FLOOR.
     Labels, boxes, fg and the gt index are integers or copies: exact.

LOSS (tal_sum / tal_loss / tal_loss_finalize), one thread per (image, anchor)
 L1. Sums.  A sum of fp32 terms added in any order has error <= n r sum|t| + sum d_t, n = the most additions one term meets:
     in-thread additions + 6 xor-shuffle steps + one atomic per wave of the grid.  S = max(sum ts, 1) is continuous in the sum:
     d_S = n_S r sum|ts|.  w = sum_c ts[a, c]: d_w = nc r w.
 L2. Class term  t = max(x, 0) - x y + log1pf(expf(-|x|)),  e = exp(-|x|):
         d_t = r (|x y| + |max(x, 0) - x y| + |t|) + 2 U_EXP r e / (1 + e) + 2 U_LOG1P r log1p(e).
     sigmoid s = 1 / (1 + expf(-x)): the exponential enters through -(1 - s), the addition and the division r each:
         d_s = s ((1 - s) 2 U_EXP + 2) r + FLOOR.
     gx = w_class (s - y) / S:  d_gx = HO (w_class (d_s + r |s - y|) / S + |gx| (2 r + d_S / S)).
 L3. DFL expectation of one side, p_k = softmax(l)_k, E = sum p_k k.  e_k = expf(fl(l_k - m)): rel re_k = r |l_k - m| + 2 U_EXP r.
     den = sum e_k (nb additions): rel(den) = sum p_k re_k + nb r.  The same e_k enter numerator and denominator:
         d_E = sum p_k re_k |k - E| + r sum p_k k + 2 nb r E + r E.
     Box: x1 = fl(ax - E_0) ...: d_x = d_E + r |x|.  Target X = tb / stride: exact for the power-of-two strides, r |X| otherwise.
 L4. IoU / GIoU with running errors (cancellations are charged where they happen):
         w1 = x2 - x1, h1 = (y2 - y1) + eps, w2, h2; iw_ = min(x2, X2) - max(x1, X1) with the error of the selected operands; inter;
         a1 = w1 h1, a2 = w2 h2; uni = ((a1 + a2) - inter) + eps; iou = inter / uni;
         cw, ch; C = cw ch + eps; t = C - uni (d_t = d_C + d_uni + r |t|); q = t / C; giou = iou - q; l_iou = (1 - giou) w.
     Every selection (x1 > X1, iw_ > 0, ...) must be decided: loss() asserts |difference| > its error, which includes the exact ties at
     which torch splits the gradient of max / min and the kernel's strict comparisons do not.
 L5. d giou / d coordinate k:  du = da - di;  num = di uni - inter du (d_num = d(di uni) + d(inter du) + r |num|);
     dg = num / (uni uni) [+ (du C - uni dc) / (C C), the same way].  Every term is local to the anchor.
 L6. DFL target tt = clip(fl(a - X), 0, reg_max - 0.01f): d_tt = r |a - X| + d_X (0 where decidedly clipped).  wl = tr - tt and
     wr = tt - tl are exact given tt; the interpolated cross-entropy is continuous and piecewise linear in tt with slope
     |l_k - l_k+1|, the weights are hat functions with slope 1 -- so a floor that flips within d_tt stays inside the bound.
         lse = m + logf(den): d_lse = rel(den) + 2 U_LOG r |log den| + r |lse|
         term = ((lse - l_tl) wl + (lse - l_tr) wr) 0.25 w summed over the four sides in the thread.
 L7. Gradient of the DFL logits, per element:
         p_k: rel re_k + rel(den) + r;   dL/dE = ((w_iou (-dg)) sgn) w / S;   cd = ((w_dfl 0.25) w) / S
         g = fl(fl(fl(dL/dE p) fl(k - E)) + fl(cd fl(fl(p - wl_k) - wr_k)))
     with d(k - E) = d_E + r |k - E| and d(wl_k) = d_tt on the bins within two of tt.  No term is proportional to a tensor maximum.
 L8. Outputs: out_i = fl(fl(weight acc_i) / S): rel 2 r + d_S / S on top of L1; total = fl(fl(out_0 + out_1) + out_2).

SPLIT / MERGE / TARGETS_PAD are restated in the kernels' own arithmetic (numpy float32, one rounding per operation) and compared
bit for bit.
"""
import math

import numpy as np
import torch

from tests.bn_ref import FLOOR, HO, R, ratio  # noqa: F401  (ratio is re-exported for the tests)

F64 = torch.float64
U_EXP, U_LOG, U_LOG1P, U_POW = 2.0, 4.0, 2.0, 3.0        # ulp; see the docstring
F32 = np.float32


# ---- assigner ------------------------------------------------------------------------------------------------------------------
class Assign:
    """attributes of assign(): fg, idx, tl, tb, ts (float64), b_ts, excluded (B,) bool, counts and margins"""


def _iou64(g, p, eps):
    """g (..., 4), p (..., 4) float64, broadcastable -> iou, rel(iou) of A1"""
    x1, y1 = np.maximum(g[..., 0], p[..., 0]), np.maximum(g[..., 1], p[..., 1])
    x2, y2 = np.minimum(g[..., 2], p[..., 2]), np.minimum(g[..., 3], p[..., 3])
    ov = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    a1 = np.clip(g[..., 2] - g[..., 0], 0, None) * np.clip(g[..., 3] - g[..., 1], 0, None)
    a2 = np.clip(p[..., 2] - p[..., 0], 0, None) * np.clip(p[..., 3] - p[..., 1], 0, None)
    uni = a1 + a2 - ov + eps
    d_uni = 3 * R * (a1 + a2 + ov) + R * (np.abs(a1 + a2) + np.abs(a1 + a2 - ov) + np.abs(uni))
    iou = ov / uni
    return iou, HO * (4 * R + d_uni / uni)


def _iou_bits32(g, p, eps):
    """the kernel's own (ov, uni) in numpy float32: only used to recognise EXACT ties"""
    g, p, z = g.astype(F32), p.astype(F32), F32(0)
    x1, y1 = np.maximum(g[..., 0], p[..., 0]), np.maximum(g[..., 1], p[..., 1])
    x2, y2 = np.minimum(g[..., 2], p[..., 2]), np.minimum(g[..., 3], p[..., 3])
    ov = np.maximum(x2 - x1, z) * np.maximum(y2 - y1, z)
    a1 = np.maximum(g[..., 2] - g[..., 0], z) * np.maximum(g[..., 3] - g[..., 1], z)
    a2 = np.maximum(p[..., 2] - p[..., 0], z) * np.maximum(p[..., 3] - p[..., 1], z)
    uni = a1 + a2 - ov + F32(eps)
    return ov, uni


def _decided(v, e, keys, members, others):
    """every x in `members` against every y in `others`: v_x - e_x > v_y + e_y, or an exact tie (equal keys)"""
    if len(members) == 0 or len(others) == 0:
        return True
    for x in members:
        for y in others:
            if keys[x] == keys[y]:
                continue
            if not v[x] - e[x] > v[y] + e[y]:
                return False
    return True


def assign(ps, pb, pts, gl, gb, mg, topk=13, alpha=1.0, beta=6.0, eps=1e-9):
    """ps (B, A, nc) scores, pb (B, A, 4) predicted xyxy, pts (A, 2), gl (B, G[, 1]), gb (B, G, 4), mg (B, G[, 1]): numpy float32."""
    ps, pb, pts, gb = (np.asarray(t, dtype=F32).astype(np.float64) for t in (ps, pb, pts, gb))
    B, A, nc = ps.shape
    G = gb.shape[1]
    gl = np.asarray(gl, dtype=F32).astype(np.float64).reshape(B, G)
    mg = np.asarray(mg, dtype=F32).astype(np.float64).reshape(B, G)
    eps = float(F32(eps))
    lab = gl.astype(np.int64)
    labw = np.where(lab < 0, lab + nc, lab)                                      # torch indexing with -1 wraps around
    sc = np.take_along_axis(ps.transpose(0, 2, 1), labw[:, :, None].repeat(A, 2), 1)     # (B, G, A)
    iou, rel_iou = _iou64(gb[:, :, None, :], pb[:, None, :, :], eps)
    ov32, uni32 = _iou_bits32(gb[:, :, None, :], pb[:, None, :, :], eps)
    met = sc ** alpha * iou ** beta
    rel_m = HO * (beta * rel_iou + (4 * U_POW + 1) * R)
    e_m = np.where(met > 0, met * rel_m + FLOOR, 0.0)
    e_iou = np.where(iou > 0, iou * rel_iou + FLOOR, 0.0)
    diffs = np.stack([pts[None, None, :, 0] - gb[:, :, None, 0], pts[None, None, :, 1] - gb[:, :, None, 1],
                      gb[:, :, None, 2] - pts[None, None, :, 0], gb[:, :, None, 3] - pts[None, None, :, 1]], -1)
    inbox = diffs.min(-1) > eps
    und_in = (np.abs(diffs - eps) <= R * np.abs(diffs)).any(-1)                   # (B, G, A)
    assert met.dtype == np.float64 and iou.dtype == np.float64 and diffs.dtype == np.float64
    masked = np.where(inbox, met, 0.0)
    e_mk = np.where(inbox, e_m, 0.0)
    r = Assign()
    r.excluded = np.zeros(B, dtype=bool)
    r.n_pairs = r.n_pairs_undecided = r.n_multi = r.n_multi_undecided = 0
    r.min_topk_gap, r.min_iou_gap = math.inf, math.inf
    r.min_inbox_margin = float(np.abs(diffs - eps).min()) if G else math.inf
    pos = np.zeros((B, G, A), dtype=bool)
    k = min(int(topk), A)
    for b in range(B):
        for g in range(G):
            if mg[b, g] <= 0:
                continue
            r.n_pairs += 1
            v, e = masked[b, g].copy(), e_mk[b, g]
            keys, canon = [], {}
            for a in range(A):
                key = 0 if v[a] == 0 else (sc[b, g, a], float(ov32[b, g, a]), float(uni32[b, g, a]))
                keys.append(key)
                v[a] = canon.setdefault(key, v[a])                               # an exact tie sorts as one value
            order = np.argsort(-v, kind="stable")
            top, rest = order[:k], order[k:]
            und = bool(und_in[b, g].any())
            if len(rest):
                und = und or not _decided(v, e, keys, top, rest)
                if v[top[-1]] > 0 and keys[top[-1]] != keys[rest[0]]:
                    r.min_topk_gap = min(r.min_topk_gap, (v[top[-1]] - v[rest[0]]) / v[top[-1]])
            if und:
                r.n_pairs_undecided += 1
                r.excluded[b] = True
            pos[b, g, top] = inbox[b, g, top]
    cnt = pos.sum(1)                                                             # (B, A)
    idx = np.where(cnt > 0, pos.argmax(1), 0)
    for b, a in zip(*np.nonzero(cnt > 1)):
        r.n_multi += 1
        v, e = iou[b, :, a].copy(), e_iou[b, :, a]
        keys, canon = [], {}
        for g in range(G):
            key = 0 if ov32[b, g, a] == 0 else (float(ov32[b, g, a]), float(uni32[b, g, a]))
            keys.append(key)
            v[g] = canon.setdefault(key, v[g])
        best = int(np.argmax(v))                                                 # the first maximum
        others = [g for g in range(G) if g != best]
        if not _decided(v, e, keys, [best], others):
            r.n_multi_undecided += 1
            r.excluded[b] = True
        gaps = [v[best] - v[g] for g in others if keys[g] != keys[best]]
        if gaps:
            r.min_iou_gap = min(r.min_iou_gap, min(gaps))
        idx[b, a] = best
    fg = cnt > 0
    bi = np.arange(B)[:, None]
    own = np.zeros((B, G, A), dtype=bool)
    own[bi, idx, np.arange(A)[None, :]] = fg
    pos_am = np.where(own, met, 0.0).max(-1)                                     # (B, G)
    pos_ov = np.where(own, iou, 0.0).max(-1)
    rmax_m = np.where(own, rel_m, 0.0).max(-1)
    rmax_o = np.where(own, rel_iou, 0.0).max(-1)
    m_a = met[bi, idx, np.arange(A)[None, :]]
    am, ao = pos_am[bi, idx], pos_ov[bi, idx]
    score = np.where(fg, m_a * ao / (am + eps), 0.0)
    rel = rel_m[bi, idx, np.arange(A)[None, :]] + rmax_o[bi, idx] + (rmax_m[bi, idx] * am + R * (am + eps)) / (am + eps) + 2 * R
    b_score = np.where(score > 0, HO * score * rel + FLOOR, 0.0)
    tl = np.maximum(lab[bi, idx], 0)
    r.fg, r.idx, r.tl, r.tb = fg, idx.astype(np.int32), tl, gb[bi, idx].astype(F32)
    r.ts = np.zeros((B, A, nc))
    r.b_ts = np.zeros((B, A, nc))
    np.put_along_axis(r.ts, tl[..., None], score[..., None], -1)
    np.put_along_axis(r.b_ts, tl[..., None], b_score[..., None], -1)
    r.pos, r.cnt, r.metric, r.iou, r.inbox = pos, cnt, met, iou, inbox
    assert r.ts.dtype == np.float64 and r.b_ts.dtype == np.float64
    return r


# ---- loss ----------------------------------------------------------------------------------------------------------------------
class Loss:
    """attributes of loss(): out (4,), b_out (4,), gs, b_gs (B, A, nc), gd, b_gd (B, A, 4 nb), S, w -- all float64"""


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a) if not isinstance(a, torch.Tensor) else a.detach().cpu()).to(torch.float32).to(F64)


def _sum_adds(n_threads_terms, in_thread):
    """n of L1 for tal_loss_kernel: in-thread additions + 6 shuffle steps + one atomic per wave of ceil(n / 256) blocks"""
    return in_thread + 6 + 4 * (-(-n_threads_terms // 256))


def loss(ps, pd, anc_s, stride, tb, ts, fg, reg_max, iou_type, w_class, w_iou, w_dfl):
    ps, pd, anc_s, stride, tb, ts = map(_t, (ps, pd, anc_s, stride, tb, ts))
    fg = torch.as_tensor(np.asarray(fg)).bool()
    stride = stride.reshape(-1)
    B, A, nc = ps.shape
    nb = reg_max + 1
    giou_kind = {"iou": False, "giou": True}[iou_type]
    w_class, w_iou, w_dfl = (float(F32(v)) for v in (w_class, w_iou, w_dfl))
    eps = float(F32(1e-7))
    hi = float(F32(reg_max) - F32(0.01))
    o = Loss()
    # -- reference values: the written spec (oracle/v8.py::_tal_terms) in float64, gradients by autograd
    x = ps.clone().requires_grad_(True)
    l = pd.clone().reshape(B, A, 4, nb).requires_grad_(True)
    S = torch.clamp(ts.sum(), min=1.0)
    w = ts.sum(-1)                                                               # (B, A)
    t_cls = torch.clamp(x, min=0) - x * ts + torch.log1p(torch.exp(-x.abs()))
    proj = torch.arange(nb, dtype=F64)
    p = torch.softmax(l, -1)
    E = (p * proj).sum(-1)                                                       # (B, A, 4)
    ax, ay = anc_s[:, 0][None], anc_s[:, 1][None]
    x1, y1, x2, y2 = ax - E[..., 0], ay - E[..., 1], ax + E[..., 2], ay + E[..., 3]
    T = tb / stride[None, :, None]
    X1, Y1, X2, Y2 = T.unbind(-1)
    w1, h1, w2, h2 = x2 - x1, y2 - y1 + eps, X2 - X1, Y2 - Y1 + eps
    iw_, ih_ = torch.minimum(x2, X2) - torch.maximum(x1, X1), torch.minimum(y2, Y2) - torch.maximum(y1, Y1)
    iw, ih = iw_.clamp(min=0), ih_.clamp(min=0)
    inter = iw * ih
    a1, a2 = w1 * h1, w2 * h2
    uni = a1 + a2 - inter + eps
    iou = inter / uni
    cw, ch = torch.maximum(x2, X2) - torch.minimum(x1, X1), torch.maximum(y2, Y2) - torch.minimum(y1, Y1)
    C = cw * ch + eps
    giou = iou - (C - uni) / C if giou_kind else iou
    fgf = fg.to(F64)
    t_iou = (1.0 - giou) * w * fgf
    tdist = torch.stack([ax - X1, ay - Y1, X2 - ax, Y2 - ay], -1)                # (B, A, 4)
    tt = tdist.clamp(0.0, hi)
    tl_ = tt.floor().long()
    tr_ = tl_ + 1
    wl, wr = tr_.to(F64) - tt, tt - tl_.to(F64)
    lse = torch.logsumexp(l, -1)
    ce = (lse - l.gather(-1, tl_[..., None])[..., 0]) * wl + (lse - l.gather(-1, tr_[..., None])[..., 0]) * wr
    t_dfl = ce * 0.25 * w[..., None] * fgf[..., None]                            # (B, A, 4)
    L_cls, L_iou, L_dfl = t_cls.sum() / S, t_iou.sum() / S, t_dfl.sum() / S
    o_iou, o_dfl, o_cls = w_iou * L_iou, w_dfl * L_dfl, w_class * L_cls
    total = o_iou + o_dfl + o_cls
    total.backward()
    o.out = torch.stack([o_iou, o_dfl, o_cls, total]).detach()
    o.gs, o.gd = x.grad, l.grad.reshape(B, A, 4 * nb)
    assert o.out.dtype == F64 and o.gs.dtype == F64 and o.gd.dtype == F64
    o.S, o.w = float(S), w
    # -- bounds
    with torch.no_grad():
        l = l.detach(); x = x.detach()
        n_ts = B * A * nc
        blocks = min(-(-n_ts // 256), 1024)
        n_S = -(-n_ts // (blocks * 256)) + 6 + 4 * blocks
        d_S = n_S * R * float(ts.abs().sum())
        rS = d_S / float(S)
        d_w = nc * R * ts.abs().sum(-1)
        # L2
        xa = x.abs()
        e = torch.exp(-xa)
        d_t = R * ((x * ts).abs() + (torch.clamp(x, min=0) - x * ts).abs() + t_cls.detach().abs()) + 2 * U_EXP * R * e / (1 + e) \
            + 2 * U_LOG1P * R * torch.log1p(e)
        n_cls = _sum_adds(B * A, nc)
        E_cls = HO * (d_t.sum() + n_cls * R * t_cls.detach().abs().sum())
        s = torch.sigmoid(x)
        d_s = s * ((1 - s) * 2 * U_EXP + 2) * R + FLOOR
        gx = w_class * (s - ts) / S
        o.b_gs = HO * (w_class * (d_s + R * (s - ts).abs()) / S + gx.abs() * (2 * R + rS)) + FLOOR
        # L3
        m = l.max(-1, keepdim=True)[0]
        re = R * (l - m).abs() + 2 * U_EXP * R
        pk = p.detach()
        Ek = E.detach()
        rel_den = (pk * re).sum(-1) + nb * R                                     # (B, A, 4)
        d_E = (pk * re * (proj - Ek[..., None]).abs()).sum(-1) + R * (pk * proj).sum(-1) + (2 * nb + 1) * R * Ek
        crd = torch.stack([x1, y1, x2, y2], -1).detach()                         # predicted coordinates
        d_crd = d_E + R * crd.abs()
        T32 = (tb.to(torch.float32) / stride[None, :, None].to(torch.float32)).to(F64)
        d_T = torch.where(T32 == T, torch.zeros_like(T), R * T.abs())
        # L4: selections and their margins
        sel_lo = crd[..., :2] > T[..., :2]                                       # x1 > X1, y1 > Y1
        sel_hi = crd[..., 2:] < T[..., 2:]                                       # x2 < X2, y2 < Y2
        margin = (crd - T).abs() - (d_crd + d_T)
        fgm = fg[..., None]
        assert bool((margin[fgm.expand_as(margin)] > 0).all()), "a predicted coordinate ties with its target coordinate within the fp32 error"
        d_min_hi = torch.where(sel_hi, d_crd[..., 2:], d_T[..., 2:])             # error of min(x2, X2), min(y2, Y2)
        d_max_lo = torch.where(sel_lo, d_crd[..., :2], d_T[..., :2])             # error of max(x1, X1), max(y1, Y1)
        d_max_hi = torch.where(sel_hi, d_T[..., 2:], d_crd[..., 2:])
        d_min_lo = torch.where(sel_lo, d_T[..., :2], d_crd[..., :2])
        i_ = torch.stack([iw_, ih_], -1).detach()
        d_i_ = d_min_hi + d_max_lo + R * i_.abs()
        assert bool(((i_.abs() - d_i_)[fg] > 0).all()), "an intersection extent is 0 within the fp32 error"
        on = i_ > 0
        d_iwh = torch.where(on, d_i_, torch.zeros_like(d_i_))
        iwv, ihv = iw.detach(), ih.detach()
        d_iw, d_ih = d_iwh[..., 0], d_iwh[..., 1]
        interv = inter.detach()
        d_inter = iwv * d_ih + ihv * d_iw + R * interv
        w1v, h1v, w2v, h2v = (v.detach() for v in (w1, h1, w2, h2))
        d_w1 = d_crd[..., 0] + d_crd[..., 2] + R * w1v.abs()
        d_h1 = d_crd[..., 1] + d_crd[..., 3] + R * (y2 - y1).detach().abs() + R * h1v.abs()
        d_w2 = d_T[..., 0] + d_T[..., 2] + R * w2v.abs()
        d_h2 = d_T[..., 1] + d_T[..., 3] + R * (Y2 - Y1).abs() + R * h2v.abs()
        a1v, a2v = a1.detach(), a2.detach()
        d_a1 = w1v.abs() * d_h1 + h1v.abs() * d_w1 + R * a1v.abs()
        d_a2 = w2v.abs() * d_h2 + h2v.abs() * d_w2 + R * a2v.abs()
        univ = uni.detach()
        d_uni = d_a1 + d_a2 + d_inter + R * ((a1v + a2v).abs() + (a1v + a2v - interv).abs() + univ.abs())
        iouv = iou.detach()
        d_iou = d_inter / univ.abs() + iouv.abs() * d_uni / univ.abs() + R * iouv.abs()
        cwv, chv, Cv = cw.detach(), ch.detach(), C.detach()
        d_cw = d_max_hi[..., 0] + d_min_lo[..., 0] + R * cwv.abs()
        d_ch = d_max_hi[..., 1] + d_min_lo[..., 1] + R * chv.abs()
        d_C = cwv.abs() * d_ch + chv.abs() * d_cw + R * (cwv * chv).abs() + R * Cv.abs()
        d_g = d_iou
        if giou_kind:
            tq = Cv - univ
            d_tq = d_C + d_uni + R * tq.abs()
            q = tq / Cv
            d_q = d_tq / Cv.abs() + q.abs() * d_C / Cv.abs() + R * q.abs()
            d_g = d_iou + d_q + R * giou.detach().abs()
        omg = (1.0 - giou.detach())
        ti = omg * w
        d_ti = ((d_g + R * omg.abs()) * w + omg.abs() * d_w + R * ti.abs()) * fgf
        n_iou = _sum_adds(B * A, 0)
        E_iou = HO * (d_ti.sum() + n_iou * R * (ti.abs() * fgf).sum())
        # L5
        zero = torch.zeros_like(iwv)
        di = torch.stack([torch.where(on[..., 0] & sel_lo[..., 0], -ihv, zero), torch.where(on[..., 1] & sel_lo[..., 1], -iwv, zero),
                          torch.where(on[..., 0] & sel_hi[..., 0], ihv, zero), torch.where(on[..., 1] & sel_hi[..., 1], iwv, zero)], -1)
        d_di = torch.stack([d_ih, d_iw, d_ih, d_iw], -1) * (di != 0)
        da = torch.stack([-h1v, -w1v, h1v, w1v], -1)
        d_da = torch.stack([d_h1, d_w1, d_h1, d_w1], -1)
        du = da - di
        d_du = d_da + d_di + R * du.abs()
        U4, dU4, I4, dI4 = univ[..., None], d_uni[..., None], interv[..., None], d_inter[..., None]
        n1, n2 = di * U4, I4 * du
        d_n1 = di.abs() * dU4 + U4.abs() * d_di + R * n1.abs()
        d_n2 = I4.abs() * d_du + du.abs() * dI4 + R * n2.abs()
        num = n1 - n2
        d_num = d_n1 + d_n2 + R * num.abs()
        den2 = U4 * U4
        dg = num / den2
        d_dg = d_num / den2 + dg.abs() * (2 * dU4 / U4.abs() + 2 * R)
        if giou_kind:
            C4, dC4 = Cv[..., None], d_C[..., None]
            dc = torch.stack([torch.where(~sel_lo[..., 0], -chv, zero), torch.where(~sel_lo[..., 1], -cwv, zero),
                              torch.where(~sel_hi[..., 0], chv, zero), torch.where(~sel_hi[..., 1], cwv, zero)], -1)
            d_dc = torch.stack([d_ch, d_cw, d_ch, d_cw], -1) * (dc != 0)
            m1, m2 = du * C4, U4 * dc
            d_m1 = du.abs() * dC4 + C4.abs() * d_du + R * m1.abs()
            d_m2 = U4.abs() * d_dc + dc.abs() * dU4 + R * m2.abs()
            num2 = m1 - m2
            d_num2 = d_m1 + d_m2 + R * num2.abs()
            add = num2 / (C4 * C4)
            d_add = d_num2 / (C4 * C4) + add.abs() * (2 * dC4 / C4.abs() + 2 * R)
            d_dg = d_dg + d_add + R * (dg + add).abs()
            dg = dg + add
        # L6
        tdv = tdist
        d_T4 = torch.stack([d_T[..., 0], d_T[..., 1], d_T[..., 2], d_T[..., 3]], -1)
        d_tt = R * tdv.abs() + d_T4
        clipped = ((tdv < 0) & (tdv.abs() > d_tt)) | ((tdv > hi) & ((tdv - hi) > d_tt))
        d_tt = torch.where(clipped, torch.zeros_like(d_tt), d_tt)
        logden = (lse.detach() - m[..., 0])
        d_lse = rel_den + 2 * U_LOG * R * logden.abs() + R * lse.detach().abs()
        ltl, ltr = l.gather(-1, tl_[..., None])[..., 0], l.gather(-1, tr_[..., None])[..., 0]
        A1, A2 = lse.detach() - ltl, lse.detach() - ltr
        slope = (l[..., 1:] - l[..., :-1]).abs().max(-1)[0]
        cev = ce.detach()
        d_ce = (d_lse + R * A1.abs()) * wl + R * (A1 * wl).abs() + (d_lse + R * A2.abs()) * wr + R * (A2 * wr).abs() + slope * d_tt + R * cev.abs()
        td = cev * 0.25 * w[..., None]
        d_td = (0.25 * d_ce * w[..., None] + 0.25 * cev.abs() * d_w[..., None] + R * td.abs()) * fgf[..., None]
        n_dfl = _sum_adds(B * A, 4)
        E_dfl = HO * (d_td.sum() + n_dfl * R * (td.abs() * fgf[..., None]).sum())
        # L7
        rel_p = re + rel_den[..., None] + R
        d_p = pk * rel_p + FLOOR
        w4 = w[..., None]
        dLdE = w_iou * (-dg) * torch.tensor([-1.0, -1.0, 1.0, 1.0], dtype=F64) * w4 / S          # (B, A, 4)
        d_dLdE = (w_iou * w4 / S) * d_dg + dLdE.abs() * (3 * R + rS) + (w_iou * dg.abs() / S) * d_w[..., None]
        kE = proj - Ek[..., None]                                                # (B, A, 4, nb)
        d_kE = d_E[..., None] + R * kE.abs()
        g1 = dLdE[..., None] * pk * kE
        d_g1 = (pk * kE).abs() * d_dLdE[..., None] + (dLdE[..., None] * kE).abs() * d_p + (dLdE[..., None] * pk).abs() * d_kE + 2 * R * g1.abs()
        cd = w_dfl * 0.25 * w4 / S
        d_cd = cd * (3 * R + rS) + (w_dfl * 0.25 / S) * d_w[..., None]
        wlk = torch.zeros_like(pk).scatter_(-1, tl_[..., None], wl[..., None])
        wrk = torch.zeros_like(pk).scatter_(-1, tr_[..., None], wr[..., None])
        near = (proj - tt[..., None]).abs() < 2.0
        inner = pk - wlk - wrk
        d_inner = d_p + near * d_tt[..., None] + R * (pk - wlk).abs() + R * inner.abs()
        g2 = cd[..., None] * inner
        d_g2 = inner.abs() * d_cd[..., None] + cd[..., None] * d_inner + R * g2.abs()
        b_gd = (HO * (d_g1 + d_g2 + R * (g1 + g2).abs()) + FLOOR) * fgf[..., None, None]
        o.b_gd = b_gd.reshape(B, A, 4 * nb)
        # L8
        acc = torch.stack([t_iou.detach().sum(), t_dfl.detach().sum(), t_cls.detach().sum()])
        E_acc = torch.stack([E_iou, E_dfl, E_cls])
        wt = torch.tensor([w_iou, w_dfl, w_class], dtype=F64)
        b3 = HO * (wt * E_acc / S + o.out[:3].abs() * (2 * R + rS))
        b_tot = b3.sum() + R * (o.out[0] + o.out[1]).abs() + R * o.out[3].abs()
        o.b_out = torch.cat([b3, b_tot[None]])
        assert o.b_out.dtype == F64 and o.b_gs.dtype == F64 and o.b_gd.dtype == F64
    return o


# ---- split / merge / targets_pad: the kernels' own arithmetic, bit for bit ----------------------------------------------------------
def _box32(x, y, w, h, img_w, img_h):
    """normalised xywh -> xyxy pixels in fp32, one rounding per operation (ComputeTalLoss.preprocess)"""
    iw, ih, half = F32(img_w), F32(img_h), F32(0.5)
    x, y, w, h = F32(x) * iw, F32(y) * ih, F32(w) * iw, F32(h) * ih
    x1, y1 = x - w * half, y - h * half
    return np.array([x1, y1, x1 + w, y1 + h], dtype=F32)


def pseudo_split(t9, valid, lo, hi, nc, with_obj, with_bbox, with_cls, img_w, img_h):
    """t9 (n, 9) float64, valid (n,) or None, lo / hi (nc,) float64 -> dict of the eight outputs, flat over the n rows"""
    t9 = np.asarray(t9, dtype=np.float64)
    n = t9.shape[0]
    o = dict(glabel_r=np.full(n, -1, F32), gbox_r=np.zeros((n, 4), F32), glabel_u=np.full(n, -1, F32), gbox_u=np.zeros((n, 4), F32),
             mask_r=np.zeros(n, F32), mask_u=np.zeros(n, F32), u_score=np.zeros(n, F32), u_flags=np.zeros(n, np.uint8))
    for i in range(n):
        r = t9[i]
        ok = valid is None or bool(valid[i])
        c = int(np.trunc(r[1])) if ok else 0
        c = min(max(c, 0), nc - 1)
        conf, oc, cc = r[6], r[7], r[8]
        rel = ok and conf >= hi[c]
        unc = ok and not rel and conf >= lo[c]
        bx = _box32(r[2], r[3], r[4], r[5], img_w, img_h)
        if rel:
            o["glabel_r"][i], o["gbox_r"][i], o["mask_r"][i] = F32(c), bx, 1
        if unc:
            o["glabel_u"][i], o["gbox_u"][i], o["mask_u"][i] = F32(c), bx, 1
            o["u_score"][i] = F32(oc if with_obj else conf)
            if with_obj:
                o["u_flags"][i] = (1 if (with_bbox and oc >= 0.99) else 0) | (2 if (with_cls and cc >= 0.99) else 0)
    return o


def merge_pseudo(ts_r, tb_r, fg_r, ts_u, tb_u, fg_u, idx_u, u_score, u_flags):
    """-> (ts, tb, fg_box, scale): the uncertain owner of an anchor wins; scale is what multiplied the source scores"""
    ts_r, tb_r, ts_u, tb_u, u_score = (np.asarray(t, dtype=F32) for t in (ts_r, tb_r, ts_u, tb_u, u_score))
    B, A, nc = ts_r.shape
    ts, tb = np.zeros((B, A, nc), F32), np.zeros((B, A, 4), F32)
    fgb, scale = np.zeros((B, A), np.uint8), np.zeros((B, A), F32)
    for b in range(B):
        for a in range(A):
            if fg_u[b, a]:
                f = int(u_flags[b, idx_u[b, a]])
                scale[b, a] = F32(1) if f & 2 else u_score[b, idx_u[b, a]]
                fgb[b, a] = f & 1
                ts[b, a], tb[b, a] = ts_u[b, a] * scale[b, a], tb_u[b, a]
            elif fg_r[b, a]:
                scale[b, a], fgb[b, a] = 1, 1
                ts[b, a], tb[b, a] = ts_r[b, a], tb_r[b, a]
            else:
                tb[b, a] = tb_r[b, a]
    return ts, tb, fgb, scale


def targets_pad(t, B, G, img_w, img_h):
    """t (n, 6) float32 [img, cls, x, y, w, h] -> (out (B, G, 5), mask (B, G)); slot = number of earlier rows of the same image"""
    t = np.asarray(t, dtype=F32).reshape(-1, 6)
    out, mask = np.zeros((B, G, 5), F32), np.zeros((B, G), F32)
    out[..., 0] = -1
    img = np.trunc(t[:, 0]).astype(np.int64)
    for i in range(t.shape[0]):
        if img[i] < 0 or img[i] >= B:
            continue
        rank = int((img[:i] == img[i]).sum())
        if rank >= G:
            continue
        bx = _box32(t[i, 2], t[i, 3], t[i, 4], t[i, 5], img_w, img_h)
        out[img[i], rank, 0], out[img[i], rank, 1:] = t[i, 1], bx
        mask[img[i], rank] = 1 if ((bx[0] + bx[1]) + bx[2]) + bx[3] > 0 else 0
    return out, mask
