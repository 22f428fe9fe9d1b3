"""Zero-tolerance tier on CHANNEL SLICES WITH LIVE NEIGHBOURS: every operand of the conv, dgrad, wgrad and BatchNorm-sum kernels is a
window `wide[..., off:off + C]` of a wider (N, H, W, ld) buffer whose other channels hold live data, as in the model (the C3 stem's
3c-wide buffer, the halves of its 2c-wide y / dy, gradients arriving as slices of a concat gradient, SPPF and the neck concats).

* READ operands lie in POISON (64.0: exact in fp32, bf16 and fp16, 20 times the largest operand of the conv problems, and a value no
  window of the element-wise tests is filled with): a read that strays out of the window and meets a non-zero weight moves an
  integer result, and the comparison is `torch.equal` against the fp64 references of
  tests/exact_ref.py (whose exactness preconditions are asserted on the reference alone).  Not NaN: a kernel may multiply real slack
  by zero-padded weights.
* OUTPUTS go into windows of a buffer filled with a SENTINEL pattern of small integers, and after the call the slack must be
  `torch.equal` to its pre-call copy: a store outside the window is seen even when it stores zeros.
* Three layouts per operand of C channels (all multiples of 8): (ld, off) = (3C, 0) the first window -- a read past C lands in poison;
  (3C, 2C) the last window -- the slice ends exactly at the allocation's last element, so a buffer-descriptor range computed from C
  instead of ld returns zeros for the last rows; (C + 16, 8) the smallest legal offset.  Operands of one call take different layouts
  (and, where they have the same channel count, different pixel strides), so that a kernel using one operand's stride for another
  reads poison.  The GPU runs all three layouts of every case; the emulator runs one per case (case index % 3) and the
  256-channel cases on one ragged 256-row tile pair, as tests/test_exact_conv.py::test_dgrad_bn_backward_sums_bit_equal shrinks them.

The cases are rows of SELECT (tests/test_conv.py), at least one per kernel family, with the kernel names asserted as that file's
_check_instantiation does.  There is no tolerance in this file except in test_bn_act_bwd_on_the_halves_of_one_buffer (behind an rsqrt
and an exp: the bounds of tests/test_norm_spatial.py::test_bn_silu_fwd_bwd, unchanged).  The last test pins the operand validation of
the five conv entry points (host logic: no kernel runs).  What this file sees and the older tests do not is recorded in
profiles/strided_tests_seeded_defects.txt.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import exact_ref as E
from tests.test_conv import DTYPES, GLDS, RS128, RS64, S1, SELECT, _same, kn
from tests.test_exact_conv import BN_BWD, LD, OFF, dev_of, pow2_scale, same, same_sums, tile_hint

POISON = 64.0
LP = [torch.bfloat16, torch.float16]
OTHER = {0: 2, 1: 2, 2: 1}      # a layout whose pixel stride differs from layout L's at the same channel count (3C against C + 16)


def layout(C, L):
    assert C % 8 == 0 and C != 8, "3C and C + 16 are different multiples of 8"
    return [(3 * C, 0), (3 * C, 2 * C), (C + 16, 8)][L]


def embed(hip, t, dt, ld, off, fill, shape=None):
    """`wide[..., off:off + C]` of an (N, H, W, ld) tensor pre-filled with `fill` -- a float: that value everywhere (the poison of a
    read operand); an int: the seed of a sentinel pattern of integers in [-3, 3] (outputs).  The window holds `t` (any floating
    tensor of exactly representable values), or stays filled when t is None (`shape` then gives the window's shape)."""
    N, H, W, C = t.shape if t is not None else shape
    assert ld % 8 == 0 and off % 8 == 0 and off + C <= ld
    if isinstance(fill, float):
        wide = torch.full((N, H, W, ld), fill, dtype=dt, device=hip.device)
    else:
        wide = E.int_tensor((N, H, W, ld), -3, 3, 1.0, fill).to(dt).to(hip.device)
    if t is not None:
        wide[..., off:off + C] = t.to(device=hip.device, dtype=dt)
    v = wide[..., off:off + C]
    assert v._base is wide
    return v


def emb(hip, t, dt, L, fill, shape=None):
    C = t.shape[3] if t is not None else shape[3]
    return embed(hip, t, dt, *layout(C, L), fill, shape=shape)


def guard(*views):
    """pre-call copies of the whole buffers behind output windows"""
    return [(v, v._base.clone()) for v in views]


def slack_unchanged(guards, what):
    for v, before in guards:
        wide, C = v._base, v.shape[3]
        off = v.storage_offset() - wide.storage_offset()
        now = wide.clone()
        now[..., off:off + C] = before[..., off:off + C]
        if not torch.equal(now, before):
            raise AssertionError(f"{what}: written outside the window [{off}, {off + C}) of a {wide.shape[3]}-wide buffer: "
                                 + E.first_difference(now.cpu(), before.cpu()))


# ---- the cases: rows of SELECT by kernel family --------------------------------------------------------------------------------
FAMILIES = [
    ("stream", S1, [(2, 13, 11, 64, 64, 1, 1, 0), (1, 17, 19, 128, 128, 1, 1, 0), (2, 9, 10, 256, 256, 1, 1, 0), (1, 8, 8, 64, 24, 1, 1, 0)]),
    ("pprs", "conv_gemm_pprs_kernel", [(2, 20, 20, 256, 256, 3, 1, 1), (1, 5, 5, 64, 264, 3, 1, 1)]),
    ("rs", "conv_gemm_rs_kernel<", [(2, 12, 12, 128, 128, 3, 1, 1), (1, 9, 11, 64, 40, 3, 1, 1), (1, 9, 11, 256, 72, 3, 1, 1)]),
    ("pp", "conv_gemm_pp_kernel", [(2, 20, 20, 128, 256, 3, 2, 1), (1, 15, 15, 64, 128, 3, 2, 1), (2, 24, 24, 32, 64, 3, 2, 1)]),
    ("glds", GLDS, [(2, 20, 20, 512, 512, 1, 1, 0), (1, 12, 12, 512, 256, 1, 1, 0)]),
    ("wgrad_rs", "conv_wgrad_rs_kernel<", [(2, 24, 24, 64, 128, 3, 2, 1)]),
]
_SEL = {c[0]: c for c in SELECT}
CASES = [_SEL[c] for _, _, cs in FAMILIES for c in cs]         # KeyError: SELECT no longer has the row
_MACS = sorted(range(len(CASES)), key=lambda i: E.Problem(CASES[i][0]).M * E.Problem(CASES[i][0]).K * CASES[i][0][4])
FP32_CASES = set(_MACS[:3])
RUNS = [(i, dt) for i in range(len(CASES)) for dt in LP] + [(i, torch.float32) for i in sorted(FP32_CASES)]
_PROBLEMS = {}


def problem(case, seed=0):
    """one Problem per (geometry, seed) for the whole module: the fp64 references are computed once and shared, never modified"""
    if (case, seed) not in _PROBLEMS:
        _PROBLEMS[(case, seed)] = E.Problem(case, seed=seed)
    return _PROBLEMS[(case, seed)]


def test_every_kernel_family_is_among_the_cases():
    """the names SELECT pins for the cases of a family contain that family's kernel (forward, a dgrad class or the wgrad); the stride-2
    cases bring the four parity classes, and the weight-gradient table has its rs, tr and stride-2 row-sharing kernels"""
    for fam, needle, cs in FAMILIES:
        names = [n for c in cs for n in [_SEL[c][1]] + list(_SEL[c][2] or []) + [_SEL[c][3]]]
        assert any(needle in n for n in names), (fam, names)
    assert {RS128, RS64} <= {c[1] for c in CASES}
    kws = {c[3] for c in CASES}
    assert any(n.startswith("conv_wgrad_tr_kernel") for n in kws) and "conv_wgrad_rs_kernel<128, 64, 2, 2, 2>" in kws
    assert sum(c[0][6] == 2 and len(c[2]) == 4 for c in CASES) >= 4


def assert_names(case, kf, kd, kw, dt):
    s = case[6]
    assert _same(kn("fwd", dt, *case), kf)
    names = [kn("dgrad", dt, *case, parity_class=c) for c in range(s * s)]
    assert len(names) == len(kd) and all(_same(a, b) for a, b in zip(names, kd)), names
    assert kn("wgrad", dt, *case) == kw


def check_forward(hip, P, dt, L):
    from efficientteacher_amd import _lib, ops
    from efficientteacher_amd.flat_state import BN_SHARDS
    N, H, W, Cin, Cout, k, s, p = P.case
    yref = E.stored(P.y(), dt)
    sums = P.sums()
    ysref = E.stored(P.ys(), dt)
    hint, hint_res = tile_hint("fwd", dt, P.case), tile_hint("fwd_res", dt, P.case)
    x, w = emb(hip, P.x, dt, L, POISON), dev_of(hip, P.w, dt)
    # dense output
    same(ops.conv2d_fwd(x, w, s, p), yref, hint)
    # ... and the plain layer into a sentinel-filled slice (the guard-free store pass of interior tiles: no residual, no sums)
    out = emb(hip, None, dt, (L + 1) % 3, 100, shape=(N, P.OH, P.OW, Cout))      # (another layout than x's: Cin == Cout cases too)
    g = guard(out)
    ops.conv2d_fwd(x, w, s, p, out=out)
    same(out, yref, hint)
    slack_unchanged(g, "plain output into a slice")
    # sums set: partial rows, and for the 16-bit types the sharded accumulator
    xs, ws = emb(hip, P.xs, dt, L, POISON), dev_of(hip, P.ws, dt)
    y, st = ops.conv2d_fwd(xs, ws, s, p, want_stats=True)
    same(y, ysref, hint)
    same_sums(st.sum(0), sums, "partial rows")
    if dt != torch.float32:
        full = torch.zeros((BN_SHARDS, 2, LD), dtype=torch.float32, device=hip.device)
        y = ops.conv2d_fwd(xs, ws, s, p, shards=(full.view(-1)[OFF:], LD))
        same(y, ysref, hint)
        same_sums(full.sum(0)[:, OFF:OFF + Cout], sums, "sharded accumulator")
        tot = full.sum(0)
        tot[:, OFF:OFF + Cout] = 0
        assert torch.count_nonzero(tot) == 0, "sums added outside the layer's channel range of the accumulator"
    # full epilogue: relu(acc * 2^j + integer) + integer residual (its own pixel stride), into a sentinel-filled slice
    sc, bi = pow2_scale(Cout), E.int_tensor((Cout,), -4, 4, 1.0, P.seed + 8, torch.float32)
    ref2 = torch.relu(P.y() * sc.double() + bi.double()) + P.res_out()
    E.require_exact(4 * P.K * 9 + 4 + 3, "epilogue value")
    ref2 = E.stored(ref2, dt)
    epi = dict(scale=sc.to(hip.device), bias=bi.to(hip.device), act=ops.ACT_RELU)
    oshape = (N, P.OH, P.OW, Cout)
    res = emb(hip, P.res_out(), dt, OTHER[L], POISON)
    out = emb(hip, None, dt, L, 101, shape=oshape)
    assert res.stride(2) != out.stride(2)
    g = guard(out)
    ops.conv2d_fwd(x, w, s, p, residual=res, out=out, **epi)
    same(out, ref2, hint_res)
    slack_unchanged(g, "epilogue into a slice")
    # one-buffer forms of the eval-mode C3 and the bottleneck: the residual IS the output ...
    buf = emb(hip, P.res_out(), dt, L, 102)
    g = guard(buf)
    ops.conv2d_fwd(x, w, s, p, residual=buf, out=buf, **epi)
    same(buf, ref2, hint_res)
    slack_unchanged(g, "residual is out")
    # ... and residual = window 0, out = window 1 of one 3C-wide buffer, window 2 someone else's
    out = embed(hip, None, dt, 3 * Cout, Cout, 103, shape=oshape)
    three = out._base
    three[..., :Cout] = dev_of(hip, P.res_out(), dt)
    g = guard(out)
    ops.conv2d_fwd(x, w, s, p, residual=three[..., :Cout], out=out, **epi)
    same(out, ref2, hint_res)
    slack_unchanged(g, "residual and out in disjoint windows of one buffer")
    # any other overlap of the two is rejected on the host: nothing is launched, nothing is written
    before = three.clone()
    for r_, o_ in ((three[..., 8:8 + Cout], three[..., :Cout]), (three[..., :Cout], three[..., 8:8 + Cout])):
        with pytest.raises(_lib.EtHipError):
            ops.conv2d_fwd(x, w, s, p, residual=r_, out=o_, **epi)
    assert torch.equal(three, before)


def check_dgrad(hip, P, dt, L):
    """through the public call: a stride-2 layer is one launch per parity class (and zero_lattice_kernel where no tap reaches a
    class), all writing into the strided dx"""
    from efficientteacher_amd import ops
    N, H, W, Cin, Cout, k, s, p = P.case
    dxref = P.dx()
    dy = emb(hip, P.dy, dt, L, POISON)
    wT = ops.weight_transpose(dev_of(hip, P.w, dt))
    hint = tile_hint("dgrad", dt, P.case)
    hint_full = tile_hint("dgrad_full", dt, P.case) if s == 1 else hint
    same(ops.conv2d_dgrad(dy, wT, (H, W), s, p), E.stored(dxref, dt), hint)
    r = P.res_in()
    both = E.stored(dxref + r, dt)
    if s == 1:
        same(ops.conv2d_dgrad(dy, wT, (H, W), s, p, residual=emb(hip, r, dt, OTHER[L], POISON)), both, hint_full)
    out = emb(hip, r, dt, OTHER[L], 104)
    g = guard(out)
    ops.conv2d_dgrad(dy, wT, (H, W), s, p, out=out, accumulate=True)
    same(out, both, hint_full)
    slack_unchanged(g, "dgrad accumulate")
    out = emb(hip, None, dt, L, 105, shape=(N, H, W, Cin))
    g = guard(out)
    ops.conv2d_dgrad(dy, wT, (H, W), s, p, out=out)
    same(out, E.stored(dxref, dt), hint)
    slack_unchanged(g, "dgrad into a slice")


def check_wgrad(hip, P, dt, L):
    """conv2d_wgrad and a group of three (every item another layout, one dense): pre-filled dw += the gradient"""
    from efficientteacher_amd import ops
    N, H, W, Cin, Cout, k, s, p = P.case
    hint = tile_hint("wgrad", dt, P.case)

    def pre(seed):
        return E.int_tensor((Cout, k, k, Cin), -3, 3, 1.0, seed, torch.float32)

    def want(Q, seed):
        assert Q.dw().abs().max().item() + 3 < E.LIMIT
        return E.stored(Q.dw() + pre(seed).double(), torch.float32)
    x, dy = emb(hip, P.x, dt, L, POISON), emb(hip, P.dy, dt, OTHER[L], POISON)
    assert x.stride(2) != dy.stride(2)
    dw = pre(P.seed + 9).to(hip.device)
    ops.conv2d_wgrad(x, dy, dw, k, s, p)
    same(dw, want(P, P.seed + 9), hint)
    probs = [P, problem(P.case, 1), problem(P.case, 2)]
    lays = [(L, OTHER[L]), None, (OTHER[L], L)]
    items = []
    for i, (Q, ll) in enumerate(zip(probs, lays)):
        xi = emb(hip, Q.x, dt, ll[0], POISON) if ll else dev_of(hip, Q.x, dt)
        dyi = emb(hip, Q.dy, dt, ll[1], POISON) if ll else dev_of(hip, Q.dy, dt)
        items.append((xi, dyi, pre(50 + i).to(hip.device)))
    assert len({(a.stride(2), b.stride(2)) for a, b, _ in items}) == 3
    ops.conv2d_wgrad_grouped(items, k, s, p)
    for i, (Q, (_, _, dw)) in enumerate(zip(probs, items)):
        same(dw, want(Q, 50 + i), lambda idx, i=i: f"item {i} of 3: " + hint(idx))


@pytest.mark.parametrize("idx,dtype", RUNS, ids=[f"{CASES[i][0]}-{str(dt)[6:]}" for i, dt in RUNS])
def test_conv_on_slices_bit_equal(hip, idx, dtype):
    case, kf, kd, kw = CASES[idx]
    if dtype != torch.float32:
        assert_names(case, kf, kd, kw, dtype)        # (the fp32 parity mode has its own, smaller table)
    N, H, W, Cin = case[:4]
    if hip.emulated and Cin >= 256 and N * H * W > 17 * 17:
        case = (1, 17, 17) + case[3:]
    P = problem(case)
    for L in ([idx % 3] if hip.emulated else [0, 1, 2]):
        check_forward(hip, P, dtype, L)
        check_dgrad(hip, P, dtype, L)
        check_wgrad(hip, P, dtype, L)


@pytest.mark.parametrize("case", BN_BWD, ids=[str(c) for c in BN_BWD])
def test_dgrad_bn_backward_sums_on_slices_bit_equal(hip, case):
    """et_conv2d_dgrad_bn as tests/test_exact_conv.py::_dgrad_bn_case defines dz and both sums, with the producer's y (`bn.y`, as the
    first half of the C3 stem's y is), dy and the residual each embedded at its own pixel stride"""
    from efficientteacher_amd import ops
    N, H, W, Cin, Cout, k = case
    dtypes = DTYPES
    if hip.emulated and Cin >= 256:
        N, H, W = 1, 17, 17
        dtypes = LP
    p = k // 2
    P = problem((N, H, W, Cin, Cout, k, 1, p))
    yprod = E.int_tensor((N, H, W, Cin), -3, 3, 1.0, 61)
    scale, shift = pow2_scale(Cin), E.int_tensor((Cin,), -2, 2, 1.0, 62, torch.float32)
    for dtype in dtypes:
        wT = ops.weight_transpose(dev_of(hip, P.w, dtype))
        for L in ([BN_BWD.index(case) % 3] if hip.emulated else [0, 1, 2]):
            dy = emb(hip, P.dy, dtype, OTHER[L], POISON)
            y = emb(hip, yprod, dtype, L, POISON)
            for residual in (None, P.res_in()):
                dzref = E.stored(P.dx() + (residual if residual is not None else 0), dtype)
                assert (dzref.double().abs().reshape(-1, Cin).sum(0) * 3).max().item() < E.LIMIT
                res = embed(hip, residual, dtype, Cin + 24, 16, POISON) if residual is not None else None
                assert res is None or res.stride(2) != y.stride(2)
                for act in (ops.ACT_RELU, ops.ACT_NONE):
                    u = yprod * scale.double() + shift.double()
                    gate = (u > 0).double() if act == ops.ACT_RELU else torch.ones_like(u)
                    du = (dzref.double() * gate).reshape(-1, Cin)
                    want = torch.stack([du.sum(0), (du * yprod.reshape(-1, Cin)).sum(0)])
                    hand = ops.BnBwdSums(y, scale.to(hip.device), shift.to(hip.device), act)
                    dz = ops.conv2d_dgrad(dy, wT, (H, W), 1, p, residual=res, bn=hand)
                    same(dz, dzref, tile_hint("dgrad_full", dtype, P.case))
                    part = hand.take(dz)
                    assert part is not None
                    got = part.sum(0).cpu().double()
                    assert torch.equal(got, want), (f"BN-backward sums differ in {int((got != want).any(0).sum())} channels "
                                                    f"(layout {L}, act {act}, residual {residual is not None})")


# ---- non-GEMM kernels whose result is exact on integers: every tensor argument embedded, outputs into sentinel slices ------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 9, 11, 40), (1, 16, 16, 128), (2, 7, 5, 264)])
def test_bn_act_fwd_and_act_bwd_on_slices_bit_equal(hip, shape, dtype):
    """the exact forms of tests/test_exact_conv.py::test_bn_act_fwd_and_act_bwd_bit_equal"""
    from efficientteacher_amd import ops
    N, H, W, C = shape
    y = E.int_tensor(shape, -100, 100, 1.0, 72)
    res = E.int_tensor(shape, -3, 3, 1.0, 73)
    dz = E.int_tensor(shape, -50, 50, 1.0, 75)
    sc, sh = pow2_scale(C), E.int_tensor((C,), -4, 4, 1.0, 74, torch.float32)
    for L in (0, 1, 2):
        yv = emb(hip, y, dtype, L, POISON)
        for act in (ops.ACT_RELU, ops.ACT_NONE):
            for r in (None, res):
                v = y * sc.double() + sh.double()
                v = (torch.relu(v) if act == ops.ACT_RELU else v) + (r if r is not None else 0)
                out = emb(hip, None, dtype, (L + 1) % 3, 106, shape=shape)
                g = guard(out)
                ops.bn_act_fwd(yv, sc.to(hip.device), sh.to(hip.device), act, residual=emb(hip, r, dtype, OTHER[L], POISON) if r is not None else None, out=out)
                same(out, E.stored(v, dtype))
                slack_unchanged(g, "bn_act_fwd")
        out = emb(hip, None, dtype, L, 107, shape=shape)
        g = guard(out)
        ops.act_bwd(emb(hip, dz, dtype, OTHER[L], POISON), yv, ops.ACT_RELU, out=out)
        same(out, E.stored(dz * (y > 0), dtype))
        slack_unchanged(g, "act_bwd")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 6, 7, 40), (1, 10, 10, 128)])
def test_upsample_and_maxpool_on_slices_bit_equal(hip, shape, dtype):
    """upsample2x_fwd / _bwd (plain and accumulate) and maxpool5_fwd / _bwd (with base=): the SPPF and neck concats"""
    from efficientteacher_amd import ops
    N, H, W, C = shape
    up = (N, 2 * H, 2 * W, C)
    x = E.int_tensor(shape, -3, 3, 1.0, 78)
    dy = E.int_tensor(up, -20, 20, 1.0, 76)
    pre = E.int_tensor(shape, -20, 20, 1.0, 77)
    g_, base = E.int_tensor(shape, -20, 20, 1.0, 79), E.int_tensor(shape, -20, 20, 1.0, 80)
    pref = F.max_pool2d(x.permute(0, 3, 1, 2), 5, 1, 2).permute(0, 2, 3, 1).contiguous()
    n_, y_, x_, c_ = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    for L in (0, 1, 2):
        xv = emb(hip, x, dtype, L, POISON)
        out = emb(hip, None, dtype, OTHER[L], 108, shape=up)
        g = guard(out)
        ops.upsample2x_fwd(xv, out=out)
        same(out, E.stored(x.repeat_interleave(2, 1).repeat_interleave(2, 2), dtype))
        slack_unchanged(g, "upsample2x_fwd")
        dyv = emb(hip, dy, dtype, L, POISON)
        fold = dy.reshape(N, H, 2, W, 2, C).sum((2, 4))
        out = emb(hip, None, dtype, OTHER[L], 109, shape=shape)
        g = guard(out)
        ops.upsample2x_bwd(dyv, out=out)
        same(out, E.stored(fold, dtype))
        slack_unchanged(g, "upsample2x_bwd")
        out = emb(hip, pre, dtype, OTHER[L], 110)
        g = guard(out)
        ops.upsample2x_bwd(dyv, out=out, accumulate=True)
        same(out, E.stored(pre + fold, dtype))
        slack_unchanged(g, "upsample2x_bwd accumulate")
        # max pool 5x5 stride 1 pad 2; the routing of ties is pinned through the kernel's own index map, as in tests/test_exact_conv.py
        out = emb(hip, None, dtype, (L + 1) % 3, 111, shape=shape)
        g = guard(out)
        _, idx = ops.maxpool5_fwd(xv, out=out)
        same(out, E.stored(pref, dtype))
        slack_unchanged(g, "maxpool5_fwd")
        ii = idx.cpu().long()
        assert int(ii.max()) < 25
        sy, sx = y_ + ii // 5 - 2, x_ + ii % 5 - 2
        assert bool(((sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)).all())
        assert torch.equal(x[n_, sy, sx, c_], pref), "the index map does not point at a maximum of its window"
        want = base.clone()
        want.index_put_((n_.reshape(-1), sy.reshape(-1), sx.reshape(-1), c_.reshape(-1)), g_.reshape(-1), accumulate=True)
        out = emb(hip, None, dtype, L, 112, shape=shape)
        g = guard(out)
        ops.maxpool5_bwd(emb(hip, g_, dtype, (L + 1) % 3, POISON), idx, base=emb(hip, base, dtype, OTHER[L], POISON), out=out)
        same(out, E.stored(want, dtype))
        slack_unchanged(g, "maxpool5_bwd")


# ---- bn_act_bwd on the two halves of one y / one dy (behind an rsqrt and an exp: tolerance, the existing bounds) -----------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 7, 9, 32), (2, 40, 40, 24)])
def test_bn_act_bwd_on_the_halves_of_one_buffer(hip, shape, dtype):
    """As C3StemFn.backward calls it: y is (N, H, W, 2C), each half has its own BatchNorm, its dz arrives as a slice of a wider
    gradient and its result goes into its half of ONE dy.  Both forms of the reduce pass (partial rows, sharded accumulator) against
    torch autograd in fp64 with the bounds of test_bn_silu_fwd_bwd; the other half of dy (a sentinel, then the first half's result)
    stays bit-unchanged; and dy, dgamma and dbeta of a half are bit-equal whatever the neighbour half of y and the slack around dz
    hold -- on integer data, where the sums are exact in any order (see below), in both forms."""
    from efficientteacher_amd import ops
    from efficientteacher_amd.flat_state import BN_SHARDS
    from tests.test_norm_spatial import _mk, _tol
    N, H, W, C = shape
    x = _mk(hip, (N, H, W, 16), dtype, 1)
    w = _mk(hip, (2 * C, 1, 1, 16), dtype, 2, 0.3)
    y, stats = ops.conv2d_fwd(x, w, 1, 0, want_stats=True)
    gamma = _mk(hip, (2 * C,), torch.float32, 3, 0.2) + 1
    beta = _mk(hip, (2 * C,), torch.float32, 4, 0.1)
    scale, shift, mean, invstd = ops.bn_finalize(stats, N * H * W, gamma, beta, 1e-3, 0.03)
    dzs = [_mk(hip, shape, dtype, 6), _mk(hip, shape, dtype, 7)]
    yr = F.conv2d(x.double().cpu().permute(0, 3, 1, 2), w.double().cpu().permute(0, 3, 1, 2)).requires_grad_(True)
    bn = torch.nn.BatchNorm2d(2 * C, eps=1e-3, momentum=0.03).double()
    with torch.no_grad():
        bn.weight.copy_(gamma.cpu()); bn.bias.copy_(beta.cpu())
    bn.train()
    F.silu(bn(yr)).backward(torch.cat(dzs, 3).double().cpu().permute(0, 3, 1, 2))
    ref = yr.grad.permute(0, 2, 3, 1)

    def run(h, form, ybuf, dzh, dz_fill, dy, aff, act):
        """one half: dz embedded in `dz_fill`, y and out the half's windows of ybuf / dy; aff = (scale, shift, mean, invstd) of 2C channels"""
        sl = slice(h * C, (h + 1) * C)
        dz = embed(hip, dzh, dtype, *layout(C, (h + 1) % 3), dz_fill)
        dg, db = torch.zeros(C, device=hip.device), torch.zeros(C, device=hip.device)
        sh = (torch.zeros((BN_SHARDS, 2, LD), dtype=torch.float32, device=hip.device).view(-1)[OFF:], LD) if form == "shards" else None
        ops.bn_act_bwd(dz, ybuf[..., sl], gamma[sl], *(a[sl] for a in aff), act, dg, db, out=dy[..., sl], shards=sh)
        return dg, db

    for form in ("rows", "shards"):
        dy = E.int_tensor((N, H, W, 2 * C), -3, 3, 1.0, 113).to(dtype).to(hip.device)
        for h in (0, 1):
            sl, other = slice(h * C, (h + 1) * C), slice((1 - h) * C, (2 - h) * C)
            before = dy.clone()
            dg, db = run(h, form, y, dzs[h], POISON, dy, (scale, shift, mean, invstd), ops.ACT_SILU)
            assert torch.equal(dy[..., other], before[..., other]), f"{form}: half {h} wrote into the other half of dy"
            r = ref[..., sl]
            err = (dy[..., sl].double().cpu() - r).abs().max().item()
            print(f"{form} half {h}: max |dy - ref| = {err:.3e}, bound {_tol(dtype) * max(1.0, r.abs().max().item()) * 2:.3e}")
            assert err <= _tol(dtype) * max(1.0, r.abs().max().item()) * 2, err
            assert torch.allclose(dg.cpu().double(), bn.weight.grad[sl], rtol=_tol(dtype) * 10, atol=_tol(dtype) * 20)
            assert torch.allclose(db.cpu().double(), bn.bias.grad[sl], rtol=_tol(dtype) * 10, atol=_tol(dtype) * 20)
    # Independence from the neighbours, bit for bit.  The block reduction of the reduce pass (bn_act_bwd_reduce_kernel) adds with fp32
    # LDS atomics, whose order differs from run to run on the GPU: on real-valued data neither form is bit-deterministic, so two
    # runs need not agree in the last bit whatever the neighbours hold.  On integer data the sums are exact in any order: y and dz integers in [-3, 3], ReLU behind a power-of-two scale and an integer shift (an exact gate), an integer mean
    # and a power-of-two invstd.  Then dbeta = sum du and dgamma = invstd * sum du * (y - mean) are integers times a power of two
    # below 2**24, EQUAL to the fp64 sums, and dy -- one deterministic expression of them -- is bit-equal between the two poisons.
    yi = E.int_tensor((N, H, W, 2 * C), -3, 3, 1.0, 114)
    dzi = [E.int_tensor(shape, -3, 3, 1.0, 115), E.int_tensor(shape, -3, 3, 1.0, 116)]
    sc2, sh2 = pow2_scale(2 * C), E.int_tensor((2 * C,), -2, 2, 1.0, 117, torch.float32)
    mu2, is2 = E.int_tensor((2 * C,), -2, 2, 1.0, 118, torch.float32), pow2_scale(2 * C).flip(0).contiguous()
    aff2 = tuple(t.to(hip.device) for t in (sc2, sh2, mu2, is2))
    for form in ("rows", "shards"):
        for h in (0, 1):
            sl, other = slice(h * C, (h + 1) * C), slice((1 - h) * C, (2 - h) * C)
            du = dzi[h] * (yi[..., sl] * sc2[sl].double() + sh2[sl].double() > 0)
            want_db = du.reshape(-1, C).sum(0)
            want_dg = (du * (yi[..., sl] - mu2[sl].double())).reshape(-1, C).sum(0) * is2[sl].double()
            assert (du.abs() * 5).reshape(-1, C).sum(0).max().item() * 4 < E.LIMIT
            got = []
            for y_fill, dz_fill in ((POISON, POISON), (-37.0, -5.0)):
                ybuf = dev_of(hip, yi, dtype).clone()
                ybuf[..., other] = y_fill
                dy = E.int_tensor((N, H, W, 2 * C), -3, 3, 1.0, 119).to(dtype).to(hip.device)
                before = dy.clone()
                dg, db = run(h, form, ybuf, dzi[h], dz_fill, dy, aff2, ops.ACT_RELU)
                assert torch.equal(dy[..., other], before[..., other]), f"{form}: half {h} wrote into the other half of dy"
                assert torch.equal(db.cpu().double(), want_db), f"{form} half {h}: dbeta is not the exact sum (neighbour fill {y_fill})"
                assert torch.equal(dg.cpu().double(), want_dg), f"{form} half {h}: dgamma is not the exact sum (neighbour fill {y_fill})"
                got.append((dy[..., sl].clone(), dg, db))
            for a, b, what in zip(got[0], got[1], ("dy", "dgamma", "dbeta")):
                assert torch.equal(a, b), f"{form} half {h}: {what} depends on the contents of the neighbour half"


# ---- operand validation of the five conv entry points (host logic: must never reach a launch) --------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("how", ["window at half a vector", "pixel stride C + half a vector", "pixel stride below C"])
def test_conv_entry_points_reject_unaligned_or_overlapping_pixels(hip, how, dtype):
    """ops._nhwc lets `wide[..., 4:4 + C]` and an ld = C + 4 view through (bf16; 2 for fp32): et_conv2d_fwd, _dgrad, _dgrad_bn, _wgrad
    and _wgrad_grouped return -2 for each operand in turn -- a base that is not 16-byte aligned, a pixel stride that is not whole
    16-byte vectors, a pixel stride below the channel count -- before anything is launched (the same calls on the good operands run)"""
    from efficientteacher_amd import _lib, ops
    N, H, W, Cin, Cout, k, s, p = 1, 6, 5, 16, 24, 3, 1, 1
    half = 2 if dtype == torch.float32 else 4

    def good(C):
        return torch.zeros((N, H, W, C), dtype=dtype, device=hip.device)

    def bad(C):
        if how == "window at half a vector":
            return torch.zeros((N, H, W, C + 2 * half), dtype=dtype, device=hip.device)[..., half:half + C]
        if how == "pixel stride C + half a vector":
            return torch.zeros((N, H, W, C + half), dtype=dtype, device=hip.device)[..., :C]
        ld = C - 2 * half
        return torch.zeros((N * H * W * C,), dtype=dtype, device=hip.device).as_strided((N, H, W, C), (H * W * ld, W * ld, ld, 1))
    w = torch.zeros((Cout, k, k, Cin), dtype=dtype, device=hip.device)
    wT = ops.weight_transpose(w)
    sc = torch.ones(Cin, device=hip.device)
    dw = lambda: torch.zeros((Cout, k, k, Cin), dtype=torch.float32, device=hip.device)
    bn = lambda t: ops.BnBwdSums(t, sc, sc, ops.ACT_NONE)
    calls = {
        "fwd x": lambda b: ops.conv2d_fwd(b(Cin), w, s, p),
        "fwd out": lambda b: ops.conv2d_fwd(good(Cin), w, s, p, out=b(Cout)),
        "fwd residual": lambda b: ops.conv2d_fwd(good(Cin), w, s, p, residual=b(Cout)),
        "dgrad dy": lambda b: ops.conv2d_dgrad(b(Cout), wT, (H, W), s, p),
        "dgrad out": lambda b: ops.conv2d_dgrad(good(Cout), wT, (H, W), s, p, out=b(Cin)),
        "dgrad residual": lambda b: ops.conv2d_dgrad(good(Cout), wT, (H, W), s, p, residual=b(Cin)),
        "dgrad_bn dy": lambda b: ops.conv2d_dgrad(b(Cout), wT, (H, W), s, p, bn=bn(good(Cin))),
        "dgrad_bn bn.y": lambda b: ops.conv2d_dgrad(good(Cout), wT, (H, W), s, p, bn=bn(b(Cin))),
        "wgrad x": lambda b: ops.conv2d_wgrad(b(Cin), good(Cout), dw(), k, s, p),
        "wgrad dy": lambda b: ops.conv2d_wgrad(good(Cin), b(Cout), dw(), k, s, p),
        "grouped x": lambda b: ops.conv2d_wgrad_grouped([(good(Cin), good(Cout), dw()), (b(Cin), good(Cout), dw())], k, s, p),
        "grouped dy": lambda b: ops.conv2d_wgrad_grouped([(good(Cin), good(Cout), dw()), (good(Cin), b(Cout), dw())], k, s, p),
    }
    for what, call in calls.items():
        t = bad(Cin)
        ops._nhwc(t)                                   # the Python side does not object
        try:
            call(bad)
        except _lib.EtHipError:
            continue
        raise AssertionError(f"{what}: accepted ({how}, {dtype})")
    for call in calls.values():
        call(lambda C: good(C))
