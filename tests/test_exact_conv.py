"""Zero-tolerance tier: the conv kernels (forward, BatchNorm statistics in both forms, dgrad, wgrad) and the non-GEMM kernels whose
result is exact on integers, BIT-EQUAL to an fp64 reference on small-integer operands (tests/exact_ref.py: every product and partial
sum stays below 2**24, so fp32 accumulation is exact in any order and the 16-bit store is one deterministic rounding of an integer).
A single dropped, duplicated or misplaced element anywhere fails `torch.equal`; there is no tolerance in this file.  The only numeric
conditions are the exactness preconditions and the coverage conditions of tests/exact_ref.py, evaluated on the reference before a
kernel output is looked at.

This file is the test-size tier (emulator and GPU, fixture `hip`) over every entry of CASES and SELECT of tests/test_conv.py;
tests/test_exact_fullsize.py runs the same comparisons at the bench's own shapes and batches on the GPU.  What this tier sees and the
tolerance tests do not is recorded in profiles/exact_tests_seeded_defects.txt (four seeded one-line defects).

It cannot pin anything behind an rsqrt, an exp or a non-power-of-two scale (BatchNorm normalise / backward apply, SiLU, losses):
those keep their tolerance tests.
"""
import re

import pytest
import torch

from tests import exact_ref as E
from tests.test_conv import CASES, DTYPES, FLAT_TWIN_CASES, PPRS_CASES, SELECT, STREAM_CASES

LD, OFF = 1040, 264        # sharded accumulator: row length / this layer's first channel inside it (as a BN layer inside the arena)


def tile_hint(op, dt, case):
    """-> f(index): which tile of the kernel the library launches for (op, case) a differing output index falls in.  A stride-2 dgrad
    is one launch per parity class of the input pixel: the class of the differing pixel selects the name."""
    from efficientteacher_amd import ops
    N, H, W, Cin, Cout, k, s, p = case

    def tile(name):
        a = [int(v) for v in re.findall(r", (\d+)", name)]
        if name.startswith("conv1x1_stream"):      # <T, KC, WN, TN, WM, TMW, NS, WGS, FULL>: 32 * WM * TMW rows, all channels in one tile
            return 32 * a[3] * a[4], 1 << 30, ""
        if len(a) >= 2:                            # <T, BM, BN, ...>
            return a[0], a[1], ""
        return 256, 256, " (256 x 256 tile: the name does not carry it)"

    def f(idx):
        n, y, x, c = idx
        if op == "wgrad":
            return f"dw[cout {n}, tap ({y}, {x}), cin {c}] of {ops.kernel_name(op, dt, *case)}"
        if op.startswith("dgrad") and s == 2:
            pc = (y % 2) * 2 + x % 2
            name = ops.kernel_name(op, dt, *case, parity_class=pc)
            qw, qh = (W - x % 2 + 1) // 2, (H - y % 2 + 1) // 2
            pix = (n * qh + y // 2) * qw + x // 2
            bm, bn, note = tile(name)
            return f"(n, y, x, c) = {idx}: parity class {pc}, class pixel {pix}, row tile {pix // bm} / column tile {c // bn} of {name}{note}"
        name = ops.kernel_name(op, dt, *case)
        oh, ow = (H, W) if op.startswith("dgrad") else E.out_hw(H, W, k, s, p)
        pix = (n * oh + y) * ow + x
        bm, bn, note = tile(name)
        return f"(n, y, x, c) = {idx}: pixel {pix}, row tile {pix // bm} / column tile {c // bn} of {name}{note}"
    return f


def same(got, want, hint=""):
    got = got.detach().cpu() if got.device.type == "cpu" else got
    want = want.to(got.device)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        raise AssertionError(E.first_difference(got, want, hint))


def same_sums(st2, sums, what):
    """st2: (2, C) fp32 sums of the kernel; sums: int64 (sum, sum of squares) of the reference"""
    got = st2.detach().cpu().to(torch.float64)
    want = torch.stack(sums).to(torch.float64)
    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).any(0)).reshape(-1)
        c = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {got.shape[1]} channels differ; first channel {c}: got {got[:, c].tolist()} want {want[:, c].tolist()}")


def dev_of(hip, t, dt):
    return t.to(dt).to(hip.device)        # the operands are integers of magnitude <= 4: exact in every storage type


def pow2_scale(C):
    return torch.tensor([0.5, 1.0, 2.0, 4.0], dtype=torch.float32).repeat((C + 3) // 4)[:C].contiguous()


def check_forward(hip, P, dt, stats_forms=("rows", "shards")):
    """dense y; sums-set y + statistics as partial rows and as the sharded accumulator; residual + ReLU + power-of-two scale + integer
    bias into a channel slice"""
    from efficientteacher_amd import ops
    from efficientteacher_amd.flat_state import BN_SHARDS
    N, H, W, Cin, Cout, k, s, p = P.case
    yref = E.stored(P.y(), dt)                                       # preconditions + coverage first
    sums = P.sums()
    ysref = E.stored(P.ys(), dt)
    x, w = dev_of(hip, P.x, dt), dev_of(hip, P.w, dt)
    same(ops.conv2d_fwd(x, w, s, p), yref, tile_hint("fwd", dt, P.case))
    xs, ws = dev_of(hip, P.xs, dt), dev_of(hip, P.ws, dt)
    if "rows" in stats_forms:
        y, st = ops.conv2d_fwd(xs, ws, s, p, want_stats=True)
        same(y, ysref, tile_hint("fwd", dt, P.case))
        same_sums(st.sum(0), sums, "partial rows")
    if "shards" in stats_forms and dt != torch.float32:              # the fp32 parity mode keeps the partial rows
        full = torch.zeros((BN_SHARDS, 2, LD), dtype=torch.float32, device=hip.device)
        y = ops.conv2d_fwd(xs, ws, s, p, shards=(full.view(-1)[OFF:], LD))
        same(y, ysref, tile_hint("fwd", dt, P.case))
        same_sums(full.sum(0)[:, OFF:OFF + Cout], sums, "sharded accumulator")
        assert torch.count_nonzero(full[:, :, :OFF]) == 0 and torch.count_nonzero(full[:, :, OFF + Cout:]) == 0
    # epilogue: relu(acc * 2^j + integer) + integer residual, into a slice of a wider buffer
    sc, bi = pow2_scale(Cout), E.int_tensor((Cout,), -4, 4, 1.0, P.seed + 8, torch.float32)
    ref2 = torch.relu(P.y() * sc.double() + bi.double()) + P.res_out()
    E.require_exact(4 * P.K * 9 + 4 + 3, "epilogue value")
    ref2 = E.stored(ref2, dt)
    wide = torch.zeros((N, P.OH, P.OW, Cout + 16), dtype=dt, device=hip.device)
    ops.conv2d_fwd(x, w, s, p, scale=sc.to(hip.device), bias=bi.to(hip.device), act=ops.ACT_RELU, residual=dev_of(hip, P.res_out(), dt),
                   out=wide[..., 8:8 + Cout])
    if k != 6:                                                       # (the stem kernel declines residuals: the generic kernel runs)
        same(wide[..., 8:8 + Cout], ref2, tile_hint("fwd_res", dt, P.case))
    else:
        same(wide[..., 8:8 + Cout], ref2)
    assert torch.count_nonzero(wide[..., :8]) == 0 and torch.count_nonzero(wide[..., 8 + Cout:]) == 0


def check_dgrad(hip, P, dt):
    """plain (every parity class of a stride-2 layer through the public call), + residual, accumulate into a pre-filled integer out,
    output into a channel slice.  The fused residual is a stride-1 feature: et_conv2d_dgrad REJECTS residual= at stride 2 (asserted);
    a stride-2 layer adds into an existing gradient through accumulate=True, which is compared."""
    from efficientteacher_amd import ops
    N, H, W, Cin, Cout, k, s, p = P.case
    dxref = P.dx()
    dy = dev_of(hip, P.dy, dt)
    wT = ops.weight_transpose(dev_of(hip, P.w, dt))
    same(wT, E.stored(P.w.permute(3, 1, 2, 0).contiguous(), dt))
    hint = tile_hint("dgrad", dt, P.case)
    same(ops.conv2d_dgrad(dy, wT, (H, W), s, p), E.stored(dxref, dt), hint)
    r = P.res_in()
    both = E.stored(dxref + r, dt)
    hint_full = tile_hint("dgrad_full", dt, P.case) if s == 1 else hint
    if s == 1:
        same(ops.conv2d_dgrad(dy, wT, (H, W), s, p, residual=dev_of(hip, r, dt)), both, hint_full)
    else:
        from efficientteacher_amd import _lib
        with pytest.raises(_lib.EtHipError):
            ops.conv2d_dgrad(dy, wT, (H, W), s, p, residual=dev_of(hip, r, dt))
    out = dev_of(hip, r, dt).clone()
    ops.conv2d_dgrad(dy, wT, (H, W), s, p, out=out, accumulate=True)
    same(out, both, hint_full)
    wide = torch.zeros((N, H, W, Cin + 16), dtype=dt, device=hip.device)
    ops.conv2d_dgrad(dy, wT, (H, W), s, p, out=wide[..., 8:8 + Cin])
    same(wide[..., 8:8 + Cin], E.stored(dxref, dt), hint)
    assert torch.count_nonzero(wide[..., :8]) == 0 and torch.count_nonzero(wide[..., 8 + Cin:]) == 0


def check_wgrad(hip, P, dt):
    """conv2d_wgrad ACCUMULATES: into a pre-filled integer dw"""
    from efficientteacher_amd import ops
    N, H, W, Cin, Cout, k, s, p = P.case
    dwref = P.dw()
    pre = E.int_tensor((Cout, k, k, Cin), -3, 3, 1.0, P.seed + 9, torch.float32)
    assert dwref.abs().max().item() + 3 < E.LIMIT
    dw = pre.clone().to(hip.device)
    ops.conv2d_wgrad(dev_of(hip, P.x, dt), dev_of(hip, P.dy, dt), dw, k, s, p)
    same(dw, E.stored(dwref + pre.double(), torch.float32), tile_hint("wgrad", dt, P.case))


def check_case(hip, case, dt, dgrad=True, wgrad=True):
    P = E.Problem(case)
    check_forward(hip, P, dt)
    if dgrad:
        check_dgrad(hip, P, dt)
    if wgrad:
        check_wgrad(hip, P, dt)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_cases_bit_equal(hip, case, dtype):
    N, H, W, Cin, Cout, k, s, p = case
    check_case(hip, case, dtype, dgrad=(Cin % 8 == 0 and Cout % 8 == 0 and k != 6), wgrad=(Cout % 8 == 0))


@pytest.mark.parametrize("case,kf,kd,kw", SELECT, ids=[str(c[0]) for c in SELECT])
def test_bench_instantiations_bit_equal(hip, case, kf, kd, kw):
    """every instantiation the bench launches (the table of tests/test_conv.py, whose names that file pins).  bf16 at every size; fp16 and
    fp32 too on the GPU, and on the emulator for the cases below 6e7 multiply-adds (the rule tests/test_conv.py uses for its fp16
    table: the small cases cover every kernel family)."""
    N, H, W, Cin, Cout, k = case[:6]
    dts = DTYPES if not (hip.emulated and N * H * W * Cin * Cout * k * k > 6e7) else [torch.bfloat16]
    for dt in dts:
        check_case(hip, case, dt, dgrad=kd is not None, wgrad=kw is not None)


_TWINS = {str(c[0]): c for c in PPRS_CASES + FLAT_TWIN_CASES}


@pytest.mark.parametrize("case", [c[0] for c in _TWINS.values()], ids=list(_TWINS))
def test_flat_address_twins_bit_equal(hip, case, monkeypatch):
    """ET_CONV_BUF_DMA=0: the flat-address twins of the row-shift, stream and 1x1 weight-gradient kernels, on the cases
    test_row_shift_flat_address_twins / test_stream_and_1x1_wgrad_flat_address_twins use"""
    monkeypatch.setenv("ET_CONV_BUF_DMA", "0")
    check_case(hip, case, torch.bfloat16)


@pytest.mark.parametrize("dma_late,seed", [(1, 3), (0, 5), (1, 11)])
def test_bit_equal_under_adversarial_schedules(emu, dma_late, seed, monkeypatch):
    """the cases of test_lds_dma_pipelines_under_adversarial_schedules (its re-staged stem problem included) under the emulator's
    race-exposing modes"""
    emu.configure(dma_late, seed)
    for case, kf, kd, kw in (SELECT[0], SELECT[1], SELECT[4], SELECT[8], SELECT[3], SELECT[5]):
        check_case(emu, case, torch.bfloat16)
    monkeypatch.setenv("ET_CONV_STEM_WGS", "2")          # 6 tiles on 2 persistent workgroups: the single patch buffer is re-staged
    check_forward(emu, E.Problem((1, 20, 300, 8, 48, 6, 2, 2)), torch.bfloat16)


@pytest.mark.parametrize("wgs", [1, 3])
@pytest.mark.parametrize("dma_late,seed", [(1, 3), (0, 5), (1, 11)])
def test_stream_kernel_tile_loop_bit_equal(emu, dma_late, seed, wgs, monkeypatch):
    """conv1x1_stream_kernel with a grid of 1 / 3 persistent workgroups (the cases and schedules of
    test_stream_kernel_tile_loop_under_adversarial_schedules): every workgroup walks several row tiles and its statistics accumulate
    over them -- a tile visited twice or left out changes y or a sum by an integer"""
    monkeypatch.setenv("ET_CONV_S1_WGS", str(wgs))
    emu.configure(dma_late, seed)
    for case, kf, kd, kw in STREAM_CASES:
        check_case(emu, case, torch.bfloat16, wgrad=False)


GROUPED = [((2, 10, 10, 32, 48, 3, 1, 1), 2), ((2, 10, 10, 32, 48, 3, 1, 1), 3), ((2, 12, 12, 64, 128, 1, 1, 0), 3),
           ((1, 10, 10, 256, 256, 3, 1, 1), 8), ((1, 10, 10, 256, 256, 3, 2, 1), 8), ((2, 24, 24, 64, 128, 3, 2, 1), 2)]


@pytest.mark.parametrize("case,n", GROUPED, ids=[f"{c}x{n}" for c, n in GROUPED])
def test_wgrad_grouped_bit_equal(hip, case, n):
    """conv2d_wgrad_grouped with 2, 3 and 8 items (one of them a channel slice of a wider buffer): each pre-filled dw += its own
    gradient.  bf16 and fp16; the eight-item 256-channel groups run in bf16 only on the emulator (the GPU runs both)."""
    from efficientteacher_amd import ops
    N, H, W, Cin, Cout, k, s, p = case
    probs = [E.Problem(case, seed=i + 1) for i in range(n)]
    for dtype in ([torch.bfloat16] if (hip.emulated and n == 8) else [torch.bfloat16, torch.float16]):
        items, refs = [], []
        for i, P in enumerate(probs):
            x = dev_of(hip, P.x, dtype)
            if i == 1:
                wide = torch.ones((N, H, W, Cin + 16), dtype=dtype, device=hip.device)
                wide[..., 8:8 + Cin] = x
                x = wide[..., 8:8 + Cin]
            pre = E.int_tensor((Cout, k, k, Cin), -3, 3, 1.0, 50 + i, torch.float32)
            refs.append(E.stored(P.dw() + pre.double(), torch.float32))
            items.append((x, dev_of(hip, P.dy, dtype), pre.clone().to(hip.device)))
        ops.conv2d_wgrad_grouped(items, k, s, p)
        for i, ((_, _, dw), ref) in enumerate(zip(items, refs)):
            same(dw, ref, lambda idx, i=i: f"{dtype} item {i} of {n}: " + tile_hint("wgrad", dtype, case)(idx))


BN_BWD = [(2, 12, 12, 64, 40, 3), (2, 20, 20, 256, 256, 3), (3, 10, 10, 32, 128, 1), (2, 9, 11, 256, 256, 1), (1, 13, 13, 128, 128, 1), (2, 9, 9, 64, 64, 1)]


@pytest.mark.parametrize("case", BN_BWD, ids=[str(c) for c in BN_BWD])
def test_dgrad_bn_backward_sums_bit_equal(hip, case):
    """et_conv2d_dgrad_bn (the cases of test_dgrad_with_fused_bn_backward_sums), activation ReLU / none.  The kernel's formula
    (conv_epilogue_act, `bn_bwd_sums`): u = y * scale + shift; gate = (u > 0) for ReLU, 1 for none; du = dz * gate with dz the value
    AS STORED (rounded to the storage type); sums of du and du * y.  With y an integer of magnitude <= 3, scale a power of two and
    shift an integer, u is an exact dyadic number, the gate is exact, du and du * y are integers: pinned are dz (bit-equal) and
    BOTH sums (equal to the int64 sums over the stored dz), provided sum |dz| * 3 < 2**24 per channel (asserted on the reference).
    SiLU's gate is behind an exp: not pinned here.  All three storage types; on the emulator the 256-channel cases run one ragged
    256-row tile pair in the two 16-bit types (fp32 never selects the 256-row tiles), the GPU runs the full cases in all three."""
    N, H, W, Cin, Cout, k = case
    dtypes = DTYPES
    if hip.emulated and Cin >= 256:
        N, H, W = 1, 17, 17
        dtypes = [torch.bfloat16, torch.float16]
    for dtype in dtypes:
        _dgrad_bn_case(hip, (N, H, W, Cin, Cout, k), dtype)


def _dgrad_bn_case(hip, case, dtype):
    from efficientteacher_amd import ops
    N, H, W, Cin, Cout, k = case
    p = k // 2
    P = E.Problem((N, H, W, Cin, Cout, k, 1, p))
    dy = dev_of(hip, P.dy, dtype)
    wT = ops.weight_transpose(dev_of(hip, P.w, dtype))
    yprod = E.int_tensor((N, H, W, Cin), -3, 3, 1.0, 61)
    scale, shift = pow2_scale(Cin), E.int_tensor((Cin,), -2, 2, 1.0, 62, torch.float32)
    for residual in (None, P.res_in()):
        dzref = E.stored(P.dx() + (residual if residual is not None else 0), dtype)
        for act in (ops.ACT_RELU, ops.ACT_NONE):
            u = yprod * scale.double() + shift.double()
            gate = (u > 0).double() if act == ops.ACT_RELU else torch.ones_like(u)
            du = (dzref.double() * gate).reshape(-1, Cin)
            assert (dzref.double().abs().reshape(-1, Cin).sum(0) * 3).max().item() < E.LIMIT
            want = torch.stack([du.sum(0), (du * yprod.reshape(-1, Cin)).sum(0)])
            hand = ops.BnBwdSums(dev_of(hip, yprod, dtype), scale.to(hip.device), shift.to(hip.device), act)
            dz = ops.conv2d_dgrad(dy, wT, (H, W), 1, p, residual=dev_of(hip, residual, dtype) if residual is not None else None, bn=hand)
            same(dz, dzref, tile_hint("dgrad_full", dtype, P.case))
            part = hand.take(dz)
            assert part is not None
            got = part.sum(0).cpu().double()
            assert torch.equal(got, want), f"BN-backward sums differ in {int((got != want).any(0).sum())} channels (act {act}, residual {residual is not None})"


# ---- non-GEMM kernels whose result is exact on integers -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 9, 11, 256), (1, 7, 5, 24), (3, 20, 20, 64)])
def test_colsum_bit_equal(hip, shape, dtype):
    from efficientteacher_amd import ops
    N, H, W, C = shape
    wide = E.int_tensor((N, H, W, C + 16), -3, 3, 1.0, 71)
    x = dev_of(hip, wide, dtype)[..., 8:8 + C]
    out = torch.full((C,), 5.0, dtype=torch.float32, device=hip.device)
    ops.colsum(x, out)
    same(out, (wide[..., 8:8 + C].reshape(-1, C).sum(0) + 5).float())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 9, 11, 40), (1, 16, 16, 128), (2, 7, 5, 264)])
def test_bn_act_fwd_and_act_bwd_bit_equal(hip, shape, dtype):
    """et_bn_act_fwd with a power-of-two scale, an integer shift, ReLU and an integer residual, in and out of channel slices;
    et_act_bwd (ReLU) on integer gradients"""
    from efficientteacher_amd import ops
    N, H, W, C = shape
    y = E.int_tensor(shape, -100, 100, 1.0, 72)
    res = E.int_tensor(shape, -3, 3, 1.0, 73)
    sc, sh = pow2_scale(C), E.int_tensor((C,), -4, 4, 1.0, 74, torch.float32)
    yw = torch.zeros((N, H, W, C + 16), dtype=dtype, device=hip.device)
    yw[..., 8:8 + C] = dev_of(hip, y, dtype)
    outw = torch.zeros((N, H, W, C + 8), dtype=dtype, device=hip.device)
    for act in (ops.ACT_RELU, ops.ACT_NONE):
        for r in (None, res):
            v = y * sc.double() + sh.double()
            v = (torch.relu(v) if act == ops.ACT_RELU else v) + (r if r is not None else 0)
            outw.zero_()
            ops.bn_act_fwd(yw[..., 8:8 + C], sc.to(hip.device), sh.to(hip.device), act, residual=dev_of(hip, r, dtype) if r is not None else None,
                           out=outw[..., :C])
            same(outw[..., :C], E.stored(v, dtype))
            assert torch.count_nonzero(outw[..., C:]) == 0
    dz = E.int_tensor(shape, -50, 50, 1.0, 75)
    got = ops.act_bwd(dev_of(hip, dz, dtype), dev_of(hip, y, dtype), ops.ACT_RELU)
    same(got, E.stored(dz * (y > 0), dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 6, 7, 40), (1, 10, 10, 128)])
def test_upsample_bwd_accumulate_and_maxpool_bwd_base_bit_equal(hip, shape, dtype):
    """et_upsample2x_bwd with accumulate (out += the four gradients of a pixel) and et_maxpool5_bwd with base= on integer gradients:
    the input has many ties (integers in [-3, 3]), so the routing of a tie is pinned through the kernel's own index map"""
    from efficientteacher_amd import ops
    N, H, W, C = shape
    dy = E.int_tensor((N, 2 * H, 2 * W, C), -20, 20, 1.0, 76)
    pre = E.int_tensor(shape, -20, 20, 1.0, 77)
    out = dev_of(hip, pre, dtype).clone()
    ops.upsample2x_bwd(dev_of(hip, dy, dtype), out=out, accumulate=True)
    want = pre + dy.reshape(N, H, 2, W, 2, C).sum((2, 4))
    same(out, E.stored(want, dtype))
    same(ops.upsample2x_bwd(dev_of(hip, dy, dtype)), E.stored(want - pre, dtype))
    # max pool 5x5 stride 1 pad 2: idx (uint8) is the window position of the maximum the forward chose
    x = E.int_tensor(shape, -3, 3, 1.0, 78)
    pooled, idx = ops.maxpool5_fwd(dev_of(hip, x, dtype))
    ref = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 5, 1, 2).permute(0, 2, 3, 1)
    same(pooled, E.stored(ref.contiguous(), dtype))
    g = E.int_tensor(shape, -20, 20, 1.0, 79)
    base = E.int_tensor(shape, -20, 20, 1.0, 80)
    ii = idx.cpu().long()
    assert int(ii.max()) < 25
    n_, y_, x_, c_ = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    sy, sx = y_ + ii // 5 - 2, x_ + ii % 5 - 2
    assert bool(((sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)).all())
    assert torch.equal(x[n_, sy, sx, c_], ref), "the index map does not point at a maximum of its window"
    want = base.clone()
    want.index_put_((n_.reshape(-1), sy.reshape(-1), sx.reshape(-1), c_.reshape(-1)), g.reshape(-1), accumulate=True)
    got = ops.maxpool5_bwd(dev_of(hip, g, dtype), idx, base=dev_of(hip, base, dtype))
    same(got, E.stored(want, dtype))
