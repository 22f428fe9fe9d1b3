"""Every conv kernel family and every epilogue form, per element against float64 at the DERIVED bounds of tests/conv_ref.py (the derivation
is that module's docstring): no blanket tolerance, no element excluded, no max(1, ...) floor, one reference per case for all paths.

Cases: the SELECT table of tests/test_conv.py in bf16 and fp16 (each row is the smallest shape that selects one named instantiation; the
kernel names are asserted as _check_instantiation does, so a change of tile policy cannot silently drop a family from these checks), the
six CASES of test_conv.py in fp32, a 1x1 stride-2 dgrad whose parity classes 1 ... 3 no tap reaches, and a forward with 36 output channels
(the scalar tail of the epilogue: no row of SELECT has a ragged 8-channel group).
Paths:  forward  plain + partial statistics | shards= | scale + bias + SiLU + residual (+ statistics of the full plan) into a channel
                 slice of a sentinel-filled buffer | the same with ReLU | scale + bias + SiLU without a residual (the plain plan)
        dgrad    plain | + residual (stride 1) | accumulate onto a non-zero output
        wgrad    into a non-zero dw0 | a second call | conv2d_wgrad_grouped with one item on a slice (one 3x3 row)
Operand sets (from the shape alone, on the CPU):
    unit     randn operands, weights * 1 / sqrt(K)
    wide     each output channel's weights (dgrad: each input channel's) times 2^-12, 2^-8, 2^-4, 1, 2^4 cycling with the channel index, the
             epilogue scale over the same set (cycling five times slower) times a random sign; bias, residual and dw0 follow their channel:
             one tensor holds channels five orders of magnitude apart and fp16 outputs reach into the subnormal range
    cancel   input channel 0 == 1, channel 1 == -1 and every filter carries the same large weight on both (one tap one ulp apart), so
             |y64| << A; a bias of 64 that the residual removes, so the stored value is far below the pre-store terms
    aligned  non-negative operands: |y64| == A, the only set in which the accumulator charge 2 (K + 1) r A stays below the store
             rounding at K in the thousands (a double rounding or a truncating store of such a layer is invisible under the other three);
             output channel 0 is one constant just below a rounding boundary of the storage type, so that its rounding errors add up
All sets of a (row, dtype) run inside ONE test.  The worst error / bound per (tier, kernel, output, dtype) is printed at the end of the
module (pytest -s) and, when ET_CONV_SHARP_REPORT names a file, written there as JSON; NOTEBOOK.md holds the table of both tiers and the
mutations that decided whether the bounds are sharp."""
import functools
import json
import os

import pytest
import torch

from tests import conv_ref
from tests.test_conv import CASES, SELECT, _same, kn

OPSETS = ("unit", "wide", "cancel", "aligned")
FACTORS = (2.0 ** -12, 2.0 ** -8, 2.0 ** -4, 1.0, 2.0 ** 4)
SENTINEL = 7.0
BIG_W, BIG_BIAS = 16.0, 64.0
GROUPED_ROW = (1, 9, 11, 64, 40, 3, 1, 1)
STRIDE2_1X1 = (1, 8, 8, 16, 32, 1, 2, 0)
RAGGED_COUT = (1, 9, 11, 64, 36, 3, 1, 1)        # Cout is not whole 8-channel groups: the scalar tail of the epilogue (forward only)
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    rows = sorted(RECORD.items())
    for (tier, kernel, out, dt), v in rows:
        print(f"conv_sharp {tier:3s} {dt:9s} {out:12s} {v:.4f}  {kernel}")
    dst = os.environ.get("ET_CONV_SHARP_REPORT")
    if dst:
        with open(dst, "w") as fh:
            json.dump([[*k, v] for k, v in rows], fh, indent=0)


def _next_up(t):
    """the neighbouring value of larger magnitude in t's own format"""
    it = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return (t.contiguous().view(it) + 1).view(t.dtype)


@functools.lru_cache(maxsize=8)
def _operands(case, opset, dtype):
    """every operand of a case on the CPU, in the storage type (scale, bias, dw0: fp32), from the shape alone"""
    N, H, W, Cin, Cout, k, s, p = case
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    g = torch.Generator().manual_seed((N * 1000003 + H * 10007 + W * 101 + Cin * 13 + Cout * 7 + k + OPSETS.index(opset) * 7919) % (2 ** 31))
    rn = lambda *sh: torch.randn(*sh, generator=g)
    x, w = rn(N, H, W, Cin), rn(Cout, k, k, Cin) * (k * k * Cin) ** -0.5
    sc, bi = rn(Cout).abs() + 0.5, rn(Cout)
    res = rn(N, OH, OW, Cout)
    dy, w2 = rn(N, OH, OW, Cout), rn(Cout, k, k, Cin) * (k * k * Cout) ** -0.5          # dgrad: the operand roles swap, K = taps * Cout
    r2, dx0 = rn(N, H, W, Cin), rn(N, H, W, Cin)
    dyw, dw0 = dy.clone(), rn(Cout, k, k, Cin)
    co, ci = torch.arange(Cout), torch.arange(Cin)
    if opset == "wide":
        fw = torch.tensor(FACTORS)[co % 5]
        fs = torch.tensor(FACTORS)[(co // 5) % 5]
        w = w * fw.view(-1, 1, 1, 1)
        sc = fs * torch.where(rn(Cout) < 0, -1.0, 1.0)
        bi, res = bi * fw * fs, res * fw * fs
        fi = torch.tensor(FACTORS)[ci % 5]
        w2, r2, dx0 = w2 * fi, r2 * fi, dx0 * fi
        dyw, dw0 = dyw * fw, dw0 * fw.view(-1, 1, 1, 1)
    if opset == "aligned":
        x, w, dy, w2, dyw = x.abs(), w.abs(), dy.abs(), w2.abs(), dyw.abs()
    o = {n: t.to(dtype) for n, t in dict(x=x, w=w, res=res, dy=dy, w2=w2, r2=r2, dx0=dx0, dyw=dyw).items()}
    if opset == "aligned":
        # output channel 0 is the SAME value in every pixel, 0.98 of half a storage-type spacing above 1 (its centre tap -- inside the
        # image for every pixel of every case -- reads two constant input channels): the stored value is 1 everywhere, so sums taken
        # from the stored values instead of the accumulators are off by the same amount in every pixel, not by a random walk
        hu = 0.98 * 2.0 ** -{torch.bfloat16: 8, torch.float16: 11, torch.float32: 12}[dtype]
        o["x"][..., 0], o["x"][..., 1] = 1.0, 1.0
        o["w"][0] = 0.0
        o["w"][0, k // 2, k // 2, 0], o["w"][0, k // 2, k // 2, 1] = 1.0, hu
    if opset == "cancel":
        big = (BIG_W * (1.0 + (co % 3).float())).to(dtype)
        o["x"][..., 0], o["x"][..., 1] = 1.0, -1.0
        o["w"][..., 0] = big.view(-1, 1, 1)
        o["w"][..., 1] = big.view(-1, 1, 1)
        o["w"][:, k // 2, k // 2, 1] = _next_up(big)                        # the two channels cancel to one ulp of the large weight
        bi = torch.full((Cout,), BIG_BIAS)
        o["res"] = (res - BIG_BIAS).to(dtype)
        bigi = (BIG_W * (1.0 + (ci % 3).float())).to(dtype)
        o["dy"][..., 0], o["dy"][..., 1] = 1.0, -1.0
        o["w2"][0], o["w2"][1] = bigi, bigi
        o["w2"][1, k // 2, k // 2] = _next_up(bigi)
        o["dyw"] = o["dy"]
    o["scale"], o["bias"], o["dw0"] = sc.float(), bi.float(), dw0.float()
    return o


def _run(hip, case, dtype, names=None, fwd=True, dgrad=True, wgrad=True):
    """names: (forward kernel, dgrad kernels per parity class, wgrad kernel) that the library must select, or None (fp32: recorded only)"""
    from efficientteacher_amd import ops
    from efficientteacher_amd.flat_state import BN_SHARDS
    N, H, W, Cin, Cout, k, s, p = case
    OH, OW = ops.conv_out_hw(H, W, k, s, p)
    P = N * OH * OW
    dev = hip.device
    tier = "emu" if hip.emulated else "gpu"
    dts = str(dtype).replace("torch.", "")
    args = (dtype, N, H, W, Cin, Cout, k, s, p)
    fails = []
    nf, nfr = kn("fwd", *args), kn("fwd_res", *args)
    nd = [kn("dgrad", *args, parity_class=c) for c in range(s * s)] if dgrad else []
    ndf = kn("dgrad_full", *args) if dgrad and s == 1 else " | ".join(sorted(set(nd)))
    nw = kn("wgrad", *args) if wgrad else None
    if names is not None:
        kf, kd, kw = names
        assert _same(nf, kf), nf
        if dgrad:
            assert len(nd) == len(kd) and all(_same(a, b) for a, b in zip(nd, kd)), nd
        if wgrad:
            assert nw == kw, nw
    nd = " | ".join(sorted(set(nd)))

    def check(kernel, out, got, ref, bound):
        r = conv_ref.ratio(got, ref, bound)
        key = (tier, kernel, out, dts)
        RECORD[key] = max(RECORD.get(key, 0.0), r)
        if not r <= 1.0:
            fails.append(f"{opset} {kernel} {out}: error / bound = {r:.4g}")

    def in_range(*ts):
        """on the reference alone, before any kernel output is looked at: finite, and inside the fp16 range with its bound"""
        for z, b in ts:
            assert torch.isfinite(z).all() and torch.isfinite(b).all()
            if dtype == torch.float16:
                assert (z.abs() + b).max().item() < conv_ref.FP16_MAX

    wides = []

    def sliced(C, shape3):
        full = torch.full((*shape3, (C + 7) // 8 * 8 + 16), SENTINEL, dtype=dtype, device=dev)      # whole 16-byte vectors per pixel
        wides.append((full, C))
        return full[..., 8:8 + C]

    for opset in OPSETS:
        o = {n: t.to(dev) for n, t in _operands(case, opset, dtype).items()}
        if Cout % 8:                             # a ragged Cout lives in a wider buffer: every pixel stride is whole 16-byte vectors
            res = sliced(Cout, (N, OH, OW))
            res.copy_(o["res"])
            o["res"] = res
        if fwd:
            f = conv_ref.fwd_acc(o["x"], o["w"], s, p)
            yr = conv_ref.plain(f, dtype)
            refs = {a: conv_ref.epilogue(f, dtype, o["scale"], o["bias"], a, residual=o["res"]) for a in (ops.ACT_SILU, ops.ACT_RELU)}
            lone = conv_ref.epilogue(f, dtype, o["scale"], o["bias"], ops.ACT_SILU)
            in_range(yr, lone, *refs.values())
            if opset == "cancel":
                assert (f.y64.abs() < 0.25 * f.A).all()                       # the set is what it claims: the products cancel
            if opset == "aligned":                                                 # ... nothing cancels, channel 0 is one constant above 1
                assert torch.allclose(f.y64, f.A, rtol=1e-12, atol=0.0)
                assert (f.y64[..., 0] == f.y64[0, 0, 0, 0]).all() and 1.0 < f.y64[0, 0, 0, 0].item() < 1.0 + 2.0 ** -8
            # plain forward + partial rows
            y, st = ops.conv2d_fwd(o["x"], o["w"], s, p, want_stats=True, out=sliced(Cout, (N, OH, OW)))
            check(nf, "y", y, *yr)
            n_rows = conv_ref.conv_sum_terms(P, rows=ops.stats_rows("fwd", *args))
            S, Q, E_S, E_Q = conv_ref.stats(f, n_rows)
            assert st.shape == (ops.stats_rows("fwd", *args), 2, Cout)
            check(nf, "sum rows", st.double().sum(0)[0], S, E_S)
            check(nf, "sumsq rows", st.double().sum(0)[1], Q, E_Q)
            # sharded statistics
            full = torch.zeros((BN_SHARDS, 2, Cout + 24), dtype=torch.float32, device=dev)
            y2 = ops.conv2d_fwd(o["x"], o["w"], s, p, shards=(full.view(-1)[8:], Cout + 24), out=sliced(Cout, (N, OH, OW)))
            assert torch.equal(y2, y)                                              # the statistics do not change what is stored
            tot = full.double().sum(0)
            assert torch.count_nonzero(tot[:, :8]) == 0 and torch.count_nonzero(tot[:, 8 + Cout:]) == 0
            S, Q, E_S, E_Q = conv_ref.stats(f, conv_ref.conv_sum_terms(P, adds=ops.stats_adds("fwd", *args)))
            check(nf, "sum shards", tot[0, 8:8 + Cout], S, E_S)
            check(nf, "sumsq shards", tot[1, 8:8 + Cout], Q, E_Q)
            # scale + bias + activation + residual into a channel slice, with the statistics of the full plan
            n_full = conv_ref.conv_sum_terms(P, rows=ops.stats_rows("fwd_res", *args))
            S, Q, E_S, E_Q = conv_ref.stats(f, n_full)
            for act, tag in ((ops.ACT_SILU, "silu+res"), (ops.ACT_RELU, "relu+res")):
                out = sliced(Cout, (N, OH, OW))
                _, st = ops.conv2d_fwd(o["x"], o["w"], s, p, scale=o["scale"], bias=o["bias"], act=act, residual=o["res"], out=out, want_stats=True)
                check(nfr, tag, out, *refs[act])
                check(nfr, "sum rows", st.double().sum(0)[0], S, E_S)
                check(nfr, "sumsq rows", st.double().sum(0)[1], Q, E_Q)
            # the teacher's ordinary layer, no residual: the plain plan's epilogue (the guard-free store pass of interior tiles, the
            # plain instantiations of the persistent 1x1 kernel, the stem kernel's own -- it declines a residual)
            out = sliced(Cout, (N, OH, OW))
            ops.conv2d_fwd(o["x"], o["w"], s, p, scale=o["scale"], bias=o["bias"], act=ops.ACT_SILU, out=out)
            check(nf, "silu", out, *lone)
        if dgrad:
            d = conv_ref.dgrad_acc(o["dy"], o["w2"], (H, W), s, p)
            ref_p = conv_ref.epilogue(d, dtype)
            ref_r = conv_ref.epilogue(d, dtype, residual=o["r2"]) if s == 1 else None
            ref_a = conv_ref.epilogue(d, dtype, old=o["dx0"])
            in_range(ref_p, ref_a, *([ref_r] if ref_r else []))
            if opset == "cancel":
                assert (d.y64.abs() < 0.25 * d.A)[d.Ke > 0].all()
            wT = ops.weight_transpose(o["w2"])
            assert torch.equal(wT, o["w2"].permute(3, 1, 2, 0).contiguous())
            check(nd, "dx", ops.conv2d_dgrad(o["dy"], wT, (H, W), s, p), *ref_p)
            if s == 1:
                check(ndf, "dx+res", ops.conv2d_dgrad(o["dy"], wT, (H, W), s, p, residual=o["r2"], out=sliced(Cin, (N, H, W))), *ref_r)
            acc = o["dx0"].clone()
            ops.conv2d_dgrad(o["dy"], wT, (H, W), s, p, out=acc, accumulate=True)
            check(ndf, "dx accum", acc, *ref_a)
            if k < s:                                                              # the classes no tap reaches: zero / the old value, exactly
                assert (d.Ke[:, 1::2] == 0).all() and (d.Ke[:, :, 1::2] == 0).all() and (d.Ke[:, ::2, ::2] > 0).all()
        if wgrad:
            dw = o["dw0"].clone()
            for call in ("dw", "dw 2nd call"):
                ref, b = conv_ref.wgrad(o["x"], o["dyw"], dw, k, s, p)
                assert torch.isfinite(ref).all() and torch.isfinite(b).all()
                ops.conv2d_wgrad(o["x"], o["dyw"], dw, k, s, p)
                check(nw, call, dw, ref, b)
            if case == GROUPED_ROW:
                ref, b = conv_ref.wgrad(o["x"], o["dyw"], o["dw0"], k, s, p)
                xs = sliced(Cin, (N, H, W))
                xs.copy_(o["x"])
                items = [(o["x"], o["dyw"], o["dw0"].clone()), (xs, o["dyw"], o["dw0"].clone())]
                ops.conv2d_wgrad_grouped(items, k, s, p)
                for _, _, dwi in items:
                    check(nw, "dw grouped", dwi, ref, b)
    for full, C in wides:                                                          # the neighbours of every channel slice: untouched
        assert (full[..., :8] == SENTINEL).all() and (full[..., 8 + C:] == SENTINEL).all()
    assert not fails, "\n".join(fails)


def test_cases_cover_the_table_and_the_grouped_row():
    """every row of SELECT is a case in both 16-bit types; the rows fp16 may skip on the emulator are the six of the existing fp16 table"""
    assert len(SELECT) == 25 and GROUPED_ROW in [c[0] for c in SELECT] and (1, 15, 15, 64, 128, 3, 2, 1) in [c[0] for c in SELECT]
    assert sum(_emu_skips_fp16(c[0]) for c in SELECT) == 6


def _emu_skips_fp16(case):
    N, H, W, Cin, Cout, k = case[:6]
    return N * H * W * Cin * Cout * k * k > 6e7


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case,kf,kd,kw", SELECT, ids=[str(c[0]) for c in SELECT])
def test_select_rows_meet_the_derived_bounds(hip, case, kf, kd, kw, dtype):
    if hip.emulated and dtype == torch.float16 and _emu_skips_fp16(case):
        pytest.skip("CPU emulator tier: the rule of test_bench_instantiations_elementwise_fp16 (these six rows run there in bf16); the GPU "
                    "tier runs every row in fp16 too")
    _run(hip, case, dtype, names=(kf, kd, kw), dgrad=kd is not None, wgrad=kw is not None)


@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_fp32_cases_meet_the_derived_bounds(hip, case):
    """parity mode (the exact-f32 MFMA); dgrad / wgrad where test_conv_dgrad / test_conv_wgrad run them"""
    _run(hip, case, torch.float32, dgrad=case[3] % 8 == 0 and case[4] % 8 == 0 and case[5] != 6, wgrad=case[4] % 8 == 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_stride2_1x1_dgrad_leaves_unreached_classes_exact(hip, dtype):
    """k < stride: three of the four parity classes receive no tap -- exactly zero, or exactly the old value under `accumulate`"""
    _run(hip, STRIDE2_1X1, dtype, fwd=False, wgrad=False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_ragged_cout_takes_the_scalar_tail(hip, dtype):
    """36 output channels inside a wider buffer: the last group of every pixel is stored element by element, with its own copy of
    the residual addition and the rounding"""
    _run(hip, RAGGED_COUT, dtype, dgrad=False, wgrad=False)
