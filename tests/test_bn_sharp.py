"""Train-mode BatchNorm + SiLU, every path, per element against float64 at the DERIVED bounds of tests/bn_ref.py (the derivation is
that module's docstring): no blanket tolerance, no element excluded, one reference per case for all paths.

Forward:  (a) partial rows + bn_finalize (both finalize forms) + bn_act_fwd      (b) conv2d_fwd(shards=) + bn_act_fwd_sharded
          (c) the eval affine from the updated running statistics
Backward: (a) bn_act_bwd with its reduce pass (both finalize forms)              (b) dgrad epilogue sums + bn_act_bwd(partial=)
          (c) sharded with its own reduce                                        (d) sharded with the dgrad's sums
Operand sets (from the shape only): "zero" = zero-mean channels; "cond" = per-channel |mean| / std over {0, 3, 10, 30, 100} through a
constant input channel; "edge" = an exactly constant channel, gamma = 0, negative gamma, |gamma| = 40 (u spans about +-100: gate
saturation, exp overflow -> sigmoid 0, fp16 outputs in the subnormal range).
The worst error / bound per (path, output, dtype) is printed at the end of the module (pytest -s) and, when ET_BN_SHARP_REPORT names
a file, written there as JSON; NOTEBOOK.md holds the table of both tiers."""
import functools
import json
import os

import pytest
import torch

from tests import bn_ref

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["fp32", "bf16", "fp16"]
K = 16                       # input channels of the 1x1 conv in front
RATIOS = (0.0, 3.0, 10.0, 30.0, 100.0)
SENTINEL = 7.0
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    rows = sorted(RECORD.items())
    for (tier, path, out, dt), v in rows:
        print(f"bn_sharp {tier:3s} {path:28s} {out:8s} {dt:9s} {v:.3f}")
    dst = os.environ.get("ET_BN_SHARP_REPORT")
    if dst:
        with open(dst, "w") as fh:
            json.dump([[*k, v] for k, v in rows], fh, indent=0)


@functools.lru_cache(maxsize=None)
def _operands(shape, opset, dtype, C2, k):
    """every operand of a case on the CPU, in the storage type, from the shape alone"""
    N, H, W, C = shape
    g = torch.Generator().manual_seed((N * 1000003 + H * 10007 + W * 101 + C) % (2 ** 31))
    rn = lambda *s: torch.randn(*s, generator=g)
    o = {}
    x, w = rn(N, H, W, K), rn(C, K) * 0.3
    gamma, beta = rn(C) * 0.2 + 1.0, rn(C) * 0.1
    if opset != "zero":
        x[..., K - 1] = 1.0                                   # the constant input channel: w[:, K - 1] is the mean of the output channel
        w[:, K - 1] = 0.0
    if opset == "cond":
        std = w[:, :K - 1].pow(2).sum(1).sqrt()
        c = torch.arange(C)
        w[:, K - 1] = torch.tensor(RATIOS)[c % 5] * std * (1.0 - 2.0 * ((c // 5) % 2))
    if opset == "edge":
        w[0, :] = 0.0
        w[0, K - 1] = 0.75                                    # channel 0: y == 0.75 in every pixel
        gamma[1], gamma[2], gamma[3], gamma[4] = 0.0, -1.3, 40.0, -40.0
    o["x"], o["w"] = x.to(dtype), w.to(dtype).reshape(C, 1, 1, K)
    o["gamma"], o["beta"] = gamma, beta
    o["res"] = rn(N, H, W, C).to(dtype)
    o["rm0"], o["rv0"] = rn(C) * 0.5, torch.rand(C, generator=g) + 0.5
    o["dg0"], o["db0"] = rn(C), rn(C)                           # dgamma / dbeta ACCUMULATE: start non-zero
    o["dyy"] = rn(N, H, W, C2).to(dtype)                        # the consumer's output gradient; dz = dgrad(dyy, w2) (+ shortcut gradient)
    o["w2"] = (rn(C2, k, k, C) * (1.0 / (k * k * C2) ** 0.5)).to(dtype)
    o["res2"] = rn(N, H, W, C).to(dtype)
    return o


class _Slot:
    """what BnBwdSums needs of a flat_state.BnSlot"""
    def __init__(self, pair):
        self.pair = pair

    def acquire_bwd(self):
        return self.pair


def _env_small(form):
    """ET_BN_FIN_SMALL=0 forces the distributed finalize (fp64 atomics + ticket) on these small tensors; returns the restore value"""
    old = os.environ.get("ET_BN_FIN_SMALL")
    if form == "distributed":
        os.environ["ET_BN_FIN_SMALL"] = "0"
    else:
        os.environ.pop("ET_BN_FIN_SMALL", None)
    return old


def _env_restore(old):
    if old is None:
        os.environ.pop("ET_BN_FIN_SMALL", None)
    else:
        os.environ["ET_BN_FIN_SMALL"] = old


def _run(hip, shape, opset, dtype, *, C2=16, k=1, ld=None, vectors=1, with_residual=(False, True)):
    from efficientteacher_amd import ops
    from efficientteacher_amd.flat_state import BN_SHARDS
    N, H, W, C = shape
    P, pad = N * H * W, k // 2
    vec = 4 if dtype == torch.float32 else 8
    CV = C // vec
    dev = hip.device
    o = {n: t.to(dev) for n, t in _operands(shape, opset, dtype, C2, k).items()}
    tier = "emu" if hip.emulated else "gpu"
    dts = str(dtype).replace("torch.", "")
    fails = []

    def check(path, out, got, ref, bound):
        r = bn_ref.ratio(got, ref, bound)
        key = (tier, path, out, dts)
        RECORD[key] = max(RECORD.get(key, 0.0), r)
        if not r <= 1.0:
            fails.append(f"{path} {out}: error / bound = {r:.3g}")

    # coverage, from the exported geometry
    blocks = ops._lib.load().et_bn_reduce_rows(P, C, ops.et_dtype(o["x"]))
    assert bn_ref.reduce_vectors_per_thread(P, CV, blocks) == vectors
    if vectors == 3:
        assert P * CV > 2 * blocks * 256 and (P * CV) % (blocks * 256) != 0       # some threads 3 (pair + odd tail), some 2: ragged

    slots = []

    def slot():
        """an (N, H, W, C) tensor: its own, or a channel slice of a wider buffer with live neighbours"""
        if ld is None:
            return torch.empty((N, H, W, C), dtype=dtype, device=dev)
        full = torch.full((N, H, W, ld), SENTINEL, dtype=dtype, device=dev)
        slots.append(full)
        return full[..., 8:8 + C]

    def shards():
        full = torch.zeros((BN_SHARDS, 2, C + 24), dtype=torch.float32, device=dev)
        return full, (full.view(-1)[8:], C + 24)

    def others_zero(full):
        tot = full.sum(0)
        return torch.count_nonzero(tot[:, :8]) == 0 and torch.count_nonzero(tot[:, 8 + C:]) == 0

    res = slot()
    res.copy_(o["res"])
    conv_args = (dtype, N, H, W, K, C, 1, 1, 0)
    n_fwd = max(bn_ref.conv_sum_terms(P, rows=ops.stats_rows("fwd", *conv_args)), bn_ref.conv_sum_terms(P, adds=ops.stats_adds("fwd", *conv_args)))

    # ---- forward: run every path, then one reference on the y they all stored
    fwd = {}
    for form in ("single-block", "distributed"):
        old = _env_small(form)
        try:
            y, stats = ops.conv2d_fwd(o["x"], o["w"], 1, 0, want_stats=True, out=slot())
            rm, rv = o["rm0"].clone(), o["rv0"].clone()
            sc, sh, mean, invstd = ops.bn_finalize(stats, P, o["gamma"], o["beta"], 1e-3, 0.03, rm, rv)
            z = [ops.bn_act_fwd(y, sc, sh, ops.ACT_SILU, residual=res if r else None, out=slot()) for r in with_residual]
        finally:
            _env_restore(old)
        fwd["a " + form] = dict(y=y, scale=sc, shift=sh, mean=mean, invstd=invstd, rm=rm, rv=rv, z=z)
    full, shp = shards()
    y = ops.conv2d_fwd(o["x"], o["w"], 1, 0, shards=shp, out=slot())
    z = []
    for i, r in enumerate(with_residual):       # the running statistics move once per call: a fresh pair each time, the first is kept
        rm, rv = o["rm0"].clone(), o["rv0"].clone()
        zz, sc, sh, mean, invstd = ops.bn_act_fwd_sharded(y, shp, P, o["gamma"], o["beta"], 1e-3, 0.03, rm, rv, ops.ACT_SILU,
                                                          residual=res if r else None, out=slot())
        z.append(zz)
        if i == 0:
            keep = dict(y=y, scale=sc, shift=sh, mean=mean, invstd=invstd, rm=rm, rv=rv)
    fwd["b sharded"] = dict(keep, z=z)
    assert others_zero(full)
    y = fwd["a single-block"]["y"]
    for name, v in fwd.items():
        assert torch.equal(v["y"], y), name                     # the statistics in the epilogue do not change what is stored

    f = bn_ref.forward(o["x"].reshape(P, K), o["w"].reshape(C, K), y.reshape(P, C), o["gamma"], o["beta"], o["rm0"], o["rv0"], n_fwd, dtype)
    zref = [bn_ref.z_of(f, o["res"].reshape(P, C) if r else None) for r in with_residual]
    # the reference alone stays finite and inside the fp16 range, before any kernel output is looked at
    for t in (f.y64, f.u, f.invstd, *[z for z, _ in zref]):
        assert torch.isfinite(t).all() and t.abs().max().item() < bn_ref.FP16_MAX
    check("fwd conv", "y", y, f.y64, f.b_y)
    for name, v in fwd.items():
        for out in ("scale", "shift", "mean", "invstd", "rm", "rv"):
            check("fwd " + name, out, v[out], getattr(f, out), getattr(f, "b_" + out))
        for (zr, zb), r, zk in zip(zref, with_residual, v["z"]):
            check("fwd " + name, "z+res" if r else "z", zk.reshape(P, C), zr, zb)
    # (c) eval affine from the updated running statistics of path (a)
    a = fwd["a single-block"]
    sc_e, sh_e = ops.bn_eval_affine(o["gamma"], o["beta"], a["rm"], a["rv"], 1e-3)
    ze = ops.bn_act_fwd(y, sc_e, sh_e, ops.ACT_SILU, out=slot())
    e = bn_ref.eval_affine(y.reshape(P, C), o["gamma"], o["beta"], a["rm"], a["rv"], dtype)
    zr, zb = bn_ref.z_of(e, None)
    assert torch.isfinite(zr).all() and zr.abs().max().item() < bn_ref.FP16_MAX
    check("fwd c eval", "scale", sc_e, e.scale, e.b_scale)
    check("fwd c eval", "shift", sh_e, e.shift, e.b_shift)
    check("fwd c eval", "z", ze.reshape(P, C), zr, zb)

    # ---- backward: dz = the consumer's dgrad (+ the shortcut gradient), stored once; every path reads the same dz
    wT = ops.weight_transpose(o["w2"])
    res2 = slot()
    res2.copy_(o["res2"])
    b_sh = fwd["b sharded"]
    dg_args = (dtype, N, H, W, C, C2, k, 1, pad)
    for r in with_residual:
        rr = res2 if r else None
        tag = " +res" if r else ""
        dz = ops.conv2d_dgrad(o["dyy"], wT, (H, W), 1, pad, residual=rr, out=slot())
        n_bwd, bwd = [], {}
        # (a) own reduce pass, both finalize forms
        for form in ("single-block", "distributed"):
            old = _env_small(form)
            try:
                dg, db = o["dg0"].clone(), o["db0"].clone()
                dy = ops.bn_act_bwd(dz, y, o["gamma"], a["scale"], a["shift"], a["mean"], a["invstd"], ops.ACT_SILU, dg, db, out=slot())
            finally:
                _env_restore(old)
            bwd["a " + form] = (dy, dg, db)
        n_bwd.append(bn_ref.reduce_sum_terms(P, CV, blocks, False))
        # (b) the sums ride the dgrad's epilogue (partial rows)
        hand = ops.BnBwdSums(y, a["scale"], a["shift"], ops.ACT_SILU)
        dz_b = ops.conv2d_dgrad(o["dyy"], wT, (H, W), 1, pad, residual=rr, bn=hand, out=slot())
        assert hand.partial is not None and torch.equal(dz_b, dz)                 # the epilogue sums do not change what is stored
        dg, db = o["dg0"].clone(), o["db0"].clone()
        dy = ops.bn_act_bwd(dz_b, y, o["gamma"], a["scale"], a["shift"], a["mean"], a["invstd"], ops.ACT_SILU, dg, db, partial=hand.take(dz_b), out=slot())
        bwd["b dgrad sums"] = (dy, dg, db)
        n_bwd.append(bn_ref.conv_sum_terms(P, rows=ops.stats_rows("dgrad_bn", *dg_args)))
        # (c) sharded, own reduce
        full, shp = shards()
        dg, db = o["dg0"].clone(), o["db0"].clone()
        dy = ops.bn_act_bwd(dz, y, o["gamma"], b_sh["scale"], b_sh["shift"], b_sh["mean"], b_sh["invstd"], ops.ACT_SILU, dg, db, shards=shp, out=slot())
        assert others_zero(full)
        bwd["c sharded reduce"] = (dy, dg, db)
        n_bwd.append(bn_ref.reduce_sum_terms(P, CV, blocks, True))
        # (d) sharded, the dgrad's sums
        full, shp = shards()
        hand = ops.BnBwdSums(y, b_sh["scale"], b_sh["shift"], ops.ACT_SILU, slot=_Slot(shp))
        dz_d = ops.conv2d_dgrad(o["dyy"], wT, (H, W), 1, pad, residual=rr, bn=hand, out=slot())
        part = hand.take(dz_d)
        assert part is shp and torch.equal(dz_d, dz)
        dg, db = o["dg0"].clone(), o["db0"].clone()
        dy = ops.bn_act_bwd(dz_d, y, o["gamma"], b_sh["scale"], b_sh["shift"], b_sh["mean"], b_sh["invstd"], ops.ACT_SILU, dg, db, partial=part, shards=shp, out=slot())
        assert others_zero(full)
        bwd["d sharded dgrad sums"] = (dy, dg, db)
        n_bwd.append(bn_ref.conv_sum_terms(P, adds=ops.stats_adds("dgrad_bn", *dg_args)))

        b = bn_ref.backward(f, dz.reshape(P, C), o["dg0"], o["db0"], max(n_bwd))
        for t in (b.du, b.dy, b.dgamma, b.dbeta):
            assert torch.isfinite(t).all() and t.abs().max().item() < bn_ref.FP16_MAX
        for name, (dy, dg, db) in bwd.items():
            check("bwd " + name + tag, "dy", dy.reshape(P, C), b.dy, b.b_dy)
            check("bwd " + name + tag, "dgamma", dg, b.dgamma, b.b_dgamma)
            check("bwd " + name + tag, "dbeta", db, b.dbeta, b.b_dbeta)
    for full in slots:                                               # live neighbours of every channel slice: untouched
        assert (full[..., :8] == SENTINEL).all() and (full[..., 8 + C:] == SENTINEL).all()
    assert not fails, "\n".join(fails)
    return f


def _regime(C, dtype):
    CV = C // (4 if dtype == torch.float32 else 8)
    return "1" if CV == 1 else ">=64" if CV >= 64 else "pow2" if CV & (CV - 1) == 0 else "non-pow2"


# one vector per reduce-pass thread; CV = C / vector in every regime of the block reduction: 1, a power of two below 64 (xor-fold),
# not a power of two, >= 64 (no fold)
SHAPES = [(1, 1, 2, 8), (3, 4, 4, 8), (2, 7, 9, 32), (2, 9, 11, 40), (1, 5, 5, 72), (1, 6, 7, 512)]


def test_shapes_reach_every_regime_of_the_block_reduction():
    for dt in DTYPES:
        got = {_regime(s[3], dt) for s in SHAPES}
        want = {"pow2", "non-pow2", ">=64"} | ({"1"} if dt != torch.float32 else set())       # (fp32: C % 8 == 0 makes CV >= 2)
        assert want <= got, (dt, got)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("opset", ["zero", "cond", "edge"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_path_meets_the_derived_bounds(hip, shape, opset, dtype):
    f = _run(hip, shape, opset, dtype)
    if opset == "cond" and shape[0] * shape[1] * shape[2] >= 100:
        # the set is what it claims: per-channel |mean| / std spread over two decades inside one tensor
        q = (f.mean.abs() / f.var.sqrt())
        assert q.min().item() < 0.5 and q.max().item() > 50.0
    if opset == "edge":
        assert f.var[0].item() == 0.0                                 # the exactly constant channel
        if shape[0] * shape[1] * shape[2] >= 40:
            assert f.u[:, 3].abs().max().item() > 60.0                # the gate saturates


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_three_vectors_per_reduce_thread(hip, dtype):
    """just above P * CV = 2 * 131072 (512 blocks of 256 threads), ragged: threads of the reduce pass get 3 or 2 vectors, so the paired
    loop AND its odd tail run; the conditioned operands make every lost addition visible"""
    shape = (1, 513, 256, 8) if dtype == torch.float32 else (1, 513, 512, 8)
    _run(hip, shape, "cond", dtype, vectors=3, with_residual=(True,))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_channel_slices_with_live_neighbours(hip, dtype):
    """every activation tensor (y, residual, z, dz, dy) is a 40-channel slice of a 64-channel buffer (ld > C)"""
    _run(hip, (2, 5, 6, 40), "cond", dtype, ld=64)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_dgrad_sums_on_the_256_row_tiles(hip, dtype):
    """a 3x3 256 -> 256 consumer: its dgrad runs on the 256-row ping-pong tiles in the 16-bit types (fp32 never reaches them), 289
    pixels = one full and one ragged tile"""
    from efficientteacher_amd import ops
    name = ops.kernel_name("dgrad_full", dtype, 1, 17, 17, 256, 256, 3, 1, 1)
    assert ("pprs" in name) == (dtype != torch.float32), name
    _run(hip, (1, 17, 17, 256), "cond", dtype, C2=256, k=3, with_residual=(True,))
