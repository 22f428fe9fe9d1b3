"""The stem on the loaders' uint8 image planes (conv_stem_u8_kernel, conv_stem_u8_wgrad_kernel; ops.U8Images): no packed (B,H,W,8)
tensor.  Forward: bit-equal to pack_input + conv_stem_kernel.  Weight gradient: exact on integer data, and within the packed path's own
tolerance on real data; the pad slots of the gradient arena are never written.  Dispatch: everything that is not (uint8, 3 planes, 16-bit
compute type, 6x6 stride-2 pad-2) keeps the packed path.  Lifetime: the images are read again at the end of backward."""
import numpy as np
import pytest
import torch

from tests.conftest import golden

LP = [torch.bfloat16, torch.float16]
# (H, W): OH = 22 is ragged against the 4-row tile and OW = 68 crosses the 64-column tile; (8, 8) is one partial tile that is all border
RAGGED, BORDER = (44, 136), (8, 8)
WGRAD_TOL = 1e-4        # tests/test_conv.py test_conv_wgrad: err <= 1e-4 * max(1, |ref|max), the packed path's bound against fp32 F.conv2d


def _images(hw, counts, seed, hi=256):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, hi, (n, 3) + hw, dtype=np.uint8)) for n in counts]


def _weight(hip, cout, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((cout, 6, 6, 8), generator=g) * (1.0 / 108 ** 0.5)
    w[..., 3:] = 0                                  # the packed layer's weight: pad channels are zero (and meet zero pixels anyway)
    return w.to(dtype).to(hip.device)


@pytest.mark.parametrize("dtype", LP, ids=["bf16", "fp16"])
@pytest.mark.parametrize("hw,counts,cout", [(RAGGED, (1, 2), 64), (BORDER, (1, 1), 16)], ids=["ragged 44x136, 1+2 images", "border 8x8"])
def test_forward_bit_equal_to_pack_plus_stem(hip, monkeypatch, hw, counts, cout, dtype):
    """train form (raw accumulators + BN partial sums, rows and sharded) and eval form (folded scale / bias + SiLU), a persistent grid
    smaller than the tile count: every output bit and every partial sum equals pack_input + conv_stem_kernel"""
    from efficientteacher_amd import ops
    monkeypatch.setenv("ET_CONV_STEM_WGS", "5")
    monkeypatch.delenv("ET_STEM_U8", raising=False)
    parts = [hip.t(p) for p in _images(hw, counts, 3)]
    u8 = ops.stem_input(parts, dtype, norm_scale=255.0)
    assert isinstance(u8, ops.U8Images) and tuple(u8.shape) == (sum(counts),) + hw + (8,)
    w = _weight(hip, cout, dtype, 4)
    assert ops.stem_u8_mode(u8, w, 2, 2) == 3
    packed = ops.pack_input(parts, dtype, norm_scale=255.0)
    # train form, partial rows
    y0, s0 = ops.conv2d_fwd(packed, w, 2, 2, want_stats=True)
    y1, s1 = ops.conv2d_fwd(u8, w, 2, 2, want_stats=True)
    assert torch.equal(y0.cpu().view(torch.int16), y1.cpu().view(torch.int16))
    assert s0.shape == s1.shape and torch.equal(s0.cpu(), s1.cpu())
    # train form, sharded accumulator (single-threaded adds in the emulator; on the GPU the atomics of one launch commute only up to
    # fp32 rounding, so the shards are compared by their sum against the rows' sum with the rows' own spread)
    ld = 64
    sh0 = torch.zeros((16, 2, ld), dtype=torch.float32, device=hip.device)
    sh1 = torch.zeros_like(sh0)
    ya = ops.conv2d_fwd(packed, w, 2, 2, shards=(sh0, ld))
    yb = ops.conv2d_fwd(u8, w, 2, 2, shards=(sh1, ld))
    assert torch.equal(ya.cpu().view(torch.int16), yb.cpu().view(torch.int16)) and torch.equal(ya.cpu().view(torch.int16), y0.cpu().view(torch.int16))
    assert torch.allclose(sh1.sum(0).cpu(), sh0.sum(0).cpu(), rtol=1e-5, atol=1e-4)
    # eval form
    g = torch.Generator().manual_seed(5)
    scale = (torch.rand(cout, generator=g) + 0.5).to(hip.device)
    bias = torch.randn(cout, generator=g).to(hip.device)
    z0 = ops.conv2d_fwd(packed, w, 2, 2, scale=scale, bias=bias, act=ops.ACT_SILU)
    z1 = ops.conv2d_fwd(u8, w, 2, 2, scale=scale, bias=bias, act=ops.ACT_SILU)
    assert torch.equal(z0.cpu().view(torch.int16), z1.cpu().view(torch.int16))


@pytest.mark.parametrize("dtype", LP, ids=["bf16", "fp16"])
def test_table_equals_pack_for_every_byte(hip, monkeypatch, dtype):
    """all 256 byte values down one image column, read back through one-hot taps: T(v / 255) bit for bit as pack_input makes it (an IEEE
    division; a multiplication by the rounded reciprocal is 1 ulp away for some v)"""
    from efficientteacher_amd import ops
    monkeypatch.delenv("ET_STEM_U8", raising=False)
    col = torch.arange(256, dtype=torch.int64)
    x = torch.zeros((1, 3, 256, 4), dtype=torch.uint8)
    x[0, 0, :, 0] = col.to(torch.uint8)
    x[0, 1, :, 0] = ((col * 7 + 3) % 256).to(torch.uint8)
    x[0, 2, :, 0] = (255 - col).to(torch.uint8)
    w = torch.zeros((8, 6, 6, 8))
    for c in range(3):
        w[c, 2, 2, c] = 1.0            # output row oy reads input row 2 * oy
        w[3 + c, 3, 2, c] = 1.0        # ... and 2 * oy + 1
    w = w.to(dtype).to(hip.device)
    xs = hip.t(x)
    u8 = ops.stem_input(xs, dtype, norm_scale=255.0)
    assert isinstance(u8, ops.U8Images)
    y = ops.conv2d_fwd(u8, w, 2, 2).cpu()
    packed = ops.pack_input(xs, dtype, norm_scale=255.0).cpu()
    assert torch.equal(y[0, :, 0, 0:3].view(torch.int16), packed[0, 0::2, 0, 0:3].view(torch.int16))
    assert torch.equal(y[0, :, 0, 3:6].view(torch.int16), packed[0, 1::2, 0, 0:3].view(torch.int16))
    ref = (x.float() / 255.0).permute(0, 2, 3, 1).to(dtype)
    assert torch.equal(packed[0, :, 0, :3].view(torch.int16), ref[0, :, 0, :].view(torch.int16))


def _ref_wgrad(parts, dy, norm):
    """fp32 torch.nn.grad.conv2d_weight on the CPU: (Cout, 6, 6, 3)"""
    x = torch.cat([p.cpu() for p in parts], 0).float() / norm
    g = dy.float().cpu().permute(0, 3, 1, 2).contiguous()
    dw = torch.nn.grad.conv2d_weight(x, (g.shape[1], 3, 6, 6), g, stride=2, padding=2)
    return dw.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dtype,cout", [(torch.bfloat16, 64), (torch.float16, 8)], ids=["bf16 64ch", "fp16 8ch"])
def test_wgrad_exact_on_integers(hip, monkeypatch, dtype, cout):
    """norm_scale 1, pixels 0..15, dY integers -2..2: every product and partial sum is an integer below 2^24 (checked here with torch
    alone first), so the fp32 result is exact whatever the summation order: the 3 real channels of every tap equal conv2d_weight and
    the 5 pad slots keep the sentinel they were filled with"""
    from efficientteacher_amd import ops
    monkeypatch.setenv("ET_CONV_STEM_WGS", "5")
    monkeypatch.delenv("ET_STEM_U8", raising=False)
    parts_h = _images(RAGGED, (1, 2), 11, hi=16)
    N, (H, W) = 3, RAGGED
    OH, OW = ops.conv_out_hw(H, W, 6, 2, 2)
    assert (OH, OW) == (22, 68)
    rng = np.random.default_rng(12)
    dy_h = torch.from_numpy(rng.integers(-2, 3, (N, OH, OW, cout)).astype(np.float32))
    # torch alone: the bound (sum of |products|) and the reference
    bound = _ref_wgrad([p for p in parts_h], dy_h.abs(), 1.0).max().item()
    assert bound + 7 < 2 ** 24, bound
    ref = _ref_wgrad(parts_h, dy_h, 1.0)
    parts = [hip.t(p) for p in parts_h]
    dy = hip.t(dy_h, dtype)
    u8 = ops.stem_input(parts, dtype, norm_scale=1.0)
    assert isinstance(u8, ops.U8Images)
    dw = torch.full((cout, 6, 6, 8), 7.0, dtype=torch.float32, device=hip.device)
    ops.stem_u8_wgrad(u8, dy, dw)
    got = dw.cpu()
    assert torch.equal(got[..., :3], ref + 7.0)
    assert (got[..., 3:] == 7.0).all()
    ops.stem_u8_wgrad(u8, dy, dw)                    # accumulates
    assert torch.equal(dw.cpu()[..., :3], 2 * ref + 7.0)


@pytest.mark.parametrize("dtype", LP, ids=["bf16", "fp16"])
def test_wgrad_matches_packed_path(hip, monkeypatch, dtype):
    """random images and dY: against the packed path's weight gradient with ITS tolerance against fp32 (the two differ in summation
    order only: same operand bits)"""
    from efficientteacher_amd import ops
    monkeypatch.delenv("ET_STEM_U8", raising=False)
    parts = [hip.t(p) for p in _images(RAGGED, (2, 1), 21)]
    OH, OW = ops.conv_out_hw(*RAGGED, 6, 2, 2)
    g = torch.Generator().manual_seed(22)
    dy = torch.randn((3, OH, OW, 64), generator=g).to(dtype).to(hip.device)
    u8 = ops.stem_input(parts, dtype, norm_scale=255.0)
    dw = torch.zeros((64, 6, 6, 8), dtype=torch.float32, device=hip.device)
    ops.stem_u8_wgrad(u8, dy, dw)
    old = torch.zeros_like(dw)
    ops.conv2d_wgrad(ops.pack_input(parts, dtype, norm_scale=255.0), dy, old, 6, 2, 2)
    err = (dw.cpu() - old.cpu()).abs().max().item()
    print(f"stem wgrad uint8 vs packed: max abs err {err:.3e}, |ref|max {old.abs().max().item():.3e}")
    assert err <= WGRAD_TOL * max(1.0, old.abs().max().item()), err
    assert (dw.cpu()[..., 3:] == 0).all()


def test_everything_else_keeps_the_packed_path(hip, monkeypatch):
    """float images, a 4-plane uint8 batch, fp32 compute, a first layer that is not the stem, and the knob: the reported kernel is the
    packed path's and the layer's input IS pack_input's tensor"""
    from efficientteacher_amd import ops
    monkeypatch.delenv("ET_STEM_U8", raising=False)
    bf = torch.bfloat16
    N, H, W = 2, 16, 24
    name = lambda op, dt, is_u8, C: ops.stem_kernel_name(op, dt, is_u8, C, N, H, W, 32, 6, 2, 2)
    packed_fwd = ops.kernel_name("fwd", bf, N, H, W, 8, 32, 6, 2, 2)
    packed_wg = ops.kernel_name("wgrad", bf, N, H, W, 8, 32, 6, 2, 2)
    assert packed_fwd == "conv_stem_kernel"
    assert name("fwd", bf, True, 3) == "conv_stem_u8_kernel" and name("wgrad", bf, True, 3) == "conv_stem_u8_wgrad_kernel<unsigned short>"
    assert name("wgrad", torch.float16, True, 3) == "conv_stem_u8_wgrad_kernel<et_f16>"
    assert name("fwd", bf, False, 3) == packed_fwd and name("wgrad", bf, False, 3) == packed_wg                  # float images
    assert name("fwd", bf, True, 4) == packed_fwd and name("wgrad", bf, True, 4) == packed_wg                    # 4 planes
    assert name("fwd", torch.float32, True, 3) == ops.kernel_name("fwd", torch.float32, N, H, W, 8, 32, 6, 2, 2)  # parity mode
    assert not name("fwd", torch.float32, True, 3).startswith("conv_stem_u8")
    assert ops.stem_kernel_name("fwd", bf, True, 3, N, H, W, 32, 3, 2, 1) == ops.kernel_name("fwd", bf, N, H, W, 8, 32, 3, 2, 1)   # the v8 stem
    x3, x4 = _images((H, W), (N,), 31)[0], torch.from_numpy(np.random.default_rng(32).integers(0, 256, (N, 4, H, W), dtype=np.uint8))
    xf = x3.float() / 255.0
    for x, dt in ((xf, bf), (x4, bf), (x3, torch.float32)):
        got = ops.stem_input(hip.t(x), dt)
        assert torch.is_tensor(got) and torch.equal(got.cpu(), ops.pack_input(hip.t(x), dt).cpu())
    u8 = ops.stem_input(hip.t(x3), bf)
    assert isinstance(u8, ops.U8Images)
    assert torch.equal(u8.packed().cpu().view(torch.int16), ops.pack_input(hip.t(x3), bf).cpu().view(torch.int16))
    assert ops.stem_u8_mode(u8, torch.zeros((32, 3, 3, 8), dtype=bf, device=hip.device), 2, 1) == 0
    w = torch.zeros((32, 6, 6, 8), dtype=bf, device=hip.device)
    assert ops.stem_u8_mode(u8, w, 2, 2) == 3
    for v in ("0", "1", "2"):
        monkeypatch.setenv("ET_STEM_U8", v)
        assert ops.stem_u8_mode(u8, w, 2, 2) == int(v)
        assert "ET_STEM_U8=" + v in ops.env_knobs()
    monkeypatch.setenv("ET_STEM_U8", "0")
    assert name("fwd", bf, True, 3) == packed_fwd and name("wgrad", bf, True, 3) == packed_wg


def _check_stem_calls(monkeypatch, hip, log):
    """wrap the two uint8 stem launches of a model step: each result is compared, INSIDE the step and on the step's own operands, with
    what the packed path computes from them -- the forward bit for bit, the weight gradient with the packed path's tolerance.  (Two whole
    bf16 steps are not compared with each other: their BatchNorm sums are fp32 atomics and the tiny model's deepest maps hold 16 values
    per channel, so the dY that reaches the stem already differs between two runs -- 1.7e-3 relative L2 of the stem's weight gradient
    was seen between a packed and a uint8 step on the GPU while every kernel-level comparison of this file held.)"""
    from efficientteacher_amd import ops
    fwd0, wg0 = ops._stem_u8_fwd, ops.stem_u8_wgrad

    def fwd(u8, w, stride, pad, scale, bias, act, out, want_stats, shards):
        r = fwd0(u8, w, stride, pad, scale, bias, act, out, want_stats, shards)
        y = r[0] if want_stats else r
        ref = ops.conv2d_fwd(u8.packed(), w, stride, pad, scale=scale, bias=bias, act=act)
        log.append(("fwd", len(u8.parts), torch.equal(y.cpu().view(torch.int16), ref.cpu().view(torch.int16))))
        return r

    def wgrad(u8, dy, dw):
        before = dw.detach().clone()
        wg0(u8, dy, dw)
        ref = torch.zeros_like(dw)
        ops.conv2d_wgrad(u8.packed(), dy, ref, 6, 2, 2)
        got = (dw - before).cpu()
        ref = ref.cpu()
        err = (got - ref).abs().max().item()
        log.append(("wgrad", len(u8.parts), err <= WGRAD_TOL * max(1.0, ref.abs().max().item()) and ref.abs().max().item() > 0
                    and bool((got[..., 3:] == 0).all()), err))
    monkeypatch.setattr(ops, "_stem_u8_fwd", fwd)
    monkeypatch.setattr(ops, "stem_u8_wgrad", wgrad)


@pytest.mark.parametrize("knob", [None, "0", "1", "2"], ids=["default", "packed", "forward only", "wgrad only"])
def test_model_step_takes_the_uint8_stem(hip, monkeypatch, knob):
    """one bf16 SSOD step of the tiny model on uint8 batches, every arm of ET_STEM_U8: the student's forward reads the labelled and the
    unlabelled batch as two segments, the teacher's its one batch, the weight gradient the student's two -- each checked against the packed
    path on the same operands -- and the knob switches exactly the part it names"""
    from tests.test_ssod_step import make_trainer
    g = golden("ssod_step")
    u8 = lambda a: hip.t(torch.from_numpy(np.round(a * 255).astype(np.uint8)))
    if knob is None:
        monkeypatch.delenv("ET_STEM_U8", raising=False)
    else:
        monkeypatch.setenv("ET_STEM_U8", knob)
    mode = 3 if knob is None else int(knob)
    cfg, t = make_trainer(hip, torch.bfloat16)
    log = []
    _check_stem_calls(monkeypatch, hip, log)
    out = t.train_instance(u8(g["imgs"]), hip.t(g["targets"]), None, u8(g["u_str"]), u8(g["u_ori"]), None, hip.t(g["M_s"]), 500)
    assert all(np.isfinite(float(v)) for v in out.values())
    assert sorted(e[:2] for e in log if e[0] == "fwd") == ([("fwd", 1), ("fwd", 2)] if mode & 1 else [])
    assert [e[:2] for e in log if e[0] == "wgrad"] == ([("wgrad", 2)] if mode & 2 else [])
    assert all(e[2] for e in log), log


@pytest.mark.gpu
def test_images_live_until_the_stem_wgrad_has_read_them(monkeypatch):
    """two steps fed by DevicePrefetcher (copy stream one batch ahead, device blocks recycled by the caching allocator; a third, all-zero
    batch is staged behind them).  The stem's weight gradient of each step -- read from the arena once the step's backward has joined the
    weight-gradient stream -- must be the packed path's weight gradient of THAT step's dY and of the HOST batch's pixels, uploaded afresh
    for the comparison: the packed path's tolerance.  A launch that found the next batch's pixels in the buffers is off by O(1)."""
    from efficientteacher_amd import _lib, ops
    from efficientteacher_amd.utils.prefetch import DevicePrefetcher
    from tests.conftest import _Mode
    from tests.test_ssod_step import make_trainer
    if not torch.cuda.is_available():
        pytest.fail("-m gpu selected but no GPU is visible")
    monkeypatch.delenv("ET_STEM_U8", raising=False)
    _lib._use_library_for_tests(None, False)
    hip = _Mode("cuda:0", False)
    g = golden("ssod_step")
    u8 = lambda a: torch.from_numpy(np.round(a * 255).astype(np.uint8))
    A = (u8(g["imgs"]), u8(g["u_str"]), u8(g["u_ori"]))
    B = tuple((255 - t).flip(0).contiguous() for t in A)
    C = tuple(torch.zeros_like(t) for t in A)
    targets, M_s = hip.t(g["targets"]), hip.t(g["M_s"])
    cfg, t = make_trainer(hip, torch.bfloat16)
    gw = t.model.backbone.stage1.conv._et_slot.gw
    grads, dys = [], []
    zg, sub = t.optimizer.zero_grad, ops.WGRAD_QUEUE.submit_stem_u8

    def zero_grad(*a, **k):
        grads.append(gw.detach().clone())
        return zg(*a, **k)

    def submit(u8i, dy, dw, on_done=None):
        dys.append(dy.detach().clone())
        return sub(u8i, dy, dw, on_done=on_done)
    t.optimizer.zero_grad = zero_grad
    monkeypatch.setattr(ops.WGRAD_QUEUE, "submit_stem_u8", submit)
    for i, (imgs, u_str, u_ori) in enumerate(DevicePrefetcher(iter([A, B, C]), "cuda:0", depth=1)):
        if i == 2:
            break
        t.train_instance(imgs, targets, None, u_str, u_ori, None, M_s, 500 + i)
    torch.cuda.synchronize()
    assert len(grads) == len(dys) == 2
    for i, host in enumerate((A, B)):
        ref = torch.zeros_like(grads[i])
        ops.conv2d_wgrad(ops.pack_input([hip.t(host[0]), hip.t(host[1])], torch.bfloat16), dys[i], ref, 6, 2, 2)
        err, top = (grads[i] - ref).abs().max().item(), ref.abs().max().item()
        print(f"step {i}: stem weight gradient in the arena vs packed path on the host batch: max abs err {err:.3e}, |ref|max {top:.3e}")
        assert top > 0 and err <= WGRAD_TOL * max(1.0, top), (i, err, top)
