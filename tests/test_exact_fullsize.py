"""Zero-tolerance tier at the bench's own sizes (GPU): every distinct conv layer shape of the three bench workloads, at the batches
the step launches them with, BIT-EQUAL to an fp64 CPU reference on small-integer operands (tests/exact_ref.py, tests/test_exact_conv.py).

tests/test_fullsize.py checks global properties at these sizes (inner products, linearity, run-to-run equality) and the element-wise
tests run at 1-3 images of 5...24 pixels; a defect that is deterministic and local at full size -- a wrong border tap in tiles beyond
some index, a persistent-loop tile visited twice, a statistics shard row missed when the workgroup index wraps, a split-K slice whose
last pixel is dropped -- is invisible to both (what each tier sees of four seeded defects: profiles/exact_tests_seeded_defects.txt).  Here one wrong element of y, dx, dw or of a
statistics sum fails `torch.equal`, and the message names the element and the tile of the launched kernel it falls in.

Per (workload, batch, shape), bf16 and fp16 (and the fp32 parity mode on the v5l-ssod B = 32 set): forward, the BatchNorm statistics as
partial rows and as the sharded accumulator, plain dgrad (every parity class), wgrad; forward with a residual and dgrad with a
residual for the stride-1 shapes.  The stem (k = 6) is forward-only, as in the net.  The reference of a shape is computed once and
shared by the storage types (the operands are integers of magnitude <= 3: the same numbers in each).
The dgrad that carries the producer's BatchNorm-backward sums is pinned at test sizes only (tests/test_exact_conv.py): at M > 10^5 its
sum of |dz| * |y| leaves the exact range for any dz that still exercises the rounding.

Two more tests: operands of 2**31 bytes and more (the flat-address twins at their trigger), and the weight gradients of one C3 stage
through ops.WGRAD_QUEUE (grouped launches on the side stream, joined at the end of backward) into a gradient arena.
"""
import pytest
import torch

from tests import exact_ref as E
from tests.test_exact_conv import OFF, same, same_sums, tile_hint

BATCHES = {"v5l-ssod": (16, 32, 64), "v5s-sup": (64,), "v8-sup": (32,)}      # teacher batch, student halves, joined student batch; ...

# distinct (H, W, Cin, Cout, k, s, p) of every nn.Conv2d of the workload's model at 640 px; test_shape_tables_are_the_workloads_layers
# (host only) holds these tables to tests/test_conv.py::_workload_conv_shapes
SHAPES = {
    "v5l-ssod": [
        (20, 20, 512, 512, 1, 1, 0), (20, 20, 512, 512, 3, 1, 1), (20, 20, 1024, 2, 1, 1, 0), (20, 20, 1024, 255, 1, 1, 0),
        (20, 20, 1024, 512, 1, 1, 0), (20, 20, 1024, 1024, 1, 1, 0), (20, 20, 2048, 1024, 1, 1, 0),
        (40, 40, 256, 256, 1, 1, 0), (40, 40, 256, 256, 3, 1, 1), (40, 40, 512, 2, 1, 1, 0), (40, 40, 512, 255, 1, 1, 0),
        (40, 40, 512, 256, 1, 1, 0), (40, 40, 512, 512, 1, 1, 0), (40, 40, 512, 512, 3, 2, 1), (40, 40, 512, 1024, 3, 2, 1),
        (40, 40, 1024, 256, 1, 1, 0),
        (80, 80, 128, 128, 1, 1, 0), (80, 80, 128, 128, 3, 1, 1), (80, 80, 256, 2, 1, 1, 0), (80, 80, 256, 128, 1, 1, 0),
        (80, 80, 256, 255, 1, 1, 0), (80, 80, 256, 256, 1, 1, 0), (80, 80, 256, 256, 3, 2, 1), (80, 80, 256, 512, 3, 2, 1),
        (80, 80, 512, 128, 1, 1, 0),
        (160, 160, 64, 64, 1, 1, 0), (160, 160, 64, 64, 3, 1, 1), (160, 160, 128, 64, 1, 1, 0), (160, 160, 128, 128, 1, 1, 0),
        (160, 160, 128, 256, 3, 2, 1),
        (320, 320, 64, 128, 3, 2, 1),
        (640, 640, 3, 64, 6, 2, 2),
    ],
    "v5s-sup": [
        (20, 20, 256, 256, 1, 1, 0), (20, 20, 256, 256, 3, 1, 1), (20, 20, 512, 2, 1, 1, 0), (20, 20, 512, 255, 1, 1, 0),
        (20, 20, 512, 256, 1, 1, 0), (20, 20, 512, 512, 1, 1, 0), (20, 20, 1024, 512, 1, 1, 0),
        (40, 40, 128, 128, 1, 1, 0), (40, 40, 128, 128, 3, 1, 1), (40, 40, 256, 2, 1, 1, 0), (40, 40, 256, 128, 1, 1, 0),
        (40, 40, 256, 255, 1, 1, 0), (40, 40, 256, 256, 1, 1, 0), (40, 40, 256, 256, 3, 2, 1), (40, 40, 256, 512, 3, 2, 1),
        (40, 40, 512, 128, 1, 1, 0),
        (80, 80, 64, 64, 1, 1, 0), (80, 80, 64, 64, 3, 1, 1), (80, 80, 128, 2, 1, 1, 0), (80, 80, 128, 64, 1, 1, 0),
        (80, 80, 128, 128, 1, 1, 0), (80, 80, 128, 128, 3, 2, 1), (80, 80, 128, 255, 1, 1, 0), (80, 80, 128, 256, 3, 2, 1),
        (80, 80, 256, 64, 1, 1, 0),
        (160, 160, 32, 32, 1, 1, 0), (160, 160, 32, 32, 3, 1, 1), (160, 160, 64, 32, 1, 1, 0), (160, 160, 64, 64, 1, 1, 0),
        (160, 160, 64, 128, 3, 2, 1),
        (320, 320, 32, 64, 3, 2, 1),
        (640, 640, 3, 32, 6, 2, 2),
    ],
    "v8-sup": [
        (20, 20, 68, 68, 1, 1, 0), (20, 20, 68, 68, 3, 1, 1), (20, 20, 256, 80, 1, 1, 0), (20, 20, 256, 256, 3, 1, 1),
        (20, 20, 384, 384, 3, 1, 1), (20, 20, 768, 68, 3, 1, 1), (20, 20, 768, 256, 3, 1, 1), (20, 20, 768, 384, 1, 1, 0),
        (20, 20, 768, 768, 1, 1, 0), (20, 20, 1280, 768, 1, 1, 0), (20, 20, 1536, 768, 1, 1, 0), (20, 20, 1920, 768, 1, 1, 0),
        (40, 40, 68, 68, 1, 1, 0), (40, 40, 68, 68, 3, 1, 1), (40, 40, 256, 80, 1, 1, 0), (40, 40, 256, 256, 3, 1, 1),
        (40, 40, 512, 68, 3, 1, 1), (40, 40, 512, 256, 3, 1, 1), (40, 40, 512, 512, 1, 1, 0), (40, 40, 512, 512, 3, 2, 1),
        (40, 40, 512, 768, 3, 2, 1), (40, 40, 768, 512, 1, 1, 0), (40, 40, 1280, 512, 1, 1, 0), (40, 40, 2048, 512, 1, 1, 0),
        (80, 80, 68, 68, 1, 1, 0), (80, 80, 68, 68, 3, 1, 1), (80, 80, 128, 128, 3, 1, 1), (80, 80, 256, 68, 3, 1, 1),
        (80, 80, 256, 80, 1, 1, 0), (80, 80, 256, 256, 1, 1, 0), (80, 80, 256, 256, 3, 1, 1), (80, 80, 256, 256, 3, 2, 1),
        (80, 80, 256, 512, 3, 2, 1), (80, 80, 640, 256, 1, 1, 0), (80, 80, 768, 256, 1, 1, 0), (80, 80, 1024, 256, 1, 1, 0),
        (160, 160, 64, 64, 3, 1, 1), (160, 160, 128, 128, 1, 1, 0), (160, 160, 128, 256, 3, 2, 1), (160, 160, 320, 128, 1, 1, 0),
        (320, 320, 64, 128, 3, 2, 1),
        (640, 640, 3, 64, 6, 2, 2),
    ],
}


def _pad(shape):
    h, w, ci, co, k, s, p = shape
    return h, w, (8 if k == 6 else (ci + 7) // 8 * 8), (co + 7) // 8 * 8, k, s, p        # channel counts as the nets allocate them


def _params():
    seen, out = set(), []
    for wl, batches in BATCHES.items():
        for B in batches:
            for shape in SHAPES[wl]:
                if (B, shape) in seen:
                    continue
                seen.add((B, shape))
                h, w, ci, co, k, s, p = shape
                out.append(pytest.param(wl, B, shape, id=f"{wl}-B{B}-{h}x{w}x{ci}to{co}-k{k}s{s}"))
    return out


def test_shape_tables_are_the_workloads_layers():
    """host only: SHAPES is exactly the set of distinct layer shapes of each bench workload (read off the oracle's modules), and the
    parametrize ids below cover every (batch, shape) the step launches"""
    from tests.test_conv import _workload_conv_shapes
    covered = {(v.values[1], v.values[2]) for v in _params()}
    for wl, batches in BATCHES.items():
        live = set(_workload_conv_shapes(wl))
        assert set(SHAPES[wl]) == live, (wl, sorted(live - set(SHAPES[wl])), sorted(set(SHAPES[wl]) - live))
        assert len(SHAPES[wl]) == len(set(SHAPES[wl]))
        for B in batches:
            assert all((B, s) in covered for s in live)


@pytest.fixture
def dev():
    from efficientteacher_amd import _lib
    if not torch.cuda.is_available():
        pytest.fail("-m gpu selected but no GPU is visible")
    _lib._use_library_for_tests(None, False)
    _lib.load()
    return torch.device("cuda:0")


def _dtypes(wl, B):
    return (torch.bfloat16, torch.float16) + ((torch.float32,) if (wl, B) == ("v5l-ssod", 32) else ())


@pytest.mark.gpu
@pytest.mark.parametrize("wl,B,shape", _params())
def test_bench_shape_bit_equal(dev, wl, B, shape):
    from efficientteacher_amd import ops
    from efficientteacher_amd.flat_state import BN_SHARDS
    h, w, ci, co, k, s, p = _pad(shape)
    case = (B, h, w, ci, co, k, s, p)
    P = E.Problem(case)
    back = k != 6
    what = f"{wl} B={B} {shape}"

    def up(t, dt):
        return t.to(dt).to(dev)

    # ---- references and their preconditions first: nothing of the kernels has been looked at when one of them fails
    y, sums, ys = P.y(), P.sums(), P.ys()
    yres = (y + P.res_out()) if (s == 1 and back) else None
    for dt in _dtypes(wl, B):
        tag = f"{what} {dt}: "
        x, wt = up(P.x, dt), up(P.w, dt)
        same(ops.conv2d_fwd(x, wt, s, p), E.stored(y, dt), lambda i: tag + "fwd " + tile_hint("fwd", dt, case)(i))
        if yres is not None:
            r = up(P.res_out(), dt)
            same(ops.conv2d_fwd(x, wt, s, p, residual=r), E.stored(yres, dt), lambda i: tag + "fwd_res " + tile_hint("fwd_res", dt, case)(i))
            del r
        del x, wt
        xs, ws = up(P.xs, dt), up(P.ws, dt)
        ysd = E.stored(ys, dt).to(dev)
        yk, st = ops.conv2d_fwd(xs, ws, s, p, want_stats=True)
        same(yk, ysd, lambda i: tag + "fwd (sums set) " + tile_hint("fwd", dt, case)(i))
        same_sums(st.sum(0), sums, tag + "partial rows")
        if dt != torch.float32:                                   # the fp32 parity mode keeps the partial rows
            ld = OFF + co + 16                                      # this layer's channels inside a wider accumulator row
            full = torch.zeros((BN_SHARDS, 2, ld), dtype=torch.float32, device=dev)
            yk = ops.conv2d_fwd(xs, ws, s, p, shards=(full.view(-1)[OFF:], ld))
            same(yk, ysd, lambda i: tag + "fwd (sharded) " + tile_hint("fwd", dt, case)(i))
            same_sums(full.sum(0)[:, OFF:OFF + co], sums, tag + "sharded accumulator")
            assert torch.count_nonzero(full[:, :, :OFF]) == 0 and torch.count_nonzero(full[:, :, OFF + co:]) == 0
        del xs, ws, ysd, yk, st
    P.drop("y", "ys", "xs", "ws", "res_out")
    del y, ys, yres
    if not back:
        return
    dx = P.dx()
    dxres = (dx + P.res_in()) if s == 1 else None
    for dt in _dtypes(wl, B):
        tag = f"{what} {dt}: "
        dy = up(P.dy, dt)
        wT = ops.weight_transpose(up(P.w, dt))
        same(ops.conv2d_dgrad(dy, wT, (h, w), s, p), E.stored(dx, dt), lambda i: tag + "dgrad " + tile_hint("dgrad", dt, case)(i))
        if dxres is not None:
            r = up(P.res_in(), dt)
            same(ops.conv2d_dgrad(dy, wT, (h, w), s, p, residual=r), E.stored(dxres, dt),
                 lambda i: tag + "dgrad + residual " + tile_hint("dgrad_full", dt, case)(i))
            del r
        del dy, wT
    P.drop("dx", "res_in")
    del dx, dxres
    dwref = E.stored(P.dw(), torch.float32)
    for dt in _dtypes(wl, B):
        dw = torch.zeros((co, k, k, ci), dtype=torch.float32, device=dev)
        ops.conv2d_wgrad(up(P.x, dt), up(P.dy, dt), dw, k, s, p)
        same(dw, dwref, lambda i: f"{what} {dt}: wgrad " + tile_hint("wgrad", dt, case)(i))
        del dw
    torch.cuda.empty_cache()


# ---- operands of 2**31 bytes and more: the flat-address twins at their trigger ---------------------------------------------------
def _need_memory(dev, device_gb, host_gb):
    free = torch.cuda.mem_get_info(dev)[0] / 2 ** 30
    avail = next(int(line.split()[1]) for line in open("/proc/meminfo") if line.startswith("MemAvailable")) / 2 ** 20
    if free < device_gb or avail < host_gb:
        pytest.fail(f"the 2**31-byte case needs {device_gb} GB of device and {host_gb} GB of host memory; free: {free:.1f} / {avail:.1f} GB")


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W,C,k,family", [(41, 320, 320, 256, 1, "conv1x1_stream_kernel"), (82, 320, 320, 128, 3, "conv_gemm_rs_kernel")],
                         ids=["1x1-41x320x320x256", "3x3-82x320x320x128"])
def test_operands_beyond_2_31_bytes_bit_equal(dev, N, H, W, C, k, family):
    """C -> C stride-1 layers whose bf16 activation (x for forward and wgrad, dy for dgrad and wgrad) spans [2**31 bytes, 2**31
    elements): the library stages such an operand through flat 64-bit addresses instead of buffer descriptors (`< (1ull << 31)` bytes
    in csrc/conv.hip's launch_gemm_row for the stream and row-shift kernels and in csrc/conv_host.hip's launch_wgrad for the 1x1 weight gradient) and rejects 2**31 elements.
    et_conv2d_kernel_name reports the kernel FAMILY only -- the flat twin carries the same plan and the name does not tell the two
    forms apart -- so the selection is pinned by the size predicate itself, evaluated here on the operand, with ET_CONV_BUF_DMA unset.
    Forward, dgrad and wgrad are compared in EVERY element; the reference is built a few images at a time (the images of a batch are
    independent in forward and dgrad, the weight gradient is the exact sum of the per-chunk gradients).  Forward / dgrad operands are
    integers in [-3, 3] (|y| <= 9 K < 2**24); the weight gradient sums M = N H W products, so its operands are in [-1, 1] (M < 2**24)."""
    import os
    from efficientteacher_amd import ops
    dt, p = torch.bfloat16, k // 2
    elems = N * H * W * C
    assert "ET_CONV_BUF_DMA" not in os.environ
    assert elems * 2 >= 1 << 31 and elems < 1 << 31, "the activation must lie in [2**31 bytes, 2**31 elements)"
    assert ops.kernel_name("fwd", dt, N, H, W, C, C, k, 1, p).startswith(family)
    assert ops.kernel_name("dgrad", dt, N, H, W, C, C, k, 1, p).startswith(family)
    E.require_exact(k * k * C * 9, "conv(|x|, |w|).max()")
    E.require_exact(N * H * W, "wgrad(|x|, |dy|).max()")
    _need_memory(dev, 16, 24)
    case = (N, H, W, C, C, k, 1, p)
    CH = 2
    chunks = [(n0, min(N, n0 + CH)) for n0 in range(0, N, CH)]

    def chunk(n0, n1, a, seed):
        return E.int_tensor((n1 - n0, H, W, C), -a, a, 1.0, seed * 1000 + n0, torch.int8)

    def whole(a, seed):
        t = torch.empty((N, H, W, C), dtype=dt, device=dev)
        for n0, n1 in chunks:
            t[n0:n1] = chunk(n0, n1, a, seed).to(dt).to(dev)
        return t

    w = E.int_tensor((C, k, k, C), -3, 3, 1.0, 7)
    wd = w.to(dt).to(dev)
    # forward
    x = whole(3, 1)
    y = ops.conv2d_fwd(x, wd, 1, p)
    for n0, n1 in chunks:
        ref = E.stored(E.conv_ref(chunk(n0, n1, 3, 1), w, 1, p), dt)
        same(y[n0:n1], ref, lambda i, n0=n0: f"fwd, images from {n0}: " + tile_hint("fwd", dt, case)((i[0] + n0,) + tuple(i[1:])))
    del x, y
    # dgrad
    dy = whole(3, 2)
    dx = ops.conv2d_dgrad(dy, ops.weight_transpose(wd), (H, W), 1, p)
    for n0, n1 in chunks:
        ref = E.stored(E.dgrad_ref(chunk(n0, n1, 3, 2), w, (H, W), 1, p), dt)
        same(dx[n0:n1], ref, lambda i, n0=n0: f"dgrad, images from {n0}: " + tile_hint("dgrad", dt, case)((i[0] + n0,) + tuple(i[1:])))
    del dy, dx
    # wgrad
    x, dy = whole(1, 3), whole(1, 4)
    dw = torch.zeros((C, k, k, C), dtype=torch.float32, device=dev)
    ops.conv2d_wgrad(x, dy, dw, k, 1, p)
    ref = torch.zeros((C, k, k, C), dtype=E.REF)
    for n0, n1 in chunks:
        ref += E.wgrad_ref(chunk(n0, n1, 1, 3), chunk(n0, n1, 1, 4), k, 1, p)
    same(dw, E.stored(ref, torch.float32), tile_hint("wgrad", dt, case))
    del x, dy, dw
    torch.cuda.empty_cache()


# ---- weight gradients through the product's own launch path: ops.WGRAD_QUEUE ---------------------------------------------------------
class _Bottleneck(torch.autograd.Function):
    """stands for one Bottleneck's backward: it hands its two weight gradients (3x3 cv2 first, then 1x1 cv1) to the queue, as
    efficientteacher_amd/autograd.py does from inside the autograd engine"""
    @staticmethod
    def forward(ctx, t, items):
        ctx.items = items
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        from efficientteacher_amd import ops
        for x, dy, dw, k in ctx.items:
            ops.WGRAD_QUEUE.submit(x, dy, dw, k, 1, k // 2)
        return g, None


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_wgrad_queue_arena_bit_equal(dev, dt):
    """The 3x3 and 1x1 stride-1 layers of the nine bottlenecks of YOLOv5l's C3 stage at 40 x 40 (256 -> 256, B = 32), submitted to
    ops.WGRAD_QUEUE from inside a backward pass as the fused autograd nodes do: groups of eight launched when full on the side stream
    (ET_WGRAD_STREAM default), the ninth layer of each shape flushed by the end-of-backward callback, the launching stream joined.  Read
    on the launching stream right after backward(), every slice of the (pre-filled, integer) gradient arena must hold its own layer's
    exact gradient and the gaps between the slices must be untouched -- the ordering property: nothing reads the arena before the
    side stream's launches have landed."""
    import os
    from efficientteacher_amd import ops
    assert "ET_WGRAD_STREAM" not in os.environ
    q = ops.WGRAD_QUEUE
    q.reset()
    assert q.use_side == 1 and q.group == 8
    B, H, W, C, NB = 32, 40, 40, 256, 9
    assert (H, W, C, C, 3, 1, 1) in SHAPES["v5l-ssod"] and (H, W, C, C, 1, 1, 0) in SHAPES["v5l-ssod"]
    sizes = [C * k * k * C for _ in range(NB) for k in (3, 1)]
    GAP = 48
    pre = E.int_tensor((sum(sizes) + GAP * (len(sizes) + 1),), -3, 3, 1.0, 90, torch.float32)
    want = pre.clone().double()
    arena = pre.clone().to(dev)
    blocks, off, slices = [], GAP, []
    for i in range(NB):
        items = []
        for k in (3, 1):
            P = E.Problem((B, H, W, C, C, k, 1, k // 2), seed=10 + i)
            n = C * k * k * C
            assert P.dw().abs().max().item() + 3 < E.LIMIT
            want[off:off + n] += P.dw().reshape(-1)
            items.append((P.x.to(dt).to(dev), P.dy.to(dt).to(dev), arena[off:off + n].view(C, k, k, C), k))
            slices.append((off, n, k, i))
            off += n + GAP
        blocks.append(items)
    t = torch.zeros(1, device=dev, requires_grad=True)
    out = t
    for items in blocks:
        out = _Bottleneck.apply(out, items)
    out.sum().backward()
    assert not q.pending and not q._dirty, "backward() returned with weight gradients queued or the side stream not joined"
    assert dev in q._side or torch.device("cuda", 0) in q._side, "the side stream was never used"
    got = arena.clone()                                       # on the launching stream, no synchronize: the join is what orders it
    wantf = E.stored(want, torch.float32)
    for off, n, k, i in slices:
        case = (B, H, W, C, C, k, 1, k // 2)
        same(got[off:off + n].view(C, k, k, C), wantf[off:off + n].view(C, k, k, C),
             lambda idx, i=i, case=case: f"bottleneck {i}: " + tile_hint("wgrad", dt, case)(idx))
    assert torch.equal(got.cpu(), wantf), "a gap between the gradient slices was written"
