"""Return codes of the element-wise and head entry points for ONE wrong argument per call: an unknown dtype code (-2), a NULL
required pointer (-1), a pixel stride that is not whole 16-byte vectors (-2, the NHWC entries) -- and nothing is launched on such a
call: the output tensor keeps the sentinel it was filled with.

Every entry is called through the C ABI (_lib.load()) with valid tensors of the smallest legal shape, an NHWC (1, 2, 2, 8) tensor
or 16 flat elements, 16-bit storage (ET_BF16).  The unchanged argument list returns 0 on the emulator, so each code below is
caused by the one argument that was changed.  The NHWC buffers are twice the size their shape needs: the call with ld = C + 1
would stay inside them even if it launched.
"""
import pytest
import torch

from efficientteacher_amd import _lib

B, H, W, C = 1, 2, 2, 8
P = B * H * W
BF16 = _lib.ET_BF16
SENTINEL = 7.0


class Case:
    """args: the argument list without the stream, tensors as tensors (None = NULL); out: the tensor a launch would write;
    dtype / ptrs / lds: positions in args of the dtype code, of every required pointer and of every checked pixel stride"""

    def __init__(self, args, out, dtype, ptrs, lds=()):
        self.args, self.out, self.dtype, self.ptrs, self.lds = list(args), out, dtype, ptrs, lds


def _builders(m):
    def lp(n=2 * P * C, fill=0.5):          # 16-bit tensor (bf16 storage)
        return torch.full((n,), fill, dtype=torch.bfloat16, device=m.device)

    def f32(n, fill=1.0):
        return torch.full((n,), fill, dtype=torch.float32, device=m.device)

    def out_lp(n=2 * P * C):
        return lp(n, SENTINEL)

    def out_f32(n):
        return f32(n, SENTINEL)

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=m.device)

    def u8(n):
        return torch.zeros(n, dtype=torch.uint8, device=m.device)

    def f64(n):
        return torch.zeros(n, dtype=torch.float64, device=m.device)

    ch = lambda: f32(C)

    def et_bn_act_fwd():
        z = out_lp()
        return Case([lp(), C, z, C, None, 0, BF16, P, C, ch(), ch(), 1], z, 6, (0, 2, 9, 10), (1, 3))

    def et_bn_act_bwd():
        rows = _lib.load().et_bn_reduce_rows(P, C, BF16)
        nws = rows * 2 * C + 3 * C
        dy = out_lp()
        return Case([lp(), C, lp(), C, dy, C, BF16, P, C, ch(), ch(), ch(), ch(), ch(), 1, ch(), ch(), f64(2 * C + 8),
                    f32(nws), nws], dy, 6, (0, 2, 4, 9, 10, 11, 12, 13, 17, 18), (1, 3, 5))

    def et_bn_act_bwd_from_partials():
        dy = out_lp()
        return Case([lp(), C, lp(), C, dy, C, BF16, P, C, ch(), ch(), ch(), ch(), ch(), 1, ch(), ch(),
                    f64(2 * C + 8), f32(2 * C), 1, f32(3 * C)], dy, 6,
                    (0, 2, 4, 9, 10, 11, 12, 13, 17, 18, 20), (1, 3, 5))

    def et_bn_act_fwd_sharded():
        z = out_lp()
        return Case([lp(), C, z, C, None, 0, BF16, P, C, f32(16 * 2 * C), C, float(P), ch(), ch(), 1e-3, 0.03,
                    None, None, ch(), ch(), None, None, 1], z, 6, (0, 2, 9, 12, 13, 18, 19), (1, 3))

    def et_bn_act_bwd_sharded():
        dy = out_lp()
        return Case([lp(), C, lp(), C, dy, C, BF16, P, C, ch(), ch(), ch(), ch(), ch(), 1, ch(), ch(),
                    f32(16 * 2 * C, 0.0), C, 1], dy, 6, (0, 2, 4, 9, 10, 11, 12, 13, 17), (1, 3, 5))

    def et_act_bwd():
        dy = out_lp()
        return Case([lp(), C, lp(), C, dy, C, BF16, P, C, 2], dy, 6, (0, 2, 4), (1, 3, 5))

    def et_pack_input():
        y = out_lp()
        return Case([f32(B * 3 * H * W), y, BF16, B, 3, H, W], y, 2, (0, 1))

    def et_pack_input_u8():
        y = out_lp()
        return Case([u8(B * 3 * H * W), y, BF16, B, 3, H, W, 255.0], y, 2, (0, 1))

    def et_maxpool5_fwd():
        y = out_lp()
        return Case([lp(), C, y, C, u8(2 * P * C), BF16, B, H, W, C], y, 5, (0, 2, 4), (1, 3))

    def et_maxpool5_bwd():
        dx = out_lp()
        return Case([lp(), C, u8(2 * P * C), None, 0, dx, C, BF16, B, H, W, C], dx, 7, (0, 2, 5), (1, 6))

    def et_upsample2x_fwd():
        y = out_lp(2 * 4 * P * C)
        return Case([lp(), C, y, C, BF16, B, H, W, C], y, 4, (0, 2), (1, 3))

    def et_upsample2x_bwd():
        dx = out_lp()
        return Case([lp(2 * 4 * P * C), C, dx, C, BF16, B, H, W, C, 0], dx, 4, (0, 2), (1, 3))

    def et_scale_cast():
        d = out_lp(16)
        return Case([f32(16), d, BF16, 16, 1.0, None], d, 2, (0, 1))

    def et_domain_focal():
        g = out_lp()
        return Case([lp(), C, BF16, P, 0, 1.0, g, C, f32(1, 0.0)], g, 2, (0, 8))

    def et_scale_inplace():
        x = out_lp(16)
        return Case([x, BF16, 16, -1.0, None], x, 1, (0,))

    def et_detect_decode():
        # the (1, 2, 2, 8) head output viewed as (B, na = 1, ny, nx, no = 8); z: (B, A_total = 4, no) fp32
        z = out_f32(P * C)
        return Case([lp(), BF16, B, 1, H, W, C, H * W * C, C, W * C, C, f32(2), 8.0, z, P, 0], z, 1, (0, 11, 13))

    def et_v8_decode():
        # reg_max = 1: 4 sides x 2 bins = 8 regression channels; nc = 8; out: (B, A_total = 4, 5 + nc) fp32
        o = out_f32(P * (5 + C))
        return Case([lp(), C, lp(), C, BF16, B, H, W, 1, C, 8.0, 0.5, o, P, 0], o, 4, (0, 2, 12))

    def et_weight_transpose():
        wT = out_lp(16)
        return Case([lp(16), wT, BF16, 2, 1, 8], wT, 2, (0, 1))

    def et_weight_transpose_all():
        wT = out_lp(16)
        return Case([lp(16), wT, BF16, i32([0, 2, 1, 8]), 1, 16], wT, 2, (0, 1, 3))

    def et_colsum():
        o = out_f32(C)
        return Case([lp(), BF16, P, C, C, o], o, 1, (0, 5))

    def et_cast_f32_to_lp():
        d = out_lp(16)
        return Case([f32(16), d, BF16, 16], d, 2, (0, 1))

    fs = (et_bn_act_fwd, et_bn_act_bwd, et_bn_act_bwd_from_partials, et_bn_act_fwd_sharded, et_bn_act_bwd_sharded, et_act_bwd, et_pack_input,
          et_pack_input_u8, et_maxpool5_fwd, et_maxpool5_bwd, et_upsample2x_fwd, et_upsample2x_bwd, et_scale_cast, et_domain_focal,
          et_scale_inplace, et_detect_decode, et_v8_decode, et_weight_transpose, et_weight_transpose_all, et_colsum, et_cast_f32_to_lp)
    return {f.__name__: f for f in fs}


NAMES = ["et_bn_act_fwd", "et_bn_act_bwd", "et_bn_act_bwd_from_partials", "et_bn_act_fwd_sharded", "et_bn_act_bwd_sharded", "et_act_bwd",
         "et_pack_input", "et_pack_input_u8", "et_maxpool5_fwd", "et_maxpool5_bwd", "et_upsample2x_fwd", "et_upsample2x_bwd",
         "et_scale_cast", "et_domain_focal", "et_scale_inplace", "et_detect_decode", "et_v8_decode", "et_weight_transpose",
         "et_weight_transpose_all", "et_colsum", "et_cast_f32_to_lp"]


def _call(name, args):
    return getattr(_lib.load(), name)(*[_lib.ptr(a) if isinstance(a, torch.Tensor) else a for a in args], _lib.stream())


def _wrong(name, case):
    """(what is wrong, position, value, expected code)"""
    w = [("dtype 3", case.dtype, 3, -2), ("dtype -1", case.dtype, -1, -2)]
    w += [(f"NULL argument {i}", i, None, -1) for i in case.ptrs]
    w += [(f"stride C + 1 at argument {i}", i, C + 1, -2) for i in case.lds]
    if name == "et_cast_f32_to_lp":
        w.append(("dtype ET_F32", case.dtype, _lib.ET_F32, -2))
    return w


@pytest.mark.parametrize("name", NAMES)
def test_one_wrong_argument(hip, name):
    build = _builders(hip)
    assert sorted(build) == sorted(NAMES)
    if hip.emulated:             # the argument list itself is valid (the GPU arm makes the failing calls only: it launches nothing)
        assert _call(name, build[name]().args) == 0
    for what, pos, value, code in _wrong(name, build[name]()):
        case = build[name]()
        case.args[pos] = value
        assert _call(name, case.args) == code, f"{name}, {what}"
        assert torch.equal(case.out, torch.full_like(case.out, SENTINEL)), f"{name}, {what}: the output was written"


def test_bn_reduce_rows_by_vector_width(hip):
    """et_bn_reduce_rows sizes the grid of the backward reduce pass by vectors per pixel: four fp32 or eight 16-bit elements"""
    lib = _lib.load()
    for p, c in ((P, C), (160 * 160, 64), (20 * 20 * 3, 1024)):
        assert lib.et_bn_reduce_rows(p, c, _lib.ET_BF16) == lib.et_bn_reduce_rows(p, c, _lib.ET_F16) == lib.et_bn_reduce_rows(p, c // 2, _lib.ET_F32)
