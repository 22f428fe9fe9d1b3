"""The conv family (forward with its statistics and fused epilogue, dgrad, wgrad) in float64, per element, with DERIVED error bounds for
the HIP kernels of csrc/conv.hip, csrc/conv_stem.hip and csrc/conv_wgrad.hip.  A plain module: no fixtures, no GPU.  The constants, the
store rule, the SiLU bound and the fp32-sum count are tests/bn_ref.py's (sections 1, 2, 5, 8 of its docstring); this docstring derives
what the conv kernels add.

Operands are what the kernels read: x (N, H, W, Cin), w (Cout, k, k, Cin), dy (N, OH, OW, Cout), the residual and the old output in the
storage type; scale, bias and dw in fp32.  Everything below is torch.float64 on the CPU.

The reference (what the kernels define, restated in float64)
    y64  = conv(x, w)                                   exact products, float64 sums
    S, Q = sum(y64), sum(y64^2) over the pixels         (the epilogue sums its fp32 accumulators, NOT the stored y)
    v    = y64 * scale + bias,  z0 = silu(v) | max(v, 0) | v,  z = z0 + residual + old output
    dx64 = conv_transpose(dy, w)                        the same epilogue without scale / bias / activation
    dw64 = dw0 + sum over pixels of dy (x) x

The bounds.  r, HO, FLOOR as in bn_ref.  Nothing here is fitted to a measurement.

 1. Forward accumulator.  K_e = taps_inside * Cin products really enter an output element (a conv of ones: a border pixel has fewer taps
    inside), A = conv(|x|, |w|).  One full ulp (2 r) per accumulated term, in any order (bn_ref section 1), so it holds for every K-chunking
    and tap order of every tile family, for the k-ordered fmaf chain of the fp32 MFMA, and for zero-filled (out-of-image) operands:
        |a - y64| <= e_a = 2 (K_e + 1) r A.
    The bound is relative to A, not to |y64|: where the products cancel (|y64| << A) an error of r A is legitimate.
 2. Plain store.  |y_st - y64| <= e_a + half_spacing(|y64| + e_a); fp32 outputs are the accumulator itself: e_a.
 3. Forward statistics.  Per-lane fp32 sums of a and of a * a, then xor-shuffles, LDS rows and either partial rows (folded in fp64 by
    the reader) or one fp32 atomic per workgroup on a shard.  bn_ref section 2 with n = conv_sum_terms(P, rows | adds):
        E_S = sum(e_a) + n r sum(|y64| + e_a),   E_Q = sum(2 |y64| e_a + e_a^2) + (n + 1) r sum((|y64| + e_a)^2).
 4. Fused epilogue.  v_k = fl(a * scale + bias) as an fma or as two operations -- both roundings are charged:
        d_v = |scale| e_a + r (|a scale| + |v|),   |a scale| <= (|y64| + e_a) |scale|.
    Without scale and bias (dgrad, the plain forward) v_k = a and d_v = e_a.
    ACT_SILU: v * v_rcp_f32(1 + v_exp_f32(-v log2 e)): bn_ref section 5 with u = v, d_u = d_v (FLOOR is the only absolute floor; the
    copies -- the guarded 16-bit vector path, the fp32 vector path, the scalar tail of a ragged Cout, the DEFER form of the persistent 1x1
    kernel with its constants in LDS, the stem's own -- are the same expression).  ACT_RELU: max(v, 0) is exact and 1-Lipschitz: d_v.
    The residual and -- for `accumulate` -- the old output are exact storage-type values, each added in fp32: + r |z| after each.
    The pre-store sum carries HO (r * r, r * d_v, and a's own error inside |a scale| and |z|); then the store rule (bn_ref section 8).
 5. dgrad.  The same with the roles swapped: dx64 = conv_transpose(dy, w), A from the absolute values, K_e = taps_reaching * Cout per
    input pixel (a conv_transpose of ones: for stride 2 it differs by parity class -- 1, 2, 2, 4 taps of a 3x3 -- and at the border).
    A parity class that no tap reaches (k < stride) has K_e = 0: the host fills it with zeros, or leaves the old value under
    `accumulate`; its bound is exactly 0.
 6. wgrad.  dw64 = dw0 + sum_p dy[p] x[p + tap]; P_e = pixels whose tap lies inside the image (a border tap has fewer), B = sum |dy| |x|.
    The pixel sum is split over workgroups (K-split) whose fp32 partial sums meet in hardware fp32 atomics in no fixed order; the charge of
    2 r per term and addition does not depend on the order or on where a partial sum ends, which is what makes
        |dw - dw64| <= 2 (P_e + 1) r B + r (|dw0| + |dw64|)
    valid for the K-split: the last term is the addition that meets dw0 and the rounding of the result; the S - 1 further atomics of an
    S-way split round a running total of at most |dw0| + B each and are paid from the first term, whose own use is 2 (P_e / S + 1) r B
    for even splits -- so the test's dw0 is of the order of dw64 - dw0, not orders above B.  For an interior tap of a large map
    P_e r B is of the order of the old blanket 1e-4 max|dw|: the bound is NOT much tighter there.  The gain is per element: border taps
    (small P_e), channels of small magnitude (B scales with them, a blanket relative to the tensor's maximum does not), a non-zero dw0.
"""
import torch
import torch.nn.functional as F

from tests.bn_ref import F64, FLOOR, FP16_MAX, HO, R, conv_sum_terms, half_spacing, ratio, silu_fwd_error  # noqa: F401  (re-exported)

ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2


def _d(t):
    return t.detach().to("cpu").to(F64)


def _cf(t):
    """NHWC -> NCHW"""
    return t.permute(0, 3, 1, 2)


def _cl(t):
    """NCHW -> NHWC"""
    return t.permute(0, 2, 3, 1).contiguous()


class Acc:
    """y64, A, K_e, e_a of one conv problem (output layout NHWC); P = output pixels"""


def _acc(y64, A, Ke):
    f = Acc()
    f.y64, f.A, f.Ke = y64, A, Ke.expand_as(y64)
    f.e_a = 2.0 * (f.Ke + 1.0) * R * A
    f.P = y64.shape[0] * y64.shape[1] * y64.shape[2]
    return f


def fwd_acc(x, w, stride, pad):
    """section 1: x (N, H, W, Cin), w (Cout, k, k, Cin)"""
    x, w = _cf(_d(x)), _cf(_d(w))
    conv = lambda a, b: _cl(F.conv2d(a, b, stride=stride, padding=pad))
    Ke = conv(torch.ones_like(x[:1]), torch.ones_like(w[:1]))
    return _acc(conv(x, w), conv(x.abs(), w.abs()), Ke)


def dgrad_acc(dy, w, in_hw, stride, pad):
    """section 5: dy (N, OH, OW, Cout), w (Cout, k, k, Cin) of the FORWARD conv -> dx (N, IH, IW, Cin)"""
    dy, w = _cf(_d(dy)), _cf(_d(w))
    k = w.shape[2]
    op = tuple(in_hw[i] - ((dy.shape[2 + i] - 1) * stride - 2 * pad + k) for i in range(2))
    ct = lambda a, b: _cl(F.conv_transpose2d(a, b, stride=stride, padding=pad, output_padding=op))
    Ke = ct(torch.ones_like(dy[:1]), torch.ones_like(w[:, :1]))
    f = _acc(ct(dy, w), ct(dy.abs(), w.abs()), Ke)
    assert f.y64.shape[1:3] == tuple(in_hw)
    return f


def store(z, e, dtype):
    """sections 2 / bn_ref 8: the bound of a value with pre-store error e"""
    return e if dtype == torch.float32 else e + half_spacing(z.abs() + e, dtype)


def plain(f, dtype):
    """(y64, bound) of the stored accumulator"""
    return f.y64, store(f.y64, f.e_a, dtype)


def stats(f, n_terms):
    """section 3 -> (S, Q, E_S, E_Q), each (C,)"""
    C = f.y64.shape[-1]
    y, e = f.y64.reshape(-1, C), f.e_a.reshape(-1, C)
    ya = y.abs() + e
    E_S = e.sum(0) + n_terms * R * ya.sum(0)
    E_Q = (2.0 * y.abs() * e + e * e).sum(0) + (n_terms + 1) * R * (ya * ya).sum(0)
    return y.sum(0), (y * y).sum(0), E_S, E_Q


def epilogue(f, dtype, scale=None, bias=None, act=ACT_NONE, residual=None, old=None):
    """section 4 -> (z, bound).  old: the output's contents before an `accumulate` call.  An element with K_e = 0 (section 5) under a
    plain or accumulate-only epilogue is exact."""
    y, e_a = f.y64, f.e_a
    if scale is None and bias is None:
        v, d_v = y, e_a
    else:
        sc = torch.ones(y.shape[-1], dtype=F64) if scale is None else _d(scale)
        bi = torch.zeros(y.shape[-1], dtype=F64) if bias is None else _d(bias)
        v = y * sc + bi
        d_v = sc.abs() * e_a + R * ((y.abs() + e_a) * sc.abs() + v.abs())
    if act == ACT_SILU:
        z, e = silu_fwd_error(v, d_v)
    elif act == ACT_RELU:
        z, e = torch.clamp(v, min=0.0), d_v
    else:
        z, e = v, d_v
    for t in (residual, old):
        if t is not None:
            z = z + _d(t)
            e = e + R * z.abs()
    if not (scale is None and bias is None and act == ACT_NONE and residual is None and old is None):
        e = HO * e
    b = store(z, e, dtype)
    if scale is None and bias is None and act == ACT_NONE and residual is None:
        b = torch.where(f.Ke == 0, torch.zeros_like(b), b)
    return z, b


def wgrad(x, dy, dw0, k, stride, pad):
    """section 6: x (N, H, W, Cin), dy (N, OH, OW, Cout) in the storage type, dw0 (Cout, k, k, Cin) fp32 = the buffer before the call
    -> (dw64, bound)"""
    x, dy, dw0 = _cf(_d(x)), _cf(_d(dy)), _d(dw0)
    Cout, Cin = dy.shape[1], x.shape[1]
    wg = lambda a, b: _cl(torch.nn.grad.conv2d_weight(a, (b.shape[1], a.shape[1], k, k), b, stride=stride, padding=pad))
    Pe = wg(torch.ones_like(x[:, :1]), torch.ones_like(dy[:, :1]))                       # (1, k, k, 1)
    dw = dw0 + wg(x, dy)
    B = wg(x.abs(), dy.abs())
    assert dw.shape == (Cout, k, k, Cin)
    return dw, 2.0 * (Pe + 1.0) * R * B + R * (dw0.abs() + dw.abs())
