"""Train-mode BatchNorm + SiLU of a 1x1 `Conv` block in float64, per element, with DERIVED error bounds for the HIP kernels
(csrc/norm.hip, the statistics / BatchNorm-backward sums of the conv epilogue in csrc/conv.hip).  A plain module: no fixtures, no GPU.

Operands are what the kernels read: x (P, K) and w (C, K) of the 1x1 conv in the storage type, gamma / beta (fp32), the residual and
dz in the storage type, and y_st = the y the conv kernel STORED.  Everything below is torch.float64 on the CPU.

The reference (what the kernels define, restated in float64)
    y64    = x @ w.T                                   exact products, float64 sums
    mean   = sum(y64) / P,  var = sum(y64^2) / P - mean^2      (the epilogue sums its fp32 accumulators, NOT the rounded y)
    invstd = 1 / sqrt(var + eps),  eps = float32(1e-3)
    u      = (y_st - mean) * invstd * gamma + beta     = y_st * scale + shift,  scale = gamma * invstd, shift = beta - mean * scale
    z      = silu(u) + residual
    running_mean = (1 - m) * running_mean + m * mean,  running_var = (1 - m) * running_var + m * var * P / (P - 1),  m = float32(0.03)
    du     = dz_st * silu'(u),  silu'(u) = s * (1 + u * (1 - s)),  s = 1 / (1 + exp(-u))
    dbeta += sum(du),  dgamma += sum(du * xhat),  xhat = (y_st - mean) * invstd
    dy     = gamma * invstd * (du - sum(du) / P - xhat * sum(du * xhat) / P)

The bounds.  r = 2^-24 is the unit roundoff of fp32: one fp32 operation (add, mul, fma, conversion from fp64) returns its exact result
times (1 + d), |d| <= r.  A `^` marks the upper end of a per-channel quantity that itself carries an error (is^ = invstd + d_invstd,
...): the statistics terms are NOT small for an ill-conditioned channel, so they are never linearised.  The remaining second-order
products (r * r, r * d_u) are covered by the factor HO = 1 + 2^-10 on every pre-store sum.  Nothing here is fitted to a measurement.

 1. Accumulators.  a = the fp32 MFMA accumulator of y.  K products (exact for the 16-bit types, rounded once in fp32) and K - 1
    additions; the MFMA's internal addition is not documented to round to nearest, so one full ulp (2r) per accumulated term:
        |a - y64| <= e_a = 2 (K + 1) r (|x| @ |w|.T).
    y_st = a rounded to the storage type:  |y_st - y64| <= e_a + half_spacing(|y64| + e_a).
 2. Sums of fp32 terms.  A sum of terms t_i added in fp32 in ANY order has error <= n r sum|t_i|, n = the largest number of fp32
    additions one term passes through before the fp64 fold.  conv_sum_terms() / reduce_sum_terms() below count n from the exported
    geometry (et_conv2d_stats_rows_for / et_conv2d_stats_adds_for / et_bn_reduce_rows).  So
        E_S = sum(e_a) + n r sum(|y64| + e_a)
        E_Q = sum(2 |y64| e_a + e_a^2) + (n + 1) r sum((|y64| + e_a)^2)          (+1: v * v is rounded when it is not an fma)
    The fp64 fold and the fp64 finalize arithmetic (2^-53) are not counted.
 3. Statistics.  d_mean = E_S / P.  d_var = E_Q / P + 2 |mean| d_mean + d_mean^2: an ABSOLUTE error, proportional to
    kappa = 1 + mean^2 / var relative to var -- the price of fp32 sums of y and y^2 in the epilogue.  The kernel clamps var at 0, so
    invstd_k lies in [f(var + d_var), f(max(var - d_var, 0))], f(v) = 1 / sqrt(v + eps): d_invstd = the wider side of that interval
    + r f(.) for the conversion to fp32.  A constant channel (var = 0, kappa infinite) needs no special case.
    save_mean: d_mean_f = d_mean + r mean^.   save_invstd: d_invstd.
    scale = fl(gamma * invstd_k):            d_scale = |gamma| d_invstd + r |gamma| is^
    shift = fl(beta - fl(mean_f * scale)):   d_shift = |mean| d_scale + scale^ d_mean_f + r (2 mean^ scale^ + |beta|)
    running_mean = fl(fl((1 - m) rm) + fl(m mean_f)): d = m d_mean_f + 2 r ((1 - m) |rm| + m mean^)
    running_var the same with unb = var P / (P - 1) converted to fp32: d_unb = d_var P / (P - 1) + r unb^.
 4. u.  Before its roundings the kernel's u is (y_st - mean_f) * scale_k + beta exactly, because ONE rounded scale_k multiplies
    both y and mean_f; so the statistics enter through |y_st - mean| and not through |y_st| + |mean|.  The ROUNDINGS of the folded
    form are absolute in |y * scale|, |mean * scale| and |beta|:
        d_u = |y_st - mean| d_scale_stat + scale^ d_mean_f                        d_scale_stat = |gamma| d_invstd
              + r (|y_st| scale^ + 2 mean^ scale^ + |beta| + |gamma| is^ |y_st - mean| + |u|)
    (rounding of scale, of mean_f * scale, of the subtraction, of y * scale, of the final addition).
 5. SiLU.  s_k = v_rcp_f32(1 + v_exp_f32(-u log2 e)).  The product with log2 e and the rounded constant move the exponent by
    2 |u| r relative to e^-u, v_exp_f32 is 1 ulp = 2 r; e enters s through -(1 - s); the addition is r, v_rcp_f32 1 ulp = 2 r:
        rel(s_k) <= ev_s = ((1 - s)(2 |u| + 2) + 3) r.
    Absolute floor FLOOR = 2^-126 on s_k: v_exp_f32 returns +inf for -u > 88.7, so s_k = 0 where s = e^u < 2^-127, and v_rcp_f32 /
    v_exp_f32 flush denormal results; no other floor exists.
        silu:  d_z0 = |u| (s ev_s + FLOOR) + r |z0| + |silu'(u)| d_u + 0.25 d_u^2           (|silu''| <= 0.5, Taylor)
        z = fl(z0 + residual): + r |z|.
    The gate g = s (1 + u (1 - s)) as the three copies compute it (act_grad, the dgrad epilogue's bn_bwd_sums):
        d_s = s ev_s + FLOOR;  q = fl(1 - s): d_q = d_s + r (1 - s);  p = fl(u q): d_p = |u| d_q + r |u| (1 - s);
        w = fl(1 + p): d_w = d_p + r |1 + p|;  g = fl(s w): d_g = s d_w + |w| d_s + r |g|;  + 0.5 d_u  (|g'| = |silu''| <= 0.5).
        du = fl(dz g): d_du = |dz| d_g + r |du|.
 6. Backward totals.  S1 = sum du: E_1 = sum d_du + n r sum(|du| + d_du).  The second total is formed from sums of du and du * y:
    is_f (s2 - mean_f s1), per THREAD in fp32 in the reduce kernel (three roundings), once per channel in fp64 after a dgrad
    epilogue.  Before roundings that is is_f sum du_k (y - mean_f), so
        E_2 = sum d_du |y - mean| is^ + sum (|du| + d_du)(d_mean_f is^ + |y - mean| d_invstd)
              + is^ (n + 4) r (sum (|du| + d_du) |y| + mean^ sum (|du| + d_du))
    -- the last line is kappa again: the terms du * y and mean * du cancel.
    dbeta = fl(dbeta0 + (float)S1): E_1 + r (|S1| + E_1) + r (|dbeta| + E_1); dgamma the same with E_2.
 7. dy.  k0 = fl(gamma is_f), k1 = (float)(S1 / P), k2 = (float)(S2 / P), w = fl(is_f k2); the apply pass evaluates
    A du + (B y + D), A = k0, B = fl(-k0 w), D = fl(k0 fl(fl(mean_f w) - k1)) = k0 (du - k1 - w (y - mean_f)) before roundings:
        d_k0 = |gamma| d_invstd + r |gamma| is^,  d_k1 = E_1 / P + r k1^,  d_k2 = E_2 / P + r k2^,
        d_w  = is^ d_k2 + |k2| d_invstd + r is^ k2^
        d_dy = k0^ (d_du + d_k1 + |y - mean| d_w + w^ d_mean_f) + d_k0 |du - k1 - w (y - mean)|
               + r (3 k0^ w^ |y| + 2 k0^ (2 mean^ w^ + k1^) + k0^ (|du| + d_du) + |dy|)
    (roundings of B, B y, mean_f w, the subtraction, D, B y + D, A du and the last addition).
 8. Store.  A value v computed with pre-store error e is within e + half the spacing of the storage type at |v_ref| + e of the
    reference (round to nearest even: v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32), subnormal spacing included.
"""
import math

import numpy as np
import torch

R = 2.0 ** -24
HO = 1.0 + 2.0 ** -10
FLOOR = 2.0 ** -126
EPS = float(np.float32(1e-3))
MOM = float(np.float32(0.03))
ONE_M = float(np.float32(1.0) - np.float32(0.03))
F64 = torch.float64
_FMT = {torch.float32: (24, -126), torch.bfloat16: (8, -126), torch.float16: (11, -14)}      # significand bits, minimum exponent
FP16_MAX = 65504.0


def half_spacing(v, dtype):
    """half the distance between neighbouring values of `dtype` at magnitude v (float64 tensor), subnormal range included"""
    p, emin = _FMT[dtype]
    _, e = torch.frexp(v.abs())                                  # |v| = m 2^e, 0.5 <= m < 1  (e = 0 for v = 0)
    e = torch.clamp(e - 1, min=emin).to(F64)
    return torch.exp2(e - p)


def conv_sum_terms(P, rows=None, adds=None):
    """n of section 2 for the conv epilogue's sums.  A partial row (or the sum a workgroup adds to a shard) holds one workgroup's /
    wave's share of the P pixels, rounded up to whole tiles of at most 256 rows at both ends; a sharded sum then meets up to `adds`
    earlier atomic additions on its address.  Never more than P: a term meets at most P - 1 additions of something other than zero."""
    if adds is not None:
        return min(P, -(-P // adds) + 512 + adds)
    return min(P, -(-P // rows) + 512)


def reduce_vectors_per_thread(P, CV, blocks):
    return -(-(P * CV) // (blocks * 256))


def reduce_sum_terms(P, CV, blocks, sharded):
    """n for the reduce pass of bn_act_bwd: vectors per thread (pairs are added first: + 1), <= 6 xor-shuffle steps, <= 256 LDS
    atomics per address, then fp64 partial rows -- or one fp32 atomic per block on shard (block % 16); never more than P"""
    n = reduce_vectors_per_thread(P, CV, blocks) + 1 + 6 + 256
    return min(P, n + (-(-blocks // 16) if sharded else 0))


def _d(t):
    return t.detach().to("cpu").to(F64)


def _sigmoid(u):
    return 1.0 / (1.0 + torch.exp(-u))


class Ref:
    """attributes: reference values (float64) and `b_<name>` bounds; see forward() / backward()"""


def _act_bounds(u, d_u):
    """(s, ev_s) of section 5"""
    s = _sigmoid(u)
    ev_s = ((1.0 - s) * (2.0 * u.abs() + 2.0) + 3.0) * R
    return s, ev_s


def silu_fwd_error(u, d_u):
    """(silu(u), d_z0 of section 5): the activation alone -- before the residual, the factor HO and the store"""
    s, ev_s = _act_bounds(u, d_u)
    z0 = u * s
    g = s * (1.0 + u * (1.0 - s))
    return z0, u.abs() * (s * ev_s + FLOOR) + R * z0.abs() + g.abs() * d_u + 0.25 * d_u * d_u


def _silu_fwd(u, d_u, res, dtype):
    z0, e = silu_fwd_error(u, d_u)
    z = z0 if res is None else z0 + res
    if res is not None:
        e = e + R * z.abs()
    e = HO * e
    return z, e + half_spacing(z.abs() + e, dtype)


def _affine_u(y_st, mean, gamma, beta, invstd, d_is, d_mean_f, mean_h, is_h):
    """u and d_u of section 4 (per element) + the per-channel scale / shift with their bounds"""
    sc = gamma * invstd
    sh = beta - mean * sc
    d_sc_stat = gamma.abs() * d_is
    d_sc = d_sc_stat + R * gamma.abs() * is_h
    sc_h = sc.abs() + d_sc
    d_sh = mean.abs() * d_sc + sc_h * d_mean_f + R * (2.0 * mean_h * sc_h + beta.abs())
    xc = y_st - mean
    u = xc * sc + beta
    d_u = xc.abs() * d_sc_stat + sc_h * d_mean_f + R * (y_st.abs() * sc_h + 2.0 * mean_h * sc_h + beta.abs()
                                                       + gamma.abs() * is_h * xc.abs() + u.abs())
    return sc, sh, HO * d_sc, HO * d_sh, u, HO * d_u


def z_of(f, residual):
    """(z, b_z) = silu(u) + residual (None: without) for forward()'s / eval_affine()'s result"""
    return _silu_fwd(f.u, f.d_u, None if residual is None else _d(residual), f.dtype)


def from_stored(y_st, gamma, beta, dtype):
    """for a test that feeds the backward WITHOUT a conv in front: the statistics of the stored y itself, which the test computes
    in float64 and rounds once to fp32 (`mean`, `invstd`), scale = gamma * invstd and shift = beta - mean * scale in fp32.  That is
    forward() with exact accumulators (e_a = 0) and no fp32 sums (n = 0): only the roundings of section 3 remain."""
    y = _d(y_st)
    C = y.shape[1]
    one = torch.ones(C)
    return forward(y, torch.eye(C, dtype=F64), y, gamma, beta, 0.0 * one, one, 0, dtype, acc_ulps=0.0)


def forward(x, w, y_st, gamma, beta, rm0, rv0, n_terms, dtype, acc_ulps=2.0):
    """x (P, K), w (C, K), y_st (P, C) in the storage type, gamma / beta / rm0 / rv0 (C,) fp32; n_terms: section 2.
    -> Ref with y64, mean, var, invstd, scale, shift, u, rm, rv and b_y, b_mean, b_invstd, b_scale, b_shift, b_rm, b_rv; z: z_of()."""
    x, w, y_st, gamma, beta, rm0, rv0 = map(_d, (x, w, y_st, gamma, beta, rm0, rv0))
    P, K = x.shape
    f = Ref()
    f.P, f.dtype, f.y_st, f.gamma, f.beta = P, dtype, y_st, gamma, beta
    f.y64 = x @ w.T
    e_a = acc_ulps * (K + 1) * R * (x.abs() @ w.abs().T)
    f.b_y = e_a + half_spacing(f.y64.abs() + e_a, dtype)
    ya = f.y64.abs() + e_a
    E_S = e_a.sum(0) + n_terms * R * ya.sum(0)
    E_Q = (2.0 * f.y64.abs() * e_a + e_a * e_a).sum(0) + (n_terms + 1) * R * (ya * ya).sum(0)
    f.mean = f.y64.sum(0) / P
    f.var = ((f.y64 - f.mean) ** 2).sum(0) / P                 # == sum(y64^2) / P - mean^2, without the cancellation
    d_mean = E_S / P
    f.d_var = E_Q / P + 2.0 * f.mean.abs() * d_mean + d_mean * d_mean
    f.kappa = 1.0 + f.mean ** 2 / f.var
    inv = lambda v: 1.0 / torch.sqrt(v + EPS)
    f.invstd = inv(f.var)
    lo, hi = inv(f.var + f.d_var), inv(torch.clamp(f.var - f.d_var, min=0.0))
    f.d_is = torch.maximum(f.invstd - lo, hi - f.invstd) + R * hi
    f.is_h = f.invstd + f.d_is
    f.mean_h = f.mean.abs() + d_mean
    f.d_mean_f = d_mean + R * f.mean_h
    f.b_mean, f.b_invstd = f.d_mean_f, f.d_is
    f.scale, f.shift, f.b_scale, f.b_shift, f.u, f.d_u = _affine_u(y_st, f.mean, gamma, beta, f.invstd, f.d_is, f.d_mean_f, f.mean_h, f.is_h)
    f.rm = ONE_M * rm0 + MOM * f.mean
    f.b_rm = HO * (MOM * f.d_mean_f + 2.0 * R * (ONE_M * rm0.abs() + MOM * f.mean_h))
    k = P / (P - 1.0) if P > 1 else 1.0
    unb = f.var * k
    d_unb = f.d_var * k + R * (unb + f.d_var * k)
    f.rv = ONE_M * rv0 + MOM * unb
    f.b_rv = HO * (MOM * d_unb + 2.0 * R * (ONE_M * rv0.abs() + MOM * (unb + d_unb)))
    return f


def eval_affine(y_st, gamma, beta, rm, rv, dtype):
    """the eval-mode affine from the running statistics the kernel holds (rm, rv: its fp32 outputs, taken as operands):
    scale = gamma / sqrtf(rv + eps) -- addition r, sqrtf and the division 1 ulp each (2 r; half of the addition's r passes the
    square root): 5 r relative, written as an error of `invstd`; shift and u as in sections 3 / 4 with d_mean = 0.
    -> Ref with scale, shift, u and b_scale, b_shift; z: z_of()"""
    y_st, gamma, beta, rm, rv = map(_d, (y_st, gamma, beta, rm, rv))
    e = Ref()
    inv = 1.0 / torch.sqrt(rv + EPS)
    d_is = 5.0 * R * inv
    zero = torch.zeros_like(rm)
    e.dtype = dtype
    e.scale, e.shift, e.b_scale, e.b_shift, e.u, e.d_u = _affine_u(y_st, rm, gamma, beta, inv, d_is, zero, rm.abs(), inv + d_is)
    return e


def backward(f, dz_st, dgamma0, dbeta0, n_terms, silu=True):
    """f: forward()'s result (the backward kernels read the forward's fp32 scale / shift / mean / invstd, so its statistics errors
    carry over); dz_st (P, C) in the storage type; dgamma0 / dbeta0: the buffers' contents before the call; silu=False: no
    activation (the gate is the constant 1: du = dz exactly).
    -> Ref with du, dbeta, dgamma, dy and b_dbeta, b_dgamma, b_dy"""
    dz, dg0, db0 = map(_d, (dz_st, dgamma0, dbeta0))
    P, dtype, y, gamma = f.P, f.dtype, f.y_st, f.gamma
    b = Ref()
    u, d_u = f.u, f.d_u
    s, ev_s = _act_bounds(u, d_u)
    d_s = s * ev_s + FLOOR
    d_q = d_s + R * (1.0 - s)
    p = u * (1.0 - s)
    d_p = u.abs() * d_q + R * p.abs()
    wv = 1.0 + p
    d_w = d_p + R * wv.abs()
    g = s * wv
    d_g = s * d_w + wv.abs() * d_s + R * g.abs() + 0.5 * d_u
    if not silu:
        g, d_g = torch.ones_like(u), torch.zeros_like(u)
    b.du = dz * g
    d_du = HO * (dz.abs() * d_g + R * b.du.abs())
    dua = b.du.abs() + d_du
    xc = y - f.mean
    xhat = xc * f.invstd
    S1 = b.du.sum(0)
    S2 = (b.du * xhat).sum(0)
    E1 = HO * (d_du.sum(0) + n_terms * R * dua.sum(0))
    E2 = HO * ((d_du * xc.abs()).sum(0) * f.is_h + (dua * (f.d_mean_f * f.is_h + xc.abs() * f.d_is)).sum(0)
               + f.is_h * (n_terms + 4) * R * ((dua * y.abs()).sum(0) + f.mean_h * dua.sum(0)))
    b.dbeta = db0 + S1
    b.dgamma = dg0 + S2
    b.b_dbeta = E1 + R * (S1.abs() + E1) + R * (b.dbeta.abs() + E1)
    b.b_dgamma = E2 + R * (S2.abs() + E2) + R * (b.dgamma.abs() + E2)
    k0, k1, k2 = gamma * f.invstd, S1 / P, S2 / P
    d_k0 = gamma.abs() * f.d_is + R * gamma.abs() * f.is_h
    k0_h = k0.abs() + d_k0
    d_k1 = E1 / P + R * (k1.abs() + E1 / P)
    k1_h = k1.abs() + d_k1
    d_k2 = E2 / P + R * (k2.abs() + E2 / P)
    k2_h = k2.abs() + d_k2
    wc = f.invstd * k2
    d_wc = f.is_h * d_k2 + k2.abs() * f.d_is + R * f.is_h * k2_h
    wc_h = wc.abs() + d_wc
    T = b.du - k1 - wc * xc
    b.dy = k0 * T
    e = k0_h * (d_du + d_k1 + xc.abs() * d_wc + wc_h * f.d_mean_f) + d_k0 * T.abs() \
        + R * (3.0 * k0_h * wc_h * y.abs() + 2.0 * k0_h * (2.0 * f.mean_h * wc_h + k1_h) + k0_h * dua + b.dy.abs())
    e = HO * e
    b.b_dy = e + half_spacing(b.dy.abs() + e, dtype)
    return b


def ratio(got, ref, bound):
    """worst |got - ref| / bound over all elements (0 / 0 -> 0: an exact result under a zero bound passes); inf / nan in `got` -> inf"""
    got = _d(got).reshape(ref.shape)
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))
    return float(r.max())
