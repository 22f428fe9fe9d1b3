"""Exact integer conv problems and their fp64 reference (plain module: no tests, no fixtures).

With small integer operands every product and every partial sum below 2**24 is exact in fp32 IN ANY ORDER (MFMA accumulation, split-K,
LDS pre-reduction, fp32 atomics over the statistics shards), and the 16-bit store is a deterministic round-to-nearest-even of an exact
integer: a kernel's output must be BIT-EQUAL to `reference.to(dtype)` at any size.  This module makes such problems (`Problem`),
computes the references with torch's own CPU convolution in fp64, and asserts the EXACTNESS PRECONDITIONS on the reference alone,
before any kernel output is looked at (a violated precondition is an AssertionError of the test, never a skip).

Operand sets of a Problem -- derived from K = taps * Cin and M = output pixels only, never tuned per case:

* the DENSE set (x, w, dy uniform integers in [-3, 3]; residuals too): y, dx and dw.  |y| <= 9 K < 2**24 for every K of the nets
  (K <= 9216) by the triangle inequality -- where such an a-priori bound holds it stands for the `conv(|x|, |w|).max() < 2**24` it
  dominates, where it does not the absolute-operand convolution itself is evaluated.  Mean y**2 = 16 K, so K >= 512 gives |y| > 256
  somewhere (beyond the 8 significand bits of bf16: the store rounding is exercised -- asserted), and at least half of y is non-zero
  (asserted).  The weight gradient sums M products: dy is drawn from [-a, a] with a = min(3, (2**24 - 1) // (3 M)), a >= 1 required.
* the SUMS set (x, w uniform integers in [-1, 1], x thinned to density min(1, 2**23 / (M K 4/9))): the BatchNorm statistics, whose
  sum of squares over M pixels must stay below 2**24 per channel: mean y**2 = K * (2/3 dx) * (2/3) is held to 2**23 / M, a factor of two
  of room for the spread over channels; sum |y| <= sum y**2 for integers.  Both per-channel conditions are asserted on the reference.
"""
import torch
import torch.nn.functional as F

LIMIT = 1 << 24            # integers of magnitude <= 2**24 are exact in fp32; every bound below is strict
A_DENSE = 3
REF = torch.float64


def int_tensor(shape, lo, hi, density, seed, dtype=REF):
    """uniform integers in [lo, hi], each zeroed with probability 1 - density; seeded CPU generator"""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    t = torch.randint(int(lo), int(hi) + 1, tuple(shape), generator=g, dtype=torch.int8)
    if density < 1.0:
        t = t * (torch.rand(tuple(shape), generator=g) < density).to(torch.int8)
    return t.to(dtype)


def out_hw(h, w, k, s, p):
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def conv_ref(x, w, s, p):
    """x (N,H,W,Cin), w (Cout,KH,KW,Cin) -> y (N,OH,OW,Cout); fp64, torch's CPU convolution"""
    return F.conv2d(_nchw(x.to(REF)), _nchw(w.to(REF)), stride=s, padding=p).permute(0, 2, 3, 1).contiguous()


def _conv_backward(x_like, dy, w_like, s, p, mask):
    # the convolution-backward autograd itself calls, without running the forward first
    return torch.ops.aten.convolution_backward(_nchw(dy.to(REF)), _nchw(x_like), _nchw(w_like), None, (s, s), (p, p), (1, 1), False, (0, 0), 1, mask)


def dgrad_ref(dy, w, in_hw, s, p):
    """dx (N,IH,IW,Cin) of conv(x, w) for the upstream gradient dy (N,OH,OW,Cout)"""
    N, (IH, IW), Cin = dy.shape[0], in_hw, w.shape[3]
    x_like = torch.empty((N, IH, IW, Cin), dtype=REF)
    gi = _conv_backward(x_like, dy, w.to(REF), s, p, (True, False, False))[0]
    return gi.permute(0, 2, 3, 1).contiguous()


def wgrad_ref(x, dy, k, s, p):
    """dw (Cout,KH,KW,Cin)"""
    w_like = torch.empty((dy.shape[3], k, k, x.shape[3]), dtype=REF)
    gw = _conv_backward(x.to(REF), dy, w_like, s, p, (False, True, False))[1]
    return gw.permute(0, 2, 3, 1).contiguous()


def require_exact(bound, what, exact=None):
    """the exactness precondition `... < 2**24`: an a-priori bound (triangle inequality) where it already proves it, else the
    quantity itself (`exact()`: the operation on absolute operands)"""
    if bound < LIMIT:
        return
    assert exact is not None, f"{what}: a-priori bound {bound} >= 2**24"
    v = float(exact())
    assert v < LIMIT, f"{what}: {v} >= 2**24 -- not exact in fp32, pick other inputs"


def stored(ref, dtype):
    """what a kernel must store: the exact (integer or dyadic) fp64 value, exactly representable in fp32 (asserted), rounded to nearest
    even into `dtype`"""
    f = ref.to(torch.float32)
    assert torch.equal(f.to(REF), ref), "reference is not representable in fp32"
    if dtype == torch.float16:
        assert ref.abs().max().item() <= 65504, "reference leaves the fp16 range"
    return f.to(dtype)


def column_sums(y):
    """per-channel (sum y, sum y*y) as int64, with their exactness preconditions"""
    yi = y.reshape(-1, y.shape[-1]).to(torch.int64)
    assert torch.equal(yi.to(REF), y.reshape(-1, y.shape[-1])), "not integers"
    s1, s2, sa = yi.sum(0), (yi * yi).sum(0), yi.abs().sum(0)
    assert sa.max().item() < LIMIT, f"sum |y| = {sa.max().item()} >= 2**24"
    assert s2.max().item() < LIMIT, f"sum y*y = {s2.max().item()} >= 2**24"
    return s1, s2


class Problem:
    """one conv geometry (N, H, W, Cin, Cout, k, s, p) with its operand sets and references, built lazily and cached on the object"""

    def __init__(self, case, seed=0):
        self.case = tuple(case)
        N, H, W, Cin, Cout, k, s, p = self.case
        self.N, self.H, self.W, self.Cin, self.Cout, self.k, self.s, self.p = self.case
        self.OH, self.OW = out_hw(H, W, k, s, p)
        self.M = N * self.OH * self.OW
        self.K = k * k * Cin
        self.seed = 1000 * seed
        self._c = {}
        self.a_dy = min(A_DENSE, (LIMIT - 1) // (A_DENSE * self.M))

    def _get(self, name, fn):
        if name not in self._c:
            self._c[name] = fn()
        return self._c[name]

    # ---- dense set -------------------------------------------------------------------------------------------------
    @property
    def x(self):
        return self._get("x", lambda: int_tensor((self.N, self.H, self.W, self.Cin), -A_DENSE, A_DENSE, 1.0, self.seed + 1))

    @property
    def w(self):
        return self._get("w", lambda: int_tensor((self.Cout, self.k, self.k, self.Cin), -A_DENSE, A_DENSE, 1.0, self.seed + 2))

    @property
    def dy(self):
        assert self.a_dy >= 1, f"M = {self.M}: no integer dy keeps the weight gradient below 2**24"
        return self._get("dy", lambda: int_tensor((self.N, self.OH, self.OW, self.Cout), -self.a_dy, self.a_dy, 1.0, self.seed + 3))

    def res_out(self):
        return self._get("res_out", lambda: int_tensor((self.N, self.OH, self.OW, self.Cout), -A_DENSE, A_DENSE, 1.0, self.seed + 4))

    def res_in(self):
        return self._get("res_in", lambda: int_tensor((self.N, self.H, self.W, self.Cin), -A_DENSE, A_DENSE, 1.0, self.seed + 5))

    def y(self):
        """dense forward reference, with the forward precondition and the coverage conditions"""
        def make():
            require_exact(self.K * A_DENSE * A_DENSE, "conv(|x|, |w|).max()", lambda: conv_ref(self.x.abs(), self.w.abs(), self.s, self.p).max())
            y = conv_ref(self.x, self.w, self.s, self.p)
            assert torch.count_nonzero(y).item() * 2 >= y.numel(), "fewer than half of the outputs are non-zero"
            if self.K >= 512:
                assert y.abs().max().item() > 256, "K >= 512 but no |y| > 256: the 16-bit rounding is not exercised"
            return y
        return self._get("y", make)

    def dx(self):
        def make():
            require_exact(self.k * self.k * self.Cout * A_DENSE * self.a_dy, "dgrad(|dy|, |w|).max()",
                          lambda: dgrad_ref(self.dy.abs(), self.w.abs(), (self.H, self.W), self.s, self.p).max())
            return dgrad_ref(self.dy, self.w, (self.H, self.W), self.s, self.p)
        return self._get("dx", make)

    def dw(self):
        def make():
            require_exact(self.M * A_DENSE * self.a_dy, "wgrad(|x|, |dy|).max()",
                          lambda: wgrad_ref(self.x.abs(), self.dy.abs(), self.k, self.s, self.p).max())
            return wgrad_ref(self.x, self.dy, self.k, self.s, self.p)
        return self._get("dw", make)

    # ---- sums set ----------------------------------------------------------------------------------------------------
    @property
    def density_xs(self):
        return min(1.0, (LIMIT / 2) / (self.M * self.K * 4.0 / 9.0))

    @property
    def xs(self):
        return self._get("xs", lambda: int_tensor((self.N, self.H, self.W, self.Cin), -1, 1, self.density_xs, self.seed + 6))

    @property
    def ws(self):
        return self._get("ws", lambda: int_tensor((self.Cout, self.k, self.k, self.Cin), -1, 1, 1.0, self.seed + 7))

    def ys(self):
        def make():
            require_exact(self.K, "conv(|xs|, |ws|).max()")
            return conv_ref(self.xs, self.ws, self.s, self.p)
        return self._get("ys", make)

    def sums(self):
        """int64 (sum, sum of squares) per channel of ys, preconditions asserted"""
        return self._get("sums", lambda: column_sums(self.ys()))

    def drop(self, *names):
        for n in names:
            self._c.pop(n, None)


def first_difference(got, want, tile_hint=""):
    """message for a failed torch.equal of two NHWC (or 4-D weight) tensors: count of differing elements, the first differing index
    decoded to its four coordinates, both values there, and the caller's tile hint"""
    ne = (got != want) | (got.isnan() != want.isnan())
    cnt = int(ne.sum().item())
    if cnt == 0:
        return "equal"
    flat = int(torch.nonzero(ne.reshape(-1))[0].item())
    idx, r = [], flat
    for d in reversed(got.shape):
        idx.append(r % d)
        r //= d
    idx = tuple(reversed(idx))
    return (f"{cnt} of {got.numel()} elements differ; first at {idx} (flat {flat}): got {got[idx].item()} want {want[idx].item()}"
            + (f"; {tile_hint(idx) if callable(tile_hint) else tile_hint}" if tile_hint else ""))
