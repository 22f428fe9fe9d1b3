// The host layer of the convolution (layout and tile: the header of conv.hip): launch geometry, kernel selection, the plan tables, the C
// ABI entry points and the introspection behind the tests and bench.py.  No kernel lives here but zero_lattice_kernel: every
// other kernel and its launch is in conv.hip, conv_wgrad.hip or conv_stem.hip, reached through the launch functions of conv_host.h.  Compiles in seconds.
#include "conv_host.h"

// An NHWC operand of `ch` channels over pixel stride `ld` (nullptr: an optional operand that is absent).  Every kernel family reads and
// writes it in 16-byte vectors (u32x4 / float4 loads and stores, LDS-DMA, buffer descriptors) at base + pixel * ld + 8-channel
// group without looking at the address: the channels lie inside the pixel, the pixel stride is whole vectors (`vec` elements of
// 16 bytes) and the base is 16-byte aligned, or the entry point returns -2 before any launch.
static bool nhwc_ok(const void* p, int ld, int ch, int vec) {
    return !p || (ld >= ch && ld % vec == 0 && ((uintptr_t)p & 15) == 0);
}

static int fill_common(GatherGeom& g, int N, int IH, int IW, int Cin, int ldx, int QH, int QW, int OH, int OW,
                       int Cout, int ldy, int vec) {
    if (Cin % vec) return -2;
    g.N = N; g.IH = IH; g.IW = IW; g.Cin = Cin; g.ldx = ldx;
    g.QH = QH; g.QW = QW; g.M = N * QH * QW;
    g.OH = OH; g.OW = OW; g.Cout = Cout; g.ldy = ldy;
    g.CV = Cin / vec; g.KV = g.T * g.CV;
    g.dQW = make_fastdiv(QW); g.dQH = make_fastdiv(QH); g.dCV = make_fastdiv(g.CV); g.dW1 = make_fastdiv(QW + 1);
    // K-chunk order: channel chunk outer / tap inner; XCD-contiguous tile ranges (both were knobs in r01 / r02; two single-knob
    // sweeps of the step showed no other setting within noise of these: profiles/r02_step_knob_sweep*_same_box.log)
    const int tap_inner = 1, xcd_swz = 1;
    g.tap_inner = tap_inner; g.xcd_swz = xcd_swz;
    if ((long long)N * IH * IW * ldx >= (1ll << 31) || (long long)Cout * g.TT * Cin >= (1ll << 31)) return -2;
    return 0;
}

// ---- launch geometry of the two gather-GEMM uses (ONE copy: the launchers and et_conv2d_kernel_name both call these) -----------
static int fwd_geom(GatherGeom& g, int N, int IH, int IW, int Cin, int ldx, int Cout, int KH, int KW, int stride, int pad, int ldy,
                    int vec) {
    const int OH = (IH + 2 * pad - KH) / stride + 1, OW = (IW + 2 * pad - KW) / stride + 1;
    g.T = g.TT = KH * KW;
    for (int ky = 0; ky < KH; ++ky)
        for (int kx = 0; kx < KW; ++kx) {
            const int t = ky * KW + kx;
            g.dy[t] = (signed char)(ky - pad); g.dx[t] = (signed char)(kx - pad); g.wt[t] = (unsigned char)t;
        }
    for (int t = 0; t < g.T; ++t) g.tapinfo[t] = (g.dy[t] & 0xff) | ((g.dx[t] & 0xff) << 8) | ((int)g.wt[t] << 16);
    g.isy = g.isx = stride; g.osy = g.osx = 1; g.ooy = g.oox = 0;
    return fill_common(g, N, IH, IW, Cin, ldx, OH, OW, OH, OW, Cout, ldy, vec);
}

// dgrad of output-parity class (py, px): returns 1 when the class has no pixel, 0 on success (g.T may be 0: no tap reaches it)
static int dgrad_geom(GatherGeom& g, int py, int px, int N, int IH, int IW, int Cin, int ldx, int Cout, int KH, int KW, int stride,
                      int pad, int ldy, int vec) {
    const int OH = (IH + 2 * pad - KH) / stride + 1, OW = (IW + 2 * pad - KW) / stride + 1;
    g.TT = KH * KW;
    int t = 0;
    for (int ky = 0; ky < KH; ++ky) {
        if ((py + pad - ky) % stride) continue;
        for (int kx = 0; kx < KW; ++kx) {
            if ((px + pad - kx) % stride) continue;
            // floor division is exact here (remainder checked above, also for negatives)
            g.dy[t] = (signed char)((py + pad - ky) / stride);
            g.dx[t] = (signed char)((px + pad - kx) / stride);
            g.wt[t] = (unsigned char)(ky * KW + kx);
            ++t;
        }
    }
    g.T = t;
    for (int q = 0; q < t; ++q) g.tapinfo[q] = (g.dy[q] & 0xff) | ((g.dx[q] & 0xff) << 8) | ((int)g.wt[q] << 16);
    g.isy = g.isx = 1; g.osy = g.osx = stride; g.ooy = py; g.oox = px;
    const int QH = (IH - py + stride - 1) / stride, QW = (IW - px + stride - 1) / stride;
    if (QH <= 0 || QW <= 0) return 1;              // a 1-pixel-high / -wide input has no pixel in this parity class
    // the "gathered" tensor of dgrad is dy (OH x OW x Cout), the written one is dx (IH x IW x Cin)
    return fill_common(g, N, OH, OW, Cout, ldy, QH, QW, IH, IW, Cin, ldx, vec);
}

// ---- kernel selection ---------------------------------------------------------------------------------
// ONE place decides which instantiation runs; et_conv2d_kernel_name() reports the same decision to the tests and
// to bench.py's roofline tags (there is no second copy of this logic on the Python side).

// conv1x1_stream_kernel's contract: one tap at the pixel itself (1x1, stride 1, pad 0: forward and dgrad alike), whole 64-channel
// chunks with K = 64 | 128 | 256, all output channels in one tile (<= 256, whole 8-channel groups), identity pixel map
static bool s1_eligible(const GatherGeom& g) {
    if (g.T != 1 || g.TT != 1 || g.dy[0] || g.dx[0] || g.isy != 1 || g.isx != 1 || g.osy != 1 || g.osx != 1 || g.ooy || g.oox) return false;
    if (g.QH != g.IH || g.QW != g.IW || g.OH != g.QH || g.OW != g.QW) return false;
    if (g.Cin != 64 && g.Cin != 128 && g.Cin != 256) return false;
    if (g.Cout > 256 || g.Cout % 8 || g.ldx % 8 || g.ldy % 8) return false;
    if (g.Cin == 256 && g.Cout <= 64) return false;                       // no instantiation (no such layer)
    return true;
}

// conv_gemm_rs_kernel's contract: 3x3 taps in kernel-row order (three consecutive taps share dy, dx in [-1, 1]), stride 1,
// output lattice = the gathered tensor's own pixels, whole 64-channel chunks
static bool rs_eligible(const GatherGeom& g, int BM, int unit_rows) {
    if (g.T != 9 || g.isy != 1 || g.isx != 1 || g.osy != 1 || g.osx != 1 || g.ooy || g.oox) return false;
    if (g.QH != g.IH || g.QW != g.IW || g.OH != g.QH || g.OW != g.QW || g.CV % 8 || g.QW < 2) return false;
    if (BM + 2 + (BM + 2 + g.QW - 1) / g.QW + 1 > unit_rows) return false;             // the pad slots of a BM-pixel tile fit the unit
    if ((long long)(g.N * g.QH + 1) * (g.QW + 1) >= (1ll << 31)) return false;
    const int sgn = g.dy[0] < 0 ? 1 : -1;
    for (int t = 0; t < 9; ++t)
        if (g.dy[t] != sgn * (t / 3 - 1) || g.dx[t] != sgn * (t % 3 - 1) || g.wt[t] != t) return false;
    return true;
}

// ---- the plan tables: the row lists of conv_host.h as GemmPlan rows, ONE object per family (a plan is a pointer into them) -------------
#define ET_S1(KC_, WN_, TN_, WM_, TMW_, NS_, WGS_, FULL_) {GEMM_S1, 32 * TMW_ * WM_, 32 * TN_ * WN_, WM_, WN_, 8, NS_, true, WGS_, KC_, TN_, FULL_},
#define ET_GLDS(BM_, BN_, WM_, WN_, BKV_, NS_, UT_) {GEMM_GLDS, BM_, BN_, WM_, WN_, BKV_, NS_, UT_, 0, 0, 0, 0},
#define ET_REG(BM_, BN_, WM_, WN_, BKV_, UT_) {GEMM_REG, BM_, BN_, WM_, WN_, BKV_, 2, UT_, 0, 0, 0, 0},
#define ET_RS(BM_, BN_, WM_, WN_) {GEMM_RS, BM_, BN_, WM_, WN_, 8, 2, true, 0, 0, 0, 0},
const GemmPlan s1_rows[] = {ET_S1_ROWS};
const GemmPlan glds_rows[] = {ET_GLDS_ROWS};
const GemmPlan reg_rows[] = {ET_REG_ROWS};
const GemmPlan rs_rows[] = {ET_RS_ROWS};
#undef ET_S1
#undef ET_GLDS
#undef ET_REG
#undef ET_RS
static const GemmPlan pp_row{GEMM_PP, 256, 256, 2, 4, 8, 2, true, 0, 0, 0, 0};       // conv_gemm_pp_kernel<T>, conv_gemm_pprs_kernel<T>:
static const GemmPlan pprs_row{GEMM_PPRS, 256, 256, 2, 4, 8, 2, true, 0, 0, 0, 0};   // one instantiation per type

// the row of a family's table that pred accepts; null = no such instantiation (the launch then fails with -2)
template <typename Row, size_t N, typename Pred> static const Row* find_row(const Row (&rows)[N], Pred pred) {
    for (const Row& r : rows)
        if (pred(r)) return &r;
    return nullptr;
}

// conv1x1_stream_kernel: the row by K, column tile and epilogue.  full = the launch needs residual / accumulate / BN-backward sums
// in the epilogue.
static const GemmPlan* plan_s1(const GatherGeom& g, bool full) {
    const int BN = g.Cout > 128 ? 256 : (g.Cout > 64 ? 128 : 64);
    const int kc = g.Cin / 64;
    return find_row(s1_rows, [&](const GemmPlan& r) { return r.kc == kc && r.BN == BN && (r.full != 0) == full; });
}

static const GemmPlan* plan_gemm(const GatherGeom& g, int elem_bytes, bool have_zero_page, bool full_epilogue = false) {
    // Build-time constants that were tuning knobs in r01 / r02 (swept on the step, profiles/r02_step_knob_sweep*_same_box.log, and
    // per layer, profiles/r02_microbench_narrow_k.log): GEMMs with K <= 128 elements use the 128x64 tile (3 workgroups per CU for
    // the HBM-bound short-K 1x1 layers; at K = 256 the 128-wide tile re-reads the activations half as often: 150 -> 124 us on
    // 256->256 @80x80, B=64); the LDS ring shape follows K (below).  The whole-code-path switches of r02-r04 (ET_CONV_GLDS / _BIG /
    // _PP / _BIG_MINFILL / _S1 / _RS / _PPRS / _STEM) are gone with their losing arms: each has a same-box A/B file under profiles/
    // (NOTEBOOK.md rounds 2-4); the register-staged kernel remains for fp32 parity mode and for callers without a zero page.
    constexpr int narrow_k = 128;
    const bool bf16 = elem_bytes == 2;
    const bool wide = g.Cout > 64 && !(narrow_k > 0 && g.T * g.Cin <= narrow_k);
    const bool glds = have_zero_page;
    const int BN = wide ? 128 : 64, BKV = g.CV % 8 == 0 ? 8 : 4;
    const bool utap = g.CV % 4 == 0;
    // the 128-row tile of either staging form: NS-deep ring of BKV-vector chunks (the register-staged kernel has no ring: NS = 2)
    const auto tiled = [&](int bkv, int ns) {
        const auto want = [&](const GemmPlan& r) { return r.BM == 128 && r.BN == BN && r.BKV == bkv && r.NS == ns && r.utap == utap; };
        return glds ? find_row(glds_rows, want) : find_row(reg_rows, want);
    };
    if (!(bf16 && glds && g.CV % 8 == 0)) return tiled(BKV, 2);
    // 1x1 layers with K <= 256 and <= 256 output channels: the persistent streaming kernel, also for the dgrads with a residual /
    // accumulate / BN-backward sums in the epilogue.  Measured (profiles/r04_mb_1x1_stream_kernel_ab.txt, r04_stream_full_and_fuse_ab_current_build.txt): plain layers
    // 4.4-5.3 TB/s against 3.7-5.1 of the tiled kernels (128->128 @80x80: 54 -> 46 us, 256->256 @80x80: 111 -> 86-97 us); step, same
    // box, alternating, tiled kernels / stream kernel for the plain layers only / for all = 53.18 / 52.27-52.46 / 52.10-52.13 ms.  The FULL epilogue only pays since its reads are issued a
    // slab round at a time (conv_epilogue_act, EPF): with one load + wait per store iteration it LOST to the tiled kernels
    // (128->128 @80x80 with residual + sums: 105 -> 111 us) -- those loads return in order BEHIND every LDS-DMA piece the ring has in
    // flight, and the tiled kernels hide that latency across four short-lived workgroups per CU.
    if (s1_eligible(g)) return plan_s1(g, full_epilogue);
    // short-K GEMMs (K <= 256, i.e. <= 4 chunks of 64) run 32-wide chunks in a 3-deep ring -- 48 KB of LDS, three
    // workgroups per CU, two chunks in flight each (measured 3-10 % on the 1x1 layers); everything else the 64-wide
    // double buffer (deeper rings or taller 4-wave tiles cost occupancy and lose: profiles/)
    enum { RING_SHORT_K, RING_128, RING_256 };
    int ring = g.T * g.Cin <= 256 ? RING_SHORT_K : RING_128;
    // 8-wave 256x256 tile (one workgroup per CU, half the L2->LDS bytes per flop): 3x3 layers with >= 256 output
    // channels, and deep 1x1 layers when the grid fills whole residency rounds reasonably
    if (g.Cout >= 256) {
        const int n_cu = device_cus();
        const long long blocks = (long long)((g.M + 255) / 256) * ((g.Cout + 255) / 256);
        const double rounds = (double)blocks / n_cu;
        const bool fills = (double)((blocks + n_cu - 1) / n_cu) / rounds <= 1.35;
        // (a grid that leaves most CUs without a 256x256 tile -- the teacher's 32-image 20x20 layers: 100 tiles -- still runs it: 128x128
        // tiles for such grids won isolated and lost on the step three times, profiles/r02_microbench_big_tile_minfill.log,
        // r03_big_tile_minfill_ab.txt, NOTEBOOK.md round 4: the 256x256 tile costs less CU-time and the other stream fills the rest)
        if (g.TT > 1 || (g.T * g.Cin >= 512 && fills)) ring = RING_256;
    }
    // 3x3 stride-1 layers on the 128-row tiles: activation rows shared by the three taps of a kernel row
    if (ring == RING_128 && rs_eligible(g, 128, RS_A_ROWS(128))) return find_row(rs_rows, [&](const GemmPlan& r) { return r.BM == 128 && r.BN == BN; });
    if (ring == RING_256) return rs_eligible(g, 256, PPRS_ROWS) ? &pprs_row : &pp_row;
    return ring == RING_SHORT_K ? tiled(4, 3) : tiled(BKV, 2);
}

// the name rocprofv3 prints for the plan's kernel (template arguments spelled as the demangler does)
static const char* dtype_tname(int dtype) { return dtype == ET_F32 ? "float" : (dtype == ET_F16 ? "et_f16" : "unsigned short"); }
static void plan_name(const GemmPlan& p, int dtype, char* buf, int n) {
    const char* t = dtype_tname(dtype);
    if (p.kind == GEMM_S1) snprintf(buf, n, "conv1x1_stream_kernel<%s, %d, %d, %d, %d, %d, %d, %d, %s>", t, p.kc, p.WN, p.tn, p.WM, p.BM / (32 * p.WM), p.NS, p.wgs, p.full ? "true" : "false");
    else if (p.kind == GEMM_PP) snprintf(buf, n, "conv_gemm_pp_kernel<%s>", t);
    else if (p.kind == GEMM_PPRS) snprintf(buf, n, "conv_gemm_pprs_kernel<%s>", t);
    else if (p.kind == GEMM_RS) snprintf(buf, n, "conv_gemm_rs_kernel<%s, %d, %d, %d, %d>", t, p.BM, p.BN, p.WM, p.WN);
    else if (p.kind == GEMM_GLDS) snprintf(buf, n, "conv_gemm_glds_kernel<%s, %d, %d, %d, %d, %d, %d, %s>", t, p.BM, p.BN, p.WM, p.WN, p.BKV, p.NS, p.utap ? "true" : "false");
    else snprintf(buf, n, "conv_gemm_kernel<%s, %d, %d, %d, %d, %d, %s>", t, p.BM, p.BN, p.WM, p.WN, p.BKV, p.utap ? "true" : "false");
}

// conv1x1_stream_kernel is persistent: as many workgroups as the chip holds at the plan's residency, never more than row tiles
// (ET_CONV_S1_WGS: tests shrink the grid to exercise the tile loop; read per call).  ONE copy: the launcher and
// et_conv2d_stats_rows_for both call this.
int s1_grid(int ntm, const GemmPlan& p) {
    int n = env_int("ET_CONV_S1_WGS", p.wgs * device_cus());
    if (n < 1) n = 1;
    return n < ntm ? n : ntm;
}

// Plan, tile grid, and on to conv.hip's launch function
static int launch_gemm(int dtype, const void* X, const void* W, void* Y, const void* zero16, GatherGeom g, const Epilogue& ep,
                       hipStream_t s) {
    if (dtype != ET_F32 && dtype != ET_BF16 && dtype != ET_F16) return -2;
    if (g.M <= 0) return 0;
    g.nfast = 1;
    const GemmPlan* const pp = plan_gemm(g, dtype == ET_F32 ? 4 : 2, zero16 != nullptr, ep.res != nullptr || ep.accumulate || ep.bn_y != nullptr);
    if (!pp) return -2;
    const GemmPlan& p = *pp;
    g.ntm = (g.M + p.BM - 1) / p.BM;
    g.ntn = (g.Cout + p.BN - 1) / p.BN;
    return launch_gemm_row(pp, dtype, X, W, Y, zero16, g, ep, s);
}

extern "C" int et_conv2d_stats_rows(int N, int OH, int OW) { return (N * OH * OW + 63) / 64; }

// ---- the stem: shape gate, persistent grid, tile fields -----------------------------------------------------------------------
static bool stem_eligible(int dtype, int Cin, int Cout, int KH, int KW, int stride, int pad, bool has_residual, bool has_zero_page) {
    return (dtype == ET_BF16 || dtype == ET_F16) && KH == 6 && KW == 6 && stride == 2 && pad == 2 && Cin == 8 && Cout <= 64 && Cout % 8 == 0 &&
           !has_residual && has_zero_page;
}
// the stem kernels are persistent (ET_CONV_STEM_WGS: tests shrink the grid to exercise the tile loop; read per launch)
int stem_grid(int ntiles) {
    int grid = env_int("ET_CONV_STEM_WGS", 2 * device_cus());
    if (grid < 1) grid = 1;
    return grid < ntiles ? grid : ntiles;
}
// image and tile fields of StemArgs / StemWgradArgs (6x6, stride 2, pad 2)
template <typename A>
static void stem_tiles(A& a, int N, int IH, int IW) {
    a.N = N; a.IH = IH; a.IW = IW;
    a.OH = (IH + 4 - 6) / 2 + 1; a.OW = (IW + 4 - 6) / 2 + 1;
    a.trn = (a.OH + STEM_TR - 1) / STEM_TR; a.tcn = (a.OW + STEM_TC - 1) / STEM_TC;
    a.ntiles = N * a.trn * a.tcn;
}

extern "C" int et_conv2d_fwd(const void* x, const void* w, void* y, int dtype, int N, int IH, int IW, int Cin,
                             int ldx, int Cout, int KH, int KW, int stride, int pad, int ldy, const float* scale,
                             const float* bias, int act, const void* residual, int ldr, float* stats_partial,
                             int stats_ld, const void* zero16, et_stream_t stream) {
    if (!x || !w || !y) return -1;
    if (KH * KW > CONV_MAX_TAPS || stride < 1 || N <= 0 || Cout <= 0 || stats_ld < 0 || (stats_ld && stats_ld < Cout)) return -2;
    const int vec = dtype == ET_F32 ? 4 : 8;
    if (!nhwc_ok(x, ldx, Cin, vec) || !nhwc_ok(y, ldy, Cout, vec) || !nhwc_ok(residual, ldr, Cout, vec) || ((uintptr_t)w & 15)) return -2;
    if (stem_eligible(dtype, Cin, Cout, KH, KW, stride, pad, residual != nullptr, zero16 != nullptr)) {
        StemArgs a;
        a.x = (const uint16_t*)x; a.w = (const uint16_t*)w; a.y = (uint16_t*)y; a.zero = (const uint16_t*)zero16;
        a.ldx = ldx; a.Cout = Cout; a.ldy = ldy;
        stem_tiles(a, N, IH, IW);
        launch_stem(false, a, dtype, scale, bias, act, stats_partial, stats_ld, (hipStream_t)stream);
        ET_CHECK_LAUNCH();
        return 0;
    }
    GatherGeom g;
    int rc = fwd_geom(g, N, IH, IW, Cin, ldx, Cout, KH, KW, stride, pad, ldy, vec);
    if (rc) return rc;
    if (residual && !(residual == (const void*)y && ldr == ldy)) {
        // the residual may BE the output (the in-place shortcut of the eval-mode C3 stem: a lane loads the element it is about to store);
        // any other overlap of the two ranges would let one lane's store race another lane's load
        const size_t eb = dtype == ET_F32 ? 4 : 2, npix = (size_t)g.N * g.OH * g.OW;
        const uintptr_t r0 = (uintptr_t)residual, r1 = r0 + ((npix - 1) * (size_t)ldr + (size_t)Cout) * eb;
        const uintptr_t y0 = (uintptr_t)y, y1 = y0 + ((npix - 1) * (size_t)ldy + (size_t)Cout) * eb;
        if (npix > 0 && r0 < y1 && y0 < r1) {
            // channel slices of ONE wider buffer interleave without touching: same pixel stride, disjoint channel windows
            const bool same_rows = ldr == ldy && ((r0 > y0 ? r0 - y0 : y0 - r0) % ((size_t)ldy * eb)) >= (size_t)Cout * eb &&
                                   ((r0 > y0 ? r0 - y0 : y0 - r0) % ((size_t)ldy * eb)) + (size_t)Cout * eb <= (size_t)ldy * eb;
            if (!same_rows) return -2;
        }
    }
    Epilogue ep{scale, bias, act, residual, ldr, stats_partial, 0};
    ep.stats_ld = stats_partial ? stats_ld : 0;
    rc = launch_gemm(dtype, x, w, y, zero16, g, ep, (hipStream_t)stream);
    if (rc) return rc;
    ET_CHECK_LAUNCH();
    return 0;
}

// dx pixels of an output-parity class that no tap reaches (1x1 stride-2: three of the four classes): their gradient is zero
template <typename T>
__global__ __launch_bounds__(256) void zero_lattice_kernel(T* __restrict__ dx, int N, int IH, int IW, int ldx, int Cin, int QH, int QW,
                                                           int stride, int py, int px) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)N * QH * QW * Cin;
    if (i >= total) return;
    const int c = (int)(i % Cin);
    long long q = i / Cin;
    const int qx = (int)(q % QW); q /= QW;
    const int qy = (int)(q % QH);
    const int n = (int)(q / QH);
    dx[(((long long)n * IH + qy * stride + py) * IW + qx * stride + px) * ldx + c] = T(0);
}

static int conv2d_dgrad_impl(const void* dy, const void* wT, void* dx, int dtype, int N, int IH, int IW, int Cin,
                             int ldx, int Cout, int KH, int KW, int stride, int pad, int ldy, int accumulate,
                             const void* residual, int ldr, const void* bn_y, int ld_bn, const float* bn_scale,
                             const float* bn_shift, int bn_act, float* bn_stats, int bn_stats_ld, const void* zero16, et_stream_t stream) {
    // dx[n,iy,ix,ci] = sum_{ky,kx,co} dy[n,(iy+pad-ky)/s,(ix+pad-kx)/s,co] * wT[ci,ky,kx,co]
    if (!dy || !wT || !dx) return -1;
    if (KH * KW > CONV_MAX_TAPS || stride < 1 || stride > 2 || N <= 0) return -2;
    if (residual && stride != 1) return -2;        // the fused shortcut-gradient add is a stride-1 (Bottleneck) feature
    if (bn_y && (stride != 1 || !bn_scale || !bn_shift || !bn_stats || Cin % 8 || bn_stats_ld < 0 || (bn_stats_ld && bn_stats_ld < Cin))) return -2;   // one launch, whole channel groups
    const int vec = dtype == ET_F32 ? 4 : 8;
    if (!nhwc_ok(dy, ldy, Cout, vec) || !nhwc_ok(dx, ldx, Cin, vec) || !nhwc_ok(residual, ldr, Cin, vec) || !nhwc_ok(bn_y, ld_bn, Cin, vec) ||
        ((uintptr_t)wT & 15)) return -2;
    for (int py = 0; py < stride; ++py)
        for (int px = 0; px < stride; ++px) {
            GatherGeom g;
            int rc = dgrad_geom(g, py, px, N, IH, IW, Cin, ldx, Cout, KH, KW, stride, pad, ldy, vec);
            if (rc == 1) continue;
            if (rc) return rc;
            const int t = g.T, QH = g.QH, QW = g.QW;
            Epilogue ep{nullptr, nullptr, ACT_NONE, residual, ldr, bn_y ? bn_stats : nullptr, accumulate,
                        bn_y, ld_bn, bn_scale, bn_shift, bn_act, bn_y ? bn_stats_ld : 0};   // dx = dgrad (+ residual) (+ BN-backward sums)
            if (t == 0) {            // no tap reaches this class (k < stride): zero gradient unless the caller accumulates
                const long long total = (long long)N * QH * QW * Cin;
                if (!accumulate && total > 0) {
                    if (dtype == ET_F32) hipLaunchKernelGGL((zero_lattice_kernel<float>), dim3(et_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (float*)dx, N, IH, IW, ldx, Cin, QH, QW, stride, py, px);
                    else hipLaunchKernelGGL((zero_lattice_kernel<uint16_t>), dim3(et_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (uint16_t*)dx, N, IH, IW, ldx, Cin, QH, QW, stride, py, px);
                }
                continue;
            }
            rc = launch_gemm(dtype, dy, wT, dx, zero16, g, ep, (hipStream_t)stream);
            if (rc) return rc;
        }
    ET_CHECK_LAUNCH();
    return 0;
}

extern "C" int et_conv2d_dgrad(const void* dy, const void* wT, void* dx, int dtype, int N, int IH, int IW, int Cin,
                               int ldx, int Cout, int KH, int KW, int stride, int pad, int ldy, int accumulate,
                               const void* residual, int ldr,
                               const void* zero16, et_stream_t stream) {
    return conv2d_dgrad_impl(dy, wT, dx, dtype, N, IH, IW, Cin, ldx, Cout, KH, KW, stride, pad, ldy, accumulate, residual, ldr,
                             nullptr, 0, nullptr, nullptr, 0, nullptr, 0, zero16, stream);
}

extern "C" int et_conv2d_dgrad_bn(const void* dy, const void* wT, void* dx, int dtype, int N, int IH, int IW, int Cin,
                                  int ldx, int Cout, int KH, int KW, int pad, int ldy, const void* residual, int ldr,
                                  const void* bn_y, int ld_bn, const float* bn_scale, const float* bn_shift, int bn_act,
                                  float* bn_stats_partial, int bn_stats_ld, const void* zero16, et_stream_t stream) {
    if (!bn_y) return -1;
    return conv2d_dgrad_impl(dy, wT, dx, dtype, N, IH, IW, Cin, ldx, Cout, KH, KW, 1, pad, ldy, 0, residual, ldr, bn_y, ld_bn,
                             bn_scale, bn_shift, bn_act, bn_stats_partial, bn_stats_ld, zero16, stream);
}

// launch geometry of the weight gradient (ONE copy: the launcher and et_conv2d_kernel_name both call this)
static void wgrad_geom(WgradGeom& g, int N, int IH, int IW, int Cin, int ldx, int Cout, int KH, int KW, int stride, int pad, int ldy) {
    const int OH = (IH + 2 * pad - KH) / stride + 1, OW = (IW + 2 * pad - KW) / stride + 1;
    g.N = N; g.IH = IH; g.IW = IW; g.Cin = Cin; g.ldx = ldx;
    g.QH = OH; g.QW = OW; g.P = N * OH * OW; g.Cout = Cout; g.ldy = ldy;
    g.isy = g.isx = stride; g.T = KH * KW; g.NC = g.T * Cin;
    g.dQW = make_fastdiv(OW); g.dQH = make_fastdiv(OH); g.dCin = make_fastdiv(Cin); g.dW1 = make_fastdiv(OW + 1);
    g.PP = N * OH * (OW + 1);
    g.ident = (KH == 1 && KW == 1 && stride == 1 && pad == 0 && OH == IH && OW == IW) ? 1 : 0;
    g.buf = 0;                   // set per launch (launch_wgrad): needs the group's pixel strides
    for (int ky = 0; ky < KH; ++ky)
        for (int kx = 0; kx < KW; ++kx) {
            g.dy[ky * KW + kx] = (signed char)(ky - pad);
            g.dx[ky * KW + kx] = (signed char)(kx - pad);
        }
}

// the weight-gradient tables: the row lists of conv_host.h as WgradRow rows
#define ET_WG(BM_, BN_, WM_, WN_) {WGRAD_TR, BM_, BN_, WM_, WN_, 0},
#define ET_WGRS(BM_, BN_, WM_, WN_, ST_) {WGRAD_RS, BM_, BN_, WM_, WN_, ST_},
#define ET_WGREG(BM_, BN_) {WGRAD_REG, BM_, BN_, 2, 2, 0},
const WgradRow wg_rows[] = {ET_WG_ROWS};
const WgradRow wgrs_rows[] = {ET_WGRS_ROWS};
const WgradRow wgreg_rows[] = {ET_WGREG_ROWS};
#undef ET_WG
#undef ET_WGRS
#undef ET_WGREG

static const WgradRow* plan_wgrad(const WgradGeom& g, int elem_bytes, bool have_zero_page) {
    const bool wideN = g.NC > 64;
    const bool tallM = g.Cout > 64;            // Cout <= 64 layers: a 64-row tile wastes no MFMA rows
    struct { bool tr; int bm, bn; bool rs; int rs_stride; } p{false, tallM ? 128 : 64, wideN ? 128 : 64, false, 1};
    // bf16 + zero page: LDS-DMA staging with transposing LDS reads
    p.tr = elem_bytes == 2 && have_zero_page;
    // 256-wide tiles (8 waves, one workgroup per CU): half the L2->LDS bytes per flop of the 128^2 tile
    if (p.tr) {
        // measured (B=64 YOLOv5l shapes): the 256^2 tile wins on the 3x3 layers with >= 256 output channels
        // (691-765 TFLOP/s vs ~600), 128x256 on the 128-channel stride-1 3x3 layers; 1x1 layers keep 128^2
        if (g.T > 1 && g.Cout >= 256 && g.NC >= 256) { p.bm = 256; p.bn = 256; }
        else if (g.T > 1 && g.isy == 1 && g.NC >= 256 && g.Cout == 128) p.bn = 256;
        // 1x1 layers with >= 512 channels on both sides (MFMA-bound: 256 flop per byte) take the 256^2 tile as well; below that the
        // layers are HBM-bound and 128^2 (two workgroups per CU) wins.  Same-box A/B on the step (profiles/r06_wgrad_1x1_tile_ab.txt):
        // wgrad family 9.74 / 9.79 -> 9.67 / 9.67 ms; 256^2 from 256 channels 9.82 / 9.78, 128 x 256 9.95, 256 x 128 9.98
        else if (g.T == 1 && g.Cout >= 512 && g.NC >= 512) { p.bm = 256; p.bn = 256; }
    }
    // 3x3 stride-1 pad-1 layers: the three taps of a kernel row share both staged operands (conv_wgrad_rs_kernel)
    if (p.tr && g.T == 9 && g.isy == 1 && g.isx == 1 && g.dy[0] == -1 && g.dx[0] == -1 && g.dy[8] == 1 && g.dx[8] == 1 &&
        g.QH == g.IH && g.QW == g.IW && g.QW >= 2 && 64 / (g.QW + 1) + 2 <= g.QH &&
        (long long)g.N * g.IH * g.IW * (g.ldx > g.ldy ? g.ldx : g.ldy) < (1ll << 31)) {          // 32-bit element offsets in the kernel
        if (g.Cout >= 128 && g.Cin >= 128) { p.rs = true; p.bm = 128; p.bn = 128; }
        else if (g.Cout <= 64 && g.Cin <= 64) { p.rs = true; p.bm = 64; p.bn = 64; }
    }
    // 3x3 stride-2 pad-1 layers with an even input size (the down-sampling convs of the backbone / neck): the stride-2 form of the same
    // kernel (two X rows per K-slot).  Isolated, B = 64 (profiles/r04_mb_3x3_wgrad_stride2_ab.txt): 64->128 @320: 504 -> 396 us (the
    // 128x64 tile, two workgroups per CU); with >= 128 input channels the 128x128 tile needs 102 KB of LDS = ONE workgroup per CU and
    // loses to the 256x256 per-tap tile (512->1024 @40: 307 -> 365 us): only the 64-input-channel layers take this form.
    if (p.tr && g.T == 9 && g.isy == 2 && g.isx == 2 && g.dy[0] == -1 && g.dx[0] == -1 && g.dy[8] == 1 && g.dx[8] == 1 &&
        g.IH == 2 * g.QH && g.IW == 2 * g.QW && g.QW >= 2 && 64 / (g.QW + 1) + 2 <= g.QH && g.Cout >= 128 && g.Cin >= 64 && g.Cin < 128 &&
        (long long)g.N * g.IH * g.IW * (g.ldx > g.ldy ? g.ldx : g.ldy) < (1ll << 31)) {
        p.rs = true; p.rs_stride = 2; p.bm = 128; p.bn = 64;
    }
    if (p.rs) return find_row(wgrs_rows, [&](const WgradRow& r) { return r.bm == p.bm && r.bn == p.bn && r.stride == p.rs_stride; });
    const auto tile = [&](const WgradRow& r) { return r.bm == p.bm && r.bn == p.bn; };
    return p.tr ? find_row(wg_rows, tile) : find_row(wgreg_rows, tile);
}
static void wgrad_plan_name(const WgradRow& p, int dtype, char* buf, int n) {
    const char* t = dtype_tname(dtype);
    if (p.kind == WGRAD_RS && p.stride == 2) snprintf(buf, n, "conv_wgrad_rs_kernel<%s, %d, %d, %d, %d, 2>", t, p.bm, p.bn, p.wm, p.wn);   // a default argument is not printed
    else if (p.kind == WGRAD_RS) snprintf(buf, n, "conv_wgrad_rs_kernel<%s, %d, %d, %d, %d>", t, p.bm, p.bn, p.wm, p.wn);
    else if (p.kind == WGRAD_TR) snprintf(buf, n, "conv_wgrad_tr_kernel<%s, %d, %d, %d, %d>", t, p.bm, p.bn, p.wm, p.wn);
    else snprintf(buf, n, "conv_wgrad_kernel<%s, %d, %d>", t, p.bm, p.bn);
}

// Split K so that the grid is a whole number of residency rounds: up to cap (= workgroups per CU x CUs) workgroups run at once,
// and a grid a little OVER a multiple of that costs a whole extra round (e.g. 36 tiles x 29 splits = 1044 workgroups on 1024
// slots).  Fewer splits also mean fewer fp32 atomics on dW.  Measured: ONE full round of co-resident workgroups with >= ~25 chunks
// (1600 pixels) each beats two shorter rounds (prologue, first-chunk latency and the atomic epilogue are per workgroup).
// len = the reduction length (pixels / padded slots), chunk = the kernel's K-chunk; per = slice length, a multiple of chunk.
struct SplitK { int per, nsk; };
static SplitK wgrad_split_k(int len, int chunk, int tiles, int cap) {
    const int max_sk = max(1, len / (chunk * 25));
    auto eff = [&](int k) { const int b = tiles * k; return (double)b / ((double)((b + cap - 1) / cap) * cap); };
    int sk = max(1, min(cap / tiles, max_sk));
    // grids that cannot fill one round evenly: take the split (a few rounds at most) that wastes least
    if (eff(sk) < 0.8)
        for (int k = sk + 1; k <= min(max_sk, max(4, 2 * cap / tiles)); ++k)
            if (eff(k) > eff(sk) + 0.1) sk = k;
    sk = max(1, min(sk, max_sk));
    int per = (len + sk - 1) / sk;
    per = ((per + chunk - 1) / chunk) * chunk;
    return SplitK{per, (len + per - 1) / per};
}

// Plan, tile grid and K-split, and on to conv_wgrad.hip's launch function
static int launch_wgrad(int dtype, const WgradGroup& grp, const void* zero16, WgradGeom& g, hipStream_t s) {
    if (dtype != ET_F32 && dtype != ET_BF16 && dtype != ET_F16) return -2;
    const int eb = dtype == ET_F32 ? 4 : 2, BKP = 8 * (16 / eb);   // BKP: K-chunk of the per-tap kernels, 8 vectors of pixels
    const WgradRow* const wp = plan_wgrad(g, eb, zero16 != nullptr);
    if (!wp) return -2;
    const bool tr = wp->kind == WGRAD_TR;
    const int bm = wp->bm, bn = wp->bn, n_cu = device_cus();
    g.xcd = 1;                                     // the K-splits of one dW tile share an XCD (a knob until r02: always on)
    g.ntm = (g.Cout + bm - 1) / bm;
    if (wp->kind == WGRAD_RS) {
        // the split policy over the padded raster, in 64-slot chunks
        g.ntn = 3 * ((g.Cin + bn - 1) / bn);
        // stride 1: 68 KB / 34 KB of LDS, 8 / 4 waves, <= 128 VGPRs; stride 2: 67 KB (4 waves)
        const int slots = wp->stride == 2 ? 2 : (bm == 128 ? 2 : 4);
        const SplitK sk = wgrad_split_k(g.PP, 64, grp.n * g.ntn * g.ntm, slots * n_cu);
        g.Pper = sk.per; g.nsk = sk.nsk;
        return launch_wgrad_row(wp, dtype, grp, zero16, g, s);
    }
    g.ntn = (g.NC + bn - 1) / bn;
    // `slots` workgroups of this tile fit on a CU (LDS- or register-limited); the whole group shares the split
    const int lds_kb = tr ? (bm + bn) / 4 : 64;                // 2 stages x 64 pixels x (bm+bn) channels x 2 B
    const int slots = tr ? max(1, min(160 / lds_kb, bm * bn <= 64 * 64 ? 5 : (bm * bn <= 128 * 64 ? 3 : 2))) : 2;
    const SplitK sk = wgrad_split_k(g.P, BKP, grp.n * g.ntn * g.ntm, slots * n_cu);
    g.Pper = sk.per; g.nsk = sk.nsk;
    if (tr) {
        // 1x1 stride-1 layers: buffer-descriptor pieces when every tensor of the group spans < 2^31 bytes (conv_wgrad_tr_kernel, g.buf)
        g.buf = g.ident && env_int("ET_CONV_BUF_DMA", 1);
        for (int k = 0; k < grp.n && g.buf; ++k)
            if ((size_t)g.P * grp.it[k].ldx * 2 >= (1ull << 31) || (size_t)g.P * grp.it[k].ldy * 2 >= (1ull << 31)) g.buf = 0;
    }
    return launch_wgrad_row(wp, dtype, grp, zero16, g, s);
}

extern "C" int et_conv2d_wgrad_grouped(const et_wgrad_item* items, int n_items, int dtype, int N, int IH, int IW, int Cin,
                                       int Cout, int KH, int KW, int stride, int pad, const void* zero16,
                                       et_stream_t stream) {
    // for every item: dw[co,ky,kx,ci] += sum_{n,oy,ox} dy[n,oy,ox,co] * x[n,oy*s+ky-pad,ox*s+kx-pad,ci]   (fp32, atomic)
    if (!items || n_items <= 0 || n_items > WGRAD_MAX_GROUP) return -1;
    if (KH * KW > CONV_MAX_TAPS || stride < 1 || N <= 0) return -2;
    const int vec = dtype == ET_F32 ? 4 : 8;
    if (Cin % vec || Cout % vec) return -2;
    WgradGroup grp;
    grp.n = n_items;
    for (int i = 0; i < n_items; ++i) {
        if (!items[i].x || !items[i].dy || !items[i].dw) return -1;
        if (!nhwc_ok(items[i].x, items[i].ldx, Cin, vec) || !nhwc_ok(items[i].dy, items[i].ldy, Cout, vec) || ((uintptr_t)items[i].dw & 15)) return -2;
        grp.it[i].x = (const uint16_t*)items[i].x; grp.it[i].dy = (const uint16_t*)items[i].dy; grp.it[i].dw = items[i].dw;
        grp.it[i].ldx = items[i].ldx; grp.it[i].ldy = items[i].ldy;
    }
    for (int i = n_items; i < WGRAD_MAX_GROUP; ++i) grp.it[i] = grp.it[0];
    WgradGeom g;
    wgrad_geom(g, N, IH, IW, Cin, items[0].ldx, Cout, KH, KW, stride, pad, items[0].ldy);
    if (g.P <= 0) return 0;
    const int rc = launch_wgrad(dtype, grp, zero16, g, (hipStream_t)stream);
    if (rc) return rc;
    ET_CHECK_LAUNCH();
    return 0;
}

extern "C" int et_conv2d_wgrad(const void* x, const void* dy, float* dw, int dtype, int N, int IH, int IW, int Cin,
                               int ldx, int Cout, int KH, int KW, int stride, int pad, int ldy, const void* zero16,
                               et_stream_t stream) {
    const et_wgrad_item one{x, dy, dw, ldx, ldy};
    return et_conv2d_wgrad_grouped(&one, 1, dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad, zero16, stream);
}

// ---- the stem on the loaders' uint8 images (no packed tensor) ------------------------------------------------------------------
// ET_STEM_U8 (read per call; for the A/B): bit 1 = forward from the uint8 planes, bit 2 = weight gradient from them; default 3, 0 = the packed path
static int stem_u8_mode(int dtype, int in_is_u8, int C, int IW, int Cout, int KH, int KW, int stride, int pad) {
    if (!in_is_u8 || C != 3 || (dtype != ET_BF16 && dtype != ET_F16) || KH != 6 || KW != 6 || stride != 2 || pad != 2 || IW % 4 ||
        Cout > 64 || Cout % 8 || Cout < 8)
        return 0;
    return env_int("ET_STEM_U8", 3) & 3;
}
template <typename A>
static int stem_u8_segments(A& a, const void* const* seg_ptrs, const int* seg_counts, int n_segs, int IH, int IW) {
    if (!seg_ptrs || !seg_counts || n_segs < 1 || n_segs > STEM_MAX_SEGS || IH < 1 || IW < 4 || IW % 4) return -2;
    int n = 0;
    for (int s = 0; s < STEM_MAX_SEGS; ++s) {
        a.seg[s] = s < n_segs ? (const uint8_t*)seg_ptrs[s] : (const uint8_t*)seg_ptrs[0];
        a.seg_b[s] = s < n_segs ? n : 0x7fffffff;
        if (s < n_segs) {
            if (seg_counts[s] < 1 || !seg_ptrs[s] || ((uintptr_t)seg_ptrs[s] & 3)) return -2;      // quads are read as aligned dwords
            n += seg_counts[s];
        }
    }
    if ((long long)n * 3 * IH * IW >= (1ll << 40)) return -2;
    return n;
}

extern "C" int et_conv2d_stem_u8_fwd(const void* const* seg_ptrs, const int* seg_counts, int n_segs, float norm_scale, const void* w,
                                     void* y, int dtype, int IH, int IW, int Cout, int ldy, const float* scale, const float* bias,
                                     int act, float* stats, int stats_ld, const void* zero16, et_stream_t stream) {
    if (!w || !y || !zero16 || !(stem_u8_mode(dtype, 1, 3, IW, Cout, 6, 6, 2, 2) & 1) || ldy < Cout || ldy % 8 || act < 0 || act > 2) return -2;
    StemArgs a;
    const int N = stem_u8_segments(a, seg_ptrs, seg_counts, n_segs, IH, IW);
    if (N < 0) return N;
    a.norm = norm_scale;
    a.x = nullptr; a.zero = (const uint16_t*)zero16;      // the weight rows beyond Cout still come from the zero page
    a.w = (const uint16_t*)w; a.y = (uint16_t*)y;
    a.ldx = 8; a.Cout = Cout; a.ldy = ldy;
    stem_tiles(a, N, IH, IW);
    if (a.OH < 1 || a.OW < 1) return -2;
    launch_stem(true, a, dtype, scale, bias, act, stats, stats_ld, (hipStream_t)stream);
    ET_CHECK_LAUNCH();
    return 0;
}

extern "C" int et_conv2d_stem_u8_wgrad(const void* const* seg_ptrs, const int* seg_counts, int n_segs, float norm_scale, const void* dy,
                                       float* dw, int dtype, int IH, int IW, int Cout, int ldy, const void* zero16, et_stream_t stream) {
    if (!dy || !dw || !zero16 || !(stem_u8_mode(dtype, 1, 3, IW, Cout, 6, 6, 2, 2) & 2) || ldy < Cout || ldy % 8 || ((uintptr_t)dy & 15)) return -2;
    StemWgradArgs a;
    const int N = stem_u8_segments(a, seg_ptrs, seg_counts, n_segs, IH, IW);
    if (N < 0) return N;
    a.norm = norm_scale;
    a.dy = (const uint16_t*)dy; a.zero = (const uint16_t*)zero16; a.dw = dw;
    a.ldy = ldy; a.Cout = Cout;
    stem_tiles(a, N, IH, IW);
    if (a.OH < 1 || a.OW < 1) return -2;
    const int grid = stem_grid(a.ntiles);
    launch_stem_u8_wgrad(a, dtype, grid, (hipStream_t)stream);
    ET_CHECK_LAUNCH();
    return 0;
}

// ---- introspection (tests, bench.py) -----------------------------------------------------------------------
// What the entry points launch for a problem, found through the functions they call themselves (stem_eligible, fwd_geom /
// dgrad_geom / wgrad_geom, plan_gemm / plan_wgrad).  op as et_conv2d_kernel_name numbers it; arguments of the FORWARD conv.
struct ConvChoice {
    enum { STEM, GEMM, WGRAD } kind;
    int stem_pixels, stem_ntiles;                // STEM: output pixels, tiles
    GatherGeom g; const GemmPlan* gemm;          // GEMM
    const WgradRow* wgrad;                       // WGRAD
};
static int resolve_conv(ConvChoice& c, int op, int dtype, int N, int IH, int IW, int Cin, int Cout, int KH, int KW, int stride, int pad,
                        bool have_zero_page, int parity_class) {
    if (KH * KW > CONV_MAX_TAPS || stride < 1 || N <= 0 || op < 0 || op > 4) return -2;
    const int eb = dtype == ET_F32 ? 4 : 2, vec = dtype == ET_F32 ? 4 : 8;
    if (op == 2) {
        WgradGeom g;
        wgrad_geom(g, N, IH, IW, Cin, Cin, Cout, KH, KW, stride, pad, Cout);
        c.kind = ConvChoice::WGRAD; c.wgrad = plan_wgrad(g, eb, have_zero_page);
        return c.wgrad ? 0 : -2;
    }
    const bool full = op >= 3;
    if (op == 0 || op == 4) {
        if (stem_eligible(dtype, Cin, Cout, KH, KW, stride, pad, full, have_zero_page)) {
            StemArgs a;
            stem_tiles(a, N, IH, IW);
            c.kind = ConvChoice::STEM; c.stem_pixels = N * a.OH * a.OW; c.stem_ntiles = a.ntiles;
            return 0;
        }
        if (fwd_geom(c.g, N, IH, IW, Cin, Cin, Cout, KH, KW, stride, pad, Cout, vec)) return -2;
    } else {
        if (stride > 2) return -2;
        const int py = parity_class / stride, px = parity_class % stride;
        if (py >= stride) return -2;
        if (dgrad_geom(c.g, py, px, N, IH, IW, Cin, Cin, Cout, KH, KW, stride, pad, Cout, vec)) return -2;
    }
    c.kind = ConvChoice::GEMM; c.gemm = plan_gemm(c.g, eb, have_zero_page, full);
    return c.gemm ? 0 : -2;
}

extern "C" int et_conv2d_kernel_name(int op, int dtype, int N, int IH, int IW, int Cin, int Cout, int KH, int KW, int stride,
                                     int pad, int have_zero_page, int parity_class, char* buf, int buflen) {
    // op 0 = forward, 1 = dgrad (stride 2: parity_class 0..3 selects one of its four launches), 2 = wgrad, 3 = dgrad whose epilogue
    // adds a residual / accumulates / carries BN-backward sums (et_conv2d_dgrad with residual or accumulate, et_conv2d_dgrad_bn), 4 =
    // forward with a residual (the eval-mode Bottleneck shortcut): the persistent 1x1 kernel has separate instantiations for those.
    // Arguments as for et_conv2d_fwd (Cin/Cout of the FORWARD conv).  Writes the name of the kernel instantiation the
    // corresponding entry point launches, spelled as rocprofv3 prints it.  Host only; launches nothing.
    if (!buf || buflen < 8) return -1;
    ConvChoice c;
    const int rc = resolve_conv(c, op, dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad, have_zero_page != 0, parity_class);
    if (rc) return rc;
    if (c.kind == ConvChoice::STEM) snprintf(buf, buflen, "conv_stem_kernel");       // rocprofv3: "void conv_stem_kernel<ACT>(StemArgs)"
    else if (c.kind == ConvChoice::WGRAD) wgrad_plan_name(*c.wgrad, dtype, buf, buflen);
    else plan_name(*c.gemm, dtype, buf, buflen);
    return 0;
}

// the statistics entry points number their ops 0 = stats_partial of et_conv2d_fwd, 1 = bn_stats_partial of et_conv2d_dgrad_bn (stride
// 1), 2 = stats_partial of an et_conv2d_fwd call that ALSO passes a residual (launch_gemm then selects the full-epilogue plan, whose
// persistent 1x1 form has another tile height and grid: asking with op 0 for such a call used to return the plain plan's row count
// -- ADVICE r04): resolve_conv's 0, 3 and 4
static int resolve_stats(ConvChoice& c, int op, int dtype, int N, int IH, int IW, int Cin, int Cout, int KH, int KW, int stride, int pad,
                         int have_zero_page) {
    if (op < 0 || op > 2 || (op == 1 && stride != 1)) return -2;
    return resolve_conv(c, op == 0 ? 0 : (op == 1 ? 3 : 4), dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad, have_zero_page != 0, 0);
}

extern "C" int et_conv2d_stats_rows_for(int op, int dtype, int N, int IH, int IW, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                        int have_zero_page) {
    // rows of the partial-statistics buffer the kernel selected for this problem writes.  Arguments of the FORWARD conv.  One row
    // per 64 output pixels for the tiled kernels; the persistent 1x1 kernel writes one row per (workgroup, row group).
    ConvChoice c;
    const int rc = resolve_stats(c, op, dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad, have_zero_page);
    if (rc) return rc;
    if (c.kind == ConvChoice::STEM) return (c.stem_pixels + 63) / 64;
    if (c.gemm->kind == GEMM_S1) return s1_grid((c.g.M + c.gemm->BM - 1) / c.gemm->BM, *c.gemm) * c.gemm->WM;
    return (c.g.M + 63) / 64;
}

extern "C" int et_conv2d_stats_adds_for(int op, int dtype, int N, int IH, int IW, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                        int have_zero_page) {
    // fp32 atomic additions PER CHANNEL (all shards together) of the same call with a SHARDED accumulator (stats_ld > 0): every
    // kernel adds once per workgroup that covers the channel -- the persistent kernels (stem, 1x1 stream) once per resident
    // workgroup, the tiled kernels once per row tile (conv_stats_add_sharded_wg).  adds / ET_BN_SHARDS of them meet on one address.
    ConvChoice c;
    const int rc = resolve_stats(c, op, dtype, N, IH, IW, Cin, Cout, KH, KW, stride, pad, have_zero_page);
    if (rc) return rc;
    if (c.kind == ConvChoice::STEM) return stem_grid(c.stem_ntiles);
    const int ntm = (c.g.M + c.gemm->BM - 1) / c.gemm->BM;
    return c.gemm->kind == GEMM_S1 ? s1_grid(ntm, *c.gemm) : ntm;
}

extern "C" int et_conv2d_stem_kernel_name(int op, int dtype, int in_is_u8, int C, int N, int IH, int IW, int Cout, int KH, int KW, int stride,
                                          int pad, char* buf, int buflen) {
    // the stem as the MODEL calls it -- an image batch of C planes, uint8 or float -- op 0 = forward, 2 = weight gradient: the uint8
    // kernels when they take the problem (stem_u8_mode: shape, 16-bit compute type, ET_STEM_U8), else what et_conv2d_kernel_name says
    // about the packed 8-channel image
    if (!buf || buflen < 32 || (op != 0 && op != 2)) return -1;
    const int mode = stem_u8_mode(dtype, in_is_u8, C, IW, Cout, KH, KW, stride, pad);
    if (op == 0 && (mode & 1)) { snprintf(buf, buflen, "conv_stem_u8_kernel"); return 0; }
    if (op == 2 && (mode & 2)) { snprintf(buf, buflen, "conv_stem_u8_wgrad_kernel<%s>", dtype == ET_F16 ? "et_f16" : "unsigned short"); return 0; }
    return et_conv2d_kernel_name(op, dtype, N, IH, IW, 8, Cout, KH, KW, stride, pad, 1, 0, buf, buflen);
}
