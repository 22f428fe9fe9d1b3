// Host-only declarations shared by the conv host layer (conv_host.hip) and the kernel files, whose launch functions it calls.
// The dtype / activation dispatch (with_dtype, with_act) is et_host.h's, shared with the kernel files outside the conv family.
#pragma once
#include "et_host.h"
#include "conv_device.h"

static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static int device_cus() {
    static const int n_cu = [] { hipDeviceProp_t p; int d = 0; return (hipGetDevice(&d) == hipSuccess && hipGetDeviceProperties(&p, d) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256; }();
    return n_cu;
}

enum { GEMM_REG = 0, GEMM_GLDS = 1, GEMM_PP = 2, GEMM_RS = 3, GEMM_PPRS = 4, GEMM_S1 = 5 };

// ---- the instantiations: ONE row list per kernel family (a row = the template arguments after T) --------------------------------
// Each list is expanded twice: into a table of GemmPlan rows (conv_host.hip: ONE object per family), which the plan functions search
// and plan_name / s1_grid / the statistics-row count read, and into the dispatch of the launch function in the file that holds the
// family's kernels, which instantiates the row at the same index.  A plan IS a pointer to a table row: the name reported and the
// kernel launched cannot describe different tuples.
//      conv1x1_stream_kernel (+ _flat twin; its header explains the register budget): K/64 WN TN WM TMW NS WGS FULL (= residual /
//      accumulate / BN-backward sums in the epilogue)
#define ET_S1_ROWS \
    ET_S1(4, 4, 2, 1, 1, 8, 2, false)  /* four waves, 64-channel wave tiles, two workgroups per CU */ \
    ET_S1(4, 2, 2, 2, 1, 6, 2, false)  \
    ET_S1(2, 4, 2, 1, 2, 6, 2, false)  /* ring: 8 x 4 KB / 6 x 8 KB / 3 x 16 KB beside the 16-row slabs */ \
    ET_S1(2, 2, 2, 2, 2, 3, 2, false)  \
    ET_S1(2, 1, 2, 4, 1, 3, 2, false)  \
    ET_S1(1, 4, 2, 1, 2, 6, 2, false)  \
    ET_S1(1, 2, 2, 2, 2, 3, 2, false)  \
    ET_S1(1, 1, 2, 4, 1, 3, 2, false)  \
    ET_S1(4, 8, 1, 1, 1, 16, 1, true)  /* eight waves, 32-channel wave tiles, one workgroup per CU */ \
    ET_S1(4, 4, 1, 2, 1, 10, 1, true)  \
    ET_S1(2, 4, 2, 1, 1, 8, 2, true)   \
    ET_S1(2, 2, 2, 2, 1, 6, 2, true)   \
    ET_S1(2, 1, 2, 4, 1, 3, 2, true)   \
    ET_S1(1, 4, 2, 1, 1, 8, 2, true)   \
    ET_S1(1, 2, 2, 2, 1, 6, 2, true)   \
    ET_S1(1, 1, 2, 4, 1, 3, 2, true)
//      conv_gemm_glds_kernel: BM BN WM WN BKV NS UTAP (NS = 3, the short-K ring: 16-bit types only)
#define ET_GLDS_ROWS \
    ET_GLDS(128, 128, 2, 2, 4, 3, true)  ET_GLDS(128, 64, 2, 2, 4, 3, true)  /* short-K: 32-wide chunks, 3-deep ring */ \
    ET_GLDS(128, 128, 2, 2, 8, 2, true)  ET_GLDS(128, 64, 2, 2, 8, 2, true)  \
    ET_GLDS(128, 128, 2, 2, 4, 2, true)  ET_GLDS(128, 64, 2, 2, 4, 2, true)  \
    ET_GLDS(128, 128, 2, 2, 4, 2, false) ET_GLDS(128, 64, 2, 2, 4, 2, false)
//      conv_gemm_kernel: BM BN WM WN BKV UTAP
#define ET_REG_ROWS \
    ET_REG(128, 128, 2, 2, 8, true)  ET_REG(128, 64, 2, 2, 8, true)  \
    ET_REG(128, 128, 2, 2, 4, true)  ET_REG(128, 64, 2, 2, 4, true)  \
    ET_REG(128, 128, 2, 2, 4, false) ET_REG(128, 64, 2, 2, 4, false)
//      conv_gemm_rs_kernel (+ its _flat twin): BM BN WM WN
#define ET_RS_ROWS ET_RS(128, 128, 2, 2) ET_RS(128, 64, 2, 2)

struct GemmPlan { int kind, BM, BN, WM, WN, BKV, NS; bool utap; int wgs, kc, tn, full; };   // wgs / kc / tn / full: conv1x1_stream_kernel only

// the weight-gradient instantiations, one row list per family as for the gather-GEMMs above (expanded into the WgradRow tables of
// conv_host.hip and into the launches of conv_wgrad.hip's launch_wgrad_row)
//      conv_wgrad_tr_kernel: BM BN WM WN
#define ET_WG_ROWS \
    ET_WG(256, 256, 2, 4) ET_WG(256, 128, 4, 2) ET_WG(256, 64, 4, 1) \
    ET_WG(128, 256, 2, 4) ET_WG(128, 128, 2, 2) ET_WG(128, 64, 2, 2) \
    ET_WG(64, 256, 1, 4)  ET_WG(64, 128, 2, 2)  ET_WG(64, 64, 2, 2)
//      conv_wgrad_rs_kernel: BM BNC WM WN STRIDE
#define ET_WGRS_ROWS ET_WGRS(128, 128, 2, 4, 1) ET_WGRS(64, 64, 2, 2, 1) ET_WGRS(128, 64, 2, 2, 2)
//      conv_wgrad_kernel (register-staged, 256 threads): BM BN
#define ET_WGREG_ROWS ET_WGREG(128, 128) ET_WGREG(128, 64) ET_WGREG(64, 128) ET_WGREG(64, 64)
enum { WGRAD_REG = 0, WGRAD_TR = 1, WGRAD_RS = 2 };
struct WgradRow { int kind, bm, bn, wm, wn, stride; };

#pragma GCC visibility push(hidden)                // cross-file, not part of the C ABI
// the row tables: defined ONCE, in conv_host.hip (a plan is compared by address)
extern const GemmPlan s1_rows[], glds_rows[], reg_rows[], rs_rows[];
extern const WgradRow wg_rows[], wgrs_rows[], wgreg_rows[];
// persistent-grid sizes (conv_host.hip: the launches and the statistics entry points share them)
int s1_grid(int ntm, const GemmPlan& p);
int stem_grid(int ntiles);
// One launch function per kernel file: the dtype switch and the file's row lists expanded as launches.  pp / wp: the plan, a row of
// its family's table; g: complete (launch_gemm / launch_wgrad of conv_host.hip set the tile grid and the split).  0, or -2 when no
// instantiation exists for (row, dtype).
int launch_gemm_row(const GemmPlan* pp, int dtype, const void* X, const void* W, void* Y, const void* zero16, const GatherGeom& g,
                    const Epilogue& ep, hipStream_t s);                        // conv.hip
int launch_wgrad_row(const WgradRow* wp, int dtype, const WgradGroup& grp, const void* zero16, WgradGeom g, hipStream_t s);   // conv_wgrad.hip
void launch_stem(bool u8, StemArgs& a, int dtype, const float* scale, const float* bias, int act, float* stats, int stats_ld,
                 hipStream_t s);                                               // conv_stem.hip
void launch_stem_u8_wgrad(const StemWgradArgs& a, int dtype, int grid, hipStream_t s);
#pragma GCC visibility pop
