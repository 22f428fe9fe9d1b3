// What more than one conv kernel file uses (layout and tile: the header of conv.hip): vector types, fast division, the gather geometry
// and epilogue arguments, one K-chunk of MFMAs, the slot swizzle of the transposing LDS reads -- and the kernel-argument structs and
// tile constants that the host layer (conv_host.hip) fills and reads.
#pragma once
#include "et_device.h"
#include "../../include/et_hip.h"
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;   // 16-byte register vector (SSA, no struct)
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ u32x4 mk4(unsigned a, unsigned b, unsigned c, unsigned d) { u32x4 v = {a, b, c, d}; return v; }
// "this register is defined HERE": whatever load produced it has completed in front of this point, and later uses depend on
// this (empty) instruction instead of the load
__device__ __forceinline__ void et_pin_loaded(u32x4& v) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
}

// one v_mfma_f32_32x32x16 of the 16-bit storage format T (uint16_t = bf16, et_f16 = IEEE half): a, b = 8 K-contiguous values per lane
// (V = any 16-byte register vector: u32x4, or the s16x8 the transposing LDS reads return)
template <typename T, typename V> __device__ __forceinline__ f32x16 et_mfma32(const V a, const V b, const f32x16 c) {
    static_assert(sizeof(V) == 16, "8 x 16-bit operands");
    if constexpr (std::is_same<T, et_f16>::value)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

#define CONV_MAX_TAPS 36
#define RS_A_ROWS(BM) ((BM) + 16)    // LDS rows of conv_gemm_rs_kernel's activation unit: BM + 2 pixels + one pad slot per image row
#define PPRS_ROWS 320                // LDS rows of conv_gemm_pprs_kernel's activation unit (five 64-row pieces: its header)

struct FastDiv {
    uint32_t magic, shift, d;
};
static FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    if (d == 0) d = 1;           // degenerate geometry (empty lattice): such launches are skipped, but never divide by zero here
    f.d = d;
    uint32_t s = 0;
    while ((1ull << s) < d) ++s;
    f.shift = s;
    f.magic = (uint32_t)((((1ull << 32) * ((1ull << s) - d)) / d) + 1);
    return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
    return (__umulhi(n, f.magic) + n) >> f.shift;   // exact for n < 2^31
}

struct GatherGeom {
    int N, IH, IW, Cin, ldx;     // gathered tensor (NHWC), channels per tap, pixel stride (elements)
    int QH, QW, M;               // output lattice and its size N*QH*QW
    int OH, OW, Cout, ldy;       // written tensor, pixel stride
    int isy, isx;                // gathered coord = q*is + d[tap]
    int osy, osx, ooy, oox;      // written coord  = q*os + oo
    int T, TT;                   // taps in this launch / taps per weight row (row = TT*Cin)
    int CV, KV;                  // Cin/VEC, T*CV
    int tap_inner;               // K-chunk order: 1 = channel-chunk outer / tap inner (L2-friendly), 0 = tap outer
    int xcd_swz;                 // 1 = remap blockIdx.x so that neighbouring pixel tiles share an XCD (L2)
    int ntm, ntn, nfast;         // tile grid (1-D launch, decoded in-kernel); nfast: channel tiles of a pixel tile adjacent
    FastDiv dQW, dQH, dCV, dW1;  // dW1: by QW + 1 (conv_gemm_rs_kernel's padded raster)
    signed char dy[CONV_MAX_TAPS], dx[CONV_MAX_TAPS];
    unsigned char wt[CONV_MAX_TAPS];
    int tapinfo[CONV_MAX_TAPS];  // (dy & 0xff) | (dx & 0xff) << 8 | wt << 16 : one scalar load per chunk
};

struct Epilogue {
    const float* scale;     // [Cout] or null: v = acc*scale (folded eval-mode BatchNorm)
    const float* bias;      // [Cout] or null
    int act;                // ACT_* (et_host.h)
    const void* res;        // residual (same dtype, added after act) or null
    int ldr;
    float* stats;           // partial BN statistics [gridDim.x][2][Cout] or null
    int accumulate;         // out += result
    // BatchNorm-BACKWARD statistics of the layer whose activation gradient this launch produces (dgrad only): with
    // bn_y set, `stats` receives per-tile sums of  du = v * act'(y*bn_scale + bn_shift)  and  du * y  over the final
    // values v (after residual / accumulate) instead of the forward sums -- the reduce pass of et_bn_act_bwd is then
    // skipped for this tensor (its dz / y re-read, 4 B per element, becomes one y read inside this epilogue)
    const void* bn_y;
    int ld_bn;
    const float* bn_scale;
    const float* bn_shift;
    int bn_act;
    // stats_ld != 0: `stats` is a SHARDED accumulator [ET_BN_SHARDS][2][stats_ld] (zero before the launch) instead of partial rows:
    // every wave ADDS its sums into shard blockIdx.x % ET_BN_SHARDS (16 shards: workgroups are dealt round-robin to the 8 XCDs, so a
    // shard is touched from ONE XCD and two shards share an XCD) with hardware fp32 atomics, and the consumer
    // (et_bn_act_fwd_sharded / et_bn_act_bwd_sharded) folds the ET_BN_SHARDS shards itself -- no finalize launch per layer
    int stats_ld;
};

template <int BKV> __device__ __forceinline__ int lds_swz(int r) {
    if constexpr (BKV == 8) return ((r >> 1) & 7) ^ ((r >> 4) & 3);
    else return (r >> 2) & 3;
}


// ---- one K-chunk of MFMAs from LDS --------------------------------------------------------------
struct NoBetween { __device__ __forceinline__ void operator()(int) const {} };
template <typename T, int BM, int BN, int WM, int WN, int BKV, typename BETWEEN = NoBetween>
__device__ __forceinline__ void mma_chunk(const u32x4* __restrict__ sm, f32x16 (&acc)[BM / WM / 32][BN / WN / 32],
                                          int wm, int wn, int lane, BETWEEN between = BETWEEN()) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    const int l31 = lane & 31, g = lane >> 5;
    // Software-pipelined over the k-steps: the fragments of step kk+1 are requested BEFORE the MFMAs of step
    // kk are issued (two fragment register sets), so the LDS latency overlaps TM*TN MFMAs instead of
    // stalling the wave in front of them.  The sched_barrier keeps the compiler from sinking the reads
    // back below the MFMAs; the waitcnt pass then waits for the older set only (lgkmcnt(TM+TN)).
    u32x4 af[2][TM], bf[2][TN];
    auto fetch = [&](int kk, int set) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            const int r = wm * (BM / WM) + tm * 32 + l31;
            af[set][tm] = sm[r * BKV + ((kk * 2 + g) ^ lds_swz<BKV>(r))];
        }
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int r = wn * (BN / WN) + tn * 32 + l31;
            bf[set][tn] = sm[(BM + r) * BKV + ((kk * 2 + g) ^ lds_swz<BKV>(r))];
        }
    };
    fetch(0, 0);
#pragma unroll
    for (int kk = 0; kk < BKV / 2; ++kk) {
        const int cur = kk & 1;
        if (kk + 1 < BKV / 2) {
            fetch(kk + 1, cur ^ 1);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                if constexpr (sizeof(T) == 2) {
                    acc[tm][tn] = et_mfma32<T>(af[cur][tm], bf[cur][tn], acc[tm][tn]);
                } else {
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(af[cur][tm].x), __uint_as_float(bf[cur][tn].x), acc[tm][tn], 0, 0, 0);
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(af[cur][tm].y), __uint_as_float(bf[cur][tn].y), acc[tm][tn], 0, 0, 0);
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(af[cur][tm].z), __uint_as_float(bf[cur][tn].z), acc[tm][tn], 0, 0, 0);
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(af[cur][tm].w), __uint_as_float(bf[cur][tn].w), acc[tm][tn], 0, 0, 0);
                }
            }
        between(kk);
    }
}

// ---- transposing LDS reads (ds_read_b64_tr_b16: conv_wgrad_tr_kernel's header): the slot swizzle of a [pixel][channel] tile -------
template <int SLOTS> __device__ __forceinline__ int tr_swz(int p) {
    if constexpr (SLOTS >= 16) return 4 * (p & 3);
    else return 4 * ((p >> 1) & 1);
}
// the X tile of the stride-2 row-sharing weight gradient: a fragment's 16 K-slots are 16 ALTERNATE rows (2 * slot + tap), so the
// swizzle is taken from the row PAIR -- rows 0, 2, 4, 6 (and 1, 3, 5, 7) get four different values, and it repeats every 8 rows
template <int SLOTS> __device__ __forceinline__ int tr_swz2(int p) {
    if constexpr (SLOTS >= 16) return 4 * ((p >> 1) & 3);
    else return 4 * ((p >> 2) & 1);
}

// ---- kernel arguments and tile constants of the stem kernels (conv_stem.hip) ------------------------------------------------------
#define STEM_TR 4
#define STEM_TC 64
#define STEM_PH 12                      // patch rows = 2 * TR + 4
#define STEM_PITCH 132                  // patch columns = 2 * TC + 4
#define STEM_PSLOTS (7 * 256)           // 12 * 132 = 1584 slots, rounded up to whole staging instructions
#define STEM_WPITCH 37
#define STEM_WSLOTS (10 * 256)          // 64 * 37 = 2368 slots, rounded up
#define STEM_MAX_SEGS 4

struct StemArgs {
    const uint16_t* x; const uint16_t* w; uint16_t* y; const uint16_t* zero;
    int N, IH, IW, ldx, OH, OW, ldy, Cout;
    int trn, tcn, ntiles;               // tile grid per image: rows, cols; total tiles
    const float* scale; const float* bias; int act;
    float* stats; int stat_rows;        // [stat_rows][2][Cout] or null
    int stats_ld;                       // != 0: sharded accumulator [ET_BN_SHARDS][2][stats_ld] (Epilogue::stats_ld)
    // the uint8 form (conv_stem_u8_kernel): the image is NOT the packed tensor x but up to four runs of uint8 NCHW images (3 planes each);
    // image n belongs to the last segment whose first image seg_b[s] <= n (unused segments: seg_b = INT_MAX); value = byte / norm
    const uint8_t* seg[STEM_MAX_SEGS]; int seg_b[STEM_MAX_SEGS]; float norm;
};

struct StemWgradArgs {
    const uint8_t* seg[STEM_MAX_SEGS]; int seg_b[STEM_MAX_SEGS]; float norm;
    const uint16_t* dy; const uint16_t* zero; float* dw;
    int N, IH, IW, OH, OW, ldy, Cout;
    int trn, tcn, ntiles;
};

// ---- kernel arguments of the weight-gradient kernels (conv_wgrad.hip) -------------------------------------------------------------
struct WgradGeom {
    int N, IH, IW, Cin, ldx;     // X (gathered operand)
    int QH, QW, P;               // dY lattice (== dY tensor), P = N*QH*QW
    int Cout, ldy;               // dY channels / pixel stride
    int isy, isx;
    int T, NC;                   // taps, NC = T*Cin columns of dW
    int xcd;                     // 1 = remap the linear workgroup id so that one K-split's tiles share an XCD
    int Pper;                    // pixels per split-K slice (multiple of the K-chunk)
    int ntn, ntm, nsk;           // tile grid: column tiles, cout tiles, K splits (1-D launch, decoded in-kernel)
    FastDiv dQW, dQH, dCin, dW1; // dW1: by QW + 1 (conv_wgrad_rs_kernel's padded raster)
    int PP;                      // padded slots N*QH*(QW+1) (conv_wgrad_rs_kernel's GEMM-K)
    int ident;                   // 1 = every tap reads X at the dY pixel itself (1x1, stride 1, pad 0): X row = dY row, no decode
    int buf;                     // ident layers: stage through buffer descriptors (host: both tensors < 2^31 bytes, ET_CONV_BUF_DMA != 0)
    signed char dy[CONV_MAX_TAPS], dx[CONV_MAX_TAPS];
};

// Up to WGRAD_MAX_GROUP layers of IDENTICAL geometry in one launch (et_conv2d_wgrad_grouped): the K-split that
// fills the chip is then shared by the whole group, so every dW address receives group-size times fewer fp32
// atomics (measured with s_memtime stamps: the atomic epilogue is 23-27 % of a workgroup's lifetime when a
// single 256-channel layer is split 28-64 ways; the L2 atomic rate, ~1 TB/s, does not depend on scope).
#define WGRAD_MAX_GROUP 16
struct WgradItem { const uint16_t* x; const uint16_t* dy; float* dw; int ldx, ldy; };
struct WgradGroup { WgradItem it[WGRAD_MAX_GROUP]; int n; };
