// Implicit-GEMM convolution on the gfx950 matrix cores: forward, dgrad and wgrad of the
// conv in `Conv` (reference models/backbone/common.py:471-481; shapes: SURVEY.md appendix A), the
// Detect output convs (models/head/yolov5_head.py:30) and the netD 1x1 convs (yolo_ssod.py:224-238).
//
// Layout: activations NHWC (channels contiguous), weights [Cout][KH][KW][Cin] -- so the GEMM K axis
// (tap, ci) is contiguous for BOTH MFMA operands and every global access is a 16-byte vector.
//
//   gather-GEMM (fwd, dgrad):  D[pixel, cout] = sum_{tap, ci} X[gather(pixel, tap), ci] * W[cout, tap, ci]
//       A rows = output-lattice pixels, B rows = output channels.  dgrad is the same kernel run on dY
//       with the transposed weight and a tap table of (dy,dx) input offsets; stride-2 dgrad is split
//       into its 4 output-parity classes so that no MFMA work is spent on structurally-zero taps.
//   wgrad:  dW[cout, (tap,ci)] = sum_pixel dY[pixel, cout] * X[gather(pixel,tap), ci]; K = pixels, so
//       both operands are transposed on the fly: each lane loads VEC pixel-rows of VEC channels
//       (16 B each, coalesced along channels), transposes the VECxVEC block in registers and writes
//       K(pixel)-contiguous 16-byte rows to LDS.  Split-K over pixels, fp32 atomicAdd into the grad.
//
// Tile: 256 threads = 4 waves, BM x BN block tile (128x128 / 128x64), each wave a 64x64 or 64x32
// sub-tile of 32x32 MFMAs (v_mfma_f32_32x32x16_bf16; parity mode: exact-f32 v_mfma_f32_32x32x2_f32).
// LDS rows hold BKV 16-byte K-vectors, XOR-swizzled so that the ds_read_b128 fragment reads of a
// lane group hit 16 distinct (bank-half, slot) pairs; double buffered, one barrier per K-chunk,
// next chunk's global loads are issued before the MFMAs of the current one.
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
// workgroups per CU the short-K 128x64 tile (32-wide chunks, 3-deep ring, 36 KB of LDS) is compiled for: 3 = 129 VGPRs, 4 = 128 + two spilled
// dwords.  Four resident workgroups keep more bytes in flight on these HBM-bound 1x1 layers: step 53.70 -> 53.38 ms, same box, two
// alternations (profiles/r03_shortk_four_workgroups_ab.txt)
#ifndef ET_S1_NT
#define ET_S1_NT 1               // non-temporal LDS-DMA for the stream kernel's activation rows: every row is read once, by one CU
                                 // (isolated, B = 64: 128->64 @160 119.7 -> 113.0 us, 128->128 @160 160 -> 153, 256->256 @80 86 -> 83; 0 = default
                                 // policy; on the activation units of the ping-pong row-shift tile the same hint LOST 1-2 %: 116.5 -> 118.6 us)
#endif
#ifndef ET_GLDS_SHORTK_WGS
#define ET_GLDS_SHORTK_WGS 4
#endif
#define RS_A_ROWS(BM) ((BM) + 16)    // LDS rows of conv_gemm_rs_kernel's activation unit: BM + 2 pixels + one pad slot per image row

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

// chunk-uniform tap lookup: the index is made provably wave-uniform so that the table read is a scalar
// (SMEM) load -- a vector load here would put an s_waitcnt vmcnt(0) in the middle of the LDS-DMA burst
__device__ __forceinline__ void tap_lookup_uniform(const GatherGeom& g, int tap, int& dy, int& dx, int& wt) {
    const int ti = g.tapinfo[__builtin_amdgcn_readfirstlane(tap)];
    dy = (int)(signed char)(ti & 0xff);
    dx = (int)(signed char)((ti >> 8) & 0xff);
    wt = (ti >> 16) & 0xff;
}

enum { ACT_NONE = 0, ACT_SILU = 1, ACT_RELU = 2 };

struct Epilogue {
    const float* scale;     // [Cout] or null: v = acc*scale (folded eval-mode BatchNorm)
    const float* bias;      // [Cout] or null
    int act;
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

// Workgroup -> tile.  The launch is 1-D over ntm x ntn tiles.  Workgroups are dealt round-robin to the 8 XCDs
// (private L2 each): with xcd_swz the linear id is remapped so that each XCD owns a contiguous range of the
// tile sequence, and with nfast that sequence runs over the channel tiles of one pixel tile first -- the
// workgroups that read the same activation rows (and, for 3x3, the halo rows of the neighbouring pixel
// tiles) are then co-resident on one XCD and share them through its L2 instead of each pass over the
// channel tiles re-fetching the whole activation tensor through the fabric (placement only: results do not
// depend on it).
__device__ __forceinline__ void tile_of_block(const GatherGeom& g, int& bx, int& by) {
    int id = blockIdx.x;
    if (g.nfast) {
        if (g.xcd_swz) {
            const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = id & 7, k = id >> 3;
            id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;     // bijective for any nb
        }
        bx = id / g.ntn;
        by = id - bx * g.ntn;
    } else {
        by = id / g.ntm;
        bx = id - by * g.ntm;
        if (g.xcd_swz) {
            const int nb = g.ntm, q = nb >> 3, r = nb & 7, xcd = bx & 7, k = bx >> 3;
            bx = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
        }
    }
}

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

// ---- shared epilogue of the gather-GEMM kernels -----------------------------------------------------
// LDS floats the epilogue needs: one private [32][BN/WN + 4] fp32 slab per wave
template <int BM, int BN, int WM, int WN, int SROWS = 32> struct EpiLds {
    static constexpr int WCOLS = BN / WN, SLD = WCOLS + 4, SLAB = SROWS * SLD;
    static constexpr int FLOATS = WM * WN * SLAB;
    static constexpr int VEC16 = (FLOATS * 4 + 15) / 16;
};

// scale/bias/activation in registers (a lane owns ONE output channel per 32x32 tile), BN partial statistics
// from the raw accumulators; then every wave transposes its own accumulator tile, 32 rows at a time, through
// a PRIVATE fp32 LDS slab so that the global stores are 16-byte vectors along the channel axis -- no
// workgroup barrier anywhere in the store path (measured with s_memtime stamps: the previous version, which
// staged half the block tile per __syncthreads round with a run-time activation switch per element, spent
// 12.5 k cycles on a 128x64 tile and 23 k on 128x128 -- 22 % of a 3x3 and 45-60 % of a 1x1 layer's
// workgroup lifetime).  residual / accumulate are vector loads.
// SROWS = rows of the private slab: 32 (one MFMA tile per round) or 16 (two rounds per tile, half the LDS: the persistent 1x1
// kernel keeps its operand ring resident beside the slabs).
// The per-lane statistics live in an EpiSums the caller owns: the tiled kernels pass a fresh one per tile and let the epilogue write
// it out (DEFER = false); the persistent 1x1 kernel accumulates over ALL its tiles and writes one partial row per workgroup at the
// end (DEFER = true, conv_epilogue_write_stats).  MODE 0: every feature behind run-time flags; MODE 1: plain layer only -- no
// residual, no accumulate, no BN-backward sums (their code and registers are compiled out: the caller guarantees the flags are off).
template <int TN> struct EpiSums {
    float ssum[TN], ssq[TN];        // forward: per-lane sums of the raw accumulators / their squares (lane owns one channel per column tile)
    float bs1[8], bs2[8];           // BN-backward: sums of du and du * y over this lane's 8 channels of the store phase
    // per-channel constants staged in LDS by the caller: [scale | bias | bn_scale | bn_shift], `cstride` floats each, indexed by the
    // channel inside the workgroup's column range (DEFER callers only; the tiled kernels read global memory once per tile).  A
    // persistent kernel must not read them from global memory per tile: the wait for such a load sits behind every LDS-DMA piece
    // the ring has in flight (vector-memory loads retire in order)
    const float* cst = nullptr;
    int cstride = 0;
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) { ssum[tn] = 0.f; ssq[tn] = 0.f; }
#pragma unroll
        for (int e = 0; e < 8; ++e) { bs1[e] = 0.f; bs2[e] = 0.f; }
    }
};

// one partial row (rows, 2, Cout) of this WAVE's sums: channels n0 + wn * WCOLS ..., row `row`; `zero_rows` further rows are zeroed
template <int BN, int WN, int MODE>
__device__ __forceinline__ void conv_epilogue_write_stats(EpiSums<BN / WN / 32>& st, const GatherGeom& g, const Epilogue& ep, int n0, int lane,
                                                          int wn, int row, int zero_rows, int nrows) {
    constexpr int TN = BN / WN / 32, WCOLS = BN / WN, CVN = WCOLS / 8;
    const int l31 = lane & 31, hi = lane >> 5;
    const int scv = lane % CVN;
    const int co = n0 + wn * WCOLS + scv * 8;
    const bool bnb = MODE == 1 ? false : ep.bn_y != nullptr;
    if (bnb) {
        // BN-backward sums: lanes of a wave that share a channel group (same scv, different srow) are CVN apart: xor-reduce over
        // the srow bits, lane scv then holds the sums of its 8 channels
#pragma unroll
        for (int e = 0; e < 8; ++e)
            for (int m = CVN; m < 64; m <<= 1) { st.bs1[e] += __shfl_xor(st.bs1[e], m); st.bs2[e] += __shfl_xor(st.bs2[e], m); }
        if (ep.stats_ld) {
            if (lane < CVN && co + 8 <= g.Cout) {
                float* d0 = ep.stats + ((size_t)(blockIdx.x % ET_BN_SHARDS) * 2) * ep.stats_ld + co;
#pragma unroll
                for (int e = 0; e < 8; ++e) { unsafeAtomicAdd(d0 + e, st.bs1[e]); unsafeAtomicAdd(d0 + ep.stats_ld + e, st.bs2[e]); }
            }
        } else if (lane < CVN && co + 8 <= g.Cout) {
            for (int r = 0; r <= zero_rows; ++r) {
                if (row + r >= nrows) break;
                float* d0 = ep.stats + ((size_t)(row + r) * 2 + 0) * g.Cout + co;
                float* d1 = ep.stats + ((size_t)(row + r) * 2 + 1) * g.Cout + co;
                if (r == 0) {
                    *(float4*)d0 = make_float4(st.bs1[0], st.bs1[1], st.bs1[2], st.bs1[3]); *(float4*)(d0 + 4) = make_float4(st.bs1[4], st.bs1[5], st.bs1[6], st.bs1[7]);
                    *(float4*)d1 = make_float4(st.bs2[0], st.bs2[1], st.bs2[2], st.bs2[3]); *(float4*)(d1 + 4) = make_float4(st.bs2[4], st.bs2[5], st.bs2[6], st.bs2[7]);
                } else {
                    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                    *(float4*)d0 = z; *(float4*)(d0 + 4) = z; *(float4*)d1 = z; *(float4*)(d1 + 4) = z;
                }
            }
        }
    } else {
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const float sv = st.ssum[tn] + __shfl_xor(st.ssum[tn], 32);   // the two lane halves hold the two row halves of a channel
            const float qv = st.ssq[tn] + __shfl_xor(st.ssq[tn], 32);
            const int cc = n0 + wn * WCOLS + tn * 32 + l31;
            if (ep.stats_ld) {
                if (hi == 0 && cc < g.Cout) {
                    float* d0 = ep.stats + ((size_t)(blockIdx.x % ET_BN_SHARDS) * 2) * ep.stats_ld + cc;
                    unsafeAtomicAdd(d0, sv); unsafeAtomicAdd(d0 + ep.stats_ld, qv);
                }
            } else if (hi == 0 && cc < g.Cout) {
                for (int r = 0; r <= zero_rows; ++r) {
                    if (row + r >= nrows) break;
                    ep.stats[((size_t)(row + r) * 2 + 0) * g.Cout + cc] = r == 0 ? sv : 0.f;
                    ep.stats[((size_t)(row + r) * 2 + 1) * g.Cout + cc] = r == 0 ? qv : 0.f;
                }
            }
        }
    }
}

// Sharded statistics of a workgroup (Epilogue::stats_ld != 0): the sums of its WM wave rows meet in LDS first, then ONE atomic per
// channel and workgroup (et_conv2d_stats_adds_for counts them).  The workgroups of a persistent grid finish together, so their
// atomics arrive together and queue per address in the memory-side atomic units (~25 ns each, r05): gridDim.x / ET_BN_SHARDS deep
// instead of WM times that.  r06: the tiled kernels end their epilogue with the same pre-reduction (n0 = the tile's first channel) --
// the barrier sits AFTER every wave's store passes, where a wave that is done could only idle until its workgroup retires anyway --
// which halves the additions per address of the 2-wave-row tiles and brings the 3200-tile layers (128 -> 128 3x3 @80, 512 -> 128 @80)
// under the sharding threshold (ops.SHARD_MAX_ADDS): the step's 28 remaining finalize launches go away.
// red: LDS, WM * 2 * BN floats, free to use once every wave has passed the barrier inside.
template <int BN, int WN, int WM, int MODE>
__device__ __forceinline__ void conv_stats_add_sharded_wg(EpiSums<BN / WN / 32>& st, const GatherGeom& g, const Epilogue& ep, int tid, int lane,
                                                          int wm, int wn, float* red, int n0 = 0) {
    constexpr int TN = BN / WN / 32, WCOLS = BN / WN, CVN = WCOLS / 8;
    const int l31 = lane & 31, hi = lane >> 5;
    const bool bnb = MODE == 1 ? false : ep.bn_y != nullptr;
    __syncthreads();
    float* const r0 = red + (wm * 2) * BN + wn * WCOLS;
    if (bnb) {
        const int scv = lane % CVN;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            for (int m = CVN; m < 64; m <<= 1) { st.bs1[e] += __shfl_xor(st.bs1[e], m); st.bs2[e] += __shfl_xor(st.bs2[e], m); }
        if (lane < CVN) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { r0[scv * 8 + e] = st.bs1[e]; r0[BN + scv * 8 + e] = st.bs2[e]; }
        }
    } else {
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const float sv = st.ssum[tn] + __shfl_xor(st.ssum[tn], 32);
            const float qv = st.ssq[tn] + __shfl_xor(st.ssq[tn], 32);
            if (hi == 0) { r0[tn * 32 + l31] = sv; r0[BN + tn * 32 + l31] = qv; }
        }
    }
    __syncthreads();
    float* const dst = ep.stats + ((size_t)(blockIdx.x % ET_BN_SHARDS) * 2) * ep.stats_ld + n0;
    for (int i = tid; i < 2 * BN; i += 64 * WM * WN) {
        const int t = i / BN, c = i % BN;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < WM; ++w) v += red[(w * 2 + t) * BN + c];
        if (n0 + c < g.Cout) unsafeAtomicAdd(dst + (size_t)t * ep.stats_ld + c, v);
    }
}

template <typename T, int BM, int BN, int WM, int WN, int ACT, int SROWS = 32, int MODE = 0, bool DEFER = false, bool EPF = true>
__device__ __forceinline__ void conv_epilogue_act(f32x16 (&acc)[BM / WM / 32][BN / WN / 32], u32x4* lds_raw, T* __restrict__ Y,
                                                  const GatherGeom& g, const Epilogue& ep, int bx, int m0, int n0, int tid,
                                                  int lane, int wm, int wn, EpiSums<BN / WN / 32>& st) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    static_assert(SROWS == 32 || SROWS == 16, "slab rows");
    constexpr int NH = 32 / SROWS;                 // slab rounds per 32-row MFMA tile
    using L = EpiLds<BM, BN, WM, WN, SROWS>;
    constexpr int WCOLS = L::WCOLS, SLD = L::SLD;
    constexpr int CVN = WCOLS / 8;                 // 8-channel groups per slab row
    constexpr int RPI = 64 / CVN;                  // slab rows stored per wave iteration
    static_assert(RPI <= SROWS, "a store iteration covers at most one slab");
    const int l31 = lane & 31, hi = lane >> 5;
    const int wave = wm * WN + wn;
    float* const stg = (float*)lds_raw + wave * L::SLAB;
    float (&ssum)[TN] = st.ssum;
    float (&ssq)[TN] = st.ssq;
    float (&bs1)[8] = st.bs1;
    float (&bs2)[8] = st.bs2;
    const bool ident = (g.osy == 1 && g.osx == 1 && g.ooy == 0 && g.oox == 0 && g.QH == g.OH && g.QW == g.OW);
    float csc[TN], cbi[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int co = n0 + wn * WCOLS + tn * 32 + l31;
        const bool cok = co < g.Cout;
        if constexpr (DEFER) {           // (a persistent caller: compile-time, so that the LDS address space is inferred)
            csc[tn] = st.cst[co - n0];
            cbi[tn] = st.cst[st.cstride + co - n0];
        } else {
            csc[tn] = (ep.scale && cok) ? ep.scale[co] : 1.0f;
            cbi[tn] = (ep.bias && cok) ? ep.bias[co] : 0.0f;
        }
    }
    const int srow = lane / CVN, scv = lane % CVN;  // this lane's (row, channel group) in the store phase
    const int co = n0 + wn * WCOLS + scv * 8;
    // BN-backward statistics mode: this lane owns 8 channels in the store phase; per-channel affine in registers
    const bool bnb = MODE == 1 ? false : ep.bn_y != nullptr;
    const void* const ep_res = MODE == 1 ? nullptr : ep.res;
    const bool ep_accumulate = MODE == 1 ? false : (bool)ep.accumulate;
    // (wave-uniform is enough: the store pass has no workgroup barrier.  Per wave since r05: the waves of a ragged tile whose own rows
    // are all inside keep the fast pass)
    const bool lean = ident && !bnb && ep_res == nullptr && !ep_accumulate && m0 + (wm + 1) * (BM / WM) <= g.M && n0 + BN <= g.Cout;
    float bsc[8], bsh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { bsc[e] = 1.f; bsh[e] = 0.f; }
    if (bnb && co + 8 <= g.Cout) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if constexpr (DEFER) { bsc[e] = st.cst[2 * st.cstride + co - n0 + e]; bsh[e] = st.cst[3 * st.cstride + co - n0 + e]; }
            else { bsc[e] = ep.bn_scale[co + e]; bsh[e] = ep.bn_shift[co + e]; }
        }
    }
    // sums of du = dz * act'(y*s + b) and du*y over 8 channels of one pixel; the activation kind is resolved by ONE uniform
    // branch per call (it used to be a scalar compare-and-branch chain per element: ~25 instructions each)
    auto bn_bwd_sums = [&](const float (&dz8)[8], const float (&y8)[8]) {
        auto body = [&](auto act_tag) {
            constexpr int BACT = decltype(act_tag)::value;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float u = y8[e] * bsc[e] + bsh[e];
                float gact = 1.f;
                if constexpr (BACT == ACT_SILU) { const float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-u)); gact = sg * (1.0f + u * (1.0f - sg)); }
                else if constexpr (BACT == ACT_RELU) gact = u > 0.f ? 1.f : 0.f;
                const float du = dz8[e] * gact;
                bs1[e] += du;
                bs2[e] += du * y8[e];
            }
        };
        if (ep.bn_act == ACT_SILU) body(std::integral_constant<int, ACT_SILU>{});
        else if (ep.bn_act == ACT_RELU) body(std::integral_constant<int, ACT_RELU>{});
        else body(std::integral_constant<int, ACT_NONE>{});
    };
    // The epilogue's global READS (residual | accumulate, the producer's y for the BN-backward sums) of a slab round are issued at the
    // TOP of the round, all its iterations at once, and consumed after the slab phase: read inside the store loop, each of them was
    // a load followed by its own s_waitcnt -- 4-16 exposed memory latencies per wave tile (seen in the ISA of the first persistent
    // 1x1 kernel; the same code made the 3x3 dgrads 35 us slower when they carried the BN-backward sums, and every eval-mode
    // Bottleneck.cv2 pays it for its shortcut).  One round ahead would hide them completely but costs 64 VGPRs, and even these 32
    // make the register-bound kernels spill (the 256x256 tiles: 190-380 spill instructions, the four-workgroup short-K tile: 46):
    // those pass EPF = false and keep the load in the store loop.
    constexpr int NIT = SROWS / RPI;
    constexpr bool PF = EPF && sizeof(T) == 2 && MODE == 0;
    const bool pf_on = PF && !lean && (ep_res != nullptr || ep_accumulate || bnb);
    const bool pf_a_is_res = ep_res != nullptr;                  // the A buffer holds the residual, else the old output (accumulate)
    u32x4 pf_a[NIT], pf_b[NIT];
    auto pix_of = [&](int p) -> long long {
        if (ident) return p;
        const uint32_t t1 = fdiv((uint32_t)p, g.dQW), qx = p - t1 * g.QW;
        const uint32_t n = fdiv(t1, g.dQH), qy = t1 - n * g.QH;
        return ((long long)n * g.OH + (qy * g.osy + g.ooy)) * g.OW + (qx * g.osx + g.oox);
    };
#pragma unroll
    for (int tmh = 0; tmh < TM * NH; ++tmh) {
        const int tm = tmh / NH, hoff = (tmh % NH) * SROWS;      // accumulator tile, first tile row of this slab round
        if constexpr (PF) {
            if (pf_on) {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int p = m0 + wm * (BM / WM) + tm * 32 + hoff + it * RPI + srow;
                    if (p < g.M && co + 8 <= g.Cout) {
                        const long long pix = pix_of(p);
                        if (pf_a_is_res) pf_a[it] = *(const u32x4*)((const T*)ep_res + pix * ep.ldr + co);
                        else if (ep_accumulate) pf_a[it] = *(const u32x4*)(Y + pix * g.ldy + co);
                        if (bnb) pf_b[it] = *(const u32x4*)((const T*)ep.bn_y + pix * ep.ld_bn + co);
                    }
                }
            }
        }
#pragma unroll
        for (int rr = 0; rr < 16 / NH; ++rr) {
            const int r = (tmh % NH) * (16 / NH) + rr;
            const int row = (rr & 3) + 8 * (rr >> 2) + 4 * hi;   // row inside the slab (accumulator register r <-> tile row hoff + row)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                float v = acc[tm][tn][r];
                ssum[tn] += v;
                ssq[tn] += v * v;
                v = v * csc[tn] + cbi[tn];
                if constexpr (ACT == ACT_SILU) v = v * __builtin_amdgcn_rcpf(1.0f + __expf(-v));
                else if constexpr (ACT == ACT_RELU) v = fmaxf(v, 0.f);
                stg[row * SLD + tn * 32 + l31] = v;
            }
        }
        // the slab is private to this wave: LDS executes a wave's operations in order; the wait + wave barrier
        // only keep the compiler (and the CPU emulator's per-lane fibers) from reordering across it
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        if constexpr (sizeof(T) == 2) {
            if (lean) {
                // interior tile of a plain bf16 layer (no residual / accumulate / BN-backward sums, identity pixel map): the store
                // pass without a single guard or branch, so that the compiler can overlap the slab reads of the four iterations
#pragma unroll
                for (int it = 0; it < SROWS / RPI; ++it) {
                    const int row = it * RPI + srow;
                    const long long p = m0 + wm * (BM / WM) + tm * 32 + hoff + row;
                    const float4 a = *(const float4*)(stg + row * SLD + scv * 8);
                    const float4 b = *(const float4*)(stg + row * SLD + scv * 8 + 4);
                    *(u32x4*)(Y + p * g.ldy + co) = mk4(et_lp<T>::pack(a.x, a.y), et_lp<T>::pack(a.z, a.w), et_lp<T>::pack(b.x, b.y), et_lp<T>::pack(b.z, b.w));
                }
                __builtin_amdgcn_s_waitcnt(0xC07F);
                __builtin_amdgcn_wave_barrier();
                continue;
            }
        }
#pragma unroll
        for (int it = 0; it < SROWS / RPI; ++it) {
            const int row = it * RPI + srow;
            const int p = m0 + wm * (BM / WM) + tm * 32 + hoff + row;
            if (p < g.M && co < g.Cout) {
                const long long pix = pix_of(p);
                float v[8];
                const float4 a = *(const float4*)(stg + row * SLD + scv * 8);
                const float4 b = *(const float4*)(stg + row * SLD + scv * 8 + 4);
                v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
                T* yp = Y + pix * g.ldy + co;
                if (co + 8 <= g.Cout) {
                    if constexpr (sizeof(T) == 2) {
                        if (ep_res) {
                            u32x4 rr;
                            if constexpr (PF) rr = pf_a[it];
                            else rr = *(const u32x4*)((const T*)ep_res + pix * ep.ldr + co);
                            v[0] += et_lp<T>::lo(rr.x); v[1] += et_lp<T>::hi(rr.x);
                            v[2] += et_lp<T>::lo(rr.y); v[3] += et_lp<T>::hi(rr.y);
                            v[4] += et_lp<T>::lo(rr.z); v[5] += et_lp<T>::hi(rr.z);
                            v[6] += et_lp<T>::lo(rr.w); v[7] += et_lp<T>::hi(rr.w);
                        }
                        if (ep_accumulate) {
                            u32x4 rr;
                            if (PF && !pf_a_is_res) rr = pf_a[it];       // (with a residual as well, the A buffer is taken: load here)
                            else rr = *(const u32x4*)yp;
                            v[0] += et_lp<T>::lo(rr.x); v[1] += et_lp<T>::hi(rr.x);
                            v[2] += et_lp<T>::lo(rr.y); v[3] += et_lp<T>::hi(rr.y);
                            v[4] += et_lp<T>::lo(rr.z); v[5] += et_lp<T>::hi(rr.z);
                            v[6] += et_lp<T>::lo(rr.w); v[7] += et_lp<T>::hi(rr.w);
                        }
                        const u32x4 packed = mk4(et_lp<T>::pack(v[0], v[1]), et_lp<T>::pack(v[2], v[3]), et_lp<T>::pack(v[4], v[5]),
                                                 et_lp<T>::pack(v[6], v[7]));
                        *(u32x4*)yp = packed;
                        if (bnb) {
                            // statistics of exactly what the apply pass will read back: the bf16-ROUNDED dz
                            u32x4 yy;
                            if constexpr (PF) yy = pf_b[it];
                            else yy = *(const u32x4*)((const T*)ep.bn_y + pix * ep.ld_bn + co);
                            const unsigned pw[4] = {packed.x, packed.y, packed.z, packed.w}, yw[4] = {yy.x, yy.y, yy.z, yy.w};
                            float dz8[8], y8[8];
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                dz8[e] = (e & 1) ? et_lp<T>::hi(pw[e >> 1]) : et_lp<T>::lo(pw[e >> 1]);
                                y8[e] = (e & 1) ? et_lp<T>::hi(yw[e >> 1]) : et_lp<T>::lo(yw[e >> 1]);
                            }
                            bn_bwd_sums(dz8, y8);
                        }
                    } else {
                        if (ep_res) {
                            const float* rp = (const float*)ep_res + pix * ep.ldr + co;
                            const float4 r0 = *(const float4*)rp, r1 = *(const float4*)(rp + 4);
                            v[0] += r0.x; v[1] += r0.y; v[2] += r0.z; v[3] += r0.w; v[4] += r1.x; v[5] += r1.y; v[6] += r1.z; v[7] += r1.w;
                        }
                        if (ep_accumulate) {
                            const float4 r0 = *(const float4*)yp, r1 = *(const float4*)((const float*)yp + 4);
                            v[0] += r0.x; v[1] += r0.y; v[2] += r0.z; v[3] += r0.w; v[4] += r1.x; v[5] += r1.y; v[6] += r1.z; v[7] += r1.w;
                        }
                        *(float4*)yp = make_float4(v[0], v[1], v[2], v[3]);
                        *(float4*)((float*)yp + 4) = make_float4(v[4], v[5], v[6], v[7]);
                        if (bnb) {
                            const float* bp = (const float*)ep.bn_y + pix * ep.ld_bn + co;
                            const float4 y0 = *(const float4*)bp, y1 = *(const float4*)(bp + 4);
                            const float yv8[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
                            bn_bwd_sums(v, yv8);
                        }
                    }
                } else {
                    for (int e = 0; e < 8 && co + e < g.Cout; ++e) {
                        float x = v[e];
                        if (ep_res) x += et_elem<T>::ld(((const T*)ep_res)[pix * ep.ldr + co + e]);
                        if (ep_accumulate) x += et_elem<T>::ld(yp[e]);
                        yp[e] = et_elem<T>::st(x);
                    }
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);        // slab reads done before the next 32 rows overwrite it
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (!DEFER) {
        if (ep.stats) {
            // Partial statistics, one row of the (rows, 2, Cout) buffer per 64 output rows (et_conv2d_stats_rows).  Every wave writes
            // the sums of ITS rows and channels straight to global memory -- no LDS hop, no workgroup barrier: the barrier made every
            // wave of the tile wait for the slowest one's store passes (measured with s_memtime stamps, profiles/r03_epilogue_stamps.txt:
            // 1.0 k of the 10.1 k cycles of a short-K 1x1 tile, 3.6 k of the 130 k of a 256x256 3x3 tile).  A wave whose tile part is
            // taller than 64 rows writes its sums into its first row and zeros the others it covers; rows beyond M were zero-filled
            // operands, so they add nothing.
            constexpr int RPW = (BM / WM) / 64;                      // 64-row blocks per wave
            static_assert((BM / WM) % 64 == 0, "wave tiles are whole 64-row blocks");
            // sharded accumulator: one addition per channel and WORKGROUP (the wave rows meet in LDS behind the store passes)
            if (ep.stats_ld) conv_stats_add_sharded_wg<BN, WN, WM, MODE>(st, g, ep, tid, lane, wm, wn, (float*)lds_raw, n0);
            else conv_epilogue_write_stats<BN, WN, MODE>(st, g, ep, n0, lane, wn, (m0 + wm * (BM / WM)) / 64, RPW - 1, (g.M + 63) / 64);
        }
    }
}

template <typename T, int BM, int BN, int WM, int WN, int SROWS = 32, int MODE = 0, bool DEFER = false, bool EPF = true>
__device__ __forceinline__ void conv_epilogue(f32x16 (&acc)[BM / WM / 32][BN / WN / 32], u32x4* lds_raw, T* __restrict__ Y,
                                              const GatherGeom& g, const Epilogue& ep, int bx, int m0, int n0, int tid,
                                              int lane, int wm, int wn, EpiSums<BN / WN / 32>& st) {
    // one uniform branch per workgroup instead of one per element
    if (ep.act == ACT_SILU) conv_epilogue_act<T, BM, BN, WM, WN, ACT_SILU, SROWS, MODE, DEFER, EPF>(acc, lds_raw, Y, g, ep, bx, m0, n0, tid, lane, wm, wn, st);
    else if (ep.act == ACT_RELU) conv_epilogue_act<T, BM, BN, WM, WN, ACT_RELU, SROWS, MODE, DEFER, EPF>(acc, lds_raw, Y, g, ep, bx, m0, n0, tid, lane, wm, wn, st);
    else conv_epilogue_act<T, BM, BN, WM, WN, ACT_NONE, SROWS, MODE, DEFER, EPF>(acc, lds_raw, Y, g, ep, bx, m0, n0, tid, lane, wm, wn, st);
}
// the tiled kernels: one tile per workgroup, statistics written by the epilogue itself.  EPF: see conv_epilogue_act (register headroom)
template <typename T, int BM, int BN, int WM, int WN, bool EPF = true>
__device__ __forceinline__ void conv_epilogue(f32x16 (&acc)[BM / WM / 32][BN / WN / 32], u32x4* lds_raw, T* __restrict__ Y,
                                              const GatherGeom& g, const Epilogue& ep, int bx, int m0, int n0, int tid,
                                              int lane, int wm, int wn) {
    EpiSums<BN / WN / 32> st;
    st.clear();
    conv_epilogue<T, BM, BN, WM, WN, 32, 0, false, EPF>(acc, lds_raw, Y, g, ep, bx, m0, n0, tid, lane, wm, wn, st);
}

// ---- forward / dgrad gather-GEMM ----------------------------------------------------------------
template <typename T, int BM, int BN, int WM, int WN, int BKV, bool UTAP>
__global__ __launch_bounds__(256) void conv_gemm_kernel(const T* __restrict__ X, const T* __restrict__ W,
                                                        T* __restrict__ Y, GatherGeom g, Epilogue ep) {
    constexpr int VEC = et_elem<T>::VEC;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int RPT = 256 / BKV;                 // rows covered by one pass of the 256 loader threads
    constexpr int RA = BM / RPT, RB = BN / RPT;    // 16-byte vectors per thread per chunk
    constexpr int STAGE_VEC = (BM + BN) * BKV;                       // one K-chunk of A and B
    constexpr int EPI_VEC = EpiLds<BM, BN, WM, WN>::VEC16;
    constexpr int LDS_VEC = 2 * STAGE_VEC > EPI_VEC ? 2 * STAGE_VEC : EPI_VEC;
    __shared__ __attribute__((aligned(16))) u32x4 lds_raw[LDS_VEC];
    u32x4* const lds0 = lds_raw;
    u32x4* const lds1 = lds_raw + STAGE_VEC;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    // Workgroups are dealt round-robin to the 8 XCDs (private L2 each).  With xcd_swz the pixel-tile index
    // is remapped so that each XCD owns a contiguous range of tiles: the halo rows shared by neighbouring
    // tiles of a 3x3 conv, and the weights, are then re-read from that XCD's L2 (placement only: results
    // do not depend on it).
    int bx, by;
    tile_of_block(g, bx, by);
    const int m0 = bx * BM, n0 = by * BN;
    const int lvec = tid % BKV, lrow = tid / BKV;

    // loader state: A rows are lattice pixels, B rows are output channels
    int a_off[RA], a_iy[RA], a_ix[RA];
    bool a_ok[RA];
#pragma unroll
    for (int j = 0; j < RA; ++j) {
        const int p = m0 + lrow + j * RPT;
        a_ok[j] = p < g.M;
        const uint32_t pp = a_ok[j] ? p : 0;
        const uint32_t t1 = fdiv(pp, g.dQW), qx = pp - t1 * g.QW;
        const uint32_t n = fdiv(t1, g.dQH), qy = t1 - n * g.QH;
        a_iy[j] = qy * g.isy;
        a_ix[j] = qx * g.isx;
        a_off[j] = ((n * g.IH + a_iy[j]) * g.IW + a_ix[j]) * g.ldx;
    }
    int b_off[RB];
    bool b_ok[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int co = n0 + lrow + j * RPT;
        b_ok[j] = co < g.Cout;
        b_off[j] = (b_ok[j] ? co : 0) * g.TT * g.Cin;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    const int nchunks = (g.KV + BKV - 1) / BKV;
    // Software pipeline, prefetch distance 2: two register sets (A/B) hold the K-chunks c+1 and c+2 while
    // chunk c is multiplied out of LDS.  A chunk's global loads are issued TWO MFMA phases (plus the
    // barrier) before its LDS store, which is what covers HBM latency at 2 workgroups per CU; with
    // distance 1 the kernel was latency-bound (~22 % MFMA utilisation on the 3x3 layers).
    // Loads are UNCONDITIONAL (an out-of-image / out-of-range lane reads the tensor base); the zero-fill
    // select happens at LDS-store time, AFTER the MFMAs, so nothing waits on a load early.
    u32x4 raA[RA], rbA[RB], raB[RA], rbB[RB];
    unsigned okA = 0u, okB = 0u;
    int tap_u = 0, cv_u = 0;   // UTAP: chunk-uniform tap / channel-vector cursor of the NEXT chunk to load

    auto gload = [&](int chunk, int tap_c, int cv_c, u32x4 (&ra)[RA], u32x4 (&rb)[RB]) -> unsigned {
        int tap, cv;
        bool kok = true;
        if constexpr (UTAP) {
            tap = tap_c; cv = cv_c + lvec;
        } else {
            const uint32_t kv = chunk * BKV + lvec;
            kok = kv < (uint32_t)g.KV;
            const uint32_t kk = kok ? kv : 0;
            tap = fdiv(kk, g.dCV); cv = kk - tap * g.CV;
        }
        int dy, dx, wt;
        if constexpr (UTAP) tap_lookup_uniform(g, tap, dy, dx, wt);
        else { dy = g.dy[tap]; dx = g.dx[tap]; wt = g.wt[tap]; }
        const int doff = (dy * g.IW + dx) * g.ldx + cv * VEC;
        const int woff = wt * g.Cin + cv * VEC;
        unsigned okmask = 0u;
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const bool ok = kok && a_ok[j] && (unsigned)(a_iy[j] + dy) < (unsigned)g.IH &&
                            (unsigned)(a_ix[j] + dx) < (unsigned)g.IW;
            ra[j] = *(const u32x4*)(X + (ok ? a_off[j] + doff : 0));
            okmask |= ok ? (1u << j) : 0u;
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            const bool ok = kok && b_ok[j];
            rb[j] = *(const u32x4*)(W + (ok ? b_off[j] + woff : 0));
            okmask |= ok ? (1u << (16 + j)) : 0u;
        }
        return okmask;
    };
#define ET_ADVANCE_CURSOR()                                              \
    if constexpr (UTAP) {                                                \
        if (g.tap_inner) {                                               \
            if (++tap_u >= g.T) { tap_u = 0; cv_u += BKV; }              \
        } else {                                                         \
            cv_u += BKV;                                                 \
            if (cv_u >= g.CV) { cv_u = 0; ++tap_u; }                     \
        }                                                                \
    }
    auto lstore = [&](u32x4* __restrict__ dst, const u32x4 (&ra)[RA], const u32x4 (&rb)[RB], unsigned okmask) {
        const u32x4 zero = mk4(0, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const int r = lrow + j * RPT;
            dst[r * BKV + (lvec ^ lds_swz<BKV>(r))] = ((okmask >> j) & 1u) ? ra[j] : zero;
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            const int r = lrow + j * RPT;
            dst[(BM + r) * BKV + (lvec ^ lds_swz<BKV>(r))] = ((okmask >> (16 + j)) & 1u) ? rb[j] : zero;
        }
    };

    okA = gload(0, tap_u, cv_u, raA, rbA);
    ET_ADVANCE_CURSOR();
    if (nchunks > 1) { okB = gload(1, tap_u, cv_u, raB, rbB); ET_ADVANCE_CURSOR(); }
    lstore(lds0, raA, rbA, okA);
    __syncthreads();
    // invariant at the top of an even phase c: LDS0 = chunk c, set B = chunk c+1 (in flight / landed)
    for (int c = 0; c < nchunks; c += 2) {
        if (c + 2 < nchunks) { okA = gload(c + 2, tap_u, cv_u, raA, rbA); ET_ADVANCE_CURSOR(); }
        mma_chunk<T, BM, BN, WM, WN, BKV>(lds0, acc, wm, wn, lane);
        __builtin_amdgcn_sched_barrier(0);     // keep the consumers of the prefetched vectors below the MFMAs
        if (c + 1 < nchunks) lstore(lds1, raB, rbB, okB);
        __syncthreads();
        if (c + 1 < nchunks) {
            if (c + 3 < nchunks) { okB = gload(c + 3, tap_u, cv_u, raB, rbB); ET_ADVANCE_CURSOR(); }
            mma_chunk<T, BM, BN, WM, WN, BKV>(lds1, acc, wm, wn, lane);
            __builtin_amdgcn_sched_barrier(0);
            if (c + 2 < nchunks) lstore(lds0, raA, rbA, okA);
            __syncthreads();
        }
    }

#undef ET_ADVANCE_CURSOR
    conv_epilogue<T, BM, BN, WM, WN, false>(acc, lds_raw, Y, g, ep, bx, m0, n0, tid, lane, wm, wn);
}

// ---- forward / dgrad gather-GEMM, LDS-DMA staging ------------------------------------------------------
// Same tiling, LDS image and epilogue as conv_gemm_kernel, but the K-chunks go global -> LDS with
// global_load_lds_dwordx4 (no VGPR staging, no ds_write_b128: on the register-staged kernel the 8
// ds_write_b128 per lane per chunk cost about as many LDS cycles as all the fragment reads).
// The DMA writes LDS lane-linearly (wave base + lane*16), i.e. lane (row = t/BKV, slot = t%BKV) always
// fills physical slot `slot` of its row; the XOR swizzle is therefore applied to the SOURCE: the lane
// fetches the logical K-vector  slot ^ swz(row)  (same 128-byte global segment, so coalescing is
// unchanged) and the fragment reads keep using  physical = logical ^ swz(row).  Out-of-image taps, rows
// beyond M and channels beyond Cout fetch from a 16-byte zero page instead of branching.
// (the counted waits -- s_waitcnt vmcnt(N): at most N of this wave's LDS-DMA loads still in flight -- are et_device.h's)

// NS = depth of the LDS ring of K-chunks.  Chunk c+NS-1 is issued while chunk c is being multiplied, so up to
// NS-1 chunks per workgroup are in flight all the time.  What bounds this kernel is bytes in flight per CU
// over the loaded L2/fabric latency (measured: ~10 TB/s of L2->LDS traffic with 2 x 32 KB bursts per CU,
// MFMA busy ~30 %), not LDS or MFMA issue -- hence deeper rings and, where the layer has the rows, a
// 256-row tile (1.33x the flops per staged byte).
template <typename T, int BM, int BN, int WM, int WN, int BKV, int NS, bool UTAP>
__global__ __launch_bounds__(64 * WM * WN, (NS == 3 && BKV == 4 && BM == 128) ? (BN == 64 ? ET_GLDS_SHORTK_WGS : 3) : 1) void conv_gemm_glds_kernel(const T* __restrict__ X, const T* __restrict__ W,
                                                             T* __restrict__ Y, const T* __restrict__ ZERO,
                                                             GatherGeom g, Epilogue ep) {
    constexpr int VEC = et_elem<T>::VEC;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int NT = 64 * WM * WN;             // 4 waves (2x2) or 8 waves (2x4) per workgroup
    constexpr int RPT = NT / BKV;
    constexpr int RA = BM / RPT, RB = BN / RPT;
    constexpr int STAGE_VEC = (BM + BN) * BKV;
    constexpr int EPI_VEC = EpiLds<BM, BN, WM, WN>::VEC16;
    constexpr int LDS_VEC = NS * STAGE_VEC > EPI_VEC ? NS * STAGE_VEC : EPI_VEC;
    constexpr int PER = RA + RB;                 // LDS-DMA instructions per thread per chunk
    static_assert(NS >= 2 && NS <= 5 && (NS - 2) * PER < 64, "ring depth");
    __shared__ __attribute__((aligned(16))) u32x4 lds_raw[LDS_VEC];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    int bx, by;
    tile_of_block(g, bx, by);
    const int m0 = bx * BM, n0 = by * BN;
    const int lvec = tid % BKV, lrow = tid / BKV;

    int a_off[RA], a_iy[RA], a_ix[RA], a_lv[RA];
    bool a_ok[RA];
#pragma unroll
    for (int j = 0; j < RA; ++j) {
        const int rl = lrow + j * RPT;
        const int p = m0 + rl;
        a_ok[j] = p < g.M;
        const uint32_t pp = a_ok[j] ? p : 0;
        const uint32_t t1 = fdiv(pp, g.dQW), qx = pp - t1 * g.QW;
        const uint32_t n = fdiv(t1, g.dQH), qy = t1 - n * g.QH;
        a_iy[j] = qy * g.isy;
        a_ix[j] = qx * g.isx;
        a_off[j] = ((n * g.IH + a_iy[j]) * g.IW + a_ix[j]) * g.ldx;
        a_lv[j] = lvec ^ lds_swz<BKV>(rl);                 // logical K-vector this lane stages for row rl
    }
    int b_off[RB], b_lv[RB];
    bool b_ok[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int rl = lrow + j * RPT;
        const int co = n0 + rl;
        b_ok[j] = co < g.Cout;
        b_off[j] = (b_ok[j] ? co : 0) * g.TT * g.Cin;
        b_lv[j] = lvec ^ lds_swz<BKV>(rl);
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    const int nchunks = (g.KV + BKV - 1) / BKV;
    int tap_u = 0, cv_u = 0;

    // issue the LDS-DMA of one K-chunk into `dst` (all NT threads, RA + RB instructions each)
    // pieces [q0, q1) of the chunk's PER = RA + RB LDS-DMA instructions per thread (A rows first)
    auto stage_range = [&](u32x4* dst, int chunk, int tap_c, int cv_c, int q0, int q1) {
        u32x4* const wbase = dst + wave * 64;              // wave-uniform: lanes land at wbase[j*NT + lane]
        int udy = 0, udx = 0, uwt = 0;
        if constexpr (UTAP) tap_lookup_uniform(g, tap_c, udy, udx, uwt);   // once per chunk, before the burst
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            if (j < q0 || j >= q1) continue;
            int dy = udy, dx = udx, cv;
            bool kok = true;
            if constexpr (UTAP) {
                cv = cv_c + a_lv[j];
            } else {
                const uint32_t kv = chunk * BKV + a_lv[j];
                kok = kv < (uint32_t)g.KV;
                const uint32_t kk = kok ? kv : 0;
                const int tap = fdiv(kk, g.dCV);
                cv = kk - tap * g.CV;
                dy = g.dy[tap]; dx = g.dx[tap];
            }
            const bool ok = kok && a_ok[j] && (unsigned)(a_iy[j] + dy) < (unsigned)g.IH &&
                            (unsigned)(a_ix[j] + dx) < (unsigned)g.IW;
            const T* src = ok ? X + (a_off[j] + (dy * g.IW + dx) * g.ldx + cv * VEC) : ZERO;
            et_glds16(src, wbase + j * NT);
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            if (RA + j < q0 || RA + j >= q1) continue;
            int wt = uwt, cv;
            bool kok = true;
            if constexpr (UTAP) {
                cv = cv_c + b_lv[j];
            } else {
                const uint32_t kv = chunk * BKV + b_lv[j];
                kok = kv < (uint32_t)g.KV;
                const uint32_t kk = kok ? kv : 0;
                const int tap = fdiv(kk, g.dCV);
                cv = kk - tap * g.CV;
                wt = g.wt[tap];
            }
            const bool ok = kok && b_ok[j];
            const T* src = ok ? W + (b_off[j] + wt * g.Cin + cv * VEC) : ZERO;
            et_glds16(src, wbase + BM * BKV + j * NT);
        }
    };
    auto stage = [&](u32x4* dst, int chunk, int tap_c, int cv_c) { stage_range(dst, chunk, tap_c, cv_c, 0, PER); };
#define ET_ADVANCE_CURSOR()                                              \
    if constexpr (UTAP) {                                                \
        if (g.tap_inner) {                                               \
            if (++tap_u >= g.T) { tap_u = 0; cv_u += BKV; }              \
        } else {                                                         \
            cv_u += BKV;                                                 \
            if (cv_u >= g.CV) { cv_u = 0; ++tap_u; }                     \
        }                                                                \
    }

    // prologue: chunks 0 .. NS-2
#pragma unroll
    for (int s = 0; s < NS - 1; ++s)
        if (s < nchunks) { stage(lds_raw + s * STAGE_VEC, s, tap_u, cv_u); ET_ADVANCE_CURSOR(); }
    int rd = 0, wr = NS - 1;                       // ring slots of chunk c and of chunk c+NS-1
    for (int c = 0; c < nchunks; ++c) {
        // chunk c has landed once at most `ahead` younger chunks of this wave are still in flight
        const int ahead = min(NS - 2, nchunks - 1 - c);
        // (and lgkmcnt(0): this wave's reads of slot `wr` have COMPLETED, not merely been issued -- et_device.h)
        if constexpr (!UTAP) {
            et_wait_vmem_lds_read_done();          // table loads share vmcnt on this path: no partial waits
        } else {
            if (NS >= 5 && ahead == 3) et_wait_vmem_le_lds_read_done<(NS >= 5 ? 3 : 0) * PER>();
            else if (NS >= 4 && ahead == 2) et_wait_vmem_le_lds_read_done<(NS >= 4 ? 2 : 0) * PER>();
            else if (NS >= 3 && ahead == 1) et_wait_vmem_le_lds_read_done<(NS >= 3 ? 1 : 0) * PER>();
            else et_wait_vmem_lds_read_done();
        }
        // ... for every wave; and all reads of slot `wr` (chunk c-1) are done.  With younger chunks in flight the
        // barrier must be the bare s_barrier: __syncthreads() carries a fence that waits vmcnt(0), i.e. drains
        // the very LDS-DMA the ring keeps in flight
        if constexpr (NS > 2) __builtin_amdgcn_s_barrier(); else __syncthreads();
        if (c + NS - 1 < nchunks) { stage(lds_raw + wr * STAGE_VEC, c + NS - 1, tap_u, cv_u); ET_ADVANCE_CURSOR(); }
        mma_chunk<T, BM, BN, WM, WN, BKV>(lds_raw + rd * STAGE_VEC, acc, wm, wn, lane);
        rd = rd + 1 == NS ? 0 : rd + 1;
        wr = wr + 1 == NS ? 0 : wr + 1;
    }
    __syncthreads();                               // the epilogue reuses the ring as its staging area
#undef ET_ADVANCE_CURSOR
    // (EPF = false: the epilogue's read prefetch costs this kernel a resident workgroup -- 168 -> 194 VGPRs on the 128x128 tile)
    conv_epilogue<T, BM, BN, WM, WN, false>(acc, lds_raw, Y, g, ep, bx, m0, n0, tid, lane, wm, wn);
}

// ---- 3x3 stride-1 gather-GEMM with the activation rows shared by the three taps of a kernel row ("row shift") --------------
// conv_gemm_glds_kernel stages the activation operand once per TAP: nine times per 64-channel chunk, although the three taps
// of one kernel row (dx = -1, 0, +1 at the same dy) read the SAME pixels shifted by one raster position.  Here one unit =
// (channel chunk, kernel row) stages the tile's pixels ONCE, in a PADDED raster: LDS row index = Yg * (W + 1) + x (Yg = image
// row counted through the batch), i.e. one extra slot after every image row, staged from the zero page.  The three steps of the
// unit (dx) read their A fragments from LDS rows rr + (0 | 1 | 2), rr = this lane's padded row: x - 1 of a row's first pixel
// and x + 1 of its last one land on a pad slot, rows beyond M on zero-page rows -- no masks, no branches (a first version ANDed
// the fragments of row-end pixels with zero in registers: +18 % on the whole kernel, profiles/r03_row_shift_ablation.txt).
// Only the weight tile is staged per step: (BM + 16) + 3 * BN instead of 3 * (BM + BN) rows per unit of L2->LDS traffic.
// Ring: two A-unit slots + two B-step slots; B(s+1) is issued at the start of step s, A(u+1) at the first step of unit u, BEHIND
// that step's B so that the counted vmcnt wait of the next step releases B while A is still in flight.
// BUF (r06, the default form): LDS-DMA through buffer descriptors as in conv_gemm_pprs_kernel (its header): out-of-range lanes land as
// zeros, the kernel-row step and the channel cursor travel in the SGPR offset.  One barrier per step hands the B slot the previous
// step read back to the DMA: the wait in front of it includes lgkmcnt(0) (et_device.h et_wait_vmem_le_lds_read_done -- the race this
// kernel's buffer form exposed).
template <typename T, int BM, int BN, int WM, int WN, bool BUF>
__device__ __forceinline__ void conv_gemm_rs_body(const T* __restrict__ X, const T* __restrict__ W, T* __restrict__ Y,
                                                  const T* __restrict__ ZERO, const GatherGeom& g, const Epilogue& ep) {
    constexpr int VEC = 8, BKV = 8;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int NW = WM * WN, NT = 64 * NW;
    constexpr int RPT = NT / BKV;                        // rows per full staging pass (8 per wave)
    constexpr int CAP = RS_A_ROWS(BM);                   // LDS rows of an A unit: BM + 2 + pad slots (host: rs_eligible)
    constexpr int RAF = CAP / RPT;                       // full passes ...
    constexpr int XW = (CAP - RAF * RPT) / 8;            // ... and one more for the first XW waves
    constexpr int RA = RAF + (XW ? 1 : 0);
    constexpr int RB = BN / RPT;
    constexpr int A_VEC = CAP * BKV, B_VEC = BN * BKV;
    constexpr int RING_VEC = 2 * A_VEC + 2 * B_VEC;
    constexpr int EPI_VEC = EpiLds<BM, BN, WM, WN>::VEC16;
    constexpr int LDS_VEC = RING_VEC > EPI_VEC ? RING_VEC : EPI_VEC;
    static_assert(CAP % 8 == 0 && RA < 16 && XW < NW, "A unit = whole wave instructions; vmcnt immediate");
    __shared__ __attribute__((aligned(16))) u32x4 lds_raw[LDS_VEC];
    u32x4* const slotA = lds_raw;                        // [2][A_VEC]
    u32x4* const slotB = lds_raw + 2 * A_VEC;            // [2][B_VEC]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    int bx, by;
    tile_of_block(g, bx, by);
    const int m0 = bx * BM, n0 = by * BN;
    const int lvec = tid % BKV, lrow = tid / BKV;
    const int W1 = g.QW + 1;
    // padded index of the tile's first pixel; LDS row rho <-> padded index P0 - 1 + rho
    const uint32_t yg0 = fdiv((uint32_t)m0, g.dQW);
    const int P0 = (int)(yg0 * W1 + ((uint32_t)m0 - yg0 * g.QW));

    int a_off[RA], a_iy[RA], a_lv[RA];
    bool a_ok[RA];
#pragma unroll
    for (int q = 0; q < RA; ++q) {
        const int rho = lrow + q * RPT;
        const int P = P0 - 1 + rho;
        const uint32_t Pp = P < 0 ? 0 : P;
        const uint32_t yg = fdiv(Pp, g.dW1), xp = Pp - yg * W1;
        const uint32_t pix = yg * g.QW + xp;
        a_ok[q] = rho < CAP && P >= 0 && (int)xp < g.QW && pix < (uint32_t)g.M;
        const uint32_t ygc = a_ok[q] ? yg : 0;
        a_iy[q] = ygc - fdiv(ygc, g.dQH) * g.QH;        // image row
        a_off[q] = (a_ok[q] ? pix : 0) * g.ldx;
        a_lv[q] = lvec ^ lds_swz<BKV>(rho);
    }
    // BUF: byte offsets behind the descriptor bases (X: one image row in front of the tensor) and, per piece, which of the three kernel
    // rows leave the image (bit 3q + 1 + dy); a pixel that does not exist carries bit 31 for good
    const int rowstep = g.IW * g.ldx;
    unsigned a_nokm = 0u;
    et_rsrc rsX, rsW;
    if constexpr (BUF) {
        rsX = et_make_rsrc((const char*)X - (size_t)rowstep * sizeof(T), (unsigned)(((size_t)g.N * g.IH * g.IW * g.ldx + rowstep) * sizeof(T)));
        rsW = et_make_rsrc(W, (unsigned)((size_t)g.Cout * g.TT * g.Cin * sizeof(T)));
#pragma unroll
        for (int q = 0; q < RA; ++q) {
            a_nokm |= ((a_iy[q] > 0 ? 0u : 1u) | (a_iy[q] + 1 < g.IH ? 0u : 4u)) << (3 * q);
            a_off[q] = a_ok[q] ? (int)((a_off[q] + a_lv[q] * VEC) * (int)sizeof(T)) : (int)0x80000000;
        }
    }
    int b_off[RB], b_lv[RB];
    bool b_ok[RB];
#pragma unroll
    for (int q = 0; q < RB; ++q) {
        const int rl = lrow + q * RPT;
        const int co = n0 + rl;
        b_ok[q] = co < g.Cout;
        b_off[q] = (b_ok[q] ? co : 0) * g.TT * g.Cin;
        b_lv[q] = lvec ^ lds_swz<BKV>(rl);
        // BUF: the UNCLAMPED row -- a row beyond Cout lies beyond the weight descriptor's range and lands as zeros
        if constexpr (BUF) b_off[q] = (int)((co * g.TT * g.Cin + b_lv[q] * VEC) * (int)sizeof(T));
    }
    // byte offset (inside an A unit) of this lane's k-step-0 fragment of row tile tm at step shift s; a k-step XORs bits 5-6 of it
    // (the swizzle is an XOR on the K-vector slot): one v_xor per fragment read instead of a swizzle computation
    int abase[TM][3];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const uint32_t p = m0 + wm * (BM / WM) + tm * 32 + (lane & 31);
        const uint32_t yg = fdiv(p, g.dQW);
        const int r0 = (int)(yg * W1 + (p - yg * g.QW)) - P0;
#pragma unroll
        for (int sft = 0; sft < 3; ++sft) abase[tm][sft] = ((r0 + sft) * BKV + ((lane >> 5) ^ lds_swz<BKV>(r0 + sft))) * 16;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    // taps in kernel-row order (rs_eligible): tap = 3*j + k has dy = sgn*(j-1), dx = sgn*(k-1), weight slot tap; sgn = -1 for dgrad.
    // Arithmetic instead of the tap table: a scalar load in the loop waits lgkmcnt(0) in front of every burst.
    const int sgn = g.dy[0] < 0 ? 1 : -1;                // uniform (kernel argument)
    auto stage_a = [&](u32x4* dst, int j, int cv_c) {    // unit (channel chunk cv_c, kernel row j)
        u32x4* const wbase = dst + wave * 64;
        const int dy = sgn * (j - 1);
        const int roff = dy * g.IW * g.ldx + cv_c * VEC;
#pragma unroll
        for (int q = 0; q < RA; ++q) {
            if (q == RAF && wave >= XW) continue;        // wave-uniform: the short last pass
            if constexpr (BUF) {
                const unsigned bad = (a_nokm >> (3 * q + 1 + dy)) & 1u;
                et_bufdma16(rsX, (bad << 31) | (unsigned)a_off[q], (unsigned)(((dy + 1) * rowstep + cv_c * VEC) * (int)sizeof(T)), wbase + q * NT);
            } else {
                const bool ok = a_ok[q] && (unsigned)(a_iy[q] + dy) < (unsigned)g.IH;
                const T* src = ok ? X + (a_off[q] + roff + a_lv[q] * VEC) : ZERO;
                et_glds16(src, wbase + q * NT);
            }
        }
    };
    auto stage_b = [&](u32x4* dst, int tap, int cv_c) {
        u32x4* const wbase = dst + wave * 64;
        const int woff = tap * g.Cin + cv_c * VEC;
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            if constexpr (BUF) {
                et_bufdma16(rsW, (unsigned)b_off[q], (unsigned)(woff * (int)sizeof(T)), wbase + q * NT);
            } else {
                const T* src = b_ok[q] ? W + (b_off[q] + woff + b_lv[q] * VEC) : ZERO;
                et_glds16(src, wbase + q * NT);
            }
        }
    };
    // one step: TM x TN x 4 MFMAs, A fragments from the unit at row offset SFT
    auto mma_step = [&](const u32x4* __restrict__ sa, const u32x4* __restrict__ sb, auto shift_tag) {
        constexpr int SFT = decltype(shift_tag)::value;
        const int l31 = lane & 31, gh = lane >> 5;
        u32x4 af[2][TM], bf[2][TN];
        auto fetch = [&](int kk, int set) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) af[set][tm] = *(const u32x4*)((const char*)sa + (abase[tm][SFT] ^ (kk * 32)));
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int r = wn * (BN / WN) + tn * 32 + l31;
                bf[set][tn] = sb[r * BKV + ((kk * 2 + gh) ^ lds_swz<BKV>(r))];
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
                for (int tn = 0; tn < TN; ++tn)
                    acc[tm][tn] = et_mfma32<T>(af[cur][tm], bf[cur][tn], acc[tm][tn]);
        }
    };

    const int nunits = 3 * (g.CV / BKV);                 // (channel chunk outer, kernel row inner)
    // prologue: A(0) then B(0): both awaited together.  Step k of a unit reads the unit at row offset k (dx = k - 1); its weights
    // are tap 3j + k (forward) or 3j + 2 - k (dgrad: sgn < 0)
    stage_a(slotA, 0, 0);
    stage_b(slotB, sgn > 0 ? 0 : 2, 0);
    int j = 0, cv_u = 0, bs = 0;                         // kernel row and channel cursor of the unit; B slot of the current step
#pragma unroll 1
    for (int u = 0; u < nunits; ++u) {
        const bool more_units = u + 1 < nunits;
        int nj = j + 1, ncv = cv_u;                      // the next unit
        if (nj == 3) { nj = 0; ncv += BKV; }
        const u32x4* const sa = slotA + (u & 1) * A_VEC;
        auto step = [&](auto ktag) {
            constexpr int k = decltype(ktag)::value;
            // B(s) has landed (and A(u) at k == 0); at k == 1 the A unit issued behind B(s) may still be in flight
            // (and lgkmcnt(0): the previous step's reads of the B slot rewritten below have COMPLETED -- et_device.h)
            if (k == 1 && more_units) {
                if (wave < XW) et_wait_vmem_le_lds_read_done<RA>(); else et_wait_vmem_le_lds_read_done<RAF>();
            } else {
                et_wait_vmem_lds_read_done();
            }
            __builtin_amdgcn_s_barrier();                // ... for every wave; all reads of the slots rewritten below are done
            constexpr int kn = k < 2 ? k + 1 : 0;
            if (k < 2 || more_units) stage_b(slotB + (bs ^ 1) * B_VEC, (k < 2 ? j : nj) * 3 + (sgn > 0 ? kn : 2 - kn), k < 2 ? cv_u : ncv);
            if (k == 0 && more_units) stage_a(slotA + ((u + 1) & 1) * A_VEC, nj, ncv);
            mma_step(sa, slotB + bs * B_VEC, ktag);
            bs ^= 1;
        };
        step(std::integral_constant<int, 0>{});
        step(std::integral_constant<int, 1>{});
        step(std::integral_constant<int, 2>{});
        j = nj; cv_u = ncv;
    }
    __syncthreads();                                     // the epilogue reuses the ring as its staging area
    conv_epilogue<T, BM, BN, WM, WN>(acc, lds_raw, Y, g, ep, bx, m0, n0, tid, lane, wm, wn);
}
// conv_gemm_rs_kernel: the buffer-descriptor pieces (the default); conv_gemm_rs_flat_kernel: the same loops on flat 64-bit addresses, for
// an operand of 2^31 bytes or more (a voffset's bit 31 means "out of range") and for ET_CONV_BUF_DMA=0
template <typename T, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN, BN <= 64 ? 3 : 2) void conv_gemm_rs_kernel(const T* __restrict__ X, const T* __restrict__ W,
                                                                       T* __restrict__ Y, const T* __restrict__ ZERO,
                                                                       GatherGeom g, Epilogue ep) {
    conv_gemm_rs_body<T, BM, BN, WM, WN, true>(X, W, Y, ZERO, g, ep);
}
template <typename T, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN, BN <= 64 ? 3 : 2) void conv_gemm_rs_flat_kernel(const T* __restrict__ X, const T* __restrict__ W,
                                                                       T* __restrict__ Y, const T* __restrict__ ZERO,
                                                                       GatherGeom g, Epilogue ep) {
    conv_gemm_rs_body<T, BM, BN, WM, WN, false>(X, W, Y, ZERO, g, ep);
}

// ---- forward / dgrad gather-GEMM, 256x256 tile, two wave groups in anti-phase ("ping-pong") ----------------
// The 8-wave 256x256x64 tile of conv_gemm_glds_kernel ran its eight waves in lockstep: every wave issued the next
// chunk's eight LDS-DMA instructions and its first fragment reads at the same moment, with the matrix pipes idle
// (measured: ~3.6 k cycles per chunk against 2 k of MFMA issue; MFMA busy 34 %).  Here the two waves that share a
// SIMD (wave w and w+4: the two row groups wm = 0 / 1) run HALF A PHASE APART: while one group is in its load
// section (fragment ds_reads + one half-tile of LDS-DMA for the next chunk) the other is in its MFMA section, and
// every workgroup barrier swaps the roles -- matrix work beside memory work on every SIMD all the time
// (cdna_hip_programming.md 5 "The 256^2 8-phase template", MI355X_MICROARCH.md "Two waves per SIMD" item 5).
//
// A K-chunk (64 channels of one tap) is consumed in four phases, one 128x128 quadrant pair each:
//     ph0 (A0,B0)   ph1 (A0,B1)   ph2 (A1,B1)   ph3 (A1,B0)        8 x v_mfma_f32_32x32x16_bf16 per wave per phase
// and is staged as four HALF-TILES (128 rows x 64 k, 16 KB; two LDS-DMA instructions per thread), one per phase, each
// double buffered (8 x 16 KB = 128 KB): ph0 issues A0 of the NEXT chunk, ph1 B0, ph2 B1, ph3 A1.  A half-tile is
// therefore in flight for three to four phases, and the wait at the end of each load section is a COUNTED
// s_waitcnt vmcnt(4): "everything except the two youngest half-tiles has landed" -- never vmcnt(0) inside the loop.
// Ordering rules (cdna_hip_programming.md "Read a staged buffer one phase AFTER the wait that retires it"):
//   RAW  a wave waits for its own pieces of the half-tiles first read in phase p at the END of its load section of
//        phase p-1; every wave then passes a workgroup barrier before any wave's phase-p reads (the two groups are
//        one barrier apart, hence "one phase early").
//   WAR  buffer b of a half-tile is re-staged in chunk c for chunk c+1; its last reader was chunk c-1, whose load
//        sections ended at least three barriers earlier.
// Half-tile row order is chosen so that a wave's accumulators are the same 128x64 block as in the lockstep kernel
// (rows wm*128.., columns wn*64..): A-half i, row r  <->  tile row (r/64)*128 + i*64 + r%64 ;
// B-half j, row r  <->  tile column (r/32)*64 + j*32 + r%32.  The epilogue is shared with the other kernels.
template <int N> __device__ __forceinline__ void et_wait_vmem_le_pp() {
    __builtin_amdgcn_s_waitcnt(0x0F70 | (N & 0xF) | ((N >> 4) << 14));
}

// (r06: the buffer-descriptor form of the LDS-DMA pieces that conv_gemm_pprs_kernel uses was built for this kernel too -- per-tap
// validity as one mask bit per pixel, no VALU for a weight piece: -4.3 % cycles per launch, -2 % per-launch time, and the STEP 0.2-0.4 ms
// SLOWER: the chip runs this step at its power limit and the denser kernel lowers the clock of every other MFMA kernel by 1.3-1.7 %
// (profiles/r06_power_limit.txt); tools/probe/pp_buffer_dma.patch keeps the code.)
template <typename T>
__global__ __launch_bounds__(512, 2) void conv_gemm_pp_kernel(const T* __restrict__ X, const T* __restrict__ W,
                                                              T* __restrict__ Y, const T* __restrict__ ZERO,
                                                              GatherGeom g, Epilogue ep) {
    constexpr int BM = 256, BN = 256, WM = 2, WN = 4, BKV = 8, VEC = 8;
    constexpr int HALF_VEC = 128 * BKV;            // one half-tile in 16-byte vectors (16 KB)
    constexpr int EPI_VEC = EpiLds<BM, BN, WM, WN>::VEC16;
    constexpr int LDS_VEC = 8 * HALF_VEC > EPI_VEC ? 8 * HALF_VEC : EPI_VEC;
    __shared__ __attribute__((aligned(16))) u32x4 lds_raw[LDS_VEC];
    // half-tile kinds: 0 = A0, 1 = A1, 2 = B0, 3 = B1; buffer b of kind k at lds_raw + (2*k + b) * HALF_VEC

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;       // wm = the wave group (waves w and w+4 share a SIMD)
    int bx, by;
    tile_of_block(g, bx, by);
    const int m0 = bx * BM, n0 = by * BN;
    const int lvec = tid & 7, lrow = tid >> 3;     // staging: 64 rows x 8 K-vectors per instruction of the workgroup
    const int lv = lvec ^ lds_swz<BKV>(lrow);      // logical K-vector this lane stages (swizzle on the SOURCE)

    int a_off[2][2], a_iy[2][2], a_ix[2][2];
    unsigned a_okm = 0u, b_okm = 0u;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int p = m0 + jj * 128 + i * 64 + lrow;           // half i, LDS row jj*64 + lrow
            const bool ok = p < g.M;
            const uint32_t pp = ok ? p : 0;
            const uint32_t t1 = fdiv(pp, g.dQW), qx = pp - t1 * g.QW;
            const uint32_t n = fdiv(t1, g.dQH), qy = t1 - n * g.QH;
            a_iy[i][jj] = qy * g.isy;
            a_ix[i][jj] = qx * g.isx;
            a_off[i][jj] = ((n * g.IH + a_iy[i][jj]) * g.IW + a_ix[i][jj]) * g.ldx;
            a_okm |= ok ? (1u << (i * 2 + jj)) : 0u;
        }
    int b_off[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int r = jj * 64 + lrow;
            const int co = n0 + (r >> 5) * 64 + j * 32 + (r & 31);
            const bool ok = co < g.Cout;
            b_off[j][jj] = (ok ? co : 0) * g.TT * g.Cin;
            b_okm |= ok ? (1u << (j * 2 + jj)) : 0u;
        }

    f32x16 acc[4][2];
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    const int nchunks = g.KV / BKV;                // host: Cin % 64 == 0
    // cursor of the chunk being STAGED (wave-uniform scalars; plain selects, no references: they must stay in SGPRs)
    int tap_u = 0, cv_u = 0;
    int ti_cur = g.tapinfo[0];                     // tap table entry of the cursor's chunk, loaded one chunk AHEAD of its use
    int udy = 0, udx = 0, uwt = 0;
#define ET_PP_DECODE()                                                   \
    do {                                                                 \
        udy = (int)(signed char)(ti_cur & 0xff);                         \
        udx = (int)(signed char)((ti_cur >> 8) & 0xff);                  \
        uwt = (ti_cur >> 16) & 0xff;                                     \
    } while (0)
#define ET_PP_ADVANCE()                                                  \
    do {                                                                 \
        const int t2_ = tap_u + 1, c2_ = cv_u + BKV;                     \
        const bool wt_ = t2_ >= g.T, wc_ = c2_ >= g.CV;                  \
        const int ta_ = wt_ ? 0 : t2_, ca_ = wt_ ? c2_ : cv_u;           \
        const int cb_ = wc_ ? 0 : c2_, tb_ = wc_ ? t2_ : tap_u;          \
        tap_u = g.tap_inner ? ta_ : tb_;                                 \
        cv_u = g.tap_inner ? ca_ : cb_;                                  \
        ti_cur = g.tapinfo[__builtin_amdgcn_readfirstlane(tap_u < g.T ? tap_u : 0)]; \
    } while (0)
    // one LDS-DMA piece (jj = 0 / 1: rows 0-63 / 64-127 of the half-tile) of half-tile kind k (0 A0, 1 A1, 2 B0, 3 B1) of the cursor's chunk
    auto stage_piece = [&](int k, int buf, int jj) {
        u32x4* const wbase = lds_raw + (2 * k + buf) * HALF_VEC + wave * 64;
        if (k < 2) {
            const int i = k;
            const int doff = (udy * g.IW + udx) * g.ldx + (cv_u + lv) * VEC;
            const bool ok = (bool)((a_okm >> (i * 2 + jj)) & 1u) & ((unsigned)(a_iy[i][jj] + udy) < (unsigned)g.IH) &
                            ((unsigned)(a_ix[i][jj] + udx) < (unsigned)g.IW);
            et_glds16(ok ? X + (a_off[i][jj] + doff) : ZERO, wbase + jj * 512);
        } else {
            const int j = k - 2;
            const int woff = uwt * g.Cin + (cv_u + lv) * VEC;
            const bool ok = (b_okm >> (j * 2 + jj)) & 1u;
            et_glds16(ok ? W + (b_off[j][jj] + woff) : ZERO, wbase + jj * 512);
        }
    };
    auto stage_a = [&](int i, int buf) { stage_piece(i, buf, 0); stage_piece(i, buf, 1); };
    auto stage_b = [&](int j, int buf) { stage_piece(2 + j, buf, 0); stage_piece(2 + j, buf, 1); };

    const int l31 = lane & 31, gk = lane >> 5;
    u32x4 af[2][4], bf[4];                         // A fragments of one half (2 row tiles x 4 k-steps), B of one half
    auto load_a = [&](int i, int buf) {
        const u32x4* sm = lds_raw + (2 * i + buf) * HALF_VEC;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int r = wm * 64 + t * 32 + l31;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) af[t][kk] = sm[r * BKV + ((kk * 2 + gk) ^ lds_swz<BKV>(r))];
        }
    };
    auto load_b = [&](int j, int buf) {
        const u32x4* sm = lds_raw + (2 * (2 + j) + buf) * HALF_VEC;
        const int r = wn * 32 + l31;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) bf[kk] = sm[r * BKV + ((kk * 2 + gk) ^ lds_swz<BKV>(r))];
    };
    // 8 MFMAs of one phase; `sk >= 0`: the two LDS-DMA pieces of half-tile kind sk (next chunk, buffer sb) are issued BETWEEN
    // them (after the 2nd and the 5th), where an LDS-DMA instruction costs ~60 cycles of issue instead of the 100-185 it costs in
    // a load section that is also issuing a dozen ds_reads (MI355X_MICROARCH.md "LDS-DMA piece ... issue cost"; the other
    // placements that were measured are in tools/probe/conv_probe.hip, -DET_ABLATE=31..34, profiles/r02_pp_stage_placement_ab.txt)
    auto mfma8 = [&](int i, int j, int sk, int sb) {
        __builtin_amdgcn_s_setprio(1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                acc[2 * i + t][j] = et_mfma32<T>(af[t][kk], bf[kk], acc[2 * i + t][j]);
                const int n = kk * 2 + t;
                if (sk >= 0 && (n == 1 || n == 4)) {
                    __builtin_amdgcn_sched_barrier(0);
                    stage_piece(sk, sb, n == 1 ? 0 : 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(0);
    };

    // prologue: the four half-tiles of chunk 0 into buffer 0
    ET_PP_DECODE();
    stage_a(0, 0); stage_b(0, 0); stage_b(1, 0); stage_a(1, 0);
    ET_PP_ADVANCE();
    et_wait_vmem();
    __builtin_amdgcn_s_barrier();
#define ET_PP_BAR() __builtin_amdgcn_s_barrier()
#define ET_PP_WAIT(n) et_wait_vmem_le_pp<n>()
    if (wm == 1) __builtin_amdgcn_s_barrier();     // group 1 runs one barrier (half a phase) behind group 0

    // one chunk = four phases; `last`: nothing is staged during the final chunk and the waits drain the queue.
    // The half-tile of a phase is issued inside its MFMA section, i.e. AFTER that phase's wait: a counted wait sees the two
    // pieces of ONE younger half-tile in flight (vmcnt 2), the tail chunk drains (2, then 0).
    auto chunk = [&](int buf, auto last_tag) {
        constexpr bool LAST = decltype(last_tag)::value;
        const int nb = buf ^ 1;
        if constexpr (!LAST) ET_PP_DECODE();
        // ---- ph0: (A0, B0); issues A0 of the next chunk
        load_a(0, buf); load_b(0, buf);
        ET_PP_WAIT(2);                                                 // B1 of this chunk has landed (A1 may be in flight)
        ET_PP_BAR();
        mfma8(0, 0, LAST ? -1 : 0, nb);
        ET_PP_BAR();
        // ---- ph1: (A0, B1); issues B0'.  (Fetching B1 one phase early, during ph0's MFMAs, is a race: the OTHER wave group is one
        // barrier behind and retires its pieces of B1 only at its own ph0 wait -- tried, and the emulator's plain schedule
        // caught it; fetching B0 early for ph3 is legal but measured no gain, 5.58 vs 5.58 ms over the model's layers)
        load_b(1, buf);
        if constexpr (LAST) ET_PP_WAIT(0); else ET_PP_WAIT(2);         // A1 of this chunk has landed (A0' may be in flight)
        ET_PP_BAR();
        mfma8(0, 1, LAST ? -1 : 2, nb);
        ET_PP_BAR();
        // ---- ph2: (A1, B1); issues B1'
        load_a(1, buf);
        ET_PP_BAR();
        mfma8(1, 1, LAST ? -1 : 3, nb);
        ET_PP_BAR();
        // ---- ph3: (A1, B0); issues A1', then the cursor moves on
        load_b(0, buf);
        if constexpr (!LAST) ET_PP_WAIT(2);                            // A0', B0' have landed (B1' may be in flight)
        ET_PP_BAR();
        mfma8(1, 0, LAST ? -1 : 1, nb);
        if constexpr (!LAST) ET_PP_ADVANCE();
        ET_PP_BAR();
    };
    int buf = 0;
    for (int c = 0; c + 1 < nchunks; ++c) {
        chunk(buf, std::false_type{});
        buf ^= 1;
    }
    chunk(buf, std::true_type{});
    if (wm == 0) __builtin_amdgcn_s_barrier();     // balances group 1's extra barrier
    __syncthreads();                               // the epilogue reuses the half-tile buffers as its staging area
    conv_epilogue<T, BM, BN, WM, WN, false>(acc, lds_raw, Y, g, ep, bx, m0, n0, tid, lane, wm, wn);
#undef ET_PP_DECODE
#undef ET_PP_ADVANCE
#undef ET_PP_BAR
#undef ET_PP_WAIT
}

// ---- the ping-pong tile with the activation rows shared by the three taps of a kernel row --------------------------------
// conv_gemm_pp_kernel's schedule (two wave groups half a phase apart, four phases per K-chunk, weight half-tiles B0 / B1 double
// buffered and issued in ph1 / ph2 for the next chunk) with conv_gemm_rs_kernel's activation operand: one unit = (channel chunk,
// kernel row) = three chunks (dx) stages the tile's 256 pixels ONCE, as a padded raster of PPRS_ROWS LDS rows (one zero slot after
// every image row), in five 64-row pieces -- one per phase 0 and phase 3 of the unit's chunks, two units deep; the fragment reads of
// a chunk take rows rr + (0 | 1 | 2).  17 LDS-DMA pieces per thread and unit instead of 24, -30 % of the L2->LDS bytes; measured
// bound with the activation pieces of two taps simply dropped (timing only): -11 % on 256->256 @40^2, -8 % on 512->512 @20^2.
// In-order vmcnt accounting per wave (steady state; B1' = the two youngest pieces at every phase-3 wait):
//   ph0: [A piece]   ph1: [B0' B0']   ph2: [B1' B1']   ph3: [A piece | none in the unit's last chunk]
//   end of ph3's load section: vmcnt(2)  -> B0' (next chunk's ph0) and everything older, i.e. all activation pieces, have landed
//   end of ph0's load section: vmcnt(1) if the previous phase 3 issued a piece, else vmcnt(0) -> B1 of this chunk has landed
// RAW / WAR as in conv_gemm_pp_kernel (its header): the weight schedule is unchanged, the activation unit is written two
// units before... no: ONE unit before it is read (buffer (u+1)&1 during unit u; its last reader was unit u-1).
// BUF (r06): the LDS-DMA pieces go through BUFFER descriptors (et_bufdma16) instead of flat 64-bit addresses.  A padding lane is an
// out-of-range voffset (the hardware writes zeros: no zero page, no exec-masked 64-bit select), weight rows beyond Cout fall out of the
// descriptor's range by themselves, and everything wave-uniform about an address (tap, channel chunk, row block of the half-tile, the
// image-row step of the kernel row) is ONE SGPR: a weight piece costs no VALU at all, an activation piece two (v_bfe_u32 + v_lshl_or_b32)
// against nine to ten instructions per piece with an exec-mask round trip in the flat form.  Host: both operands < 2^31 bytes.
#define PPRS_ROWS 320
template <typename T, bool BUF>
__device__ __forceinline__ void conv_gemm_pprs_body(const T* __restrict__ X, const T* __restrict__ W, T* __restrict__ Y,
                                                    const T* __restrict__ ZERO, const GatherGeom& g, const Epilogue& ep) {
    constexpr int BM = 256, BN = 256, WM = 2, WN = 4, BKV = 8, VEC = 8;
    constexpr int HALF_VEC = 128 * BKV;            // one weight half-tile in 16-byte vectors (16 KB)
    constexpr int A_VEC = PPRS_ROWS * BKV;         // one activation unit (40 KB)
    constexpr int NPIECE = PPRS_ROWS / 64;         // 5
    constexpr int RING_VEC = 2 * A_VEC + 4 * HALF_VEC;
    constexpr int EPI_VEC = EpiLds<BM, BN, WM, WN>::VEC16;
    constexpr int LDS_VEC = RING_VEC > EPI_VEC ? RING_VEC : EPI_VEC;
    static_assert(NPIECE == 5, "one activation piece per phase 0 / phase 3 of a unit's three chunks");
    __shared__ __attribute__((aligned(16))) u32x4 lds_raw[LDS_VEC];
    u32x4* const slotA = lds_raw;                  // [2][A_VEC]
    u32x4* const slotB = lds_raw + 2 * A_VEC;      // weight half-tile j, buffer b at slotB + (2*j + b) * HALF_VEC

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;       // wm = the wave group (waves w and w+4 share a SIMD)
    int bx, by;
    tile_of_block(g, bx, by);
    const int m0 = bx * BM, n0 = by * BN;
    const int lvec = tid & 7, lrow = tid >> 3;     // staging: 64 rows x 8 K-vectors per instruction of the workgroup
    const int lv = lvec ^ lds_swz<BKV>(lrow);      // logical K-vector this lane stages (64-row pieces: the swizzle only sees lrow)
    const int W1 = g.QW + 1;
    const uint32_t yg0 = fdiv((uint32_t)m0, g.dQW);
    const int P0 = (int)(yg0 * W1 + ((uint32_t)m0 - yg0 * g.QW));   // padded index of the tile's first pixel

    int a_off[NPIECE];
    unsigned a_okm = 0u, b_okm = 0u;               // a_okm: bit 3q+1 = piece q's pixel exists, bits 3q / 3q+2 = and so does its row above / below
#pragma unroll
    for (int q = 0; q < NPIECE; ++q) {
        const int P = P0 - 1 + q * 64 + lrow;      // LDS row q*64 + lrow <-> padded index P
        const uint32_t Pp = P < 0 ? 0 : P;
        const uint32_t yg = fdiv(Pp, g.dW1), xp = Pp - yg * W1;
        const uint32_t pix = yg * g.QW + xp;
        const bool ok = P >= 0 && (int)xp < g.QW && pix < (uint32_t)g.M;
        const uint32_t ygc = ok ? yg : 0;
        const int iy = ygc - fdiv(ygc, g.dQH) * g.QH;
        a_off[q] = (ok ? pix : 0) * g.ldx;
        a_okm |= ok ? ((iy > 0 ? 1u : 0u) | 2u | (iy + 1 < g.IH ? 4u : 0u)) << (3 * q) : 0u;
        // BUF: this lane's byte offset of piece q behind the descriptor base (one image row in FRONT of the tensor, so that the
        // kernel-row step (dy + 1) * IW * ldx is never negative); a pixel that does not exist is out of range for good (bit 31)
        if constexpr (BUF) a_off[q] = ok ? (int)((a_off[q] + lv * VEC) * (int)sizeof(T)) : (int)0x80000000;
    }
    const unsigned a_nokm = ~a_okm;                // BUF: bit 3q+1+dy SET = piece q has no row at dy for this lane
    // weight rows: half-tile j, piece jj, LDS row jj*64 + lrow <-> output channel co0 + jj*128 + j*32 (one base + uniform steps)
    const int co0 = n0 + (lrow >> 5) * 64 + (lrow & 31);
    const int wrow = g.TT * g.Cin;                 // elements per weight row (uniform)
    const int b_off0 = co0 * wrow;
    // BUF descriptors: X from one image row before its first byte (see above) over the whole tensor, W over exactly Cout rows -- a row
    // beyond Cout (ragged column tile) is out of range and lands as zeros without a mask
    const int rowstep = g.IW * g.ldx;              // elements per image row of X
    et_rsrc rsX, rsW;
    unsigned voffB = 0;
    if constexpr (BUF) {
        rsX = et_make_rsrc((const char*)X - (size_t)rowstep * sizeof(T), (unsigned)(((size_t)g.N * g.IH * g.IW * g.ldx + rowstep) * sizeof(T)));
        rsW = et_make_rsrc(W, (unsigned)((size_t)g.Cout * wrow * sizeof(T)));
        voffB = (unsigned)((b_off0 + lv * VEC) * (int)sizeof(T));
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) b_okm |= (co0 + jj * 128 + j * 32 < g.Cout) ? (1u << (j * 2 + jj)) : 0u;
    const int l31 = lane & 31, gk = lane >> 5;
    // byte offset (inside an activation unit) of this lane's k-step-0 fragment: half i, row tile t, step shift s.  The k-step only
    // XORs bits 5-6 of it (the swizzle is an XOR on the K-vector slot), so a fragment address costs one v_xor, not a swizzle
    int abase[2][2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t p = m0 + wm * 128 + i * 64 + t * 32 + l31;
            const uint32_t yg = fdiv(p, g.dQW);
            const int r0 = (int)(yg * W1 + (p - yg * g.QW)) - P0;
#pragma unroll
            for (int sft = 0; sft < 3; ++sft) abase[i][t][sft] = ((r0 + sft) * BKV + (gk ^ lds_swz<BKV>(r0 + sft))) * 16;
        }

    f32x16 acc[4][2];
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    const int sgn = g.dy[0] < 0 ? 1 : -1;          // taps in kernel-row order: tap 3j+k has dy = sgn*(j-1), dx = sgn*(k-1) (rs_eligible)
    // activation piece q of unit (kernel row j, channel cursor cv) into unit buffer ub
    auto stage_a_piece = [&](int q, int ub, int j, int cv) {
        u32x4* const wbase = slotA + ub * A_VEC + q * 512 + wave * 64;
        const int dy = sgn * (j - 1);
        if constexpr (BUF) {
            const unsigned bad = (a_nokm >> (3 * q + 1 + dy)) & 1u;
            et_bufdma16(rsX, (bad << 31) | (unsigned)a_off[q], (unsigned)(((dy + 1) * rowstep + cv * VEC) * (int)sizeof(T)), wbase);
        } else {
            const bool ok = (a_okm >> (3 * q + 1 + dy)) & 1u;
            et_glds16(ok ? X + (a_off[q] + dy * g.IW * g.ldx + (cv + lv) * VEC) : ZERO, wbase);
        }
    };
    // piece jj (rows 0-63 / 64-127) of weight half-tile j of chunk (tap, cv) into buffer b
    auto stage_b_piece = [&](int j, int b, int jj, int tap, int cv) {
        u32x4* const wbase = slotB + (2 * j + b) * HALF_VEC + wave * 64;
        if constexpr (BUF) {
            et_bufdma16(rsW, voffB, (unsigned)(((jj * 128 + j * 32) * wrow + tap * g.Cin + cv * VEC) * (int)sizeof(T)), wbase + jj * 512);
        } else {
            const bool ok = (b_okm >> (j * 2 + jj)) & 1u;
            et_glds16(ok ? W + (b_off0 + (jj * 128 + j * 32) * wrow + tap * g.Cin + (cv + lv) * VEC) : ZERO, wbase + jj * 512);
        }
    };

    u32x4 af[2][4], bf[4];                         // A fragments of one half (2 row tiles x 4 k-steps), B of one half
    auto load_a = [&](int i, int ub, auto shift_tag) {
        constexpr int SFT = decltype(shift_tag)::value;
        const char* sm = (const char*)(slotA + ub * A_VEC);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) af[t][kk] = *(const u32x4*)(sm + (abase[i][t][SFT] ^ (kk * 32)));
    };
    auto load_b = [&](int j, int b) {
        const u32x4* sm = slotB + (2 * j + b) * HALF_VEC;
        const int r = wn * 32 + l31;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) bf[kk] = sm[r * BKV + ((kk * 2 + gk) ^ lds_swz<BKV>(r))];
    };
    // 8 MFMAs of one phase with up to two LDS-DMA pieces issued between them (after the 2nd and the 5th: conv_gemm_pp_kernel)
    auto mfma8 = [&](int i, int j, auto&& piece0, auto&& piece1) {
        __builtin_amdgcn_s_setprio(1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                acc[2 * i + t][j] = et_mfma32<T>(af[t][kk], bf[kk], acc[2 * i + t][j]);
                const int n = kk * 2 + t;
                if (n == 1) { __builtin_amdgcn_sched_barrier(0); piece0(); __builtin_amdgcn_sched_barrier(0); }
                if (n == 4) { __builtin_amdgcn_sched_barrier(0); piece1(); __builtin_amdgcn_sched_barrier(0); }
            }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(0);
    };
    auto nothing = [] {};

    const int nunits = 3 * (g.CV / BKV);           // (channel chunk outer, kernel row inner); host: Cin % 64 == 0
    // prologue: unit 0 and the weight half-tiles of chunk 0
#pragma unroll
    for (int q = 0; q < NPIECE; ++q) stage_a_piece(q, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 2; ++j) { stage_b_piece(j, 0, 0, sgn > 0 ? 0 : 2, 0); stage_b_piece(j, 0, 1, sgn > 0 ? 0 : 2, 0); }
    et_wait_vmem();
    __builtin_amdgcn_s_barrier();
#define ET_PP_BAR() __builtin_amdgcn_s_barrier()
#define ET_PP_WAIT(n) et_wait_vmem_le_pp<n>()
    if (wm == 1) __builtin_amdgcn_s_barrier();     // group 1 runs one barrier (half a phase) behind group 0

    int jrow = 0, cv_u = 0, bbuf = 0;              // kernel row / channel cursor of the current unit; weight buffer of the current chunk
#pragma unroll 1
    for (int u = 0; u < nunits; ++u) {
        const bool more = u + 1 < nunits;          // uniform: a next unit exists (its activation pieces are staged during this one)
        int nj = jrow + 1, ncv = cv_u;
        if (nj == 3) { nj = 0; ncv += BKV; }
        const int ub = u & 1, nub = ub ^ 1;
        // (compile-time k: a lambda per chunk)
        auto chunk = [&](auto ktag) {
            constexpr int k = decltype(ktag)::value;
            // chunk k reads the unit at row offset k (dx = k - 1); its weights are tap 3j + k (forward) or 3j + 2 - k (dgrad: sgn < 0)
            const bool stage_b = k < 2 || more;    // a next chunk exists
            const int kn = k < 2 ? k + 1 : 0;
            const int ntap = (k < 2 ? jrow : nj) * 3 + (sgn > 0 ? kn : 2 - kn), nbcv = k < 2 ? cv_u : ncv;
            const int nb = bbuf ^ 1;
            const std::integral_constant<int, k> shift{};
            // ---- ph0: (A0, B0); issues activation piece 2k of the next unit
            load_a(0, ub, shift); load_b(0, bbuf);
            if (k > 0 && more) ET_PP_WAIT(1); else ET_PP_WAIT(0);          // B1 of this chunk has landed
            ET_PP_BAR();
            mfma8(0, 0, [&] { if (more) stage_a_piece(2 * k, nub, nj, ncv); }, nothing);
            ET_PP_BAR();
            // ---- ph1: (A0, B1); issues B0 of the next chunk
            load_b(1, bbuf);
            ET_PP_BAR();
            mfma8(0, 1, [&] { if (stage_b) stage_b_piece(0, nb, 0, ntap, nbcv); }, [&] { if (stage_b) stage_b_piece(0, nb, 1, ntap, nbcv); });
            ET_PP_BAR();
            // ---- ph2: (A1, B1); issues B1 of the next chunk
            load_a(1, ub, shift);
            ET_PP_BAR();
            mfma8(1, 1, [&] { if (stage_b) stage_b_piece(1, nb, 0, ntap, nbcv); }, [&] { if (stage_b) stage_b_piece(1, nb, 1, ntap, nbcv); });
            ET_PP_BAR();
            // ---- ph3: (A1, B0); issues activation piece 2k+1 of the next unit (k < 2)
            load_b(0, bbuf);
            if (stage_b) ET_PP_WAIT(2); else ET_PP_WAIT(0);                // B0 of the next chunk and every activation piece have landed
            ET_PP_BAR();
            mfma8(1, 0, [&] { if (k < 2 && more) stage_a_piece(2 * k + 1, nub, nj, ncv); }, nothing);
            ET_PP_BAR();
            bbuf = nb;
        };
        chunk(std::integral_constant<int, 0>{});
        chunk(std::integral_constant<int, 1>{});
        chunk(std::integral_constant<int, 2>{});
        jrow = nj; cv_u = ncv;
    }
    if (wm == 0) __builtin_amdgcn_s_barrier();     // balances group 1's extra barrier
    __syncthreads();                               // the epilogue reuses the ring as its staging area
    conv_epilogue<T, BM, BN, WM, WN, false>(acc, lds_raw, Y, g, ep, bx, m0, n0, tid, lane, wm, wn);
#undef ET_PP_BAR
#undef ET_PP_WAIT
}
// conv_gemm_pprs_kernel: the buffer-descriptor pieces (the default); conv_gemm_pprs_flat_kernel: flat 64-bit addresses, for an operand
// of 2^31 bytes or more and for ET_CONV_BUF_DMA=0
template <typename T>
__global__ __launch_bounds__(512, 2) void conv_gemm_pprs_kernel(const T* __restrict__ X, const T* __restrict__ W,
                                                                T* __restrict__ Y, const T* __restrict__ ZERO,
                                                                GatherGeom g, Epilogue ep) {
    conv_gemm_pprs_body<T, true>(X, W, Y, ZERO, g, ep);
}
template <typename T>
__global__ __launch_bounds__(512, 2) void conv_gemm_pprs_flat_kernel(const T* __restrict__ X, const T* __restrict__ W,
                                                                     T* __restrict__ Y, const T* __restrict__ ZERO,
                                                                     GatherGeom g, Epilogue ep) {
    conv_gemm_pprs_body<T, false>(X, W, Y, ZERO, g, ep);
}

// ---- 1x1 stride-1 layers with <= 256 input and <= 256 output channels: persistent streaming GEMM ---------------------------
// These layers (every Bottleneck.cv1, the C3 stems and cv3 of the stride-4 / 8 / 16 stages: 60 % of the model's BatchNorm layers)
// are HBM-bound: 64-128 flop per byte of activation traffic against the chip's ~400.  As tiles of the generic gather-GEMM they ran
// at 1.3-2.9 TB/s of algorithmic traffic (profiles/r03_launch_table.txt): a workgroup lives for ONE 128 x 64|128 tile -- index
// arithmetic, a cold start of the load pipeline, four short K-chunks, an epilogue during which it has no load in flight, exit --
// and a layer is 1600-12800 such workgroups; with N = 128 output channels on a 64-wide tile every activation row is also fetched
// twice.  Here the layer is a STREAM:
//   * a workgroup is persistent (grid = resident workgroups) and walks row tiles  t = blockIdx.x, + gridDim.x, ...
//   * one tile spans ALL output channels, so every activation row is read from HBM exactly once
//   * the weights (<= 256 x 256 bf16 = 128 KB per layer) never touch LDS: each wave loads the MFMA B fragments of ITS 64 output
//     channels once, at kernel start, and keeps them in registers (KC * 32 VGPRs) for the lifetime of the workgroup
//   * the activation tile goes global -> LDS by LDS-DMA in 64-channel chunks through an NS-deep ring that runs ACROSS tile
//     boundaries: while a wave is in the epilogue of tile i the chunks of tile i + 1 (and beyond) are already in flight
//   * the epilogue is the shared one (scale / bias / activation, BN partial sums, residual, BN-backward sums, 16-byte stores) on
//     16-row slabs, so that ring + slabs of two to four workgroups fit a CU
// vmcnt accounting: a wave's outstanding vector-memory operations are its LDS-DMA pieces (in order among themselves) and the
// epilogue's stores / residual loads.  Loads retire in order, so "at most Y operations outstanding", Y = the pieces issued AFTER
// chunk q, implies chunk q has landed whatever the stores are doing (they can only make the wait conservative, never early).
// RAW: a wave waits for its own pieces of chunk q, then the workgroup barrier publishes every wave's pieces.  WAR: the slot that
// chunk q + NS - 1 overwrites held chunk q - 1, whose last reads precede that same barrier in every wave's program order.
// Register budget (two waves per SIMD, 256 VGPRs each): a wave keeps the weights of its TN * 32 output channels (KC * TN * 16
// VGPRs) and TMW * TN accumulator tiles (16 VGPRs each), and the epilogue's optional features are compiled per kernel: FULL = false
// is the plain forward layer (scale / bias / activation, forward statistics; ~70 VGPRs beside weights and accumulators), FULL = true
// adds residual, accumulate and the BN-backward sums of the dgrads (~150).  Hence the shapes (plan_gemm): plain layers run two
// workgroups of four waves per CU with 64-channel wave tiles (K = 256: 32 rows per wave, else 64); the FULL K = 256 layers run ONE
// workgroup of eight waves with 32-channel wave tiles (64 VGPRs of weights), the ring twice as deep instead of a second workgroup.
// Statistics: a lane's sums run over ALL tiles of its (persistent) workgroup and are written ONCE, as partial row
// blockIdx.x * WM + wm of a (gridDim.x * WM, 2, Cout) buffer (et_conv2d_stats_rows_for reports that row count to the caller): the
// finalize then reads a few hundred rows instead of one per 64 pixels.
// BUF (r06): the activation pieces through a buffer descriptor over the tensor's rows (et_bufdma16): a piece is ZERO vector
// instructions -- the lane's part of the address (row inside the tile, swizzled channel slot) is a constant per piece, the tile's
// first row and the channel chunk travel in the SGPR offset, and a row beyond M lies beyond the descriptor's range and lands as
// zeros -- against a compare, a 64-bit multiply-add and a select into the zero page per piece in the flat form.
template <typename T, int KC, int WN, int TN, int WM, int TMW, int NS, int WGS, bool FULL, bool BUF>
__device__ __forceinline__ void conv1x1_stream_body(const T* __restrict__ X, const T* __restrict__ W,
                                                    T* __restrict__ Y, const T* __restrict__ ZERO,
                                                    const GatherGeom& g, const Epilogue& ep) {
    constexpr int BN = 32 * TN * WN, BM = 32 * TMW * WM, BKV = 8, VEC = 8;
    constexpr int TM = TMW;                              // a wave owns 32 * TMW rows x 32 * TN output channels
    constexpr int NT = 64 * WM * WN;
    constexpr int CH_VEC = BM * BKV;                     // one chunk (BM rows x 64 channels) in 16-byte vectors
    constexpr int DT = CH_VEC < NT ? CH_VEC : NT;        // threads that stage (a 32-row chunk is 256 pieces: four waves of eight)
    constexpr int PER = CH_VEC / DT;                     // LDS-DMA instructions per staging thread per chunk
    constexpr int MODE = FULL ? 0 : 1;
    using L = EpiLds<BM, BN, WM, WN, 16>;
    static_assert(KC == 1 || KC == 2 || KC == 4, "K = 64 * KC");
    static_assert(CH_VEC % DT == 0 && DT % 64 == 0 && PER >= 1 && (NS - 1) * PER < 64 && NS >= 2 && NS <= 16, "ring");
    __shared__ __attribute__((aligned(16))) u32x4 lds_raw[NS * CH_VEC + L::VEC16 + BN];
    u32x4* const ring = lds_raw;
    u32x4* const slabs = lds_raw + NS * CH_VEC;
    float* const cst = (float*)(lds_raw + NS * CH_VEC + L::VEC16);      // [scale | bias | bn_scale | bn_shift][BN]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, gk = lane >> 5;
    const int lvec = tid % BKV, lrow = tid / BKV;
    constexpr int RPT = DT / BKV;                        // rows per staging pass
    const bool stager = wave * 64 < DT;                  // wave-uniform

    // ---- per-channel epilogue constants -> LDS, once (EpiSums::cst)
    for (int c = tid; c < BN; c += NT) {
        const bool cok = c < g.Cout;
        cst[c] = (ep.scale && cok) ? ep.scale[c] : 1.0f;
        cst[BN + c] = (ep.bias && cok) ? ep.bias[c] : 0.0f;
        cst[2 * BN + c] = (FULL && ep.bn_y && cok) ? ep.bn_scale[c] : 1.0f;
        cst[3 * BN + c] = (FULL && ep.bn_y && cok) ? ep.bn_shift[c] : 0.0f;
    }

    // ---- staging: piece j of a chunk = LDS rows lrow + j * RPT; the swizzle is applied to the SOURCE (conv_gemm_glds_kernel)
    int a_row[PER], a_lv[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        a_row[j] = lrow + j * RPT;
        a_lv[j] = (lvec ^ lds_swz<BKV>(a_row[j])) * VEC;
    }
    et_rsrc rsX;
    if constexpr (BUF) {                                 // [X, end of row M - 1's channels): a row >= M is out of range by itself
        rsX = et_make_rsrc(X, (unsigned)(((size_t)(g.M - 1) * g.ldx + KC * 64) * sizeof(T)));
#pragma unroll
        for (int j = 0; j < PER; ++j) a_row[j] = (a_row[j] * g.ldx + a_lv[j]) * (int)sizeof(T);      // the lane's byte offset inside a tile
    }
    const int ntiles = g.ntm;
    const int my_tiles = ((int)blockIdx.x < ntiles) ? (ntiles - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
    const int total = my_tiles * KC;                     // chunks this workgroup consumes
    int is_tile = blockIdx.x, is_kc = 0, is_slot = 0, issued = 0;     // cursor of the next chunk to ISSUE (uniform)
    auto issue = [&]() {
        if (stager) {
            u32x4* const wbase = ring + is_slot * CH_VEC + wave * 64;
            const int m0i = is_tile * BM;
            const unsigned soff = (unsigned)(((size_t)m0i * g.ldx + is_kc * 64) * sizeof(T));     // BUF; host: the tensor spans < 2^31 bytes
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                if constexpr (BUF) {
#if ET_S1_NT
                    et_bufdma16_nt(rsX, (unsigned)a_row[j], soff, wbase + j * DT);
#else
                    et_bufdma16(rsX, (unsigned)a_row[j], soff, wbase + j * DT);
#endif
                } else {
                    const int p = m0i + a_row[j];
                    const T* src = p < g.M ? X + ((size_t)p * g.ldx + is_kc * 64 + a_lv[j]) : ZERO;
#if ET_S1_NT
                    et_glds16_nt(src, wbase + j * DT);
#else
                    et_glds16(src, wbase + j * DT);
#endif
                }
            }
        }
        ++issued;
        if (++is_kc == KC) { is_kc = 0; is_tile += gridDim.x; }
        is_slot = is_slot + 1 == NS ? 0 : is_slot + 1;
    };
#pragma unroll
    for (int s = 0; s < NS - 1; ++s)
        if (issued < total) issue();

    // ---- this wave's weights -> registers: B fragment (column tile tn, k-step ks) = 8 consecutive K elements of output channel co
    u32x4 bw[TN][KC * 4];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int co = wn * (32 * TN) + tn * 32 + l31;
        const bool cok = co < g.Cout;
        const T* wr = W + (size_t)(cok ? co : 0) * g.Cin + gk * VEC;
#pragma unroll
        for (int ks = 0; ks < KC * 4; ++ks) {
            bw[tn][ks] = *(const u32x4*)(wr + ks * 16);          // unconditional load (row 0 for a channel beyond Cout), zeroed below
            if (!cok) bw[tn][ks] = mk4(0, 0, 0, 0);
        }
    }
    // The weights (and with them the ring's first chunks, issued just above) must have LANDED before the tile loop starts, so
    // that the loop's MFMAs read registers with no load pending on them: left to the compiler, the wait for these loads is a
    // vmcnt(0) in front of the first MFMA of EVERY tile -- it drains the ring once per tile (seen in the ISA of the first
    // version; a plain s_waitcnt here does not help, the loads are sunk below it into the loop preheader).  et_pin_loaded is an
    // empty asm that redefines the register: the loads complete in front of it, the loop depends on its output.
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int ks = 0; ks < KC * 4; ++ks) et_pin_loaded(bw[tn][ks]);
    __syncthreads();                                     // ... and the constants are visible to every wave

    // byte offset of this lane's k-step-0 fragment inside a chunk: row tile tm; a k-step XORs bits 5-6 of it (the swizzle is an XOR
    // on the K-vector slot)
    int abase[TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int r = wm * (32 * TMW) + tm * 32 + l31;
        abase[tm] = (r * BKV + (gk ^ lds_swz<BKV>(r))) * 16;
    }

    EpiSums<TN> st;
    st.clear();
    st.cst = cst;
    st.cstride = BN;
    int rd = 0, q = 0;
    for (int i = 0; i < my_tiles; ++i) {
        const int m0 = ((int)blockIdx.x + i * (int)gridDim.x) * BM;
        f32x16 acc[TM][TN];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc, ++q) {
            // chunk q has landed once at most `ahead` younger chunks of this wave are outstanding (see the header); a wave that
            // stages nothing has nothing to wait for
            const int ahead = min(NS - 2, total - 1 - q);
            switch (ahead) {             // uniform; NS <= 16
#define ET_S1_WAIT(A) case A: et_wait_vmem_le_lds_read_done<((A) <= NS - 2 ? (A) : 0) * PER>(); break;
                ET_S1_WAIT(1) ET_S1_WAIT(2) ET_S1_WAIT(3) ET_S1_WAIT(4) ET_S1_WAIT(5) ET_S1_WAIT(6) ET_S1_WAIT(7)
                ET_S1_WAIT(8) ET_S1_WAIT(9) ET_S1_WAIT(10) ET_S1_WAIT(11) ET_S1_WAIT(12) ET_S1_WAIT(13) ET_S1_WAIT(14)
#undef ET_S1_WAIT
                default: et_wait_vmem_lds_read_done(); break;
            }
            __builtin_amdgcn_s_barrier();                // (lgkmcnt(0) above: issue() rewrites the slot the previous chunk read -- et_device.h)
            if (issued < total) issue();
            const char* const sa = (const char*)(ring + rd * CH_VEC);
            u32x4 af[2][TM];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) af[0][tm] = *(const u32x4*)(sa + abase[tm]);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int cur = kk & 1;
                if (kk + 1 < 4) {
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) af[cur ^ 1][tm] = *(const u32x4*)(sa + (abase[tm] ^ ((kk + 1) * 32)));
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
                        acc[tm][tn] = et_mfma32<T>(af[cur][tm], bw[tn][kc * 4 + kk], acc[tm][tn]);
            }
            rd = rd + 1 == NS ? 0 : rd + 1;
        }
        conv_epilogue<T, BM, BN, WM, WN, 16, MODE, true>(acc, slabs, Y, g, ep, 0, m0, 0, tid, lane, wm, wn, st);
    }
    // every workgroup of the grid writes its row (also one that had no tile: zeros), so the consumer may sum all gridDim.x * WM rows
    if (ep.stats) {
        if (ep.stats_ld) conv_stats_add_sharded_wg<BN, WN, WM, MODE>(st, g, ep, tid, lane, wm, wn, (float*)ring);
        else conv_epilogue_write_stats<BN, WN, MODE>(st, g, ep, 0, lane, wn, (int)blockIdx.x * WM + wm, 0, (int)gridDim.x * WM);
    }
}
// conv1x1_stream_kernel: buffer-descriptor pieces (the default); conv1x1_stream_flat_kernel: flat addresses, for a tensor of 2^31 bytes or
// more and for ET_CONV_BUF_DMA=0
template <typename T, int KC, int WN, int TN, int WM, int TMW, int NS, int WGS, bool FULL>
__global__ __launch_bounds__(64 * WM * WN, WGS) void conv1x1_stream_kernel(const T* __restrict__ X, const T* __restrict__ W,
                                                                          T* __restrict__ Y, const T* __restrict__ ZERO,
                                                                          GatherGeom g, Epilogue ep) {
    conv1x1_stream_body<T, KC, WN, TN, WM, TMW, NS, WGS, FULL, true>(X, W, Y, ZERO, g, ep);
}
template <typename T, int KC, int WN, int TN, int WM, int TMW, int NS, int WGS, bool FULL>
__global__ __launch_bounds__(64 * WM * WN, WGS) void conv1x1_stream_flat_kernel(const T* __restrict__ X, const T* __restrict__ W,
                                                                               T* __restrict__ Y, const T* __restrict__ ZERO,
                                                                               GatherGeom g, Epilogue ep) {
    conv1x1_stream_body<T, KC, WN, TN, WM, TMW, NS, WGS, FULL, false>(X, W, Y, ZERO, g, ep);
}

// ---- the stem: 6x6 stride-2 pad-2 convolution of the packed image (8 channels, 3 used) ----------------------------
// (YoloV5BackBone.stage1, models/backbone/yolov5_backbone.py:36: Conv(3, 64, 6, 2, 2)).  As a gather-GEMM this layer is the
// worst case of the generic kernels: K = 36 taps x 8 channels, so every 16-byte LDS-DMA piece is its own (tap, pixel)
// gather and each input pixel travels L2 -> LDS nine times (measured 0.79 ms at B=64 against an HBM floor of 0.25 ms).
// Here one workgroup computes a 4 x 64 block of output pixels from ONE staged input patch (12 x 132 pixels, 25 KB: each
// input pixel is staged 1.5 times instead of 9) and reads its MFMA operands out of that patch with constant offsets:
//   * the patch keeps the image's pixel order (a patch row is one contiguous 2.1 KB run of the packed image: every staging
//     instruction of a wave is a coalesced 1 KB read); output column c, tap column kx reads patch column 2c + kx, and since
//     taps 2ks / 2ks+1 of a k-step are horizontal neighbours of one kernel row, the lane's K-half (lane >> 5) is simply one
//     more slot.  The stride-2 fragment reads are 2-way bank conflicts on 36 reads per tile -- irrelevant next to staging
//     (a de-interleaved patch, conflict-free but staged in 32-byte strides, measured 0.57 ms against this layout's figure
//     in profiles/);
//   * the whole weight matrix (64 x 288 bf16) sits in LDS for the lifetime of the (persistent) workgroup, row pitch 37
//     slots (odd: conflict-free b128 reads);
//   * operands are SWAPPED (weights = MFMA A, pixels = MFMA B): a lane then owns one output pixel and 4 consecutive
//     channels per accumulator quad, so the result is stored straight from registers in 8-byte pieces -- no LDS
//     transposition; BN statistics are accumulated per lane over all tiles of the workgroup and reduced once at the end.
// HBM-bound by construction: 57 KB of traffic and 72 MFMAs per wave per tile.
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

// image n -> its uint8 planes (wave-uniform: scalar selects over the kernel arguments)
template <typename A> __device__ __forceinline__ const uint8_t* stem_u8_image(const A& a, int n) {
    const uint8_t* p = a.seg[0];
    int b = 0;
#pragma unroll
    for (int s = 1; s < STEM_MAX_SEGS; ++s)
        if (n >= a.seg_b[s]) { p = a.seg[s]; b = a.seg_b[s]; }
    return p + (size_t)(n - b) * 3 * a.IH * a.IW;
}
// lut[v] = T(v / norm): EXACTLY pack_input4_bf16_kernel's expression (spatial.hip: IEEE division, then the pack's rounding), so a pixel
// staged through the table carries the bits the packed tensor would
template <typename T> __device__ __forceinline__ void stem_u8_fill_lut(uint16_t* lut, int tid, float norm) {
    lut[tid] = (uint16_t)(et_lp<T>::pack((float)((unsigned)tid & 0xffu) / norm, 0.f) & 0xffffu);
}

// U8 = false: the patch is staged by LDS-DMA from the packed image (a.x).  U8 = true: from the uint8 planes -- a thread fetches
// whole aligned pixel QUADS (one dword per plane; the patch's 132 columns start 2 pixels into the first of 34 quads, IW % 4 == 0: a
// quad is inside or outside the image as a whole) into registers while the previous tile's MFMAs run, and turns them into the packed
// pixel layout (r, g, b, five zeros: one 16-byte LDS write per pixel) through the table at the head of its tile.  Everything behind
// the patch -- operand offsets, MFMA order, epilogue -- is the same code, so the result is bit-identical to pack + conv_stem_kernel.
#define STEM_QPR 34                     // pixel quads per patch row: columns -4 .. 131 relative to the first output column's 2*ox
#define STEM_NQ (STEM_PH * STEM_QPR)    // 408 quads: 2 per thread
template <typename T, int ACT, bool U8>
__device__ __forceinline__ void conv_stem_body(const StemArgs& a) {            // T: the 16-bit format behind StemArgs' raw pointers
    __shared__ __attribute__((aligned(16))) u32x4 wl[STEM_WSLOTS];
    __shared__ __attribute__((aligned(16))) u32x4 pl[STEM_PSLOTS];
    __shared__ uint16_t lut[U8 ? 256 : 2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    if constexpr (U8) stem_u8_fill_lut<T>(lut, tid, a.norm);

    // ---- weights -> LDS once (pitch 37; channels >= Cout and the pad slot read the zero page)
#pragma unroll
    for (int i = 0; i < STEM_WSLOTS / 256; ++i) {
        const int slot = i * 256 + tid;
        const int ch = slot / STEM_WPITCH, tap = slot - ch * STEM_WPITCH;
        const bool ok = ch < a.Cout && tap < 36;
        et_glds16(ok ? a.w + ((size_t)ch * 36 + tap) * 8 : a.zero, wl + i * 256 + wave * 64);
    }
    // ---- this thread's patch slots: (row, column) offsets inside a patch, constant over tiles
    int s_dy[STEM_PSLOTS / 256], s_dx[STEM_PSLOTS / 256];
#pragma unroll
    for (int i = 0; i < STEM_PSLOTS / 256; ++i) {
        const int slot = i * 256 + tid;
        const int prow = slot / STEM_PITCH;
        s_dy[i] = prow < STEM_PH ? prow : -100000;          // fails every bounds check below
        s_dx[i] = slot - prow * STEM_PITCH;
    }
    float ssum[2][16], ssq[2][16];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) { ssum[cb][r] = 0.f; ssq[cb][r] = 0.f; }
    // folded-BatchNorm scale / bias (eval-mode teacher) of the channel octets this lane stores: (cb, m) -> channels cb*32 + 8*(2m + hi) .. +7.
    // Loaded ONCE per (persistent) workgroup: read inside the store loop they were 128 extra vector-memory instructions per tile,
    // in front of 72 MFMAs (the teacher's stem ran at half the student's rate per image)
    float esc[2][2][8], ebi[2][2][8];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int ch = cb * 32 + 8 * (2 * m + hi) + e;
                esc[cb][m][e] = (a.scale && ch < a.Cout) ? a.scale[ch] : 1.0f;
                ebi[cb][m][e] = (a.bias && ch < a.Cout) ? a.bias[ch] : 0.0f;
            }

    const u32x4* const wbase = wl + l31 * STEM_WPITCH + hi;                          // + cb * 32 * 37 + 2 * ks
    const u32x4* const pbase = pl + (2 * wave) * STEM_PITCH + 2 * l31 + hi;          // + pb * 64 + (ks/3) * PITCH + 2 * (ks%3)

    auto stage_patch = [&](int tile) {
        const int tc = tile % a.tcn, t2 = tile / a.tcn;
        const int tr = t2 % a.trn, n = t2 / a.trn;
        const int iy0 = 2 * tr * STEM_TR - 2, ix0 = 2 * tc * STEM_TC - 2;
#pragma unroll
        for (int i = 0; i < STEM_PSLOTS / 256; ++i) {
            const int iy = iy0 + s_dy[i], ix = ix0 + s_dx[i];
            const bool ok = (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW;
            const uint16_t* src = ok ? a.x + (((size_t)n * a.IH + iy) * a.IW + ix) * a.ldx : a.zero;
            et_glds16(src, pl + i * 256 + wave * 64);
        }
    };
    // ---- uint8 form: this thread's two quads (patch row, quad column), their bytes of the tile in flight, and whether they are inside
    int q_row[2], q_col[2];
    unsigned q_px[2][3];
    bool q_in[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = i * 256 + tid;
        q_row[i] = q < STEM_NQ ? q / STEM_QPR : -100000;
        q_col[i] = q % STEM_QPR;
        q_in[i] = false;
#pragma unroll
        for (int c = 0; c < 3; ++c) q_px[i][c] = 0u;
    }
    auto load_u8 = [&](int tile) {
        const int tc = tile % a.tcn, t2 = tile / a.tcn;
        const int tr = t2 % a.trn, n = t2 / a.trn;
        const int iy0 = 2 * tr * STEM_TR - 2, ix0 = 2 * tc * STEM_TC - 4;
        const uint8_t* const img = stem_u8_image(a, n);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int iy = iy0 + q_row[i], ix = ix0 + 4 * q_col[i];
            q_in[i] = (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                q_px[i][c] = q_in[i] ? *(const unsigned*)(img + ((size_t)c * a.IH + iy) * a.IW + ix) : 0u;
        }
    };
    auto write_patch_u8 = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int pc = 4 * q_col[i] - 2 + j;
                if (q_row[i] >= 0 && (unsigned)pc < (unsigned)STEM_PITCH) {
                    const unsigned r = lut[(q_px[i][0] >> (8 * j)) & 0xffu], g = lut[(q_px[i][1] >> (8 * j)) & 0xffu];
                    const unsigned b = lut[(q_px[i][2] >> (8 * j)) & 0xffu];
                    pl[q_row[i] * STEM_PITCH + pc] = q_in[i] ? mk4(r | (g << 16), b, 0u, 0u) : mk4(0u, 0u, 0u, 0u);
                }
            }
    };
    if constexpr (U8) {
        __syncthreads();                 // the table
        if ((int)blockIdx.x < a.ntiles) load_u8(blockIdx.x);
    } else {
        if ((int)blockIdx.x < a.ntiles) stage_patch(blockIdx.x);
    }
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int tc = tile % a.tcn, t2 = tile / a.tcn;
        const int tr = t2 % a.trn, n = t2 / a.trn;
        const int oy0 = tr * STEM_TR, ox0 = tc * STEM_TC;
        if constexpr (U8) write_patch_u8();       // every wave left the previous patch at the barrier behind its MFMAs
        et_wait_vmem();
        __syncthreads();
        if constexpr (U8) {                       // the next tile's bytes travel while this tile's MFMAs and stores run
            if (tile + (int)gridDim.x < a.ntiles) load_u8(tile + gridDim.x);
        }
        // ---- 18 k-steps (two taps of one kernel row each): 2 channel blocks x 2 pixel blocks of 32x32x16 MFMAs
        f32x16 acc[2][2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int pb = 0; pb < 2; ++pb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[cb][pb][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 18; ++ks) {
            u32x4 wf[2], pf[2];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) wf[cb] = wbase[cb * 32 * STEM_WPITCH + 2 * ks];
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) pf[pb] = pbase[pb * 64 + (ks / 3) * STEM_PITCH + 2 * (ks % 3)];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int pb = 0; pb < 2; ++pb)
                    acc[cb][pb] = et_mfma32<T>(wf[cb], pf[pb], acc[cb][pb]);
        }
        // every wave is done with the patch: the next tile's patch streams in behind this tile's epilogue
        __syncthreads();
        if constexpr (!U8) {
            if (tile + (int)gridDim.x < a.ntiles) stage_patch(tile + gridDim.x);
        }
        // ---- epilogue straight from registers: lane = pixel (l31 of block pb), register r = channel 8*(r>>2) + 4*hi + (r&3).
        // The two lanes of a pixel (hi = 0 / 1) each hold 4 of every 8 consecutive channels: they trade quads so that each
        // ends up with 8 whole channel octets -- 8 stores of 16 bytes per lane instead of 16 of 8 (the store tail of a
        // row-per-lane epilogue is issue-bound: MI355X_MICROARCH.md, "attention epilogue store tail")
        const int oy = oy0 + wave;
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            const int ox = ox0 + pb * 32 + l31;
            const bool pok = oy < a.OH && ox < a.OW;
            uint16_t* const yp = a.y + (((size_t)n * a.OH + oy) * a.OW + ox) * a.ldy;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                if (pok) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) { const float raw = acc[cb][pb][r]; ssum[cb][r] += raw; ssq[cb][r] += raw * raw; }
                }
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    // octets j0 = 2m (kept by the hi = 0 lane) and j1 = 2m + 1 (kept by the hi = 1 lane)
                    float lo4[4], hi4[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float q0 = acc[cb][pb][8 * m + e], q1 = acc[cb][pb][8 * m + 4 + e];
                        const float t = __shfl_xor(hi ? q0 : q1, 32);
                        lo4[e] = hi ? t : q0;        // channels oct*8 + e
                        hi4[e] = hi ? q1 : t;        // channels oct*8 + 4 + e
                    }
                    const int ch = cb * 32 + 8 * (2 * m + hi);
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float u = e < 4 ? lo4[e] : hi4[e - 4];
                        u = u * esc[cb][m][e] + ebi[cb][m][e];
                        if constexpr (ACT == ACT_SILU) u = u * __builtin_amdgcn_rcpf(1.0f + __expf(-u));
                        else if constexpr (ACT == ACT_RELU) u = fmaxf(u, 0.f);
                        v[e] = u;
                    }
                    if (pok && ch < a.Cout)
                        *(u32x4*)(yp + ch) = mk4(et_lp<T>::pack(v[0], v[1]), et_lp<T>::pack(v[2], v[3]), et_lp<T>::pack(v[4], v[5]), et_lp<T>::pack(v[6], v[7]));
                }
            }
        }
    }
    // ---- BN statistics: per-lane sums over this workgroup's pixels -> one partial row per workgroup, zeros elsewhere
    if (a.stats) {
        float* const red = (float*)wl;        // [4 waves][2][64]; the weights are no longer needed
        __syncthreads();
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float s1 = ssum[cb][r], s2 = ssq[cb][r];
#pragma unroll
                for (int m = 1; m < 32; m <<= 1) { s1 += __shfl_xor(s1, m); s2 += __shfl_xor(s2, m); }
                if (l31 == 0) {
                    const int ch = cb * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
                    red[(wave * 2 + 0) * 64 + ch] = s1;
                    red[(wave * 2 + 1) * 64 + ch] = s2;
                }
            }
        __syncthreads();
        if (tid < 128) {
            const int which = tid >> 6, ch = tid & 63;
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) t += red[(w * 2 + which) * 64 + ch];
            if (ch < a.Cout && a.stats_ld) {
                unsafeAtomicAdd(a.stats + ((size_t)(blockIdx.x % ET_BN_SHARDS) * 2 + which) * a.stats_ld + ch, t);
            } else if (ch < a.Cout) {
                // the consumer sums ALL stat_rows partial rows: this workgroup owns rows blockIdx.x, + gridDim.x, ...
                for (int row = blockIdx.x; row < a.stat_rows; row += gridDim.x)
                    a.stats[((size_t)row * 2 + which) * a.Cout + ch] = row == (int)blockIdx.x ? t : 0.f;
            }
        }
    }
}
template <typename T, int ACT>
__global__ __launch_bounds__(256, 2) void conv_stem_kernel(StemArgs a) { conv_stem_body<T, ACT, false>(a); }
template <typename T, int ACT>
__global__ __launch_bounds__(256, 2) void conv_stem_u8_kernel(StemArgs a) { conv_stem_body<T, ACT, true>(a); }

// ---- wgrad ----------------------------------------------------------------------------------------
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

template <typename T> struct Transposer;
template <> struct Transposer<uint16_t> {   // 8x8 block of 16-bit elements
    __device__ static __forceinline__ void run(const u32x4 (&in)[8], u32x4 (&out)[8]) {
        const uint32_t* s[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = (const uint32_t*)&in[i];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            uint32_t w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t lo = s[2 * j][c >> 1], hi = s[2 * j + 1][c >> 1];
                w[j] = (c & 1) ? ((lo >> 16) | (hi & 0xffff0000u)) : ((lo & 0xffffu) | (hi << 16));
            }
            out[c] = mk4(w[0], w[1], w[2], w[3]);
        }
    }
};
template <> struct Transposer<et_f16> : Transposer<uint16_t> {};      // moves 16-bit words: format-agnostic
template <> struct Transposer<float> {      // 4x4 block of 32-bit elements
    __device__ static __forceinline__ void run(const u32x4 (&in)[4], u32x4 (&out)[4]) {
        out[0] = mk4(in[0].x, in[1].x, in[2].x, in[3].x);
        out[1] = mk4(in[0].y, in[1].y, in[2].y, in[3].y);
        out[2] = mk4(in[0].z, in[1].z, in[2].z, in[3].z);
        out[3] = mk4(in[0].w, in[1].w, in[2].w, in[3].w);
    }
};

template <typename T, int BM, int BN>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const T* __restrict__ X, const T* __restrict__ DY,
                                                         float* __restrict__ DW, WgradGeom g) {
    constexpr int VEC = et_elem<T>::VEC, BKV = 8, WM = 2, WN = 2;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int GA = BM / VEC, GB = BN / VEC;        // channel groups per tile
    constexpr int NBLK = (GA + GB) * BKV;              // VECxVEC transposition blocks per chunk
    constexpr int ITER = (NBLK + 255) / 256;
    constexpr int BKP = BKV * VEC;                     // pixels per K-chunk
    __shared__ __attribute__((aligned(16))) u32x4 lds[2][(BM + BN) * BKV];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    // 1-D grid, remapped so that each XCD owns a contiguous range of block ids: all (cout tile, column tile)
    // blocks of one K-split read the SAME pixels of dY / X, so they should share one XCD's L2
    // (the round-robin dispatch otherwise makes every XCD fetch every pixel range).
    int bid = blockIdx.x;
    if (g.xcd) {
        const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = bid & 7, k = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
    }
    const int tx = bid % g.ntn, ty = (bid / g.ntn) % g.ntm, tz = bid / (g.ntn * g.ntm);
    const int n0 = tx * BN, m0 = ty * BM;
    const int pk_begin = tz * g.Pper;
    const int pk_end = min(g.P, pk_begin + g.Pper);

    // per-thread block descriptors (fixed over the K loop)
    bool isA[ITER], live[ITER], chan_ok[ITER];
    int grp[ITER], kvv[ITER], coff[ITER], tdy[ITER], tdx[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int blk = tid + it * 256;
        live[it] = blk < NBLK;
        isA[it] = blk < GA * BKV;
        const int b2 = isA[it] ? blk : blk - GA * BKV;
        const int G = isA[it] ? GA : GB;
        grp[it] = b2 % G;
        kvv[it] = b2 / G;
        tdy[it] = tdx[it] = 0;
        if (isA[it]) {
            const int co = m0 + grp[it] * VEC;
            chan_ok[it] = co < g.Cout;      // Cout % VEC == 0 is required by the host wrapper
            coff[it] = co;
        } else {
            const int col = n0 + grp[it] * VEC;
            chan_ok[it] = col < g.NC;
            const uint32_t cc = chan_ok[it] ? col : 0;
            const uint32_t tap = fdiv(cc, g.dCin);
            coff[it] = cc - tap * g.Cin;
            tdy[it] = g.dy[tap];
            tdx[it] = g.dx[tap];
        }
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    // Prefetch distance 2 (two raw register sets), exactly as in conv_gemm_kernel: raw 16-byte loads only
    // (unconditional, invalid lanes read the tensor base); the zero-fill select, the VECxVEC register
    // transpose and the LDS stores happen AFTER the MFMAs of the current chunk.
    u32x4 rawA[ITER][VEC], rawB[ITER][VEC];
    unsigned okA[ITER], okB[ITER];
    auto gload = [&](int pk0, u32x4 (&raw)[ITER][VEC], unsigned (&okm)[ITER]) {
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            okm[it] = 0u;
            if (!live[it]) continue;
            const int p0 = pk0 + kvv[it] * VEC;
            if (isA[it]) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const int p = p0 + i;
                    const bool ok = chan_ok[it] && p < pk_end;
                    raw[it][i] = *(const u32x4*)(DY + (ok ? (long long)p * g.ldy + coff[it] : 0));
                    okm[it] |= ok ? (1u << i) : 0u;
                }
            } else {
                const uint32_t pp = min(p0, g.P - 1);
                const uint32_t t1 = fdiv(pp, g.dQW);
                int qx = pp - t1 * g.QW;
                const uint32_t n_ = fdiv(t1, g.dQH);
                int qy = t1 - n_ * g.QH;
                int n = n_;
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const int p = p0 + i;
                    const int iy = qy * g.isy + tdy[it], ix = qx * g.isx + tdx[it];
                    const bool ok = chan_ok[it] && p < pk_end && (unsigned)iy < (unsigned)g.IH && (unsigned)ix < (unsigned)g.IW;
                    raw[it][i] = *(const u32x4*)(X + (ok ? (((long long)n * g.IH + iy) * g.IW + ix) * g.ldx + coff[it] : 0));
                    okm[it] |= ok ? (1u << i) : 0u;
                    if (++qx == g.QW) { qx = 0; if (++qy == g.QH) { qy = 0; ++n; } }
                }
            }
        }
    };
    auto lstore = [&](int buf, const u32x4 (&raw)[ITER][VEC], const unsigned (&okm)[ITER]) {
        const u32x4 zero = mk4(0, 0, 0, 0);
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            if (!live[it]) continue;
            u32x4 in[VEC], tr[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) in[i] = ((okm[it] >> i) & 1u) ? raw[it][i] : zero;
            Transposer<T>::run(in, tr);
            const int rbase = (isA[it] ? 0 : BM) + grp[it] * VEC;
#pragma unroll
            for (int c = 0; c < VEC; ++c) {
                const int rl = grp[it] * VEC + c;          // row inside its operand tile
                lds[buf][(rbase + c) * BKV + (kvv[it] ^ lds_swz<BKV>(rl))] = tr[c];
            }
        }
    };

    const int nchunks = (pk_end - pk_begin + BKP - 1) / BKP;
    if (nchunks > 0) {
        gload(pk_begin, rawA, okA);
        if (nchunks > 1) gload(pk_begin + BKP, rawB, okB);
        lstore(0, rawA, okA);
    }
    __syncthreads();
    for (int c = 0; c < nchunks; c += 2) {
        if (c + 2 < nchunks) gload(pk_begin + (c + 2) * BKP, rawA, okA);
        mma_chunk<T, BM, BN, WM, WN, BKV>(lds[0], acc, wm, wn, lane);
        __builtin_amdgcn_sched_barrier(0);
        if (c + 1 < nchunks) lstore(1, rawB, okB);
        __syncthreads();
        if (c + 1 < nchunks) {
            if (c + 3 < nchunks) gload(pk_begin + (c + 3) * BKP, rawB, okB);
            mma_chunk<T, BM, BN, WM, WN, BKV>(lds[1], acc, wm, wn, lane);
            __builtin_amdgcn_sched_barrier(0);
            if (c + 2 < nchunks) lstore(0, rawA, okA);
            __syncthreads();
        }
    }
    if (nchunks <= 0) return;
    const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = m0 + wm * (BM / WM) + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int col = n0 + wn * (BN / WN) + tn * 32 + l31;
                if (co < g.Cout && col < g.NC) atomicAdd(DW + ((size_t)co * g.NC + col), acc[tm][tn][r]);
            }
        }
}

// ---- wgrad, bf16, LDS-DMA staging + transposing LDS reads -------------------------------------------------
// Same GEMM as conv_wgrad_kernel (dW[cout, (tap,ci)] += sum_pixel dY[pixel,cout] * X[gather(pixel,tap),ci]) but the
// operand tiles stay in their natural [pixel][channel] order in LDS: they are staged with
// global_load_lds_dwordx4 (a wave lands 4 pixel rows of 256 contiguous bytes per instruction) and the
// K(=pixel)-contiguous MFMA fragments are produced by ds_read_b64_tr_b16, gfx950's transposing LDS read:
// a 16-lane group reads a [4 pixels][16 channels] block (lane t: pixel t/4, channels 4*(t%4)..+3, 8 bytes)
// and lane c receives channel c of the 4 pixels.  No VGPR staging, no register transposes, no ds_write.
// The 16-byte slots of a pixel row are XOR-swizzled by the pixel index (applied to the DMA SOURCE and to the
// read address) so that the 8 row segments a half-wave reads cover all 64 banks exactly once.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

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

// Up to WGRAD_MAX_GROUP layers of IDENTICAL geometry in one launch (et_conv2d_wgrad_grouped): the K-split that
// fills the chip is then shared by the whole group, so every dW address receives group-size times fewer fp32
// atomics (measured with s_memtime stamps: the atomic epilogue is 23-27 % of a workgroup's lifetime when a
// single 256-channel layer is split 28-64 ways; the L2 atomic rate, ~1 TB/s, does not depend on scope).
#define WGRAD_MAX_GROUP 16
struct WgradItem { const uint16_t* x; const uint16_t* dy; float* dw; int ldx, ldy; };
struct WgradGroup { WgradItem it[WGRAD_MAX_GROUP]; int n; };

template <typename T, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void conv_wgrad_tr_kernel(WgradGroup grp, const uint16_t* __restrict__ ZERO,
                                                                     WgradGeom g) {          // T: the 16-bit format behind the raw pointers
    constexpr int NT = 64 * WM * WN, BKP = 64;       // threads per workgroup; pixels (GEMM-K) per chunk
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int SA = BM / 8, SB = BN / 8;            // 16-byte slots per pixel row of the A / B tile
    constexpr int RPA = NT / SA, RPB = NT / SB;        // pixel rows staged per pass of the workgroup
    constexpr int RA = BKP / RPA, RB = BKP / RPB;      // LDS-DMA instructions per thread per chunk
    constexpr int A_VEC = BKP * SA, B_VEC = BKP * SB;  // tile sizes in 16-byte vectors
    static_assert(BKP % RPA == 0 && BKP % RPB == 0 && RPA >= 1 && RPB >= 1, "staging passes");
    __shared__ __attribute__((aligned(16))) u32x4 lds_raw[2 * (A_VEC + B_VEC)];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    int bid = blockIdx.x;
    if (g.xcd) {
        const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = bid & 7, k = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
    }
    const int per_layer = g.ntn * g.ntm * g.nsk;
    const int layer = __builtin_amdgcn_readfirstlane(bid / per_layer);     // wave-uniform: scalar kernarg loads
    bid -= layer * per_layer;
    const uint16_t* __restrict__ X = grp.it[layer].x;
    const uint16_t* __restrict__ DY = grp.it[layer].dy;
    float* __restrict__ DW = grp.it[layer].dw;
    const int ldx = grp.it[layer].ldx, ldy = grp.it[layer].ldy;
    const int tx = bid % g.ntn, ty = (bid / g.ntn) % g.ntm, tz = bid / (g.ntn * g.ntm);
    const int n0 = tx * BN, m0 = ty * BM;
    const int pk_begin = tz * g.Pper;
    const int pk_end = min(g.P, pk_begin + g.Pper);

    // per-thread staging descriptors: which (pixel row, logical 8-channel group) this lane fetches
    int a_pl[RA], a_co[RA];
    bool a_ok[RA];
#pragma unroll
    for (int j = 0; j < RA; ++j) {
        a_pl[j] = tid / SA + j * RPA;
        const int ls = (tid % SA) ^ tr_swz<SA>(a_pl[j]);
        a_co[j] = m0 + ls * 8;
        a_ok[j] = a_co[j] < g.Cout;                    // Cout % 8 == 0 (host)
    }
    int b_pl[RB], b_ci[RB], b_dy[RB], b_dx[RB];
    bool b_ok[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        b_pl[j] = tid / SB + j * RPB;
        const int ls = (tid % SB) ^ tr_swz<SB>(b_pl[j]);
        const int col = n0 + ls * 8;
        b_ok[j] = col < g.NC;
        const uint32_t cc = b_ok[j] ? col : 0;
        const uint32_t tap = fdiv(cc, g.dCin);
        b_ci[j] = cc - tap * g.Cin;
        b_dy[j] = g.dy[tap];
        b_dx[j] = g.dx[tap];
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    // 1x1 stride-1 layers, buffer form (g.buf, uniform): descriptors over [tensor, end of this K-slice's last row) -- a row at or beyond
    // pk_end is out of range and lands as zeros, a channel group beyond the tensor carries bit 31; the chunk's first row travels in the
    // SGPR offset: no vector instruction per piece (flat form: add, compare, 64-bit multiply-add, select into the zero page)
    et_rsrc rsDY, rsX;
    unsigned a_vo[RA], b_vo[RB];
    if (g.buf) {
        rsDY = et_make_rsrc(DY, (unsigned)(((size_t)(pk_end - 1) * ldy + g.Cout) * 2));
        rsX = et_make_rsrc(X, (unsigned)(((size_t)(pk_end - 1) * ldx + g.NC) * 2));
#pragma unroll
        for (int j = 0; j < RA; ++j) a_vo[j] = a_ok[j] ? (unsigned)((a_pl[j] * ldy + a_co[j]) * 2) : 0x80000000u;
#pragma unroll
        for (int j = 0; j < RB; ++j) b_vo[j] = b_ok[j] ? (unsigned)((b_pl[j] * ldx + b_ci[j]) * 2) : 0x80000000u;
    }
    auto stage = [&](u32x4* dstA, u32x4* dstB, int pk0) {
        u32x4* const wa = dstA + wave * 64;
        u32x4* const wb = dstB + wave * 64;
        if (g.buf) {
            const unsigned sa = (unsigned)((size_t)pk0 * ldy * 2), sb = (unsigned)((size_t)pk0 * ldx * 2);
#pragma unroll
            for (int j = 0; j < RA; ++j) et_bufdma16(rsDY, a_vo[j], sa, wa + j * NT);
#pragma unroll
            for (int j = 0; j < RB; ++j) et_bufdma16(rsX, b_vo[j], sb, wb + j * NT);
            return;
        }
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const int p = pk0 + a_pl[j];
            const bool ok = a_ok[j] && p < pk_end;
            const uint16_t* src = ok ? DY + ((long long)p * ldy + a_co[j]) : ZERO;
            et_glds16(src, wa + j * NT);
        }
        if (g.ident) {
            // 1x1 stride-1 layers (half of the model's weight-gradient launches, all HBM-bound): the X row IS the dY row -- no pixel
            // decode (two divisions by multiplication and four compares per staged row sat in front of every chunk's loads)
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const int p = pk0 + b_pl[j];
                const bool ok = b_ok[j] && p < pk_end;
                const uint16_t* src = ok ? X + ((long long)p * ldx + b_ci[j]) : ZERO;
                et_glds16(src, wb + j * NT);
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            const int p = pk0 + b_pl[j];
            const uint32_t pp = min(p, g.P - 1);
            const uint32_t t1 = fdiv(pp, g.dQW), qx = pp - t1 * g.QW;
            const uint32_t n = fdiv(t1, g.dQH), qy = t1 - n * g.QH;
            const int iy = qy * g.isy + b_dy[j], ix = qx * g.isx + b_dx[j];
            const bool ok = b_ok[j] && p < pk_end && (unsigned)iy < (unsigned)g.IH && (unsigned)ix < (unsigned)g.IW;
            const uint16_t* src = ok ? X + ((((long long)n * g.IH + iy) * g.IW + ix) * ldx + b_ci[j]) : ZERO;
            et_glds16(src, wb + j * NT);
        }
    };

    // fragment addressing (bytes inside one operand tile): lane l reads, for k-step ks and half r,
    // pixel 16*ks + 8*(l>>5) + 4*r + ((l&15)>>2), channels c0 + 16*((l>>4)&1) + 4*(l&3) .. +3
    const int fp = 8 * (lane >> 5) + ((lane & 15) >> 2);
    const int fc = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    auto frag = [&](const char* tile, int slots, int ks, int c0, auto swz) -> s16x8 {
        s16x8 o;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int p = 16 * ks + 4 * r + fp;
            const int ch = c0 + fc;
            const int off = (p * slots + ((ch >> 3) ^ swz(p))) * 16 + (ch & 4) * 2;
            const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(tile + off));
            o[4 * r + 0] = v[0]; o[4 * r + 1] = v[1]; o[4 * r + 2] = v[2]; o[4 * r + 3] = v[3];
        }
        return o;
    };
    auto mma = [&](const u32x4* bufA, const u32x4* bufB) {
        const char* ta = (const char*)bufA;
        const char* tb = (const char*)bufB;
#pragma unroll
        for (int ks = 0; ks < BKP / 16; ++ks) {
            s16x8 af[TM], bf[TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) af[tm] = frag(ta, SA, ks, wm * (BM / WM) + tm * 32, [](int p) { return tr_swz<SA>(p); });
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) bf[tn] = frag(tb, SB, ks, wn * (BN / WN) + tn * 32, [](int p) { return tr_swz<SB>(p); });
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc[tm][tn] = et_mfma32<T>(af[tm], bf[tn], acc[tm][tn]);
        }
    };

    u32x4* const A0 = lds_raw;
    u32x4* const B0 = lds_raw + A_VEC;
    u32x4* const A1 = lds_raw + A_VEC + B_VEC;
    u32x4* const B1 = A1 + A_VEC;
    const int nchunks = (pk_end - pk_begin + BKP - 1) / BKP;
    if (nchunks > 0) stage(A0, B0, pk_begin);
    et_wait_vmem();
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const bool odd = c & 1;
        if (c + 1 < nchunks) stage(odd ? A0 : A1, odd ? B0 : B1, pk_begin + (c + 1) * BKP);
        mma(odd ? A1 : A0, odd ? B1 : B0);
        et_wait_vmem();
        __syncthreads();
    }
    if (nchunks <= 0) return;
    const int l31 = lane & 31, hi = lane >> 5;
    if (m0 + BM <= g.Cout && n0 + BN <= g.NC) {
        // interior tile: no per-lane guards (they compiled to an exec-mask save + branch around EVERY atomic: 12 instructions
        // per atomic), one row pointer per accumulator row, the column tiles as immediate offsets
        float* const base = DW + ((size_t)(m0 + wm * (BM / WM) + 4 * hi) * g.NC + n0 + wn * (BN / WN) + l31);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float* const rowp = base + (size_t)(tm * 32 + (r & 3) + 8 * (r >> 2)) * g.NC;
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) atomicAdd(rowp + tn * 32, acc[tm][tn][r]);
            }
    } else {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = m0 + wm * (BM / WM) + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    const int col = n0 + wn * (BN / WN) + tn * 32 + l31;
                    if (co < g.Cout && col < g.NC) atomicAdd(DW + ((size_t)co * g.NC + col), acc[tm][tn][r]);
                }
            }
    }
}

// ---- weight gradient of the stem (6x6 stride 2 pad 2) from dY and the uint8 image planes ------------------------------------------
// The generic kernels run this layer on the packed image: GEMM-N = 36 taps x 8 channels = 288 columns of which 108 are real, and the
// packed tensor is gathered once per tap.  Here the image never exists in packed form.  One (persistent) workgroup owns 4 x 64 output
// pixels at a time, the forward's tile:
//   * dY (256 pixels x 64 channels) arrives by LDS-DMA in its natural [pixel][channel] order, double buffered, and is read as the
//     K(=pixel)-contiguous MFMA A operand with ds_read_b64_tr_b16, exactly as conv_wgrad_tr_kernel does;
//   * the input patch (12 x 136 pixels) is built ONCE per tile from the uint8 planes through the forward's table (stem_u8_fill_lut: the
//     same bits as the packed tensor), 8 bytes per pixel: r, g, b, 0.  The same transposing read then delivers the B operand straight
//     from it: of a 16-lane group, lane 4j + t fetches the 8 bytes of the input pixel that tap t meets at output pixel j, and lane
//     4t + c receives channel c of tap t for the four pixels.  GEMM-N = 36 taps x 4 channels = 144 (five 32-column blocks, half of
//     the last one idle); every tap reads the patch at a constant offset -- nothing is staged per tap;
//   * wave w reduces over output row w of the tile into a full 64 x 160 accumulator set that lives for the whole grid-stride loop; the
//     four sets meet in LDS at the end and ONE wave adds the real columns (channel < 3, tap < 36) into dW [cout][ky][kx][8] with fp32
//     atomics: one addition per workgroup and address, the pad slots are never touched.
// HBM traffic: dY once plus 1.5 x the image bytes (row halo), against the packed path's nine-fold gather of a 16-byte pixel.
#define SWG_PITCH 136                   // patch columns: 34 quads, column 0 = input column 2 * ox0 - 4
#define SWG_DYV (256 * 8)               // dY tile in 16-byte slots
struct StemWgradArgs {
    const uint8_t* seg[STEM_MAX_SEGS]; int seg_b[STEM_MAX_SEGS]; float norm;
    const uint16_t* dy; const uint16_t* zero; float* dw;
    int N, IH, IW, OH, OW, ldy, Cout;
    int trn, tcn, ntiles;
};

template <typename T>
__global__ __launch_bounds__(256, 2) void conv_stem_u8_wgrad_kernel(StemWgradArgs a) {
    __shared__ __attribute__((aligned(16))) u32x4 dyl[2 * SWG_DYV];                   // 64 KB; the cross-wave reduction reuses it
    __shared__ __attribute__((aligned(16))) u32x4 xl[STEM_PH * SWG_PITCH / 2];        // 8 bytes per pixel
    __shared__ uint16_t lut[256];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    stem_u8_fill_lut<T>(lut, tid, a.norm);

    // ---- staging roles (constant over tiles)
    int q_row[2], q_col[2];
    unsigned q_px[2][3];
    bool q_in[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = i * 256 + tid;
        q_row[i] = q < STEM_NQ ? q / STEM_QPR : -100000;
        q_col[i] = q % STEM_QPR;
        q_in[i] = false;
#pragma unroll
        for (int c = 0; c < 3; ++c) q_px[i][c] = 0u;
    }
    auto load_u8 = [&](int tile) {
        const int tc = tile % a.tcn, t2 = tile / a.tcn;
        const int tr = t2 % a.trn, n = t2 / a.trn;
        const int iy0 = 2 * tr * STEM_TR - 2, ix0 = 2 * tc * STEM_TC - 4;
        const uint8_t* const img = stem_u8_image(a, n);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int iy = iy0 + q_row[i], ix = ix0 + 4 * q_col[i];
            q_in[i] = (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                q_px[i][c] = q_in[i] ? *(const unsigned*)(img + ((size_t)c * a.IH + iy) * a.IW + ix) : 0u;
        }
    };
    auto write_patch = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (q_row[i] < 0) continue;
            unsigned w[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned r = lut[(q_px[i][0] >> (8 * j)) & 0xffu], g = lut[(q_px[i][1] >> (8 * j)) & 0xffu];
                const unsigned b = lut[(q_px[i][2] >> (8 * j)) & 0xffu];
                w[2 * j] = q_in[i] ? (r | (g << 16)) : 0u;
                w[2 * j + 1] = q_in[i] ? b : 0u;
            }
            u32x4* const d = xl + (q_row[i] * SWG_PITCH + 4 * q_col[i]) / 2;
            d[0] = mk4(w[0], w[1], w[2], w[3]);
            d[1] = mk4(w[4], w[5], w[6], w[7]);
        }
    };
    // dY slot i * 256 + tid: pixel slot >> 3 of the tile (row-major 4 x 64), physical 16-byte slot & 7 = channel group ^ swizzle
    auto stage_dy = [&](int tile, int buf) {
        const int tc = tile % a.tcn, t2 = tile / a.tcn;
        const int tr = t2 % a.trn, n = t2 / a.trn;
        const int oy0 = tr * STEM_TR, ox0 = tc * STEM_TC;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int slot = i * 256 + tid, p = slot >> 3;
            const int co = ((slot & 7) ^ tr_swz<8>(p)) * 8;
            const int oy = oy0 + (p >> 6), ox = ox0 + (p & 63);
            const bool ok = oy < a.OH && ox < a.OW && co < a.Cout;
            const uint16_t* src = ok ? a.dy + ((((size_t)n * a.OH + oy) * a.OW + ox) * a.ldy + co) : a.zero;
            et_glds16(src, dyl + buf * SWG_DYV + i * 256 + wave * 64);
        }
    };

    // ---- fragment addressing.  A (dY) as conv_wgrad_tr_kernel: address role = pixel 8*(l>>5) + ((l&15)>>2), channels 16*((l>>4)&1) + 4*(l&3)..+3.
    // B (patch): address role = pixel j = (l&15)>>2 (+ 8*(l>>5)), tap 8*nb + 4*((l>>4)&1) + (l&3); the lane RECEIVES column l31 = 4 * (tap - 8*nb) + channel
    const int fp = 8 * hi + ((lane & 15) >> 2);
    const int fc = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    int boff[5];
#pragma unroll
    for (int nb = 0; nb < 5; ++nb) {
        const int tap = min(8 * nb + 4 * ((lane >> 4) & 1) + (lane & 3), 35);        // columns of taps >= 36 are computed on tap 35 and dropped
        const int ky = tap / 6, kx = tap - 6 * ky;
        boff[nb] = (((2 * wave + ky) * SWG_PITCH) + kx + 2 + 2 * fp) * 8;
    }
    f32x16 acc[2][5];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 5; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;

    __syncthreads();                     // the table
    if ((int)blockIdx.x < a.ntiles) { load_u8(blockIdx.x); stage_dy(blockIdx.x, 0); }
    int it = 0;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x, ++it) {
        write_patch();                   // every wave left the previous patch at the barrier that ends the loop body
        et_wait_vmem();                  // this tile's dY has landed
        __syncthreads();
        // the next tile's bytes travel behind this tile's MFMAs: the image quads in registers (issued first: the table pass waits for them
        // alone), dY into the buffer the PREVIOUS tile read (all waves are past its reads: the barrier above)
        if (tile + (int)gridDim.x < a.ntiles) { load_u8(tile + gridDim.x); stage_dy(tile + gridDim.x, (it + 1) & 1); }
        const char* const ta = (const char*)(dyl + (it & 1) * SWG_DYV);
        const char* const tb = (const char*)xl;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            s16x8 af[2], bf[5];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int p = wave * 64 + 16 * ks + 4 * r + fp;
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    const int ch = mb * 32 + fc;
                    const int off = (p * 8 + ((ch >> 3) ^ tr_swz<8>(p))) * 16 + (ch & 4) * 2;
                    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(ta + off));
                    af[mb][4 * r + 0] = v[0]; af[mb][4 * r + 1] = v[1]; af[mb][4 * r + 2] = v[2]; af[mb][4 * r + 3] = v[3];
                }
#pragma unroll
                for (int nb = 0; nb < 5; ++nb) {
                    const int off = boff[nb] + 2 * (16 * ks + 4 * r) * 8;
                    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(tb + off));
                    bf[nb][4 * r + 0] = v[0]; bf[nb][4 * r + 1] = v[1]; bf[nb][4 * r + 2] = v[2]; bf[nb][4 * r + 3] = v[3];
                }
            }
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 5; ++nb)
                    acc[mb][nb] = et_mfma32<T>(af[mb], bf[nb], acc[mb][nb]);
        }
        __syncthreads();
    }
    // ---- the four waves' partial sums meet in wave 0 (LDS, one wave at a time), which adds the real columns into dW
    et_wait_vmem();
    float* const red = (float*)dyl;       // [160 registers][64 lanes]
#pragma unroll 1
    for (int w = 1; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 5; ++nb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[((mb * 5 + nb) * 16 + r) * 64 + lane] = acc[mb][nb][r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 5; ++nb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[mb][nb][r] += red[((mb * 5 + nb) * 16 + r) * 64 + lane];
        }
    }
    if (wave != 0 || (l31 & 3) == 3) return;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = mb * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
#pragma unroll
            for (int nb = 0; nb < 5; ++nb) {
                const int tap = 8 * nb + (l31 >> 2);
                if (co < a.Cout && tap < 36) atomicAdd(a.dw + ((size_t)co * 36 + tap) * 8 + (l31 & 3), acc[mb][nb][r]);
            }
        }
}

// ---- weight gradient of the 3x3 stride-1 layers with BOTH operands shared by the three taps of a kernel row ------------------
// conv_wgrad_tr_kernel computes one (cout tile, tap, cin tile) per workgroup: dY is staged nine times and X nine times per pixel
// chunk of a layer.  The three taps of a kernel row multiply the SAME dY rows with X rows shifted by one pixel, so here a
// workgroup owns (cout tile) x (kernel row j) x (cin tile) = three dW tiles (accumulator sets) and stages per K-chunk ONE dY
// tile and ONE X tile with two extra rows; tap k reads its B fragments k rows further down.  GEMM-K runs over the PADDED raster
// (index Yg * (W + 1) + x, one zero slot after every image row, in BOTH operands): a dY pad row contributes nothing, and
// x - 1 / x + 1 of a row's first / last pixel is the X pad slot -- no masks (conv_gemm_rs_kernel's layout).  Per 64-slot chunk:
// 64 + 72 rows staged for three taps instead of 3 * (64 + 64); fragment bases per (tap, lane) are precomputed, the k-step and the
// row half are immediates (the swizzle only depends on the row modulo 4, which 16*ks + 4*r does not change).
// STRIDE 2 (r04; 3x3 stride-2 pad-1 layers, even input size): the K axis is the padded raster of dY (= the OUTPUT lattice), and the taps
// of a kernel row read input columns 2x - 1, 2x, 2x + 1.  The X tile therefore holds TWO rows per K-slot: row 2j = input column
// 2x(j) - 1, row 2j + 1 = input column 2x(j) of slot j's pixel; tap k of slot j reads row 2j + k -- and row 2j + 2 (tap 2) IS row
// 2(j + 1) + 0: column 2x + 1 of a pixel is column 2(x + 1) - 1 of its right neighbour.  At a row end the neighbour is the pad slot
// (dY = 0 there, so what it multiplies does not matter) and the slot after it starts the next image row, whose tap 0 reads column -1:
// zero page.  One dY tile + one X tile of 129 rows per 64-slot chunk serve three taps (the per-tap kernel staged 3 x 64 X rows and ran
// these six layers at 340-700 TFLOP/s against the stride-1 kernel's ~1000).
template <typename T, int BM, int BNC, int WM, int WN, int STRIDE = 1>
__global__ __launch_bounds__(64 * WM * WN) ET_WAVES_PER_EU(STRIDE == 1 ? 4 : 2) void conv_wgrad_rs_kernel(WgradGroup grp, const uint16_t* __restrict__ ZERO, WgradGeom g) {
    constexpr int NT = 64 * WM * WN, BKP = 64, BROWS = STRIDE == 1 ? 72 : 136;      // threads; padded slots per chunk; X rows per chunk (66 / 129 used)
    constexpr int TM = BM / WM / 32, TN = BNC / WN / 32;
    constexpr int SA = BM / 8, SB = BNC / 8;                     // 16-byte slots per row of the A / B tile
    constexpr int RPA = NT / SA, RPB = NT / SB;                  // rows staged per pass of the workgroup
    constexpr int RA = BKP / RPA, RB = (BROWS + RPB - 1) / RPB;  // LDS-DMA instructions per thread per chunk (the last B pass partial)
    constexpr int A_VEC = BKP * SA, B_VEC = BROWS * SB;          // (the partial last B pass only writes rows < BROWS)
    static_assert(RPA >= 1 && RPB >= 8 && TM >= 1 && TN >= 1 && (BROWS * SB) % 64 == 0 && RB * RPB > BKP, "staging passes");
    __shared__ __attribute__((aligned(16))) u32x4 lds_raw[2 * (A_VEC + B_VEC)];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    int bid = blockIdx.x;
    if (g.xcd) {
        const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = bid & 7, k = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
    }
    const int per_layer = g.ntn * g.ntm * g.nsk;
    const int layer = __builtin_amdgcn_readfirstlane(bid / per_layer);
    bid -= layer * per_layer;
    const uint16_t* __restrict__ X = grp.it[layer].x;
    const uint16_t* __restrict__ DY = grp.it[layer].dy;
    float* __restrict__ DW = grp.it[layer].dw;
    const int ldx = grp.it[layer].ldx, ldy = grp.it[layer].ldy;
    const int tx = bid % g.ntn, ty = (bid / g.ntn) % g.ntm, tz = bid / (g.ntn * g.ntm);
    const int nci = g.ntn / 3;                       // column tiles = 3 kernel rows x cin tiles
    const int jrow = tx / nci, c0 = (tx - jrow * nci) * BNC, m0 = ty * BM;
    const int dyr = jrow - 1;                        // image-row offset of this kernel row (pad 1)
    const int W1 = g.QW + 1;
    const int k_begin = tz * g.Pper;                 // padded slots [k_begin, k_end)
    const int k_end = min(g.PP, k_begin + g.Pper);

    static_assert(BKP % RPA == 0 && BKP % RPB == 0 && RPA % 4 == 0 && RPB % (4 * STRIDE) == 0, "pieces are whole row groups; the swizzle repeats every 4 (8) rows");
    // this lane's rows: A piece j = LDS row a_pl0 + j*RPA, B piece j = row b_pl0 + j*RPB; the 8-channel group is the same for all of them
    const int a_pl0 = tid / SA, b_pl0 = tid / SB;
    const int a_co = m0 + ((tid % SA) ^ tr_swz<SA>(a_pl0)) * 8;
    const int b_ci = c0 + ((tid % SB) ^ (STRIDE == 1 ? tr_swz<SB>(b_pl0) : tr_swz2<SB>(b_pl0))) * 8;
    const bool a_okc = a_co < g.Cout, b_okc = b_ci < g.Cin;

    // Padded coordinates (image row counted through the batch, column) of piece 0's row, kept across chunks: the pieces of a chunk
    // are RPA / RPB slots apart and a chunk is a whole number of pieces, so stepping piece to piece IS the advance to the next chunk
    // -- no division in the loop (two per staged row and chunk were ~100 of the ~170 staging instructions of a chunk, four waves per
    // SIMD deep: as much VALU time as the MFMAs take).  Host guarantees 64 / (QW + 1) + 2 <= QH: one subtraction wraps the image row.
    constexpr int SPB = RPB / STRIDE;              // K-slots a B piece advances (stride 2: two X rows per slot)
    const int qa = RPA / W1, ra = RPA - qa * W1, qb = SPB / W1, rb = SPB - qb * W1;   // uniform
    const int b_par = STRIDE == 1 ? 0 : (b_pl0 & 1);   // stride 2: this lane's X rows are all even (column 2x - 1) or all odd (column 2x)
    int a_yg, a_xp, b_yg, b_xp, b_qy;              // b_yg = -1 for the slot before the first (X row r <-> slot k0 - 1 + r)
    {
        const uint32_t sl = k_begin + a_pl0;
        a_yg = fdiv(sl, g.dW1);
        a_xp = sl - a_yg * W1;
        // stride 1: X row r <-> slot k0 - 1 + r; stride 2: X row r <-> slot k0 + r / 2
        const uint32_t s1 = (STRIDE == 1 ? k_begin - 1 + b_pl0 : k_begin + (b_pl0 >> 1)) + W1;       // one padded row further down: never negative
        const uint32_t yg1 = fdiv(s1, g.dW1);
        b_xp = s1 - yg1 * W1;
        b_yg = (int)yg1 - 1;
        const int q1 = yg1 - fdiv(yg1, g.dQH) * g.QH;
        b_qy = q1 == 0 ? g.QH - 1 : q1 - 1;
    }

    f32x16 acc[3][TM][TN];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[k][tm][tn][r] = 0.f;

    // stage the chunk the row coordinates currently point at (k0 = its first slot) and leave them at the next chunk
    auto stage = [&](u32x4* dstA, u32x4* dstB, int k0) {
        u32x4* const wa = dstA + wave * 64;
        u32x4* const wb = dstB + wave * 64;
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const bool ok = a_okc && k0 + a_pl0 + j * RPA < k_end && a_xp < g.QW;
            const uint16_t* src = ok ? DY + ((size_t)(unsigned)((a_yg * g.QW + a_xp) * ldy + a_co)) : ZERO;   // host: tensors < 2^31 elements
            et_glds16(src, wa + j * NT);
            a_xp += ra; a_yg += qa;
            if (a_xp >= W1) { a_xp -= W1; a_yg += 1; }
        }
        int yg = b_yg, xp = b_xp, qy = b_qy;
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            if (j * RPB == BKP * STRIDE) { b_yg = yg; b_xp = xp; b_qy = qy; }                       // piece 0 of the next chunk
            if (RB * RPB > BROWS && j == RB - 1 && wave * 64 >= (BROWS - j * RPB) * SB) continue;   // wave-uniform: the partial pass
            bool ok;
            const uint16_t* src;
            if constexpr (STRIDE == 1) {
                ok = b_okc && yg >= 0 && k0 - 1 + b_pl0 + j * RPB < g.PP && b_pl0 + j * RPB < BROWS && xp < g.QW &&
                     (unsigned)(qy + dyr) < (unsigned)g.IH;
                src = ok ? X + ((size_t)(unsigned)((yg * g.QW + xp + dyr * g.IW) * ldx + b_ci)) : ZERO;
            } else {
                // slot (yg, xp) of the OUTPUT raster (xp == QW: the pad slot, whose even row is the previous pixel's column 2x + 1):
                // input row 2 * yg + dyr (IH = 2 * QH: image rows stay aligned through the batch), input column 2 * xp - 1 + parity
                const int col = 2 * xp - 1 + b_par, iy = 2 * qy + dyr;
                ok = b_okc && yg >= 0 && k0 + ((b_pl0 + j * RPB) >> 1) < g.PP + 1 && b_pl0 + j * RPB < BROWS && xp <= g.QW &&
                     (unsigned)col < (unsigned)g.IW && (unsigned)iy < (unsigned)g.IH && yg < g.N * g.QH;
                src = ok ? X + ((size_t)(unsigned)(((2 * yg + dyr) * g.IW + col) * ldx + b_ci)) : ZERO;
            }
            et_glds16(src, wb + j * NT);
            int dq = qb;
            xp += rb;
            if (xp >= W1) { xp -= W1; dq += 1; }
            yg += dq; qy += dq;
            if (qy >= g.QH) qy -= g.QH;
        }
    };

    // fragment bases (bytes inside an operand tile); k-step ks and row half r add (16*ks + 4*r) rows as an immediate
    const int fp = 8 * (lane >> 5) + ((lane & 15) >> 2);
    const int fc = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    int abase[TM], bbase[3][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
        const int ch = wm * (BM / WM) + tm * 32 + fc;
        abase[tm] = (fp * SA + ((ch >> 3) ^ tr_swz<SA>(fp))) * 16 + (ch & 4) * 2;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int ch = wn * (BNC / WN) + tn * 32 + fc;
            const int row = STRIDE * fp + k;                       // K-slot fp of the k-step, tap k
            bbase[k][tn] = (row * SB + ((ch >> 3) ^ (STRIDE == 1 ? tr_swz<SB>(row) : tr_swz2<SB>(row)))) * 16 + (ch & 4) * 2;
        }
    auto frag = [&](const char* tile, int base, int row_bytes, int ks) -> s16x8 {      // row_bytes: bytes per K-SLOT (stride 2: two rows)
        s16x8 o;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) s16x4*)(tile + base + (16 * ks + 4 * r) * row_bytes));
            o[4 * r + 0] = v[0]; o[4 * r + 1] = v[1]; o[4 * r + 2] = v[2]; o[4 * r + 3] = v[3];
        }
        return o;
    };
    auto mma = [&](const u32x4* bufA, const u32x4* bufB) {
        const char* ta = (const char*)bufA;
        const char* tb = (const char*)bufB;
#pragma unroll
        for (int ks = 0; ks < BKP / 16; ++ks) {
            s16x8 af[TM], bf[3][TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) af[tm] = frag(ta, abase[tm], SA * 16, ks);
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) bf[k][tn] = frag(tb, bbase[k][tn], STRIDE * SB * 16, ks);
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
                        acc[k][tm][tn] = et_mfma32<T>(af[tm], bf[k][tn], acc[k][tm][tn]);
        }
    };

    u32x4* const A0 = lds_raw;
    u32x4* const B0 = lds_raw + A_VEC;
    u32x4* const A1 = lds_raw + A_VEC + B_VEC;
    u32x4* const B1 = A1 + A_VEC;
    const int nchunks = (k_end - k_begin + BKP - 1) / BKP;
    if (nchunks <= 0) return;
    stage(A0, B0, k_begin);
    et_wait_vmem();
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const bool odd = c & 1;
        if (c + 1 < nchunks) stage(odd ? A0 : A1, odd ? B0 : B1, k_begin + (c + 1) * BKP);
        mma(odd ? A1 : A0, odd ? B1 : B0);
        et_wait_vmem();
        __syncthreads();
    }
    const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float* const tapbase = DW + (size_t)(jrow * 3 + k) * g.Cin + c0;      // dW[co][tap][ci]: row pitch NC = 9 * Cin
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = m0 + wm * (BM / WM) + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    const int ci = wn * (BNC / WN) + tn * 32 + l31;
                    if (co < g.Cout && c0 + ci < g.Cin) atomicAdd(tapbase + (size_t)co * g.NC + ci, acc[k][tm][tn][r]);
                }
            }
    }
}

// ---- small helpers ---------------------------------------------------------------------------------
// W [Cout][TT][Cin] -> WT [Cin][TT][Cout]  (operand of dgrad)
template <typename T>
__global__ __launch_bounds__(256) void weight_transpose_kernel(const T* __restrict__ w, T* __restrict__ wt, int Cout,
                                                               int TT, int Cin, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // index into wt
    if (i >= n) return;
    const int co = i % Cout;
    const int t = (i / Cout) % TT;
    const int ci = i / ((long long)Cout * TT);
    wt[i] = w[((long long)co * TT + t) * Cin + ci];
}

// All layers of the flat weight arena in ONE launch: table[l] = {element offset of layer l in the arena (the same
// in the transposed arena), Cout, TT, Cin}, sorted by offset; every thread finds its layer by bisection (the
// table is a few hundred bytes and stays in cache).  Replaces ~100 per-layer launches per training step.
template <typename T>
__global__ __launch_bounds__(256) void weight_transpose_all_kernel(const T* __restrict__ w, T* __restrict__ wt,
                                                                   const int* __restrict__ table, int nlayers, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    // the layer of the wave's first element, found once per wave (scalar bisection); lanes that already belong to
    // the next layer step forward linearly (layers are far longer than a wave)
    const long long i0 = __builtin_amdgcn_readfirstlane((int)((i >> 6) & 0x7fffffff)) * 64ll;
    if (i >= total) return;
    int lo = 0, hi = nlayers - 1;
    while (lo < hi) {                                      // largest l with table[l].off <= i0
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)(unsigned)table[mid * 4] <= i0) lo = mid; else hi = mid - 1;
    }
    while (lo + 1 < nlayers && (long long)(unsigned)table[(lo + 1) * 4] <= i) ++lo;
    const long long off = (unsigned)table[lo * 4];
    const int Cout = table[lo * 4 + 1], TT = table[lo * 4 + 2], Cin = table[lo * 4 + 3];
    const long long j = i - off;                           // index into this layer's wt
    if (j >= (long long)Cout * TT * Cin) return;           // alignment gap between layers
    const int co = j % Cout;
    const int t = (j / Cout) % TT;
    const int ci = j / ((long long)Cout * TT);
    wt[off + j] = w[off + ((long long)co * TT + t) * Cin + ci];
}

// bf16 form of the same operation in 8x8 register blocks: one thread reads eight 16-byte rows of w (8 input channels of 8
// consecutive output channels), transposes the block in registers and writes eight 16-byte rows of wt.  A wave covers a 64 x 64
// tile (lane = 8 * (cout block) + (cin block): every read instruction is eight 128-byte segments); a workgroup takes four tiles
// per iteration, workgroup (bx, layer) walks tiles bx, bx + gridDim.x, ... of its layer.  The element-per-thread kernel above
// gathers 2-byte values at a stride of a whole weight row: 240 us per step for the 92 MB of YOLOv5l against ~40 us of traffic.
__global__ __launch_bounds__(256) void weight_transpose_all_tiled_kernel(const uint16_t* __restrict__ w, uint16_t* __restrict__ wt,
                                                                         const int* __restrict__ table, int nlayers) {
    const int layer = blockIdx.y;
    const long long off = (unsigned)table[layer * 4];
    const int Cout = table[layer * 4 + 1], TT = table[layer * 4 + 2], Cin = table[layer * 4 + 3];
    if ((Cout | Cin) & 7) {
        // channels that are not whole 16-byte rows (no layer of the models here: bf16 slots are padded to 8): element by element
        const long long n = (long long)Cout * TT * Cin;
        for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
            const int co = (int)(j % Cout), t = (int)((j / Cout) % TT), ci = (int)(j / ((long long)Cout * TT));
            wt[off + j] = w[off + ((long long)co * TT + t) * Cin + ci];
        }
        return;
    }
    const int tco = (Cout + 63) >> 6, tci = (Cin + 63) >> 6;
    const int ntiles = TT * tco * tci;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int a = lane >> 3, b = lane & 7;
    const uint16_t* const wl = w + off;
    uint16_t* const wtl = wt + off;
    for (int tile = (blockIdx.x * 4 + wave); tile < ntiles; tile += gridDim.x * 4) {
        const int ic = tile % tci, r1 = tile / tci;
        const int oc = r1 % tco, t = r1 / tco;
        const int co = oc * 64 + a * 8, ci = ic * 64 + b * 8;
        if (co >= Cout || ci >= Cin) continue;                 // whole 8x8 blocks are in or out (channels are multiples of 8)
        u32x4 in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = *(const u32x4*)(wl + ((long long)(co + r) * TT + t) * Cin + ci);
        Transposer<uint16_t>::run(in, out);
#pragma unroll
        for (int c = 0; c < 8; ++c) *(u32x4*)(wtl + ((long long)(ci + c) * TT + t) * Cout + co) = out[c];
    }
}

// column sums of a [P][C] (pixel stride ld) tensor into fp32 out[C] (atomicAdd): bias gradients
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ x, int P, int C, int ld, int rows_per_block,
                                                     float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int p0 = blockIdx.y * rows_per_block, p1 = min(P, p0 + rows_per_block);
    float s = 0.f;
    for (int p = p0; p < p1; ++p) s += et_elem<T>::ld(x[(long long)p * ld + c]);
    atomicAdd(out + c, s);
}

// ---- host side -------------------------------------------------------------------------------------
// bf16 column sums with 16-byte loads: a thread owns one 8-channel vector and every (256 / CV)-th row of its block's rows (the
// element-per-thread kernel above moves 128 bytes per wave instruction: 88 us for the 210 MB of the stride-8 Detect gradient)
template <typename T>
__global__ __launch_bounds__(256) void colsum_vec8_kernel(const T* __restrict__ x, int P, int CV, int ld, int rows_per_block,
                                                          float* __restrict__ out) {
    __shared__ float red[256][9];
    const int rgs = 256 / CV;                                // row groups per block (CV divides 256: host)
    const int cv = threadIdx.x % CV, rg = threadIdx.x / CV;
    const int p0 = blockIdx.x * rows_per_block, p1 = min(P, p0 + rows_per_block);
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    if (rg < rgs) {
        int p = p0 + rg;
        for (; p + rgs < p1; p += 2 * rgs) {                 // two rows in flight
            const u32x4 a = *(const u32x4*)(x + (long long)p * ld + cv * 8), b = *(const u32x4*)(x + (long long)(p + rgs) * ld + cv * 8);
            const unsigned wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[2 * j] += et_lp<T>::lo(wa[j]) + et_lp<T>::lo(wb[j]);
                s[2 * j + 1] += et_lp<T>::hi(wa[j]) + et_lp<T>::hi(wb[j]);
            }
        }
        for (; p < p1; p += rgs) {
            const u32x4 a = *(const u32x4*)(x + (long long)p * ld + cv * 8);
            const unsigned wa[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) { s[2 * j] += et_lp<T>::lo(wa[j]); s[2 * j + 1] += et_lp<T>::hi(wa[j]); }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[threadIdx.x][e] = rg < rgs ? s[e] : 0.f;
    __syncthreads();
    // thread t < 8 * CV: channel t, summed over the row groups
    for (int c = threadIdx.x; c < CV * 8; c += 256) {
        float t = 0.f;
        for (int g = 0; g < rgs; ++g) t += red[g * CV + (c >> 3)][c & 7];
        atomicAdd(out + c, t);
    }
}

// ---- host layer -------------------------------------------------------------------------------------------------------------
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static int device_cus() {
    static const int n_cu = [] { hipDeviceProp_t p; int d = 0; return (hipGetDevice(&d) == hipSuccess && hipGetDeviceProperties(&p, d) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256; }();
    return n_cu;
}

// f(TypeTag<T>) for the storage type of an ET_* dtype; false for any other value (launch_gemm / launch_wgrad: all three types)
template <typename T> struct TypeTag { using type = T; };
template <typename F> static bool with_dtype(int dtype, F&& f) {
    if (dtype == ET_F32) f(TypeTag<float>{}); else if (dtype == ET_BF16) f(TypeTag<uint16_t>{}); else if (dtype == ET_F16) f(TypeTag<et_f16>{}); else return false;
    return true;
}

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
enum { GEMM_REG = 0, GEMM_GLDS = 1, GEMM_PP = 2, GEMM_RS = 3, GEMM_PPRS = 4, GEMM_S1 = 5 };

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

// ---- the instantiations: ONE row list per kernel family (a row = the template arguments after T) --------------------------------
// Each list is expanded twice: into a table of GemmPlan rows, which the plan functions search and plan_name / s1_grid / the
// statistics-row count read, and into launch_gemm's dispatch, which instantiates the row at the same index.  A plan IS a pointer to a
// table row: the name reported and the kernel launched cannot describe different tuples.
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
#define ET_S1(KC_, WN_, TN_, WM_, TMW_, NS_, WGS_, FULL_) {GEMM_S1, 32 * TMW_ * WM_, 32 * TN_ * WN_, WM_, WN_, 8, NS_, true, WGS_, KC_, TN_, FULL_},
#define ET_GLDS(BM_, BN_, WM_, WN_, BKV_, NS_, UT_) {GEMM_GLDS, BM_, BN_, WM_, WN_, BKV_, NS_, UT_, 0, 0, 0, 0},
#define ET_REG(BM_, BN_, WM_, WN_, BKV_, UT_) {GEMM_REG, BM_, BN_, WM_, WN_, BKV_, 2, UT_, 0, 0, 0, 0},
#define ET_RS(BM_, BN_, WM_, WN_) {GEMM_RS, BM_, BN_, WM_, WN_, 8, 2, true, 0, 0, 0, 0},
static const GemmPlan s1_rows[] = {ET_S1_ROWS};
static const GemmPlan glds_rows[] = {ET_GLDS_ROWS};
static const GemmPlan reg_rows[] = {ET_REG_ROWS};
static const GemmPlan rs_rows[] = {ET_RS_ROWS};
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
static int s1_grid(int ntm, const GemmPlan& p) {
    int n = env_int("ET_CONV_S1_WGS", p.wgs * device_cus());
    if (n < 1) n = 1;
    return n < ntm ? n : ntm;
}

template <typename T>
static int launch_gemm(const void* X, const void* W, void* Y, const void* zero16, GatherGeom g, const Epilogue& ep,
                       hipStream_t s) {
    if (g.M <= 0) return 0;
    g.nfast = 1;
    const GemmPlan* const pp = plan_gemm(g, (int)sizeof(T), zero16 != nullptr, ep.res != nullptr || ep.accumulate || ep.bn_y != nullptr);
    if (!pp) return -2;
    const GemmPlan& p = *pp;
    g.ntm = (g.M + p.BM - 1) / p.BM;
    g.ntn = (g.Cout + p.BN - 1) / p.BN;
    const T* x = (const T*)X; const T* w = (const T*)W; T* y = (T*)Y; const T* z = (const T*)zero16;
    const dim3 grid(g.ntm * g.ntn), block(64 * p.WM * p.WN);
    // the row lists again, as launches: expansion i instantiates row i of the family's table, and the plan points at its row
    int i = 0;
#define ET_TWINS(BUF_, GRID_, KERN_, FLAT_) \
    { if (BUF_) hipLaunchKernelGGL(KERN_, GRID_, block, 0, s, x, w, y, z, g, ep); else hipLaunchKernelGGL(FLAT_, GRID_, block, 0, s, x, w, y, z, g, ep); return 0; }
    if (p.kind == GEMM_REG) {
#define ET_REG(BM_, BN_, WM_, WN_, BKV_, UT_) \
    if (pp == &reg_rows[i++]) { hipLaunchKernelGGL((conv_gemm_kernel<T, BM_, BN_, WM_, WN_, BKV_, UT_>), grid, block, 0, s, x, w, y, g, ep); return 0; }
        ET_REG_ROWS
#undef ET_REG
    }
    if (p.kind == GEMM_GLDS) {
#define ET_GLDS(BM_, BN_, WM_, WN_, BKV_, NS_, UT_) \
    if constexpr (NS_ == 2 || sizeof(T) == 2) if (pp == &glds_rows[i]) { hipLaunchKernelGGL((conv_gemm_glds_kernel<T, BM_, BN_, WM_, WN_, BKV_, NS_, UT_>), grid, block, 0, s, x, w, y, z, g, ep); return 0; } \
    ++i;
        ET_GLDS_ROWS
#undef ET_GLDS
    }
    if constexpr (sizeof(T) == 2) {
        if (p.kind == GEMM_S1) {
            const dim3 sgrid(s1_grid(g.ntm, p));
            const bool s1buf = env_int("ET_CONV_BUF_DMA", 1) && (size_t)g.M * g.ldx * sizeof(T) < (1ull << 31);
#define ET_S1(KC_, WN_, TN_, WM_, TMW_, NS_, WGS_, FULL_) \
    if (pp == &s1_rows[i++]) ET_TWINS(s1buf, sgrid, (conv1x1_stream_kernel<T, KC_, WN_, TN_, WM_, TMW_, NS_, WGS_, FULL_>), (conv1x1_stream_flat_kernel<T, KC_, WN_, TN_, WM_, TMW_, NS_, WGS_, FULL_>))
            ET_S1_ROWS
#undef ET_S1
        }
        if (p.kind == GEMM_PP) {
            hipLaunchKernelGGL((conv_gemm_pp_kernel<T>), grid, block, 0, s, x, w, y, z, g, ep);
            return 0;
        }
        if (p.kind == GEMM_PPRS || p.kind == GEMM_RS) {
            // LDS-DMA pieces through buffer descriptors (et_bufdma16) unless an operand reaches 2^31 bytes (bit 31 of a lane's offset means
            // "out of range") or ET_CONV_BUF_DMA=0 asks for the flat-address twins.  On the step: -0.4 ms in 20- and 100-step runs
            // (profiles/r06_buffer_dma_default_ab.txt).  (The arm was withdrawn for a day of this round: conv_gemm_rs_kernel<128, 64> produced
            // wrong wave tiles with it -- an LDS-ring WAR race of the single-barrier kernels that the faster piece issue exposed, not a
            // property of the addressing form: et_device.h et_wait_vmem_le_lds_read_done, profiles/r06_lds_ring_war_race.txt.)
            const size_t xb = ((size_t)g.N * g.IH * g.IW * g.ldx + (size_t)g.IW * g.ldx) * sizeof(T), wb = (size_t)g.Cout * g.TT * g.Cin * sizeof(T);
            const bool buf = env_int("ET_CONV_BUF_DMA", 1) && xb < (1ull << 31) && wb < (1ull << 31);
            if (p.kind == GEMM_PPRS) ET_TWINS(buf, grid, (conv_gemm_pprs_kernel<T>), (conv_gemm_pprs_flat_kernel<T>))
#define ET_RS(BM_, BN_, WM_, WN_) \
    if (pp == &rs_rows[i++]) ET_TWINS(buf, grid, (conv_gemm_rs_kernel<T, BM_, BN_, WM_, WN_>), (conv_gemm_rs_flat_kernel<T, BM_, BN_, WM_, WN_>))
            ET_RS_ROWS
#undef ET_RS
        }
    }
#undef ET_TWINS
    return -2;
}

extern "C" int et_conv2d_stats_rows(int N, int OH, int OW) { return (N * OH * OW + 63) / 64; }

// ---- the stem: shape gate, persistent grid, tile fields -----------------------------------------------------------------------
static bool stem_eligible(int dtype, int Cin, int Cout, int KH, int KW, int stride, int pad, bool has_residual, bool has_zero_page) {
    return (dtype == ET_BF16 || dtype == ET_F16) && KH == 6 && KW == 6 && stride == 2 && pad == 2 && Cin == 8 && Cout <= 64 && Cout % 8 == 0 &&
           !has_residual && has_zero_page;
}
// the stem kernels are persistent (ET_CONV_STEM_WGS: tests shrink the grid to exercise the tile loop; read per launch)
static int stem_grid(int ntiles) {
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
// epilogue fields and launch of conv_stem_kernel / conv_stem_u8_kernel (U8); the caller has filled the operands and stem_tiles
template <bool U8>
static void launch_stem(StemArgs& a, int dtype, const float* scale, const float* bias, int act, float* stats, int stats_ld, hipStream_t s) {
    a.scale = scale; a.bias = bias; a.act = act; a.stats = stats; a.stats_ld = stats ? stats_ld : 0;
    a.stat_rows = (a.N * a.OH * a.OW + 63) / 64;        // == et_conv2d_stats_rows
    int grid = stem_grid(a.ntiles);
    if (stats && !stats_ld && grid > a.stat_rows) grid = a.stat_rows;
#define ET_STEM(T_, ACT_) \
    do { \
        if constexpr (U8) hipLaunchKernelGGL((conv_stem_u8_kernel<T_, ACT_>), dim3(grid), dim3(256), 0, s, a); \
        else hipLaunchKernelGGL((conv_stem_kernel<T_, ACT_>), dim3(grid), dim3(256), 0, s, a); \
    } while (0)
    if (dtype == ET_F16) { if (act == ACT_SILU) ET_STEM(et_f16, ACT_SILU); else if (act == ACT_RELU) ET_STEM(et_f16, ACT_RELU); else ET_STEM(et_f16, ACT_NONE); }
    else { if (act == ACT_SILU) ET_STEM(uint16_t, ACT_SILU); else if (act == ACT_RELU) ET_STEM(uint16_t, ACT_RELU); else ET_STEM(uint16_t, ACT_NONE); }
#undef ET_STEM
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
        launch_stem<false>(a, dtype, scale, bias, act, stats_partial, stats_ld, (hipStream_t)stream);
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
    if (!with_dtype(dtype, [&](auto t) { rc = launch_gemm<typename decltype(t)::type>(x, w, y, zero16, g, ep, (hipStream_t)stream); })) return -2;
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
            if (!with_dtype(dtype, [&](auto t) { rc = launch_gemm<typename decltype(t)::type>(dy, wT, dx, zero16, g, ep, (hipStream_t)stream); })) return -2;
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

// the weight-gradient instantiations, one row list per family as for the gather-GEMMs above (expanded into the WgradRow tables here
// and into the launches of launch_wgrad)
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
#define ET_WG(BM_, BN_, WM_, WN_) {WGRAD_TR, BM_, BN_, WM_, WN_, 0},
#define ET_WGRS(BM_, BN_, WM_, WN_, ST_) {WGRAD_RS, BM_, BN_, WM_, WN_, ST_},
#define ET_WGREG(BM_, BN_) {WGRAD_REG, BM_, BN_, 2, 2, 0},
static const WgradRow wg_rows[] = {ET_WG_ROWS};
static const WgradRow wgrs_rows[] = {ET_WGRS_ROWS};
static const WgradRow wgreg_rows[] = {ET_WGREG_ROWS};
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

template <typename T>
static int launch_wgrad(const WgradGroup& grp, const void* zero16, WgradGeom& g, hipStream_t s) {
    constexpr int VEC = et_elem<T>::VEC;
    constexpr int BKP = 8 * VEC;
    const WgradRow* const wp = plan_wgrad(g, (int)sizeof(T), zero16 != nullptr);
    if (!wp) return -2;
    const bool tr = wp->kind == WGRAD_TR;
    const int bm = wp->bm, bn = wp->bn, n_cu = device_cus();
    const uint16_t* z = (const uint16_t*)zero16;
    g.xcd = 1;                                     // the K-splits of one dW tile share an XCD (a knob until r02: always on)
    g.ntm = (g.Cout + bm - 1) / bm;
    int i = 0;                                     // the row lists as launches: expansion i instantiates row i of the family's table
    if constexpr (sizeof(T) == 2) {
        if (wp->kind == WGRAD_RS) {
            // the split policy over the padded raster, in 64-slot chunks
            g.ntn = 3 * ((g.Cin + bn - 1) / bn);
            // stride 1: 68 KB / 34 KB of LDS, 8 / 4 waves, <= 128 VGPRs; stride 2: 67 KB (4 waves)
            const int slots = wp->stride == 2 ? 2 : (bm == 128 ? 2 : 4);
            const SplitK sk = wgrad_split_k(g.PP, 64, grp.n * g.ntn * g.ntm, slots * n_cu);
            g.Pper = sk.per; g.nsk = sk.nsk;
            const dim3 grid(grp.n * g.ntn * g.ntm * sk.nsk);
#define ET_WGRS(BM_, BN_, WM_, WN_, ST_) \
    if (wp == &wgrs_rows[i++]) { hipLaunchKernelGGL((conv_wgrad_rs_kernel<T, BM_, BN_, WM_, WN_, ST_>), grid, dim3(64 * WM_ * WN_), 0, s, grp, z, g); return 0; }
            ET_WGRS_ROWS
#undef ET_WGRS
            return -2;
        }
    }
    g.ntn = (g.NC + bn - 1) / bn;
    // `slots` workgroups of this tile fit on a CU (LDS- or register-limited); the whole group shares the split
    const int lds_kb = tr ? (bm + bn) / 4 : 64;                // 2 stages x 64 pixels x (bm+bn) channels x 2 B
    const int slots = tr ? max(1, min(160 / lds_kb, bm * bn <= 64 * 64 ? 5 : (bm * bn <= 128 * 64 ? 3 : 2))) : 2;
    const SplitK sk = wgrad_split_k(g.P, BKP, grp.n * g.ntn * g.ntm, slots * n_cu);
    g.Pper = sk.per; g.nsk = sk.nsk;
    if constexpr (sizeof(T) == 2) {
        if (tr) {
            const dim3 grid(grp.n * g.ntn * g.ntm * sk.nsk);
            // 1x1 stride-1 layers: buffer-descriptor pieces when every tensor of the group spans < 2^31 bytes (conv_wgrad_tr_kernel, g.buf)
            g.buf = g.ident && env_int("ET_CONV_BUF_DMA", 1);
            for (int k = 0; k < grp.n && g.buf; ++k)
                if ((size_t)g.P * grp.it[k].ldx * 2 >= (1ull << 31) || (size_t)g.P * grp.it[k].ldy * 2 >= (1ull << 31)) g.buf = 0;
#define ET_WG(BM_, BN_, WM_, WN_) \
    if (wp == &wg_rows[i++]) { hipLaunchKernelGGL((conv_wgrad_tr_kernel<T, BM_, BN_, WM_, WN_>), grid, dim3(64 * WM_ * WN_), 0, s, grp, z, g); return 0; }
            ET_WG_ROWS
#undef ET_WG
            return -2;
        }
    }
    // register-staged kernel (fp32 parity mode, callers without a zero page): one launch per item
    const dim3 grid(g.ntn * g.ntm * sk.nsk), block(256);
    for (int k = 0; k < grp.n; ++k) {
        const T* xx = (const T*)grp.it[k].x; const T* yy = (const T*)grp.it[k].dy;
        float* dw = grp.it[k].dw;
        g.ldx = grp.it[k].ldx; g.ldy = grp.it[k].ldy;
        i = 0;
#define ET_WGREG(BM_, BN_) \
    if (wp == &wgreg_rows[i++]) hipLaunchKernelGGL((conv_wgrad_kernel<T, BM_, BN_>), grid, block, 0, s, xx, yy, dw, g);
        ET_WGREG_ROWS
#undef ET_WGREG
    }
    return wp->kind == WGRAD_REG ? 0 : -2;
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
    int rc = 0;
    if (!with_dtype(dtype, [&](auto t) { rc = launch_wgrad<typename decltype(t)::type>(grp, zero16, g, (hipStream_t)stream); })) return -2;
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

extern "C" int et_weight_transpose(const void* w, void* wT, int dtype, int Cout, int taps, int Cin, et_stream_t stream) {
    if (!w || !wT) return -1;
    const long long n = (long long)Cout * taps * Cin;
    if (n <= 0) return -2;
    const dim3 grid(et_cdiv(n, 256)), block(256);
    if (dtype == ET_F32)
        hipLaunchKernelGGL((weight_transpose_kernel<float>), grid, block, 0, (hipStream_t)stream, (const float*)w, (float*)wT, Cout, taps, Cin, n);
    else if (dtype == ET_BF16 || dtype == ET_F16)       // moves 16-bit words: format-agnostic
        hipLaunchKernelGGL((weight_transpose_kernel<uint16_t>), grid, block, 0, (hipStream_t)stream, (const uint16_t*)w, (uint16_t*)wT, Cout, taps, Cin, n);
    else return -2;
    ET_CHECK_LAUNCH();
    return 0;
}

extern "C" int et_weight_transpose_all(const void* w_arena, void* wT_arena, int dtype, const int* table, int n_layers,
                                       long long total_elems, et_stream_t stream) {
    if (!w_arena || !wT_arena || !table) return -1;
    if (n_layers <= 0 || total_elems <= 0) return -2;
    const dim3 grid(et_cdiv(total_elems, 256)), block(256);
    if (dtype == ET_F32)
        hipLaunchKernelGGL((weight_transpose_all_kernel<float>), grid, block, 0, (hipStream_t)stream, (const float*)w_arena,
                           (float*)wT_arena, table, n_layers, total_elems);
    else if (dtype == ET_BF16 || dtype == ET_F16) {
        // layer offsets are multiples of 16 elements and 16-bit channel counts multiples of 8 (flat_state.py): 16-byte rows (a layer
        // whose channels are not is copied element by element inside the same launch)
        if ((((uintptr_t)w_arena | (uintptr_t)wT_arena) & 15) == 0)
            hipLaunchKernelGGL(weight_transpose_all_tiled_kernel, dim3(96, n_layers), block, 0, (hipStream_t)stream,
                               (const uint16_t*)w_arena, (uint16_t*)wT_arena, table, n_layers);
        else
            hipLaunchKernelGGL((weight_transpose_all_kernel<uint16_t>), grid, block, 0, (hipStream_t)stream,
                               (const uint16_t*)w_arena, (uint16_t*)wT_arena, table, n_layers, total_elems);
    } else return -2;
    ET_CHECK_LAUNCH();
    return 0;
}

extern "C" int et_colsum(const void* x, int dtype, int P, int C, int ld, float* out, et_stream_t stream) {
    if (!x || !out) return -1;
    if (P <= 0 || C <= 0) return -2;
    const int rpb = 256;
    const dim3 grid((C + 255) / 256, (P + rpb - 1) / rpb), block(256);
    if (dtype == ET_F32) hipLaunchKernelGGL((colsum_kernel<float>), grid, block, 0, (hipStream_t)stream, (const float*)x, P, C, ld, rpb, out);
    else if (dtype == ET_BF16 || dtype == ET_F16) {
        const int CV = C / 8;
        const bool vec8 = C % 8 == 0 && ld % 8 == 0 && CV >= 1 && CV <= 256 && 256 % CV == 0 && (((uintptr_t)x) & 15) == 0;
        const int rpb2 = 256;                                  // rows per block: 8-256 rows per row group, two in flight per thread
        if (dtype == ET_BF16) {
            if (vec8) hipLaunchKernelGGL((colsum_vec8_kernel<uint16_t>), dim3((P + rpb2 - 1) / rpb2), block, 0, (hipStream_t)stream, (const uint16_t*)x, P, CV, ld, rpb2, out);
            else hipLaunchKernelGGL((colsum_kernel<uint16_t>), grid, block, 0, (hipStream_t)stream, (const uint16_t*)x, P, C, ld, rpb, out);
        } else {
            if (vec8) hipLaunchKernelGGL((colsum_vec8_kernel<et_f16>), dim3((P + rpb2 - 1) / rpb2), block, 0, (hipStream_t)stream, (const et_f16*)x, P, CV, ld, rpb2, out);
            else hipLaunchKernelGGL((colsum_kernel<et_f16>), grid, block, 0, (hipStream_t)stream, (const et_f16*)x, P, C, ld, rpb, out);
        }
    }
    else return -2;
    ET_CHECK_LAUNCH();
    return 0;
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
    launch_stem<true>(a, dtype, scale, bias, act, stats, stats_ld, (hipStream_t)stream);
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
    hipStream_t s = (hipStream_t)stream;
    if (dtype == ET_F16) hipLaunchKernelGGL((conv_stem_u8_wgrad_kernel<et_f16>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((conv_stem_u8_wgrad_kernel<uint16_t>), dim3(grid), dim3(256), 0, s, a);
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

extern "C" int et_env_knobs(char* buf, int buflen) {
    // every ET_* runtime knob that is SET in this process's environment, as "NAME=value;..." (bench.py records it).  The complete list:
    // three test hooks (persistent-grid sizes, the BatchNorm finalize form), the experimental buffer-descriptor staging of the row-shift kernels, the opt-in arms that change WHAT runs beside what (step
    // graph, weight-gradient stream, the stem on uint8 planes or on the packed image), the data-parallel transport settings, and the experiment-library path.
    static const char* names[] = {"ET_CONV_S1_WGS", "ET_CONV_STEM_WGS", "ET_CONV_BUF_DMA", "ET_BN_FIN_SMALL", "ET_STEP_GRAPH", "ET_WGRAD_STREAM", "ET_STEM_U8",
                                  "ET_ALLREDUCE_CHUNK_MB", "ET_ALLREDUCE_DTYPE", "ET_RCCL_CHANNELS", "ET_DP_SINGLE_RANK", "ET_HIP_LIB"};
    if (!buf || buflen < 1) return -1;
    int off = 0;
    buf[0] = 0;
    for (const char* n : names) {
        const char* v = getenv(n);
        if (!v) continue;
        const int w = snprintf(buf + off, buflen - off, "%s=%s;", n, v);
        if (w < 0 || w >= buflen - off) return -3;
        off += w;
    }
    return 0;
}
