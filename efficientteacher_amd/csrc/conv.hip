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
//
// This file: the forward / dgrad gather-GEMM kernels, their shared epilogue and their launch.  conv_wgrad.hip and conv_stem.hip hold the
// other kernels, conv_device.h what the kernel files share, conv_host.hip the host layer (geometry, kernel selection, plan tables, C
// ABI), conv_host.h its declarations.
#include "conv_host.h"

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


// chunk-uniform tap lookup: the index is made provably wave-uniform so that the table read is a scalar
// (SMEM) load -- a vector load here would put an s_waitcnt vmcnt(0) in the middle of the LDS-DMA burst
__device__ __forceinline__ void tap_lookup_uniform(const GatherGeom& g, int tap, int& dy, int& dx, int& wt) {
    const int ti = g.tapinfo[__builtin_amdgcn_readfirstlane(tap)];
    dy = (int)(signed char)(ti & 0xff);
    dx = (int)(signed char)((ti >> 8) & 0xff);
    wt = (ti >> 16) & 0xff;
}

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

// ---- launch: the row lists again, as launches: expansion i instantiates row i of the family's table, and the plan points at its row ---
int launch_gemm_row(const GemmPlan* pp, int dtype, const void* X, const void* W, void* Y, const void* zero16, const GatherGeom& g,
                    const Epilogue& ep, hipStream_t s) {
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const GemmPlan& p = *pp;
        const T* x = (const T*)X; const T* w = (const T*)W; T* y = (T*)Y; const T* z = (const T*)zero16;
        const dim3 grid(g.ntm * g.ntn), block(64 * p.WM * p.WN);
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
                // (profiles/r06_lds_ring_war_race.txt section 7).  (The arm was withdrawn for a day of this round: conv_gemm_rs_kernel<128, 64> produced
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
    });
}
