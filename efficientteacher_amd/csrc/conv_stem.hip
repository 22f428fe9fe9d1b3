// The stem (6x6 stride-2 pad-2): forward from the packed image or straight from the loaders' uint8 planes, the weight gradient from
// the uint8 planes, and their launches.  16-bit types only.  StemArgs / StemWgradArgs and the tile constants: conv_device.h.
#include "conv_host.h"

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

// ---- launches ------------------------------------------------------------------------------------------------------------------
// epilogue fields and launch of conv_stem_kernel / conv_stem_u8_kernel (u8); the caller has filled the operands and stem_tiles
void launch_stem(bool u8, StemArgs& a, int dtype, const float* scale, const float* bias, int act, float* stats, int stats_ld,
                 hipStream_t s) {
    a.scale = scale; a.bias = bias; a.act = act; a.stats = stats; a.stats_ld = stats ? stats_ld : 0;
    a.stat_rows = (a.N * a.OH * a.OW + 63) / 64;        // == et_conv2d_stats_rows
    int grid = stem_grid(a.ntiles);
    if (stats && !stats_ld && grid > a.stat_rows) grid = a.stat_rows;
    (void)with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        if constexpr (et_is_lp<T>::value)              // the stem kernels exist for the 16-bit types only: the callers have checked (stem_eligible, stem_u8_mode)
            with_act(act, [&](auto ac) {
                constexpr int ACT = decltype(ac)::value;
                if (u8) hipLaunchKernelGGL((conv_stem_u8_kernel<T, ACT>), dim3(grid), dim3(256), 0, s, a);
                else hipLaunchKernelGGL((conv_stem_kernel<T, ACT>), dim3(grid), dim3(256), 0, s, a);
            });
        return 0;
    });
}

void launch_stem_u8_wgrad(const StemWgradArgs& a, int dtype, int grid, hipStream_t s) {
    (void)with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        if constexpr (et_is_lp<T>::value) hipLaunchKernelGGL((conv_stem_u8_wgrad_kernel<T>), dim3(grid), dim3(256), 0, s, a);   // 16-bit only, as launch_stem
        return 0;
    });
}
