// The weight-gradient kernels -- conv_wgrad_kernel (register staging, any type), conv_wgrad_tr_kernel (LDS-DMA + transposing LDS
// reads), conv_wgrad_rs_kernel (3x3: operands shared by the taps of a kernel row) -- with their launch, and the small helpers of
// the backward pass: weight transposes (dgrad's operand) and column sums (bias gradients) with their entry points.
#include "conv_host.h"

// ---- wgrad ----------------------------------------------------------------------------------------
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

// ---- launch: the row lists again, expansion i instantiates row i of the family's table and the plan points at its row ---------------
int launch_wgrad_row(const WgradRow* wp, int dtype, const WgradGroup& grp, const void* zero16, WgradGeom g, hipStream_t s) {
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        int i = 0;
        if constexpr (sizeof(T) == 2) {
            const uint16_t* z = (const uint16_t*)zero16;
            const dim3 grid(grp.n * g.ntn * g.ntm * g.nsk);
            if (wp->kind == WGRAD_RS) {
#define ET_WGRS(BM_, BN_, WM_, WN_, ST_) \
                if (wp == &wgrs_rows[i++]) { hipLaunchKernelGGL((conv_wgrad_rs_kernel<T, BM_, BN_, WM_, WN_, ST_>), grid, dim3(64 * WM_ * WN_), 0, s, grp, z, g); return 0; }
                ET_WGRS_ROWS
#undef ET_WGRS
                return -2;
            }
            if (wp->kind == WGRAD_TR) {
#define ET_WG(BM_, BN_, WM_, WN_) \
                if (wp == &wg_rows[i++]) { hipLaunchKernelGGL((conv_wgrad_tr_kernel<T, BM_, BN_, WM_, WN_>), grid, dim3(64 * WM_ * WN_), 0, s, grp, z, g); return 0; }
                ET_WG_ROWS
#undef ET_WG
                return -2;
            }
        }
        // register-staged kernel (fp32 parity mode, callers without a zero page): one launch per item
        const dim3 grid(g.ntn * g.ntm * g.nsk), block(256);
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
    });
}

// the transposes move words: the two 16-bit formats share the uint16_t instantiation
template <typename T> using word_t = std::conditional_t<sizeof(T) == 2, uint16_t, float>;

extern "C" int et_weight_transpose(const void* w, void* wT, int dtype, int Cout, int taps, int Cin, et_stream_t stream) {
    if (!w || !wT) return -1;
    const long long n = (long long)Cout * taps * Cin;
    if (n <= 0) return -2;
    return with_dtype(dtype, [&](auto t) {
        using T = word_t<typename decltype(t)::type>;
        hipLaunchKernelGGL((weight_transpose_kernel<T>), dim3(et_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)w, (T*)wT, Cout, taps, Cin, n);
        ET_CHECK_LAUNCH();
        return 0;
    });
}

extern "C" int et_weight_transpose_all(const void* w_arena, void* wT_arena, int dtype, const int* table, int n_layers,
                                       long long total_elems, et_stream_t stream) {
    if (!w_arena || !wT_arena || !table) return -1;
    if (n_layers <= 0 || total_elems <= 0) return -2;
    return with_dtype(dtype, [&](auto t) {
        using T = word_t<typename decltype(t)::type>;
        // layer offsets are multiples of 16 elements and 16-bit channel counts multiples of 8 (flat_state.py): 16-byte rows (a layer
        // whose channels are not is copied element by element inside the same launch)
        if (sizeof(T) == 2 && (((uintptr_t)w_arena | (uintptr_t)wT_arena) & 15) == 0)
            hipLaunchKernelGGL(weight_transpose_all_tiled_kernel, dim3(96, n_layers), dim3(256), 0, (hipStream_t)stream,
                               (const uint16_t*)w_arena, (uint16_t*)wT_arena, table, n_layers);
        else
            hipLaunchKernelGGL((weight_transpose_all_kernel<T>), dim3(et_cdiv(total_elems, 256)), dim3(256), 0, (hipStream_t)stream,
                               (const T*)w_arena, (T*)wT_arena, table, n_layers, total_elems);
        ET_CHECK_LAUNCH();
        return 0;
    });
}

extern "C" int et_colsum(const void* x, int dtype, int P, int C, int ld, float* out, et_stream_t stream) {
    if (!x || !out) return -1;
    if (P <= 0 || C <= 0) return -2;
    const int rpb = 256;                                       // rows per block (vec8: 8-256 rows per row group, two in flight per thread)
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const int CV = C / 8;
        const bool vec8 = et_is_lp<T>::value && C % 8 == 0 && ld % 8 == 0 && CV >= 1 && CV <= 256 && 256 % CV == 0 && (((uintptr_t)x) & 15) == 0;
        if constexpr (et_is_lp<T>::value) {            // colsum_vec8_kernel: 16-bit inputs only
            if (vec8) hipLaunchKernelGGL((colsum_vec8_kernel<T>), dim3((P + rpb - 1) / rpb), dim3(256), 0, (hipStream_t)stream, (const T*)x, P, CV, ld, rpb, out);
        }
        if (!vec8)
            hipLaunchKernelGGL((colsum_kernel<T>), dim3((C + 255) / 256, (P + rpb - 1) / rpb), dim3(256), 0, (hipStream_t)stream, (const T*)x, P, C, ld, rpb, out);
        ET_CHECK_LAUNCH();
        return 0;
    });
}
