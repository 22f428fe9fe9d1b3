// The strong view of an unlabeled batch, generated ON THE DEVICE from the weak view.
//
// Replaces, per image, the cv2 chain of the reference's data-loader workers (utils/datasets_ssod.py:520-570):
//   random_perspective_with_M  -> cv2.warpAffine(img, M[:2], borderValue 114)      utils/datasets_ssod.py:902-945
//   augment_hsv                -> BGR2HSV, three 256-entry LUTs, HSV2BGR            utils/augmentations.py:48-61
//   cutout                     -> rectangles filled with one colour each             utils/augmentations.py:382-398
//   np.flipud / np.fliplr                                                            utils/datasets_ssod.py:552-563
// The random draws (matrix, gains, rectangles, flips) stay on the host (efficientteacher_amd/utils/augment.py, the same
// recipe as the reference); this kernel is the per-pixel work, one thread per output pixel, all stages fused: the output
// pixel is traced back through the flips, takes a cutout colour if a rectangle covers it (the LAST covering rectangle, as
// successive assignments do), else is sampled from the weak view through the inverse affine map and colour-jittered.
//
// PARITY UNPINNED: cv2 is not installed in the build image and the reference holds no image goldens, so the arithmetic
// below RESTATES OpenCV's published 8-bit algorithms -- warpAffine's fixed-point bilinear sampling (10-bit coordinates,
// 5-bit fractions, 15-bit weights, constant border per tap), the integer RGB->HSV of cvtColor (hsv_shift 12 division
// tables, H in [0,180)) and the float HSV->RGB with cvRound -- and is tested for its invariants only.
#include "et_device.h"
#include "../../include/et_hip.h"
#include <math.h>

#define AUG_MAX_CUT 32

struct AugArgs {
    const unsigned char* src;   // (B,3,H,W) weak view, RGB planes
    unsigned char* dst;         // (B,3,H,W) strong view
    const double* minv;         // [B][6] dst -> src affine map (OpenCV's inverted matrix)
    const unsigned char* lut;   // [B][3][256] hue / sat / val look-up tables, or NULL (no colour jitter)
    const int* cut;             // [B][AUG_MAX_CUT][7] x0,y0,x1,y1 (half open), r,g,b ; unused entries x1 <= x0
    const int* flags;           // [B][3] n_cut, flipud, fliplr
    int B, H, W;
    int border;                 // 114
};

__device__ __forceinline__ int aug_round(double v) { return (int)rint(v); }       // cvRound: half to even (default rounding mode)

// ---- cv2.warpAffine, INTER_LINEAR, BORDER_CONSTANT: AB_BITS 10, INTER_BITS 5, weights * 2^15.  M: the dst -> src map; (x, y): the
// destination pixel.  -> the top-left tap (sx, sy) and the weights of the taps (sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1);
// the pixel is (sum w * tap + (1 << 14)) >> 15.  Shared by strong_view_kernel and labeled_mosaic_kernel.
__device__ __forceinline__ void aug_warp_taps(const double* M, int x, int y, int& sx, int& sy, int w[4]) {
    const int round_delta = 16;                                           // AB_SCALE / INTER_TAB_SIZE / 2
    const int X0 = aug_round((M[1] * y + M[2]) * 1024.0) + round_delta, Y0 = aug_round((M[4] * y + M[5]) * 1024.0) + round_delta;
    const int X = (X0 + aug_round(M[0] * x * 1024.0)) >> 5, Y = (Y0 + aug_round(M[3] * x * 1024.0)) >> 5;
    sx = X >> 5; sy = Y >> 5;
    const int fx = X & 31, fy = Y & 31;
    w[0] = (32 - fx) * (32 - fy) * 32; w[1] = fx * (32 - fy) * 32; w[2] = (32 - fx) * fy * 32; w[3] = fx * fy * 32;
}

// ---- augment_hsv on one pixel: cvtColor RGB -> HSV, the three LUTs L[3][256] (hue, sat, val), cvtColor HSV -> RGB
__device__ __forceinline__ void aug_hsv_lut(const unsigned char* L, int& r, int& g, int& bl) {
    // ---- cvtColor RGB -> HSV (8 bit, H in [0,180)): integer division tables with hsv_shift = 12
    const int v = max(max(r, g), bl), vmin = min(min(r, g), bl);
    const int diff = v - vmin;
    const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
    const int sdiv = v ? aug_round((255 << 12) / (double)v) : 0;
    const int hdiv = diff ? aug_round((180 << 12) / (6.0 * diff)) : 0;
    const int s = (diff * sdiv + (1 << 11)) >> 12;
    int h = (vr & (g - bl)) + (~vr & ((vg & (bl - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
    h = (h * hdiv + (1 << 11)) >> 12;
    h += h < 0 ? 180 : 0;
    const int h2 = L[h & 255], s2 = L[256 + s], v2 = L[512 + v];
    // ---- cvtColor HSV -> RGB (8 bit): float sector arithmetic, cvRound to uchar
    const float fs = s2 * (1.f / 255.f), fv = v2 * (1.f / 255.f);
    float fr, fg, fb;
    if (s2 == 0) {
        fr = fg = fb = fv;
    } else {
        float hh = h2 * (6.f / 180.f);
        int sector = (int)floorf(hh);
        hh -= sector;
        if ((unsigned)sector >= 6u) { sector = 0; hh = 0.f; }
        const float tab[4] = {fv, fv * (1.f - fs), fv * (1.f - fs * hh), fv * (1.f - fs * (1.f - hh))};
        const int sd[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};      // b, g, r
        fb = tab[sd[sector][0]]; fg = tab[sd[sector][1]]; fr = tab[sd[sector][2]];
    }
    r = min(max(aug_round(fr * 255.f), 0), 255);
    g = min(max(aug_round(fg * 255.f), 0), 255);
    bl = min(max(aug_round(fb * 255.f), 0), 255);
}

__global__ __launch_bounds__(256) void strong_view_kernel(AugArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long plane = (long long)a.H * a.W;
    if (i >= (long long)a.B * plane) return;
    const int b = (int)(i / plane);
    const int rem = (int)(i - (long long)b * plane);
    const int oy = rem / a.W, ox = rem - oy * a.W;
    const int* fl = a.flags + b * 3;
    const int y = fl[1] ? a.H - 1 - oy : oy, x = fl[2] ? a.W - 1 - ox : ox;      // position before the flips
    int r, g, bl;
    int hit = -1;
    const int* cuts = a.cut + (size_t)b * AUG_MAX_CUT * 7;
    for (int k = 0; k < fl[0] && k < AUG_MAX_CUT; ++k) {
        const int* c = cuts + k * 7;
        if (x >= c[0] && x < c[2] && y >= c[1] && y < c[3]) hit = k;
    }
    if (hit >= 0) {
        r = cuts[hit * 7 + 4]; g = cuts[hit * 7 + 5]; bl = cuts[hit * 7 + 6];
    } else {
        const unsigned char* base = a.src + (size_t)b * 3 * plane;
        int sx, sy, w[4];
        aug_warp_taps(a.minv + b * 6, x, y, sx, sy, w);
        int px[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const unsigned char* p = base + ch * plane;
            auto at = [&](int yy, int xx) -> int {
                return ((unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W) ? (int)p[(size_t)yy * a.W + xx] : a.border;
            };
            const int v = w[0] * at(sy, sx) + w[1] * at(sy, sx + 1) + w[2] * at(sy + 1, sx) + w[3] * at(sy + 1, sx + 1);
            px[ch] = (v + (1 << 14)) >> 15;
        }
        r = px[0]; g = px[1]; bl = px[2];
        if (a.lut) aug_hsv_lut(a.lut + (size_t)b * 768, r, g, bl);
    }
    unsigned char* o = a.dst + (size_t)b * 3 * plane + (size_t)oy * a.W + ox;
    o[0] = (unsigned char)r; o[plane] = (unsigned char)g; o[2 * plane] = (unsigned char)bl;
}

extern "C" int et_strong_view_u8(const uint8_t* weak, uint8_t* strong, int B, int H, int W, const double* minv, const uint8_t* lut,
                                 const int* cutouts, const int* flags, int border_value, et_stream_t stream) {
    if (!weak || !strong || !minv || !cutouts || !flags) return -1;
    if (B <= 0 || H <= 0 || W <= 0) return -2;
    AugArgs a;
    a.src = weak; a.dst = strong; a.minv = minv; a.lut = lut; a.cut = cutouts; a.flags = flags;
    a.B = B; a.H = H; a.W = W; a.border = border_value;
    hipLaunchKernelGGL(strong_view_kernel, dim3(et_cdiv((long long)B * H * W, 256)), dim3(256), 0, (hipStream_t)stream, a);
    ET_CHECK_LAUNCH();
    return 0;
}

// ---- 4-image mosaic (load_mosaic_with_M, utils/datasets_ssod.py:732-782) -----------------------------------------------------
// The reference pastes four images around a random centre into a 2s x 2s canvas of border value 114 and halves it with
// cv2.resize(img4, (s, s)).  At this exact 2:1 ratio OpenCV's INTER_LINEAR resize takes its fast INTER_AREA path: an output
// pixel is (a + b + c + d + 2) >> 2 of its 2 x 2 source pixels.  Here one thread produces one output pixel (three planes)
// straight from the four source images -- the canvas is never materialised: each of the 2 x 2 canvas positions belongs to the
// quadrant given by its side of the centre and reads tile i at (cy - y1a + y1b, cx - x1a + x1b) when it lies inside the
// tile's pasted rectangle, else the border value.  tiles: [B][4][8] int64 = {device pointer of the (3, h, w) uint8 planes, h, w,
// x1a, y1a, x2a, y2a, x1b << 32 | y1b} (efficientteacher_amd/utils/augment.py mosaic_layout).  PARITY: the placement is pinned on
// the reference (tests/golden/mosaic.npz); the 2:1 resampling restates OpenCV's published algorithm and is unpinned (no cv2).
__global__ __launch_bounds__(256) void mosaic4_kernel(const long long* __restrict__ tiles, unsigned char* __restrict__ out, int B, int S,
                                                      int border) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long plane = (long long)S * S;
    if (i >= (long long)B * plane) return;
    const int b = (int)(i / plane);
    const int rem = (int)(i - (long long)b * plane);
    const int oy = rem / S, ox = rem - oy * S;
    const long long* T = tiles + (size_t)b * 32;
    // the centre: x2a of the top-left tile is xc, its y2a is yc (mosaic_layout)
    const int xc = (int)T[5], yc = (int)T[6];
    int acc[3] = {2, 2, 2};                                  // the rounding term of (a + b + c + d + 2) >> 2
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int cy = 2 * oy + dy, cx = 2 * ox + dx;
            const int q = (cy >= yc ? 2 : 0) + (cx >= xc ? 1 : 0);
            const long long* t = T + q * 8;
            const int x1a = (int)t[3], y1a = (int)t[4], x2a = (int)t[5], y2a = (int)t[6];
            if (cx >= x1a && cx < x2a && cy >= y1a && cy < y2a) {
                const unsigned char* src = (const unsigned char*)(uintptr_t)t[0];
                const int h = (int)t[1], w = (int)t[2];
                const int x1b = (int)(t[7] >> 32), y1b = (int)(t[7] & 0xffffffffll);
                const size_t o = (size_t)(cy - y1a + y1b) * w + (cx - x1a + x1b), pl = (size_t)h * w;
                acc[0] += src[o]; acc[1] += src[pl + o]; acc[2] += src[2 * pl + o];
            } else {
                acc[0] += border; acc[1] += border; acc[2] += border;
            }
        }
    unsigned char* o = out + (size_t)b * 3 * plane + (size_t)oy * S + ox;
    o[0] = (unsigned char)(acc[0] >> 2); o[plane] = (unsigned char)(acc[1] >> 2); o[2 * plane] = (unsigned char)(acc[2] >> 2);
}

extern "C" int et_mosaic4_u8(const int64_t* tiles, uint8_t* out, int B, int S, int border_value, et_stream_t stream) {
    if (!tiles || !out) return -1;
    if (B <= 0 || S <= 0 || (long long)B * S * S >= (1ll << 40)) return -2;
    hipLaunchKernelGGL(mosaic4_kernel, dim3(et_cdiv((long long)B * S * S, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)tiles, out, B, S, border_value);
    ET_CHECK_LAUNCH();
    return 0;
}

// ---- labeled batch: mosaic + random perspective (+ mixup) + HSV + flips (LoadImagesAndLabels.__getitem__, utils/datasets.py:889-1043) --
// The reference pastes four images into a 2S x 2S canvas (load_mosaic, :1219-1311), warps the canvas to S x S with
// cv2.warpAffine(img4, M[:2], dsize=(S, S), borderValue=114) (random_perspective_keypoints, utils/augmentations.py:125-167; the border
// -S/2 makes the output half the canvas), blends a second such mosaic in for mixup ((im * r + im2 * (1 - r)).astype(uint8),
// augmentations.py:409-414), runs augment_hsv and flips.  One launch does all of it for the batch and never builds a canvas: an output
// pixel is traced back through the flips, its four bilinear taps are fetched from a VIRTUAL canvas (the quadrant by the side of the
// centre, tile i at (cy - y1a + y1b, cx - x1a + x1b) inside the tile's pasted rectangle, else -- the rest of the canvas and everything
// outside it -- the border value), blended in fp64 with two rounded products and one rounded sum (this file is built without FMA
// contraction) and truncated, colour-jittered with the helpers strong_view_kernel uses, and stored.
// One thread makes FOUR adjacent output pixels of a row and stores one 32-bit word per plane (byte stores when S is no multiple of 4);
// the word is assembled in OUTPUT order, so a left-right flip needs no separate reversal.  The tile table of the image sits in LDS.
// PARITY: tile placement, matrices, ratio and LUTs are the host's (pinned on the reference, tests/golden/labeled_mosaic.npz); the warp
// sampling and the HSV round trip restate OpenCV's published algorithms as above and are unpinned (no cv2).
struct LmArgs {
    const long long* tiles;     // [B][2][4][8] rows of et_mosaic4_u8: the primary mosaic and the mixup partner
    unsigned char* dst;         // (B,3,S,S)
    const double* minv;         // [B][2][6] dst -> src affine maps
    const double* mix;          // [B] mixup ratio r
    const unsigned char* lut;   // [B][3][256] or NULL
    const int* flags;           // [B][3] has_mix, flipud, fliplr
    int B, S;
    int border;
};

struct LmTile {
    const unsigned char* p;
    int h, w, x1a, y1a, x2a, y2a, x1b, y1b;
};

__device__ __forceinline__ void lm_sample(const LmTile* T, const double* M, int x, int y, int border, int px[3]) {
    int sx, sy, w[4];
    aug_warp_taps(M, x, y, sx, sy, w);
    const int xc = T[0].x2a, yc = T[0].y2a;                     // the centre (mosaic_layout)
    int acc[3] = {1 << 14, 1 << 14, 1 << 14};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int cy = sy + (k >> 1), cx = sx + (k & 1);
        const LmTile& t = T[(cy >= yc ? 2 : 0) + (cx >= xc ? 1 : 0)];
        if (cx >= t.x1a && cx < t.x2a && cy >= t.y1a && cy < t.y2a) {
            const size_t o = (size_t)(cy - t.y1a + t.y1b) * t.w + (cx - t.x1a + t.x1b), pl = (size_t)t.h * t.w;
            acc[0] += w[k] * t.p[o]; acc[1] += w[k] * t.p[pl + o]; acc[2] += w[k] * t.p[2 * pl + o];
        } else {
            acc[0] += w[k] * border; acc[1] += w[k] * border; acc[2] += w[k] * border;
        }
    }
    px[0] = acc[0] >> 15; px[1] = acc[1] >> 15; px[2] = acc[2] >> 15;
}

__global__ __launch_bounds__(256) void labeled_mosaic_kernel(LmArgs a) {
    __shared__ LmTile T[8];
    const int b = blockIdx.y;
    if (threadIdx.x < 8) {
        const long long* t = a.tiles + ((size_t)b * 8 + threadIdx.x) * 8;
        LmTile& d = T[threadIdx.x];
        d.p = (const unsigned char*)(uintptr_t)t[0];
        d.h = (int)t[1]; d.w = (int)t[2]; d.x1a = (int)t[3]; d.y1a = (int)t[4]; d.x2a = (int)t[5]; d.y2a = (int)t[6];
        d.x1b = (int)(t[7] >> 32); d.y1b = (int)(t[7] & 0xffffffffll);
    }
    __syncthreads();
    const int S = a.S, G = (S + 3) >> 2;                       // G groups of four pixels per row
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S * G) return;
    const int oy = i / G, ox0 = (i - oy * G) * 4;
    const int* fl = a.flags + b * 3;
    const int has_mix = fl[0], ud = fl[1], lr = fl[2];
    const int y = ud ? S - 1 - oy : oy;                        // position before the flips
    const double r = a.mix[b], omr = 1.0 - r;
    const double* M = a.minv + (size_t)b * 12;
    const unsigned char* L = a.lut ? a.lut + (size_t)b * 768 : nullptr;
    unsigned word[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ox = ox0 + j;
        if (ox < S) {
            const int x = lr ? S - 1 - ox : ox;
            int px[3];
            lm_sample(T, M, x, y, a.border, px);
            if (has_mix) {
                int qx[3];
                lm_sample(T + 4, M + 6, x, y, a.border, qx);
#pragma unroll
                for (int c = 0; c < 3; ++c) px[c] = (int)((double)px[c] * r + (double)qx[c] * omr);       // astype(uint8): truncation
            }
            if (L) aug_hsv_lut(L, px[0], px[1], px[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) word[c] |= (unsigned)px[c] << (8 * j);
        }
    }
    const size_t plane = (size_t)S * S;
    unsigned char* o = a.dst + (size_t)b * 3 * plane + (size_t)oy * S + ox0;
    if ((S & 3) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *(unsigned*)(o + c * plane) = word[c];
    } else {
        for (int j = 0; j < 4 && ox0 + j < S; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c * plane + j] = (unsigned char)(word[c] >> (8 * j));
    }
}

extern "C" int et_labeled_mosaic_u8(const int64_t* tiles, const double* minv, const double* mix, const uint8_t* lut, const int* flags,
                                    uint8_t* out, int B, int S, int border_value, et_stream_t stream) {
    if (!tiles || !minv || !mix || !flags || !out) return -1;
    if (B <= 0 || B > 65535 || S <= 0 || S > 16384) return -2;
    if (((uintptr_t)out & 3) != 0) return -3;                   // the 32-bit stores
    LmArgs a;
    a.tiles = (const long long*)tiles; a.dst = out; a.minv = minv; a.mix = mix; a.lut = lut; a.flags = flags;
    a.B = B; a.S = S; a.border = border_value;
    hipLaunchKernelGGL(labeled_mosaic_kernel, dim3(et_cdiv((long long)S * ((S + 3) >> 2), 256), B), dim3(256), 0, (hipStream_t)stream, a);
    ET_CHECK_LAUNCH();
    return 0;
}

// ---- labels of the labeled batch ---------------------------------------------------------------------------------------------------
// Per source label, with the reference's dtypes (labels are float32; numpy treats the Python scalars w, h, padw, padh, s, eps as weak,
// so they enter float32 expressions as float32): xywhn2xyxy(w, h, padw, padh) in float32 (utils/general.py:640), the four corners
// times M in fp64, min / max, clip to [0, S] (augmentations.py:181-193), box_candidates(box1 = xyxy_f32 * s, box2, area_thr 0.10)
// (:261, :417-422), the new box assigned back to float32, xyxy2xywhn(w = h = S, clip to S - 1e-3) (general.py:649-658), the flips as
// 1 - v, clip(0, 1) (datasets.py:1027).  Output rows [img, cls, x, y, w, h] in the reference's order: images ascending (collate_fn),
// inside an image the primary mosaic's tiles in tile order and then the partner's, survivors in source order.  The order comes from a
// stable scan, not from atomics: one workgroup per image walks the image's rows 256 at a time, scans the keep flags and writes the
// survivors to `tmp` at the image's own row range; a second launch sums the counts of the images in front (B is a batch size: every
// workgroup reads at most B counts) and copies each image's survivors to their place.  The capacity of `out` is L_in: no overflow.
// table [B][2][4][6] int32 = {row0, row1, h, w, padw, padh} per (image, mosaic, tile): rows [row0, row1) of `labels`; the ranges
// ascend without gaps inside an image and do not overlap between images (the binding checks this before the launch).
struct LtArgs {
    const float* labels;        // (L,5) cls, x, y, w, h normalised to the source image
    const int* table;
    const double* M;            // [B][2][9]
    const double* s;            // [B][2]
    const int* flags;           // [B][3] has_mix, flipud, fliplr
    float* tmp;                 // (L,6)
    int* counts;                // [B]
    int B, S, L;
};

__global__ __launch_bounds__(256) void labeled_targets_kernel(LtArgs a) {
    __shared__ int tab[48];
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 48) tab[tid] = a.table[b * 48 + tid];
    __syncthreads();
    const int r0 = max(tab[0], 0), r1 = min(tab[7 * 6 + 1], a.L);
    const int ud = a.flags[b * 3 + 1], lr = a.flags[b * 3 + 2];
    const float S = (float)a.S, hi = (float)((double)a.S - 1e-3);
    int run = 0;
    for (int base = r0; base < r1; base += 256) {
        const int row = base + tid;
        int keep = 0, k = -1;
        float o[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (row < r1)
            for (int q = 0; q < 8; ++q)
                if (row >= tab[q * 6] && row < tab[q * 6 + 1]) k = q;
        if (k >= 0) {
            const float* lb = a.labels + (size_t)row * 5;
            const float fw = (float)tab[k * 6 + 3], fh = (float)tab[k * 6 + 2], pw = (float)tab[k * 6 + 4], ph = (float)tab[k * 6 + 5];
            const float x1 = fw * (lb[1] - lb[3] / 2) + pw, y1 = fh * (lb[2] - lb[4] / 2) + ph;
            const float x2 = fw * (lb[1] + lb[3] / 2) + pw, y2 = fh * (lb[2] + lb[4] / 2) + ph;
            const double* M = a.M + ((size_t)b * 2 + (k >> 2)) * 9;
            const double X[4] = {x1, x2, x1, x2}, Y[4] = {y1, y2, y2, y1};
            double xmin = 0, xmax = 0, ymin = 0, ymax = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double u = X[c] * M[0] + Y[c] * M[1] + M[2], v = X[c] * M[3] + Y[c] * M[4] + M[5];
                xmin = c ? fmin(xmin, u) : u; xmax = c ? fmax(xmax, u) : u;
                ymin = c ? fmin(ymin, v) : v; ymax = c ? fmax(ymax, v) : v;
            }
            const double dS = (double)a.S;
            xmin = fmin(fmax(xmin, 0.0), dS); xmax = fmin(fmax(xmax, 0.0), dS);
            ymin = fmin(fmax(ymin, 0.0), dS); ymax = fmin(fmax(ymax, 0.0), dS);
            const float sf = (float)a.s[b * 2 + (k >> 2)];
            const float w1 = x2 * sf - x1 * sf, h1 = y2 * sf - y1 * sf;
            const double w2 = xmax - xmin, h2 = ymax - ymin;
            const double ar = fmax(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16));
            const float den = w1 * h1 + 1e-16f;
            keep = (w2 > 2.0) && (h2 > 2.0) && (w2 * h2 / (double)den > 0.1) && (ar < 20.0);
            const float a0 = fminf(fmaxf((float)xmin, 0.f), hi), a1 = fminf(fmaxf((float)ymin, 0.f), hi);
            const float a2 = fminf(fmaxf((float)xmax, 0.f), hi), a3 = fminf(fmaxf((float)ymax, 0.f), hi);
            float cx = ((a0 + a2) / 2) / S, cy = ((a1 + a3) / 2) / S;
            const float bw = (a2 - a0) / S, bh = (a3 - a1) / S;
            if (ud) cy = 1 - cy;
            if (lr) cx = 1 - cx;
            o[0] = lb[0];
            o[1] = fminf(fmaxf(cx, 0.f), 1.f); o[2] = fminf(fmaxf(cy, 0.f), 1.f);
            o[3] = fminf(fmaxf(bw, 0.f), 1.f); o[4] = fminf(fmaxf(bh, 0.f), 1.f);
        }
        int inc = keep;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(inc, d);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wsum[w];
        const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (keep) {
            float* d = a.tmp + (size_t)(r0 + run + woff + inc - 1) * 6;
            d[0] = (float)b; d[1] = o[0]; d[2] = o[1]; d[3] = o[2]; d[4] = o[3]; d[5] = o[4];
        }
        run += tot;
        __syncthreads();
    }
    if (tid == 0) a.counts[b] = run;
}

__global__ __launch_bounds__(256) void labeled_targets_compact_kernel(const float* __restrict__ tmp, const int* __restrict__ counts,
                                                                      const int* __restrict__ table, float* __restrict__ out,
                                                                      int* __restrict__ n_out, int B) {
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int part = 0;
    for (int i = tid; i < b; i += 256) part += counts[i];
    part = et_wave_sum_i(part);
    if ((tid & 63) == 0) wsum[tid >> 6] = part;
    __syncthreads();
    const int off = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const int cnt = counts[b], r0 = table[b * 48];
    for (int i = tid; i < cnt * 6; i += 256) out[(size_t)off * 6 + i] = tmp[(size_t)r0 * 6 + i];
    if (b == B - 1 && tid == 0) *n_out = off + cnt;
}

extern "C" int et_labeled_mosaic_targets(const float* labels, int L_in, const int* table, const double* M, const double* s,
                                         const int* flags, int B, int S, float* tmp, int* counts, float* out, int* n_out,
                                         et_stream_t stream) {
    if (!labels || !table || !M || !s || !flags || !tmp || !counts || !out || !n_out) return -1;
    if (B <= 0 || S <= 0 || L_in <= 0 || L_in > (1 << 28)) return -2;
    LtArgs a;
    a.labels = labels; a.table = table; a.M = M; a.s = s; a.flags = flags; a.tmp = tmp; a.counts = counts;
    a.B = B; a.S = S; a.L = L_in;
    hipLaunchKernelGGL(labeled_targets_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
    ET_CHECK_LAUNCH();
    hipLaunchKernelGGL(labeled_targets_compact_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const float*)tmp, (const int*)counts,
                       table, out, n_out, B);
    ET_CHECK_LAUNCH();
    return 0;
}

// ---- letterbox batch: the OTHER branch of LoadImagesAndLabels.__getitem__ (utils/datasets.py:904-953) -------------------------------
// load_image -> letterbox(auto=False) (utils/augmentations.py:92-123: cv2.resize to new_unpad when it differs from the image, then
// copyMakeBorder with 114) -> with augment, random_perspective_keypoints' cv2.warpAffine(im, M[:2], dsize = (W, H), borderValue 114)
// (:125-167, no border argument: the output has the canvas's size), augment_hsv, flips.  Validation (rect, augment = False) takes only
// the resize and the border.  One launch per batch and no canvas: an output pixel is traced back through the flips; with has_warp its
// four bilinear taps are fetched from a VIRTUAL H x W canvas -- 114 outside the canvas (the warp's borderValue), 114 inside the
// letterbox border (copyMakeBorder's colour), the letterboxed image inside [left, left + nw) x [top, top + nh) -- and without it the
// pixel is the canvas pixel itself.  The letterboxed image is the source pixel when (nw, nh) == (w, h): the common case after
// load_image, a pad without interpolation, exact by construction.  Otherwise it is cv2.resize(im, (nw, nh), INTER_LINEAR) computed on
// the fly from four source pixels: OpenCV's 8-bit path (resize.cpp) -- per axis scale = 1 / ((double)dst / src),
// f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s, clamped to the first / last source pixel with f = 0, coefficients
// cvRound((1 - f) * 2048) and cvRound(f * 2048) as shorts; horizontal pass in int32, vertical pass
// (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.  At an exact 2:1 ratio that is (a + b + c + d + 2) >> 2, what
// mosaic4_kernel computes.  One thread makes four adjacent pixels of a row and stores one 32-bit word per plane, as
// labeled_mosaic_kernel does; W % 4 == 0 is demanded (every letterbox shape is a multiple of the stride), H != W is allowed.
// table [B][8] int64 = {device pointer of the (3, h, w) uint8 planes, h, w, nw, nh, left, top, 0}.
// PARITY: geometry, matrices and LUTs are the host's (pinned on the reference, tests/golden/letterbox.npz); the resize, the warp
// sampling and the HSV round trip restate OpenCV's published 8-bit algorithms and are unpinned (no cv2).
struct LbArgs {
    const long long* table;     // [B][8]
    unsigned char* dst;         // (B,3,H,W)
    const double* minv;         // [B][6] dst -> src affine map
    const unsigned char* lut;   // [B][3][256] or NULL
    const int* flags;           // [B][3] has_warp, flipud, fliplr
    int B, H, W;
    int border;
};

struct LbImage {
    const unsigned char* p;
    int h, w, nw, nh, left, top;
};

// one axis of cv2.resize INTER_LINEAR, 8 bit: destination index d of `dst` from `src` pixels -> first source index and the two coefficients
__device__ __forceinline__ void lb_resize_coef(int d, int dst, int src, int& s0, int& c0, int& c1) {
    const double scale = 1.0 / ((double)dst / (double)src);
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= src - 1) { s = src - 1; f = 0.f; }
    s0 = s;
    c0 = aug_round((double)((1.f - f) * 2048.f)); c1 = aug_round((double)(f * 2048.f));      // saturate_cast<short>: both lie in [0, 2048]
}

// the letterboxed image at (x, y) of its nw x nh extent, three planes
__device__ __forceinline__ void lb_pixel(const LbImage& im, int x, int y, int px[3]) {
    const size_t pl = (size_t)im.h * im.w;
    if (im.nw == im.w && im.nh == im.h) {
        const size_t o = (size_t)y * im.w + x;
        px[0] = im.p[o]; px[1] = im.p[pl + o]; px[2] = im.p[2 * pl + o];
        return;
    }
    int sx, a0, a1, sy, b0, b1;
    lb_resize_coef(x, im.nw, im.w, sx, a0, a1);
    lb_resize_coef(y, im.nh, im.h, sy, b0, b1);
    const int sx1 = min(sx + 1, im.w - 1), sy1 = min(sy + 1, im.h - 1);
    const size_t r0 = (size_t)sy * im.w, r1 = (size_t)sy1 * im.w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned char* p = im.p + c * pl;
        const int S0 = a0 * p[r0 + sx] + a1 * p[r0 + sx1], S1 = a0 * p[r1 + sx] + a1 * p[r1 + sx1];
        px[c] = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
    }
}

// the virtual canvas at (cx, cy): border outside the canvas and inside the letterbox border, the letterboxed image elsewhere
__device__ __forceinline__ void lb_canvas(const LbImage& im, int cx, int cy, int border, int px[3]) {
    const int x = cx - im.left, y = cy - im.top;           // outside the canvas implies outside the rectangle: the binding checks that
    if ((unsigned)x < (unsigned)im.nw && (unsigned)y < (unsigned)im.nh) lb_pixel(im, x, y, px);
    else px[0] = px[1] = px[2] = border;
}

__global__ __launch_bounds__(256) void letterbox_kernel(LbArgs a) {
    const int b = blockIdx.y;
    const int H = a.H, W = a.W, G = W >> 2;                  // G groups of four pixels per row
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * G) return;
    const long long* t = a.table + (size_t)b * 8;
    LbImage im;
    im.p = (const unsigned char*)(uintptr_t)t[0];
    im.h = (int)t[1]; im.w = (int)t[2]; im.nw = (int)t[3]; im.nh = (int)t[4]; im.left = (int)t[5]; im.top = (int)t[6];
    const int oy = i / G, ox0 = (i - oy * G) * 4;
    const int* fl = a.flags + b * 3;
    const int has_warp = fl[0], ud = fl[1], lr = fl[2];
    const int y = ud ? H - 1 - oy : oy;                      // position before the flips
    const double* M = a.minv + (size_t)b * 6;
    const unsigned char* L = a.lut ? a.lut + (size_t)b * 768 : nullptr;
    unsigned word[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ox = ox0 + j;
        const int x = lr ? W - 1 - ox : ox;
        int px[3];
        if (has_warp) {
            int sx, sy, w[4];
            aug_warp_taps(M, x, y, sx, sy, w);
            int acc[3] = {1 << 14, 1 << 14, 1 << 14};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int cy = sy + (k >> 1), cx = sx + (k & 1);
                int tp[3];
                if ((unsigned)cx < (unsigned)W && (unsigned)cy < (unsigned)H) lb_canvas(im, cx, cy, a.border, tp);
                else tp[0] = tp[1] = tp[2] = a.border;
                acc[0] += w[k] * tp[0]; acc[1] += w[k] * tp[1]; acc[2] += w[k] * tp[2];
            }
            px[0] = acc[0] >> 15; px[1] = acc[1] >> 15; px[2] = acc[2] >> 15;
        } else {
            lb_canvas(im, x, y, a.border, px);
        }
        if (L) aug_hsv_lut(L, px[0], px[1], px[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) word[c] |= (unsigned)px[c] << (8 * j);
    }
    const size_t plane = (size_t)H * W;
    unsigned char* o = a.dst + (size_t)b * 3 * plane + (size_t)oy * W + ox0;
#pragma unroll
    for (int c = 0; c < 3; ++c) *(unsigned*)(o + c * plane) = word[c];
}

extern "C" int et_letterbox_u8(const int64_t* table, const double* minv, const uint8_t* lut, const int* flags, uint8_t* out, int B,
                               int H, int W, int border_value, et_stream_t stream) {
    if (!table || !minv || !flags || !out) return -1;
    if (B <= 0 || B > 65535 || H <= 0 || H > 16384 || W <= 0 || W > 16384 || (W & 3) != 0) return -2;
    if (((uintptr_t)out & 3) != 0) return -3;                   // the 32-bit stores
    LbArgs a;
    a.table = (const long long*)table; a.dst = out; a.minv = minv; a.lut = lut; a.flags = flags;
    a.B = B; a.H = H; a.W = W; a.border = border_value;
    hipLaunchKernelGGL(letterbox_kernel, dim3(et_cdiv((long long)H * (W >> 2), 256), B), dim3(256), 0, (hipStream_t)stream, a);
    ET_CHECK_LAUNCH();
    return 0;
}

// ---- labels of the letterbox batch ---------------------------------------------------------------------------------------------------
// Per source label (float32), the reference's arithmetic in the reference's dtypes: xywhn2xyxy(ratio_w * w, ratio_h * h, padw, padh)
// (utils/general.py:640); with has_warp the num_points == 0 label path of random_perspective_keypoints (utils/augmentations.py:176-193,
// 261-264: corners times M in fp64, min / max, clip x to [0, W] and y to [0, H], box_candidates(box1 = xyxy_f32 * s, area_thr 0.10), the
// new box assigned back to float32); xyxy2xywhn(w = W, h = H, clip to W - 1e-3 / H - 1e-3) (general.py:649-658); the flips as 1 - v;
// clip(0, 1) (datasets.py:1027).  geom [B][4] fp64 = {ratio_w * w, ratio_h * h, padw, padh}: padw = dw / 2 can be x.5 and the scalars are
// doubles in the reference, so the table is fp64 and `wide` [B] says how numpy evaluates y = w * (x - x / 2) + padw on the float32 labels:
//   0  every scalar is a Python float (img_size an int): weak, the expression is float32 throughout;
//   1  rect, ratio the Python float 1.0 of min(r, 1.0) but padw a numpy float64 (batch_shapes is a numpy array): float32 product,
//      float64 sum, rounded to float32 by the assignment;
//   2  rect, ratio a numpy float64 too: float64 product and sum, rounded to float32 by the assignment.
// rows [B][2] int32 = {row0, row1}: the image's rows of `labels`; the ranges ascend and do not overlap (the binding checks).  Output and
// order as et_labeled_mosaic_targets: one workgroup per image scans its keep flags 256 rows at a time and writes survivors to `tmp` at
// the image's own range, a second launch adds the counts of the images in front and copies.  Without has_warp every row survives.
struct LbtArgs {
    const float* labels;        // (L,5)
    const int* rows;            // [B][2]
    const double* geom;         // [B][4]
    const int* wide;            // [B]
    const double* M;            // [B][9]
    const double* s;            // [B]
    const int* flags;           // [B][3] has_warp, flipud, fliplr
    float* tmp;                 // (L,6)
    int* counts;                // [B]
    int B, H, W, L;
};

__device__ __forceinline__ float lb_xyxy(double scale, float v, double pad, int wide) {
    if (wide == 2) return (float)(scale * (double)v + pad);
    const float p = (float)scale * v;
    return wide ? (float)((double)p + pad) : p + (float)pad;
}

__global__ __launch_bounds__(256) void letterbox_targets_kernel(LbtArgs a) {
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = max(a.rows[b * 2], 0), r1 = min(a.rows[b * 2 + 1], a.L);
    const int has_warp = a.flags[b * 3], ud = a.flags[b * 3 + 1], lr = a.flags[b * 3 + 2];
    const double* g = a.geom + (size_t)b * 4;
    const int wide = a.wide[b];
    const float fW = (float)a.W, fH = (float)a.H, hiw = (float)((double)a.W - 1e-3), hih = (float)((double)a.H - 1e-3);
    int run = 0;
    for (int base = r0; base < r1; base += 256) {
        const int row = base + tid;
        int keep = 0;
        float o[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (row < r1) {
            const float* lb = a.labels + (size_t)row * 5;
            float x1 = lb_xyxy(g[0], lb[1] - lb[3] / 2, g[2], wide), y1 = lb_xyxy(g[1], lb[2] - lb[4] / 2, g[3], wide);
            float x2 = lb_xyxy(g[0], lb[1] + lb[3] / 2, g[2], wide), y2 = lb_xyxy(g[1], lb[2] + lb[4] / 2, g[3], wide);
            keep = 1;
            if (has_warp) {
                const double* M = a.M + (size_t)b * 9;
                const double X[4] = {x1, x2, x1, x2}, Y[4] = {y1, y2, y2, y1};
                double xmin = 0, xmax = 0, ymin = 0, ymax = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double u = X[c] * M[0] + Y[c] * M[1] + M[2], v = X[c] * M[3] + Y[c] * M[4] + M[5];
                    xmin = c ? fmin(xmin, u) : u; xmax = c ? fmax(xmax, u) : u;
                    ymin = c ? fmin(ymin, v) : v; ymax = c ? fmax(ymax, v) : v;
                }
                const double dW = (double)a.W, dH = (double)a.H;
                xmin = fmin(fmax(xmin, 0.0), dW); xmax = fmin(fmax(xmax, 0.0), dW);
                ymin = fmin(fmax(ymin, 0.0), dH); ymax = fmin(fmax(ymax, 0.0), dH);
                const float sf = (float)a.s[b];
                const float w1 = x2 * sf - x1 * sf, h1 = y2 * sf - y1 * sf;
                const double w2 = xmax - xmin, h2 = ymax - ymin;
                const double ar = fmax(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16));
                const float den = w1 * h1 + 1e-16f;
                keep = (w2 > 2.0) && (h2 > 2.0) && (w2 * h2 / (double)den > 0.1) && (ar < 20.0);
                x1 = (float)xmin; y1 = (float)ymin; x2 = (float)xmax; y2 = (float)ymax;
            }
            const float a0 = fminf(fmaxf(x1, 0.f), hiw), a1 = fminf(fmaxf(y1, 0.f), hih);
            const float a2 = fminf(fmaxf(x2, 0.f), hiw), a3 = fminf(fmaxf(y2, 0.f), hih);
            float cx = ((a0 + a2) / 2) / fW, cy = ((a1 + a3) / 2) / fH;
            const float bw = (a2 - a0) / fW, bh = (a3 - a1) / fH;
            if (ud) cy = 1 - cy;
            if (lr) cx = 1 - cx;
            o[0] = lb[0];
            o[1] = fminf(fmaxf(cx, 0.f), 1.f); o[2] = fminf(fmaxf(cy, 0.f), 1.f);
            o[3] = fminf(fmaxf(bw, 0.f), 1.f); o[4] = fminf(fmaxf(bh, 0.f), 1.f);
        }
        int inc = keep;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(inc, d);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += wsum[w];
        const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (keep) {
            float* d = a.tmp + (size_t)(r0 + run + woff + inc - 1) * 6;
            d[0] = (float)b; d[1] = o[0]; d[2] = o[1]; d[3] = o[2]; d[4] = o[3]; d[5] = o[4];
        }
        run += tot;
        __syncthreads();
    }
    if (tid == 0) a.counts[b] = run;
}

__global__ __launch_bounds__(256) void letterbox_targets_compact_kernel(const float* __restrict__ tmp, const int* __restrict__ counts,
                                                                        const int* __restrict__ rows, float* __restrict__ out,
                                                                        int* __restrict__ n_out, int B) {
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    int part = 0;
    for (int i = tid; i < b; i += 256) part += counts[i];
    part = et_wave_sum_i(part);
    if ((tid & 63) == 0) wsum[tid >> 6] = part;
    __syncthreads();
    const int off = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const int cnt = counts[b], r0 = max(rows[b * 2], 0);
    for (int i = tid; i < cnt * 6; i += 256) out[(size_t)off * 6 + i] = tmp[(size_t)r0 * 6 + i];
    if (b == B - 1 && tid == 0) *n_out = off + cnt;
}

extern "C" int et_letterbox_targets(const float* labels, int L_in, const int* rows, const double* geom, const int* wide, const double* M,
                                    const double* s, const int* flags, int B, int H, int W, float* tmp, int* counts, float* out,
                                    int* n_out, et_stream_t stream) {
    if (!labels || !rows || !geom || !wide || !M || !s || !flags || !tmp || !counts || !out || !n_out) return -1;
    if (B <= 0 || H <= 0 || W <= 0 || L_in <= 0 || L_in > (1 << 28)) return -2;
    LbtArgs a;
    a.labels = labels; a.rows = rows; a.geom = geom; a.wide = wide; a.M = M; a.s = s; a.flags = flags; a.tmp = tmp; a.counts = counts;
    a.B = B; a.H = H; a.W = W; a.L = L_in;
    hipLaunchKernelGGL(letterbox_targets_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
    ET_CHECK_LAUNCH();
    hipLaunchKernelGGL(letterbox_targets_compact_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const float*)tmp,
                       (const int*)counts, rows, out, n_out, B);
    ET_CHECK_LAUNCH();
    return 0;
}
