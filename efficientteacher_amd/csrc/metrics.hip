// Detection metrics on the device: the mAP bookkeeping of the reference's validation loop (val.py:339-403) --
// scale_coords + clip_coords (utils/general.py:702-773), box_iou (utils/metrics.py:252-274), process_batch
// (val.py:123-145) and ap_per_class / compute_ap (utils/metrics.py:22-126) -- with no host round trip.
//
// No FMA contraction in this file (the pragma below; it reaches the gfx950 build and the host build of the CPU test
// tier alike): every decision is an fp32 comparison of values the reference rounds op by op.
//
//   et_val_match : one workgroup per image.  Labels and detections go to native image space in fp32 exactly as the
//                  reference does it on CPU tensors -- subtract pad, TRUE fp32 division by gain (not a multiplication
//                  by the reciprocal), clamp -- then, per detection d, one arg-max over the class-matching labels
//                      l*(d) = argmax_l iou(l, d)          (equal IoU: the lower label index)
//                  and  correct[d, i] = iou(d, l*(d)) >= iouv[i]  and no d' < d with l*(d') == l*(d) has
//                  iou(d', l*(d')) >= iouv[i].  That is what process_batch's sort / np.unique / np.unique leaves
//                  (DESIGN.md "Validation metrics"): the first unique keeps each detection's best label, the second
//                  keeps each label's LOWEST detection index, and l*(d) does not depend on the threshold.  The
//                  "no earlier detection" test is a scan over the earlier detections' (l*, threshold mask) pairs
//                  in LDS (max_det^2 / 256 integer compares per thread), so there is no table sized by the label
//                  count and no limit on labels per image; labels stream through LDS in tiles of 256 target rows.
//   et_val_ap    : grid (class, threshold) over the rows ordered by (class, conf descending).  One forward
//                  reduction gives the segment's TP total; one REVERSE pass in tiles of 256 rows with a carry gives
//                  tpc = total - (TPs behind the row), recall, precision and the precision envelope (a suffix max),
//                  and every row writes the interpolation points that fall into its own recall (AP, 101 points) or
//                  confidence (P / R / F1 curves, 1000 points, threshold 0 only) interval.  Integer counts, fp64
//                  arithmetic in numpy's operation order, no float atomics: results do not depend on scheduling.
//   et_val_confusion : the reference's ConfusionMatrix.process_batch (utils/metrics.py:137-175) in closed form, one
//                  workgroup per image, the same label tiles and the same IoU arithmetic as et_val_match (an IoU has the
//                  same bits in both).  Only images with a label AND an NMS detection count.  Detections with
//                  conf > conf_thres (strict) take part; the IoU is class-agnostic; a pair qualifies if iou > iou_thres
//                  (strict).  l*(d) = the qualifying label of largest IoU (equal IoU: the LOWER label index); label l
//                  is matched to d*(l) = the detection of LARGEST IoU among {d : l*(d) = l} (equal IoU: the LOWER
//                  detection index) -- the re-sort by IoU that process_batch of val.py leaves out is present here
//                  (utils/metrics.py:158).  matrix[predicted, true], row / column nc = background:
//                      every label l            : matrix[nc, cls(l)] += 1
//                      every winner d = d*(l)   : matrix[nc, cls(l)] -= 1, matrix[cls(d), cls(l)] += 1
//                      if the image has a match : every other filtered detection d: matrix[cls(d), nc] += 1
//                  (an image whose detections match nothing adds nothing to column nc: the reference's behaviour).
//                  int32 atomics only: exact, commutative, two runs are bit-identical.  "d is a winner" is the scan
//                  over the (l*, IoU) pairs in LDS that val_match_kernel does over (l*, mask).
//   et_val_predn : elementwise, one thread per (image, NMS slot): scale_coords + clip_coords of the box (val.py:355-356)
//                  with conf and class copied, and the top-left xywh save_one_json derives from it (val.py:70-71).
#pragma clang fp contract(off)
#include "et_device.h"
#include "../../include/et_hip.h"

#define VM_THREADS 256
#define VM_MAX_DET 1024
#define VM_PER (VM_MAX_DET / VM_THREADS)
#define VM_MAX_IOU 16
#define VM_CURVE 1000

struct VmBox { float x1, y1, x2, y2; };

// scale_coords(ratio_pad given) + clip_coords, utils/general.py:711-714 and :770-773
__device__ __forceinline__ VmBox vm_to_native(VmBox b, float gain, float padx, float pady, float w0, float h0) {
    b.x1 = (b.x1 - padx) / gain; b.x2 = (b.x2 - padx) / gain;
    b.y1 = (b.y1 - pady) / gain; b.y2 = (b.y2 - pady) / gain;
    b.x1 = fminf(fmaxf(b.x1, 0.0f), w0); b.y1 = fminf(fmaxf(b.y1, 0.0f), h0);
    b.x2 = fminf(fmaxf(b.x2, 0.0f), w0); b.y2 = fminf(fmaxf(b.y2, 0.0f), h0);
    return b;
}

__global__ __launch_bounds__(VM_THREADS) void val_match_kernel(
    const float* __restrict__ dets, int det_stride, const int* __restrict__ counts, int max_det,
    const float* __restrict__ targets, int NT, const float* __restrict__ shapes, float net_h, float net_w,
    const float* __restrict__ iouv, int niou, int single_cls, int nc, long long row0, int* __restrict__ correct,
    float* __restrict__ conf, int* __restrict__ cls, int* __restrict__ valid, int* __restrict__ nt) {
    __shared__ VmBox l_box[VM_THREADS];
    __shared__ float l_area[VM_THREADS];
    __shared__ float l_cls[VM_THREADS];
    __shared__ int l_ok[VM_THREADS];
    __shared__ int s_best[VM_MAX_DET];
    __shared__ int s_mask[VM_MAX_DET];
    __shared__ float s_iouv[VM_MAX_IOU];
    const int si = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[si], 0), max_det);
    const float* sh = shapes + (size_t)si * 5;
    const float gain = sh[0], padx = sh[1], pady = sh[2], h0 = sh[3], w0 = sh[4];
    if (tid < niou) s_iouv[tid] = iouv[tid];

    VmBox db[VM_PER];
    float da[VM_PER], dc[VM_PER], dconf[VM_PER], best[VM_PER];
    int bl[VM_PER];
#pragma unroll
    for (int q = 0; q < VM_PER; ++q) {
        const int d = tid + q * VM_THREADS;
        best[q] = -1.0f; bl[q] = -1; da[q] = 0.f; dc[q] = -1.0f; dconf[q] = 0.f;
        db[q].x1 = db[q].y1 = db[q].x2 = db[q].y2 = 0.f;
        if (d < n) {
            const float* r = dets + ((size_t)si * max_det + d) * det_stride;
            VmBox b; b.x1 = r[0]; b.y1 = r[1]; b.x2 = r[2]; b.y2 = r[3];
            db[q] = vm_to_native(b, gain, padx, pady, w0, h0);
            da[q] = (db[q].x2 - db[q].x1) * (db[q].y2 - db[q].y1);
            dconf[q] = r[4];
            dc[q] = single_cls ? 0.0f : r[5];                         // val.py:353-354
        }
    }

    for (int base = 0; base < NT; base += VM_THREADS) {
        __syncthreads();
        const int t = base + tid;
        int ok = 0;
        if (t < NT) {
            const float* g = targets + (size_t)t * 6;
            if (g[0] == (float)si) {                                   // val.py:341
                ok = 1;
                const float c = g[1];
                const float x = g[2] * net_w, y = g[3] * net_h, w = g[4] * net_w, h = g[5] * net_h;   // val.py:328
                VmBox b;                                               // xywh2xyxy, utils/general.py:630
                b.x1 = x - w / 2; b.y1 = y - h / 2; b.x2 = x + w / 2; b.y2 = y + h / 2;
                b = vm_to_native(b, gain, padx, pady, w0, h0);
                l_box[tid] = b;
                l_area[tid] = (b.x2 - b.x1) * (b.y2 - b.y1);
                l_cls[tid] = c;
                if (c >= 0.0f && c < (float)nc) atomicAdd(&nt[(int)c], 1);   // val.py:403 bincount of the label classes
            }
        }
        l_ok[tid] = ok;
        __syncthreads();
        const int lim = min(VM_THREADS, NT - base);
        for (int k = 0; k < lim; ++k) {
            if (!l_ok[k]) continue;                                    // block-uniform
            const VmBox lb = l_box[k];
            const float la = l_area[k], lc = l_cls[k];
#pragma unroll
            for (int q = 0; q < VM_PER; ++q) {
                if (lc == dc[q]) {                                     // val.py:134 (padding rows carry class -1)
                    const float iw = fmaxf(fminf(lb.x2, db[q].x2) - fmaxf(lb.x1, db[q].x1), 0.0f);
                    const float ih = fmaxf(fminf(lb.y2, db[q].y2) - fmaxf(lb.y1, db[q].y1), 0.0f);
                    const float inter = iw * ih;
                    const float iou = inter / (la + da[q] - inter);    // utils/metrics.py:274
                    if (iou > best[q]) { best[q] = iou; bl[q] = base + k; }   // strict: the lower label index keeps a tie
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < VM_PER; ++q) {
        const int d = tid + q * VM_THREADS;
        int m = 0;
        if (d < n && bl[q] >= 0)
            for (int i = 0; i < niou; ++i) m |= best[q] >= s_iouv[i] ? (1 << i) : 0;
        if (d < max_det) { s_best[d] = bl[q]; s_mask[d] = m; }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < VM_PER; ++q) {
        const int d = tid + q * VM_THREADS;
        if (d >= max_det) continue;
        int m = s_mask[d];
        if (m) {
            int taken = 0;                                             // thresholds at which an earlier detection holds l*(d)
            for (int e = 0; e < d; ++e) taken |= s_best[e] == bl[q] ? s_mask[e] : 0;
            m &= ~taken;
        }
        const long long row = row0 + (long long)si * max_det + d;
        const bool v = d < n;
        correct[row] = m;
        conf[row] = dconf[q];
        cls[row] = v ? (int)dc[q] : -1;
        valid[row] = v ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// class column of a label / detection: truncation towards zero like .int() (utils/metrics.py:148-149); -1 = outside [0, nc)
__device__ __forceinline__ int vm_class(float c, int nc) { return (c > -1.0f && c < (float)nc) ? (int)c : -1; }

__global__ __launch_bounds__(VM_THREADS) void val_confusion_kernel(
    const float* __restrict__ dets, int det_stride, const int* __restrict__ counts, int max_det,
    const float* __restrict__ targets, int NT, const float* __restrict__ shapes, float net_h, float net_w,
    float conf_thres, float iou_thres, int single_cls, int nc, int* __restrict__ matrix) {
    __shared__ VmBox l_box[VM_THREADS];
    __shared__ float l_area[VM_THREADS];
    __shared__ int l_cls[VM_THREADS];
    __shared__ int l_ok[VM_THREADS];
    __shared__ int s_best[VM_MAX_DET];
    __shared__ float s_iou[VM_MAX_DET];
    __shared__ int s_any;
    const int si = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(counts[si], 0), max_det);
    if (n == 0) return;                                                // val.py:347-350: not even the labels count
    const float* sh = shapes + (size_t)si * 5;
    const float gain = sh[0], padx = sh[1], pady = sh[2], h0 = sh[3], w0 = sh[4];
    if (tid == 0) s_any = 0;

    VmBox db[VM_PER];
    float da[VM_PER], best[VM_PER];
    int dcl[VM_PER], bl[VM_PER], blc[VM_PER];
    bool keep[VM_PER];
#pragma unroll
    for (int q = 0; q < VM_PER; ++q) {
        const int d = tid + q * VM_THREADS;
        best[q] = -1.0f; bl[q] = -1; blc[q] = -1; da[q] = 0.f; dcl[q] = -1; keep[q] = false;
        db[q].x1 = db[q].y1 = db[q].x2 = db[q].y2 = 0.f;
        if (d < n) {
            const float* r = dets + ((size_t)si * max_det + d) * det_stride;
            if (r[4] > conf_thres) {                                   // utils/metrics.py:147, strict
                keep[q] = true;
                VmBox b; b.x1 = r[0]; b.y1 = r[1]; b.x2 = r[2]; b.y2 = r[3];
                db[q] = vm_to_native(b, gain, padx, pady, w0, h0);
                da[q] = (db[q].x2 - db[q].x1) * (db[q].y2 - db[q].y1);
                dcl[q] = single_cls ? 0 : vm_class(r[5], nc);          // val.py:353-354
            }
        }
    }

    const int bg = nc * (nc + 1);                                      // row nc: background
    for (int base = 0; base < NT; base += VM_THREADS) {
        __syncthreads();
        const int t = base + tid;
        int ok = 0;
        if (t < NT) {
            const float* g = targets + (size_t)t * 6;
            if (g[0] == (float)si) {                                   // val.py:341
                ok = 1;
                VmBox b;
                if (net_w == 0.0f) {                                   // corner rows [img, cls, x1, y1, x2, y2]: process_batch's labels
                    b.x1 = g[2]; b.y1 = g[3]; b.x2 = g[4]; b.y2 = g[5];
                } else {
                    const float x = g[2] * net_w, y = g[3] * net_h, w = g[4] * net_w, h = g[5] * net_h;   // val.py:328
                    b.x1 = x - w / 2; b.y1 = y - h / 2; b.x2 = x + w / 2; b.y2 = y + h / 2;   // xywh2xyxy, utils/general.py:630
                }
                b = vm_to_native(b, gain, padx, pady, w0, h0);
                const int c = vm_class(g[1], nc);
                l_box[tid] = b;
                l_area[tid] = (b.x2 - b.x1) * (b.y2 - b.y1);
                l_cls[tid] = c;
                if (c >= 0) atomicAdd(&matrix[bg + c], 1);             // unmatched until a winner takes it back
            }
        }
        l_ok[tid] = ok;
        __syncthreads();
        const int lim = min(VM_THREADS, NT - base);
        for (int k = 0; k < lim; ++k) {
            if (!l_ok[k]) continue;                                    // block-uniform
            const VmBox lb = l_box[k];
            const float la = l_area[k];
            const int lc = l_cls[k];
#pragma unroll
            for (int q = 0; q < VM_PER; ++q) {
                if (keep[q]) {                                         // class-agnostic, utils/metrics.py:150
                    const float iw = fmaxf(fminf(lb.x2, db[q].x2) - fmaxf(lb.x1, db[q].x1), 0.0f);
                    const float ih = fmaxf(fminf(lb.y2, db[q].y2) - fmaxf(lb.y1, db[q].y1), 0.0f);
                    const float inter = iw * ih;
                    const float iou = inter / (la + da[q] - inter);    // utils/metrics.py:274
                    // :152 strict; strict again: the lower label index keeps a tie
                    if (iou > iou_thres && iou > best[q]) { best[q] = iou; bl[q] = base + k; blc[q] = lc; }
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < VM_PER; ++q) {
        const int d = tid + q * VM_THREADS;
        if (d < n) { s_best[d] = bl[q]; s_iou[d] = best[q]; }
        if (bl[q] >= 0) s_any = 1;                                     // every chosen label has a winner: the image has a match
    }
    __syncthreads();
    const int any = s_any;
#pragma unroll
    for (int q = 0; q < VM_PER; ++q) {
        const int d = tid + q * VM_THREADS;
        if (!keep[q]) continue;
        bool win = bl[q] >= 0;
        if (win)
            for (int e = 0; e < n; ++e)                                // :158-159: the label keeps its detection of largest IoU
                if (s_best[e] == bl[q] && (s_iou[e] > best[q] || (s_iou[e] == best[q] && e < d))) { win = false; break; }
        if (win) {
            if (blc[q] >= 0) {
                atomicAdd(&matrix[bg + blc[q]], -1);
                if (dcl[q] >= 0) atomicAdd(&matrix[dcl[q] * (nc + 1) + blc[q]], 1);   // :168
            }
        } else if (any && dcl[q] >= 0) {
            atomicAdd(&matrix[dcl[q] * (nc + 1) + nc], 1);             // :172-175
        }
    }
}

__global__ __launch_bounds__(VM_THREADS) void val_predn_kernel(const float* __restrict__ dets, int det_stride,
                                                               const int* __restrict__ counts, long long rows, int max_det,
                                                               const float* __restrict__ shapes, int single_cls,
                                                               float* __restrict__ predn, float* __restrict__ xywh_tl) {
    const long long row = (long long)blockIdx.x * VM_THREADS + threadIdx.x;
    if (row >= rows) return;
    const int si = (int)(row / max_det), d = (int)(row - (long long)si * max_det);
    float o[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, t[4] = {0.f, 0.f, 0.f, 0.f};
    if (d < min(max(counts[si], 0), max_det)) {
        const float* sh = shapes + (size_t)si * 5;
        const float* r = dets + (size_t)row * det_stride;
        VmBox b; b.x1 = r[0]; b.y1 = r[1]; b.x2 = r[2]; b.y2 = r[3];
        b = vm_to_native(b, sh[0], sh[1], sh[2], sh[4], sh[3]);
        o[0] = b.x1; o[1] = b.y1; o[2] = b.x2; o[3] = b.y2; o[4] = r[4];
        o[5] = single_cls ? 0.0f : r[5];                               // val.py:353-354
        const float w = b.x2 - b.x1, h = b.y2 - b.y1;                  // xyxy2xywh, utils/general.py:549-556
        t[0] = (b.x1 + b.x2) / 2 - w / 2;                              // val.py:71: centre to top-left corner
        t[1] = (b.y1 + b.y2) / 2 - h / 2;
        t[2] = w; t[3] = h;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) predn[row * 6 + k] = o[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) xywh_tl[row * 4 + k] = t[k];
}

// ------------------------------------------------------------------------------------------------------------------
// seg[c] = first row of class c in the class-sorted rows (rows of padding carry a class >= nc), c = 0..nc
__global__ __launch_bounds__(VM_THREADS) void val_ap_bounds_kernel(const int* __restrict__ cls, long long N, int nc,
                                                                   int* __restrict__ seg) {
    const int c = blockIdx.x * VM_THREADS + threadIdx.x;
    if (c > nc) return;
    long long lo = 0, hi = N;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (cls[mid] < c) lo = mid + 1; else hi = mid;
    }
    seg[c] = (int)lo;
}

// np.linspace(0, 1, num)[i] = i * (1 / (num - 1)), the last point exactly 1
__device__ __forceinline__ double vm_x101(int k) { return k == 100 ? 1.0 : (double)k * (1.0 / 100.0); }
__device__ __forceinline__ double vm_px(int i) { return i == VM_CURVE - 1 ? 1.0 : (double)i * (1.0 / (double)(VM_CURVE - 1)); }

__global__ __launch_bounds__(VM_THREADS) void val_ap_kernel(const int* __restrict__ seg, const int* __restrict__ correct,
                                                            const float* __restrict__ conf, const int* __restrict__ nt,
                                                            int niou, double* __restrict__ ap, double* __restrict__ p,
                                                            double* __restrict__ r, double* __restrict__ f1) {
    __shared__ int s_wi[4];
    __shared__ double s_wd[4];
    __shared__ double s_rec[VM_THREADS + 1], s_env[VM_THREADS + 1], s_prec[VM_THREADS + 1];
    __shared__ float s_conf[VM_THREADS + 1];
    __shared__ double s_val[101];
    __shared__ double s_last[2];
    const int c = blockIdx.x, j = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s0 = seg[c];
    const int n = seg[c + 1] - seg[c];
    const int nl = nt[c];
    const bool curves = j == 0;
    double* pc = p + (size_t)c * VM_CURVE;
    double* rc = r + (size_t)c * VM_CURVE;
    double* fc = f1 + (size_t)c * VM_CURVE;
    if (nl <= 0 || n <= 0) {                                          // utils/metrics.py:52-53: the row stays zero
        if (tid == 0) ap[(size_t)c * niou + j] = 0.0;
        if (curves)
            for (int i = tid; i < VM_CURVE; i += VM_THREADS) { pc[i] = 0.0; rc[i] = 0.0; fc[i] = 0.0; }
        return;
    }
    const int* cor = correct + s0;
    const float* cf = conf + s0;
    for (int k = tid; k < 101; k += VM_THREADS) s_val[k] = 0.0;

    int cnt = 0;
    for (int i = tid; i < n; i += VM_THREADS) cnt += (cor[i] >> j) & 1;
    cnt = et_wave_sum_i(cnt);
    if (lane == 0) s_wi[wave] = cnt;
    __syncthreads();
    const int total = s_wi[0] + s_wi[1] + s_wi[2] + s_wi[3];
    __syncthreads();

    const double nld = (double)nl + 1e-16;                            // :60
    // what lies behind the tile: the sentinel (recall 1, precision 0) of compute_ap (:111-112) to begin with
    double c_rec = 1.0, c_env = 0.0, c_prec = 0.0;
    float c_conf = 0.0f;
    int c_after = 0;
    const int ntiles = (n + VM_THREADS - 1) / VM_THREADS;
    for (int t = ntiles - 1; t >= 0; --t) {
        const int i = t * VM_THREADS + tid;
        const bool have = i < n;
        const int b = have ? (cor[i] >> j) & 1 : 0;
        int inc = b;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) s_wi[wave] = inc;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += s_wi[w];
        const int tile_total = s_wi[0] + s_wi[1] + s_wi[2] + s_wi[3];
        const int tpc = total - (c_after + tile_total - (woff + inc));   // :57 cumsum, from the far end
        const double prec = have ? (double)tpc / (double)(i + 1) : 0.0;   // :64  tpc + fpc = rows so far
        const double rec = have ? (double)tpc / nld : 1.0;
        double m = prec;                                               // :115 envelope = suffix max
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double o = __shfl_down(m, d);
            if (lane + d < 64) m = fmax(m, o);
        }
        if (lane == 0) s_wd[wave] = m;
        __syncthreads();
        double env = fmax(m, c_env);
        for (int w = wave + 1; w < 4; ++w) env = fmax(env, s_wd[w]);
        s_rec[tid] = rec; s_env[tid] = env; s_prec[tid] = prec;
        s_conf[tid] = have ? cf[i] : 0.0f;
        if (tid == 0) { s_rec[VM_THREADS] = c_rec; s_env[VM_THREADS] = c_env; s_prec[VM_THREADS] = c_prec; s_conf[VM_THREADS] = c_conf; }
        __syncthreads();
        if (have) {
            const double rn = s_rec[tid + 1], en = s_env[tid + 1];
            if (rec < rn) {
                // np.interp(x, mrec, mpre) (:121) for the x_k in [rec, rn): this row is the right-most with mrec <= x_k
                int k = (int)(rec * 100.0) - 1;
                for (k = k < 0 ? 0 : k; k < 100; ++k) {
                    const double x = vm_x101(k);
                    if (x >= rn) break;
                    if (x < rec) continue;
                    s_val[k] = x == rec ? env : (en - env) / (rn - rec) * (x - rec) + env;
                }
            }
            if (curves) {
                if (i == n - 1) { s_last[0] = rec; s_last[1] = prec; }
                else {
                    // np.interp(-px, -conf, .) (:61, :65) for the px in (conf of the next row, this row's conf]
                    const double ch = (double)s_conf[tid], cn = (double)s_conf[tid + 1];
                    if (cn < ch) {
                        const double rn1 = s_rec[tid + 1], pn1 = s_prec[tid + 1];
                        int q = (int)(cn * (double)(VM_CURVE - 1)) - 1;
                        for (q = q < 0 ? 0 : q; q < VM_CURVE; ++q) {
                            const double x = vm_px(q);
                            if (x > ch) break;
                            if (x <= cn) continue;
                            double rv = rec, pv = prec;
                            if (x != ch) {
                                const double dx = (-cn) - (-ch), u = (-x) - (-ch);
                                rv = (rn1 - rec) / dx * u + rec;
                                pv = (pn1 - prec) / dx * u + prec;
                            }
                            rc[q] = rv; pc[q] = pv;
                            fc[q] = 2 * pv * rv / (pv + rv + 1e-16);   // :74
                        }
                    }
                }
            }
        }
        c_rec = s_rec[0]; c_env = s_env[0]; c_prec = s_prec[0]; c_conf = s_conf[0];
        c_after += tile_total;
    }
    __syncthreads();
    // the leading sentinel (recall 0, precision 1) owns the x_k below the first row's recall
    if (tid == 0) {
        const double rn = c_rec, en = c_env;
        for (int k = 0; k < 100; ++k) {
            const double x = vm_x101(k);
            if (x >= rn) break;
            s_val[k] = x == 0.0 ? 1.0 : (en - 1.0) / (rn - 0.0) * (x - 0.0) + 1.0;
        }
        s_val[100] = 0.0;                                              // x = 1 meets the trailing sentinel: precision 0
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;                                                // np.trapz (:121)
        for (int k = 0; k < 100; ++k) a += (vm_x101(k + 1) - vm_x101(k)) * (s_val[k + 1] + s_val[k]) / 2.0;
        ap[(size_t)c * niou + j] = a;
    }
    if (curves) {
        // px above the best confidence: left = 0 / 1; px at or below the last row's confidence: the last row's values
        const double cmax = (double)cf[0], cmin = (double)cf[n - 1];
        for (int q = tid; q < VM_CURVE; q += VM_THREADS) {
            const double x = vm_px(q);
            double rv, pv;
            if (x > cmax) { rv = 0.0; pv = 1.0; }
            else if (x <= cmin) { rv = s_last[0]; pv = s_last[1]; }
            else continue;
            rc[q] = rv; pc[q] = pv;
            fc[q] = 2 * pv * rv / (pv + rv + 1e-16);
        }
    }
}

extern "C" int et_val_match(const float* dets, int det_row_stride, const int* counts, int B, int max_det,
                            const float* targets, int NT, const float* shapes, int net_h, int net_w, const float* iouv,
                            int niou, int single_cls, int nc, int64_t row_offset, int64_t arena_rows, int* correct,
                            float* conf, int* cls, int* valid, int* nt, et_stream_t stream) {
    if (B < 0 || NT < 0 || max_det <= 0 || max_det > VM_MAX_DET) return -2;
    if (B == 0) return 0;
    if (det_row_stride < 6 || niou <= 0 || niou > VM_MAX_IOU || nc <= 0 || net_h <= 0 || net_w <= 0) return -2;
    if (row_offset < 0 || row_offset + (int64_t)B * max_det > arena_rows) return -2;
    if (!dets || !counts || !shapes || !iouv || !correct || !conf || !cls || !valid || !nt || (NT > 0 && !targets)) return -1;
    hipLaunchKernelGGL(val_match_kernel, dim3(B), dim3(VM_THREADS), 0, (hipStream_t)stream, dets, det_row_stride, counts,
                       max_det, targets, NT, shapes, (float)net_h, (float)net_w, iouv, niou, single_cls ? 1 : 0, nc,
                       (long long)row_offset, correct, conf, cls, valid, nt);
    ET_CHECK_LAUNCH();
    return 0;
}

extern "C" int et_val_confusion(const float* dets, int det_row_stride, const int* counts, int B, int max_det,
                                const float* targets, int NT, const float* shapes, int net_h, int net_w, float conf_thres,
                                float iou_thres, int single_cls, int nc, int* matrix, et_stream_t stream) {
    if (B < 0 || NT < 0 || max_det <= 0 || max_det > VM_MAX_DET) return -2;
    if (B == 0) return 0;
    if (det_row_stride < 6 || nc <= 0 || nc > 32767 || net_h < 0 || net_w < 0 || (net_h == 0) != (net_w == 0)) return -2;
    if (!dets || !counts || !shapes || !matrix || (NT > 0 && !targets)) return -1;
    hipLaunchKernelGGL(val_confusion_kernel, dim3(B), dim3(VM_THREADS), 0, (hipStream_t)stream, dets, det_row_stride, counts,
                       max_det, targets, NT, shapes, (float)net_h, (float)net_w, conf_thres, iou_thres, single_cls ? 1 : 0, nc,
                       matrix);
    ET_CHECK_LAUNCH();
    return 0;
}

extern "C" int et_val_predn(const float* dets, int det_row_stride, const int* counts, int B, int max_det, const float* shapes,
                            int net_h, int net_w, int single_cls, float* predn, float* xywh_tl, et_stream_t stream) {
    if (B < 0 || max_det <= 0 || max_det > VM_MAX_DET) return -2;
    if (B == 0) return 0;
    if (det_row_stride < 6 || net_h <= 0 || net_w <= 0) return -2;
    if (!dets || !counts || !shapes || !predn || !xywh_tl) return -1;
    const long long rows = (long long)B * max_det;
    hipLaunchKernelGGL(val_predn_kernel, dim3((unsigned)((rows + VM_THREADS - 1) / VM_THREADS)), dim3(VM_THREADS), 0,
                       (hipStream_t)stream, dets, det_row_stride, counts, rows, max_det, shapes, single_cls ? 1 : 0, predn,
                       xywh_tl);
    ET_CHECK_LAUNCH();
    return 0;
}

extern "C" int et_val_ap_workspace_bytes(int nc, size_t* bytes) {
    if (nc <= 0 || !bytes) return -1;
    *bytes = ((size_t)(nc + 1) * sizeof(int) + 255) & ~(size_t)255;
    return 0;
}

extern "C" int et_val_ap(const int* cls, const int* correct, const float* conf, int64_t N, const int* nt, int nc, int niou,
                         double* ap, double* p, double* r, double* f1, void* workspace, size_t ws_bytes,
                         et_stream_t stream) {
    if (!nt || !ap || !p || !r || !f1 || !workspace || (N > 0 && (!cls || !correct || !conf))) return -1;
    if (nc <= 0 || niou <= 0 || niou > VM_MAX_IOU || N < 0 || N > 0x7fffffffLL) return -2;
    if (ws_bytes < (size_t)(nc + 1) * sizeof(int)) return -3;
    int* seg = (int*)workspace;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(val_ap_bounds_kernel, dim3((nc + 1 + VM_THREADS - 1) / VM_THREADS), dim3(VM_THREADS), 0, s, cls,
                       (long long)N, nc, seg);
    hipLaunchKernelGGL(val_ap_kernel, dim3(nc, niou), dim3(VM_THREADS), 0, s, seg, correct, conf, nt, niou, ap, p, r, f1);
    ET_CHECK_LAUNCH();
    return 0;
}
