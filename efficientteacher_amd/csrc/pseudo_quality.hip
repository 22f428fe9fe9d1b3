// Pseudo-label hit rate against ground truth on the device: the five progress-bar numbers tp / fp_cls / fp_loc / pse_num /
// gt_num that the reference's rank 0 computes on the host after every SSOD step (trainer/ssod_trainer.py:655-672) with
// check_pseudo_label_with_gt (utils/self_supervised_utils.py:481-585; select_targets :456-479, xywh2xyxy utils/general.py:630,
// box_iou utils/metrics.py:252-274) or, without ground truth, check_pseudo_label (:587-609).  Input is the PADDED table
// et_pseudo_label_transform writes, so nothing is compacted and nothing is read back.
//
// No FMA contraction in this file (the pragma below reaches the gfx950 build and the host build of the CPU test tier alike):
// every decision is an fp32 comparison of values the reference rounds op by op.
//
//   pq_zero_kernel   : clears the (3, M) byte flags of the workspace on the stream.
//   pq_match_kernel  : one wave per padded row, four waves per workgroup.  A row takes part only if it is valid and UNCERTAIN
//                      (thr_low[cls] <= conf < thr_high[cls], compared in fp64 on the table's value: et_select_targets'
//                      decision; the reference drops the reliable rows at :504) -- a wave-uniform test, every other wave leaves
//                      at once.  Lanes stride over the gt rows; boxes are fp32: xywh * 640, xywh2xyxy, + img * 640 on all four
//                      coordinates (the literal 640 of :515-518, not the image size), IoU in box_iou's operation order.  Three
//                      categories of (label, pseudo) pairs of the same image:
//                          tp      iou >= 0.5 and the same class
//                          fp_cls  iou >= 0.5 and another class
//                          fp_loc  0.01 < iou < 0.5, any class
//                      Per category the row picks its qualifying label of largest IoU (equal IoU: the LOWER label index; the
//                      reference leaves that to an unstable argsort) -- lane-local scan in ascending label order, then a
//                      __shfl_xor reduction on (IoU, index) -- and lane 0 sets flag[category][label] = 1 with a plain byte
//                      store (racing writers store the same value).
//   pq_finish_kernel : one workgroup.  Counts the valid / reliable / uncertain rows and the flags of each category -- the number
//                      of DISTINCT labels picked, which is what the reference's argsort / np.unique on the detection / np.unique
//                      on the label leaves -- and writes the five fp64 results.  Integer counts, one IEEE division each: no
//                      floating-point atomics, results do not depend on scheduling.
#pragma clang fp contract(off)
#include "et_device.h"
#include "../../include/et_hip.h"

#define PQ_THREADS 256
#define PQ_WAVES (PQ_THREADS / ET_WAVE)
#define PQ_FIN_THREADS 1024         // the one workgroup of pq_finish_kernel: its loop over the rows is a chain of dependent loads
#define PQ_FIN_WAVES (PQ_FIN_THREADS / ET_WAVE)
#define PQ_REF_SIZE 640.0f          // the reference's literal (utils/self_supervised_utils.py:515-518), NOT the image size
#define PQ_IOU_HIT 0.5f             // iouv = [0.5], the only value any caller passes (:481)
#define PQ_IOU_LOC 0.01f            // :536

struct PqBox { float x1, y1, x2, y2; };

// [x, y, w, h] normalised -> * 640 (:515-516), xywh2xyxy (utils/general.py:630), + img * 640 (:517-518); all fp32
__device__ __forceinline__ PqBox pq_box(float img, float x, float y, float w, float h) {
    x = x * PQ_REF_SIZE; y = y * PQ_REF_SIZE; w = w * PQ_REF_SIZE; h = h * PQ_REF_SIZE;
    const float s = img * PQ_REF_SIZE;
    PqBox b;
    b.x1 = (x - w / 2) + s; b.y1 = (y - h / 2) + s; b.x2 = (x + w / 2) + s; b.y2 = (y + h / 2) + s;
    return b;
}

// 0 = not valid or below thr_low, 1 = reliable, 2 = uncertain (select_targets :456-479; the class index is clamped as in
// et_select_targets)
__device__ __forceinline__ int pq_row_kind(const double* __restrict__ t9, const unsigned char* __restrict__ valid, long long row,
                                           const double* __restrict__ thr_low, const double* __restrict__ thr_high, int nc) {
    if (!valid[row]) return 0;
    const double* t = t9 + (size_t)row * 9;
    int c = (int)t[1];
    c = min(max(c, 0), nc - 1);
    const double conf = t[6];
    if (conf >= thr_high[c]) return 1;
    return conf >= thr_low[c] ? 2 : 0;
}

__global__ __launch_bounds__(PQ_THREADS) void pq_zero_kernel(unsigned char* __restrict__ flags, long long n) {
    const long long i = (long long)blockIdx.x * PQ_THREADS + threadIdx.x;
    if (i < n) flags[i] = 0;
}

__global__ __launch_bounds__(PQ_THREADS) void pq_match_kernel(const double* __restrict__ t9, const unsigned char* __restrict__ valid,
                                                              int N, const float* __restrict__ gt, int M,
                                                              const double* __restrict__ thr_low,
                                                              const double* __restrict__ thr_high, int nc,
                                                              unsigned char* __restrict__ flags) {
    const int lane = threadIdx.x & (ET_WAVE - 1), wave = threadIdx.x / ET_WAVE;
    const long long row = (long long)blockIdx.x * PQ_WAVES + wave;
    if (row >= N) return;                                                       // wave-uniform, as is the next test
    if (pq_row_kind(t9, valid, row, thr_low, thr_high, nc) != 2) return;
    const double* t = t9 + (size_t)row * 9;
    const float pimg = (float)t[0], pcls = (float)t[1];                         // :474 astype(np.float32) of the whole row
    const PqBox pb = pq_box(pimg, (float)t[2], (float)t[3], (float)t[4], (float)t[5]);
    const float parea = (pb.x2 - pb.x1) * (pb.y2 - pb.y1);
    float best[3] = {-1.0f, -1.0f, -1.0f};
    int bl[3] = {M, M, M};                                                      // M = no label
    for (int l = lane; l < M; l += ET_WAVE) {
        const float* g = gt + (size_t)l * 6;
        if (g[0] != pimg) continue;                                             // :526 correct_image
        const PqBox gb = pq_box(g[0], g[2], g[3], g[4], g[5]);
        const float garea = (gb.x2 - gb.x1) * (gb.y2 - gb.y1);
        const float iw = fmaxf(fminf(gb.x2, pb.x2) - fmaxf(gb.x1, pb.x1), 0.0f);
        const float ih = fmaxf(fminf(gb.y2, pb.y2) - fmaxf(gb.y1, pb.y1), 0.0f);
        const float inter = iw * ih;
        const float iou = inter / (garea + parea - inter);                      // utils/metrics.py:274, box1 = gt
        int cat = -1;
        if (iou >= PQ_IOU_HIT) cat = g[1] == pcls ? 0 : 1;                      // :533-534
        else if (iou > PQ_IOU_LOC) cat = 2;                                     // :536 (a NaN IoU qualifies nowhere)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (cat == k && iou > best[k]) { best[k] = iou; bl[k] = l; }        // strict: the lower label index keeps a tie
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float b = best[k];
        int i = bl[k];
#pragma unroll
        for (int m = ET_WAVE / 2; m >= 1; m >>= 1) {
            const float ob = __shfl_xor(b, m);
            const int oi = __shfl_xor(i, m);
            if (ob > b || (ob == b && oi < i)) { b = ob; i = oi; }
        }
        if (lane == 0 && i < M) flags[(size_t)k * M + i] = 1;
    }
}

__global__ __launch_bounds__(PQ_FIN_THREADS) void pq_finish_kernel(const double* __restrict__ t9, const unsigned char* __restrict__ valid,
                                                               int N, int M, const double* __restrict__ thr_low,
                                                               const double* __restrict__ thr_high, int nc,
                                                               const unsigned char* __restrict__ flags, int batch_size,
                                                               int with_gt, double* __restrict__ out) {
    __shared__ int s_part[PQ_FIN_WAVES][6];
    const int tid = threadIdx.x, lane = tid & (ET_WAVE - 1), wave = tid / ET_WAVE;
    int cnt[6] = {0, 0, 0, 0, 0, 0};                                            // valid, reliable, uncertain, tp, fp_cls, fp_loc
    for (int r = tid; r < N; r += PQ_FIN_THREADS) {
        cnt[0] += valid[r] ? 1 : 0;
        const int kind = pq_row_kind(t9, valid, r, thr_low, thr_high, nc);
        cnt[1] += kind == 1;
        cnt[2] += kind == 2;
    }
    if (with_gt)
        for (int k = 0; k < 3; ++k)
            for (int l = tid; l < M; l += PQ_FIN_THREADS) cnt[3 + k] += flags[(size_t)k * M + l] ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int s = et_wave_sum_i(cnt[k]);
        if (lane == 0) s_part[wave][k] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    int tot[6];
    for (int k = 0; k < 6; ++k) {
        tot[k] = 0;
        for (int w = 0; w < PQ_FIN_WAVES; ++w) tot[k] += s_part[w][k];
    }
    const double bs = (double)batch_size;
    double o[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (with_gt) {
        if (tot[0] > 0) {                                                       // no pseudo label at all: zeros (ssod_trainer.py:658-660)
            if (tot[2] > 0)                                                     // :567-574
                for (int k = 0; k < 3; ++k) o[k] = (double)tot[3 + k] / (double)tot[2];
            o[3] = (double)tot[2] / bs;                                         // :506
            o[4] = (double)M / bs;                                              // :508
        }
    } else {                                                                    // check_pseudo_label :597-609
        const double reliable = (double)tot[1] / bs, uncertain = (double)tot[2] / bs;
        const double both = reliable + uncertain;
        o[0] = both > 0.0 ? reliable / both : 0.0;                              // tp = precision_rate
        o[2] = tot[0] > 0 ? both * bs / (double)tot[0] : 0.0;                   // fp_loc = recall_rate (ssod_trainer.py:667)
        o[3] = both;
        o[4] = reliable;
    }
    for (int k = 0; k < 5; ++k) out[k] = o[k];
}

extern "C" int et_pseudo_quality_workspace_bytes(int M, size_t* bytes) {
    if (M < 0 || !bytes) return -1;
    *bytes = (3 * (size_t)M + 255) / 256 * 256 + 256;                           // never zero: M == 0 is legal
    return 0;
}

extern "C" int et_pseudo_quality(const double* targets9, const uint8_t* valid, int N, const float* gt, int M,
                                 const double* thr_low, const double* thr_high, int nc, int batch_size, int with_gt,
                                 void* workspace, double* out5, et_stream_t stream) {
    if (!targets9 || !valid || !thr_low || !thr_high || !out5) return -1;
    if (N <= 0 || M < 0 || nc <= 0 || batch_size <= 0) return -2;
    if (with_gt && (!workspace || (M > 0 && !gt))) return -1;
    hipStream_t s = (hipStream_t)stream;
    unsigned char* flags = (unsigned char*)workspace;
    if (with_gt && M > 0) {
        const long long nf = 3LL * M;
        hipLaunchKernelGGL(pq_zero_kernel, dim3((unsigned)((nf + PQ_THREADS - 1) / PQ_THREADS)), dim3(PQ_THREADS), 0, s, flags, nf);
        hipLaunchKernelGGL(pq_match_kernel, dim3((unsigned)(((long long)N + PQ_WAVES - 1) / PQ_WAVES)), dim3(PQ_THREADS), 0, s,
                           targets9, valid, N, gt, M, thr_low, thr_high, nc, flags);
    }
    hipLaunchKernelGGL(pq_finish_kernel, dim3(1), dim3(PQ_FIN_THREADS), 0, s, targets9, valid, N, with_gt ? M : 0, thr_low, thr_high,
                       nc, flags, batch_size, with_gt ? 1 : 0, out5);
    ET_CHECK_LAUNCH();
    return 0;
}
