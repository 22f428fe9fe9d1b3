// LabelMatch's end-of-epoch thresholds on the device: what update_epoch_cls_thr (utils/labelmatch.py:188-240) and gmm_policy
// (:138-189, sklearn.mixture.GaussianMixture with all three *_init arguments given) compute on the host from the per-class score
// lists, computed from the device log et_score_log_append filled, with no copy of the log and no host synchronisation.
//
// No FMA contraction in this file (the pragma below reaches the gfx950 build and the host build of the CPU test tier alike): the
// number of EM iterations is a decision on an fp64 difference, and the same source has to take it on both.
//
// Every output is a function of the MULTISET of logged pairs: the sort is total on (class, confidence), so equal keys are equal
// elements, and every sum is a fixed-shape reduction over the sorted segment (strided per thread, xor butterfly per wave, the wave
// partials added in wave order).  The only atomics are integer counters of a digit histogram in LDS.
//
//   Segment   LSD radix sort of the live pairs (index < min(*log_count, cap), read on the device) by (class ascending, confidence
//             descending).  Key of a pair: the class, then ~bits(confidence) -- confidences are positive floats, whose bit patterns
//             order like the values.  A class outside [0, nc) becomes nc and sorts behind every segment: dropped, as
//             `conf[cls == c]` drops it.  8-bit digits: four passes over the confidence, one over the class (two when nc >= 256).
//             Per pass
//               lm_hist_kernel     one wave per tile of LM_TILE pairs: digit counts of the tile -> hist[digit][tile]
//               lm_scan_kernel     one workgroup: exclusive scan of hist in place (digit-major, so the result is the global offset
//                                  of the tile's first pair of each digit)
//               lm_scatter_kernel  one wave per tile, 64 pairs a round in index order: rank of a lane among the lanes of the same
//                                  digit by eight ballots (stable), running per-digit offsets in LDS
//             Tiles are sized from the live count, so an almost empty log costs almost nothing.
//             lm_segment_kernel: seg_offset[c] = lower bound of class c in the sorted class column, c = 0 .. nc.
//   lm_threshold_kernel   one workgroup per class, looping over its segment (class sizes are very uneven; the largest class bounds
//             the time -- see DESIGN.md); workgroup nc clears the tail of sorted_conf.
//     Rank      cls_num_total[c] += n; pos_low = min(int(total / (epoch + 1)), int(n * resample_low_percent)) in the fp64
//               arithmetic of the python; thr_low = max(ignore_thres_low, s[pos_low]); a pos_low outside the segment (where the
//               reference raises IndexError) reads nothing and sets status[c] = ET_LM_RANK_OUT_OF_SEGMENT.
//     Mixture   the two-component EM of sklearn's fit in fp64: w = (1/2, 1/2), mu = (min, max), var = (1, 1);
//               E: lp_k = -(log 2pi + (x - mu_k)^2 / var_k) / 2 - log(var_k) / 2 + log w_k, norm = logsumexp_k lp_k,
//                  log_resp = lp - norm;  M, with r = exp(log_resp): nk = sum r + 10 eps, mu = sum r x / nk,
//                  var = sum r (x - mu_new)^2 / nk + 1e-6, w = nk / n renormalised; lower bound = mean norm of the E-step BEFORE the
//               M-step; stop at |change| < 1e-3 or after 100 iterations.  The variance needs the new mean, so an iteration sweeps
//               the segment twice and the second sweep recomputes the responsibilities (nothing per-sample is stored).  Both
//               components run the same instructions: a class of constant scores keeps them bit-equal.
//     Policy    one more E-step; assign = component 1 iff log_resp_1 > log_resp_0; among the component-1 samples the largest norm,
//               and among those that attain it the largest score x_top (a max over pairs (norm, x)).  The reference's
//               min{x : assign == 1 and x >= x_top} IS x_top (it belongs to the set), so thr_high = max(0, x_top); 0 when nothing
//               is assigned to component 1 or n < 4.
#pragma clang fp contract(off)
#include "et_device.h"
#include "../../include/et_hip.h"
#include <float.h>
#include <math.h>

#define LM_SORT_THREADS ET_WAVE                     // one wave per tile: the stable rank is a wave-level ballot match
#define LM_SORT_ROUNDS 32
#define LM_TILE (LM_SORT_THREADS * LM_SORT_ROUNDS)
#define LM_RADIX 256
#define LM_SCAN_THREADS 1024
#define LM_SCAN_WAVES (LM_SCAN_THREADS / ET_WAVE)
#define LM_EM_THREADS 1024
#define LM_EM_WAVES (LM_EM_THREADS / ET_WAVE)
#define LM_MAX_ITER 100                             // GaussianMixture's max_iter
#define LM_TOL 1e-3                                 // ... tol
#define LM_REG_COVAR 1e-6                           // ... reg_covar
#define LM_LOG_2PI 1.8378770664093453               // numpy's log(2 * pi)
#define LM_MIN_FIT 4                                // gmm_policy returns given_gt_thr for fewer scores (:154)

__device__ __forceinline__ long long lm_live_count(const unsigned long long* __restrict__ log_count, long long cap) {
    const unsigned long long n = *log_count;
    return n > (unsigned long long)cap ? cap : (long long)n;
}

// pair i of the pass's input: the log itself in the first pass, the previous pass's output afterwards
__device__ __forceinline__ void lm_load_pair(const float* __restrict__ conf_log, const int* __restrict__ cls_log,
                                             const unsigned* __restrict__ key_in, const unsigned* __restrict__ cls_in, int first, int nc,
                                             long long i, unsigned& key, unsigned& cls) {
    if (first) {
        key = ~__float_as_uint(conf_log[i]);
        const int c = cls_log[i];
        cls = (c < 0 || c >= nc) ? (unsigned)nc : (unsigned)c;
    } else {
        key = key_in[i];
        cls = cls_in[i];
    }
}

__device__ __forceinline__ unsigned lm_digit(unsigned key, unsigned cls, int pass) {
    return pass < 4 ? (key >> (8 * pass)) & 255u : (cls >> (8 * (pass - 4))) & 255u;
}

__global__ __launch_bounds__(LM_SORT_THREADS) void lm_hist_kernel(const float* __restrict__ conf_log, const int* __restrict__ cls_log,
                                                                  const unsigned* __restrict__ key_in, const unsigned* __restrict__ cls_in,
                                                                  const unsigned long long* __restrict__ log_count, long long cap,
                                                                  int nc, int pass, unsigned* __restrict__ hist) {
    __shared__ unsigned s_hist[LM_RADIX];
    const long long n = lm_live_count(log_count, cap);
    const long long tiles = (n + LM_TILE - 1) / LM_TILE, tile = blockIdx.x;
    if (tile >= tiles) return;                                                  // workgroup-uniform
    const int lane = threadIdx.x;
    for (int d = lane; d < LM_RADIX; d += LM_SORT_THREADS) s_hist[d] = 0;
    __syncthreads();
    for (int r = 0; r < LM_SORT_ROUNDS; ++r) {
        const long long i = tile * LM_TILE + (long long)r * LM_SORT_THREADS + lane;
        if (i < n) {
            unsigned key, cls;
            lm_load_pair(conf_log, cls_log, key_in, cls_in, pass == 0, nc, i, key, cls);
            atomicAdd(&s_hist[lm_digit(key, cls, pass)], 1u);
        }
    }
    __syncthreads();
    for (int d = lane; d < LM_RADIX; d += LM_SORT_THREADS) hist[(long long)d * tiles + tile] = s_hist[d];
}

// exclusive scan, in place, of the LM_RADIX * tiles live entries of hist: every thread owns one contiguous chunk
__global__ __launch_bounds__(LM_SCAN_THREADS) void lm_scan_kernel(const unsigned long long* __restrict__ log_count, long long cap,
                                                                  unsigned* __restrict__ hist) {
    __shared__ unsigned s_wave[LM_SCAN_WAVES];
    const long long n = lm_live_count(log_count, cap);
    const long long E = (n + LM_TILE - 1) / LM_TILE * LM_RADIX;
    const int tid = threadIdx.x, lane = tid & (ET_WAVE - 1), wave = tid / ET_WAVE;
    const long long chunk = (E + LM_SCAN_THREADS - 1) / LM_SCAN_THREADS;
    const long long lo = min(E, tid * chunk), hi = min(E, lo + chunk);
    unsigned sum = 0;
    for (long long i = lo; i < hi; ++i) sum += hist[i];
    unsigned incl = sum;
#pragma unroll
    for (int o = 1; o < ET_WAVE; o <<= 1) {
        const unsigned v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == ET_WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    unsigned run = incl - sum;
    for (int w = 0; w < wave; ++w) run += s_wave[w];
    for (long long i = lo; i < hi; ++i) {
        const unsigned v = hist[i];
        hist[i] = run;
        run += v;
    }
}

__global__ __launch_bounds__(LM_SORT_THREADS) void lm_scatter_kernel(const float* __restrict__ conf_log, const int* __restrict__ cls_log,
                                                                     const unsigned* __restrict__ key_in, const unsigned* __restrict__ cls_in,
                                                                     const unsigned long long* __restrict__ log_count, long long cap,
                                                                     int nc, int pass, const unsigned* __restrict__ offset,
                                                                     unsigned* __restrict__ key_out, unsigned* __restrict__ cls_out) {
    __shared__ unsigned s_off[LM_RADIX];
    const long long n = lm_live_count(log_count, cap);
    const long long tiles = (n + LM_TILE - 1) / LM_TILE, tile = blockIdx.x;
    if (tile >= tiles) return;                                                  // workgroup-uniform
    const int lane = threadIdx.x;
    for (int d = lane; d < LM_RADIX; d += LM_SORT_THREADS) s_off[d] = offset[(long long)d * tiles + tile];
    __syncthreads();
    for (int r = 0; r < LM_SORT_ROUNDS; ++r) {
        const long long i0 = tile * LM_TILE + (long long)r * LM_SORT_THREADS;
        if (i0 >= n) break;                                                     // workgroup-uniform
        const long long i = i0 + lane;
        const bool live = i < n;
        unsigned key = 0, cls = 0;
        if (live) lm_load_pair(conf_log, cls_log, key_in, cls_in, pass == 0, nc, i, key, cls);
        const unsigned d = lm_digit(key, cls, pass);
        unsigned long long peers = __ballot(live);                              // the live lanes that hold this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(live && bit);
            peers &= bit ? m : ~m;
        }
        const int rank = __popcll(peers & ((1ull << lane) - 1ull)), total = __popcll(peers);
        if (live) {
            const long long pos = (long long)s_off[d] + rank;
            if (pos < n) {                                                      // always: hist counted the same pairs
                key_out[pos] = key;
                cls_out[pos] = cls;
            }
        }
        __syncthreads();
        if (live && rank == total - 1) s_off[d] += (unsigned)total;            // one lane per digit present in the round
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void lm_segment_kernel(const unsigned* __restrict__ cls_sorted,
                                                         const unsigned long long* __restrict__ log_count, long long cap, int nc,
                                                         long long* __restrict__ seg) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c > nc) return;
    const long long n = lm_live_count(log_count, cap);
    long long lo = 0, hi = n;                                                   // first index whose class is >= c
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (cls_sorted[mid] < (unsigned)c) lo = mid + 1; else hi = mid;
    }
    seg[c] = lo;
}

// ---- the mixture ---------------------------------------------------------------------------------------------------------------
struct LmMix { double w[2], mu[2], var[2]; };
struct LmTerms { double log_w[2], half_log_var[2]; };                           // per-iteration constants of the E-step

__device__ __forceinline__ LmTerms lm_terms(const LmMix& p) {
    LmTerms t;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        t.log_w[k] = log(p.w[k]);
        t.half_log_var[k] = 0.5 * log(p.var[k]);
    }
    return t;
}

// one sample's E-step: norm and log_resp[2]
__device__ __forceinline__ double lm_estep(double x, const LmMix& p, const LmTerms& t, double (&log_resp)[2]) {
    double lp[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double d = x - p.mu[k];
        lp[k] = -0.5 * (LM_LOG_2PI + d * d / p.var[k]) - t.half_log_var[k] + t.log_w[k];
    }
    const double m = fmax(lp[0], lp[1]);
    const double norm = m + log(exp(lp[0] - m) + exp(lp[1] - m));
    log_resp[0] = lp[0] - norm;
    log_resp[1] = lp[1] - norm;
    return norm;
}

// sums of K values over the workgroup; every thread returns with the same K totals
template <int K> __device__ __forceinline__ void lm_block_sum(double (&v)[K], double (*s_part)[5]) {
    const int lane = threadIdx.x & (ET_WAVE - 1), wave = threadIdx.x / ET_WAVE;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = et_wave_sum_d(v[k]);
    __syncthreads();                                                            // the previous call's readers are done
    if (lane == 0)
        for (int k = 0; k < K; ++k) s_part[wave][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = 0.0;
        for (int w = 0; w < LM_EM_WAVES; ++w) t += s_part[w][k];
        v[k] = t;
    }
}

__device__ __forceinline__ double lm_score(const unsigned* __restrict__ keys, long long i) {
    return (double)__uint_as_float(~keys[i]);
}

__global__ __launch_bounds__(LM_EM_THREADS) void lm_threshold_kernel(
    const unsigned* __restrict__ key_sorted, const long long* __restrict__ seg, int nc, long long cap, int epoch, double ignore_low,
    double ignore_high, double low_percent, long long* __restrict__ cls_num_total, double* __restrict__ thr_high,
    double* __restrict__ thr_low, long long* __restrict__ n_per_class, int* __restrict__ n_iter_out, int* __restrict__ status,
    double* __restrict__ gmm, float* __restrict__ sorted_conf) {
    __shared__ double s_part[LM_EM_WAVES][5];
    __shared__ double s_best[LM_EM_WAVES][2];
    __shared__ int s_cnt[LM_EM_WAVES];
    const int tid = threadIdx.x, lane = tid & (ET_WAVE - 1), wave = tid / ET_WAVE;
    const int c = blockIdx.x;
    if (c == nc) {                                                              // the tail of sorted_conf: dropped pairs and unused capacity
        if (sorted_conf)
            for (long long i = seg[nc] + tid; i < cap; i += LM_EM_THREADS) sorted_conf[i] = 0.0f;
        return;
    }
    const long long s0 = seg[c], n = seg[c + 1] - s0;
    const unsigned* __restrict__ keys = key_sorted + s0;
    if (sorted_conf)
        for (long long i = tid; i < n; i += LM_EM_THREADS) sorted_conf[s0 + i] = __uint_as_float(~keys[i]);

    // ---- Rank (thread 0; the other threads go on)
    if (tid == 0) {
        const long long total = cls_num_total[c] + n;
        cls_num_total[c] = total;
        n_per_class[c] = n;
        int st = ET_LM_OK;
        double lo = ignore_low;
        if (n > 0) {
            const long long by_total = (long long)((double)total / (double)(epoch + 1));
            const long long by_share = (long long)((double)n * low_percent);
            const long long pos = by_total < by_share ? by_total : by_share;
            if (pos < 0 || pos >= n) st = ET_LM_RANK_OUT_OF_SEGMENT;
            else {
                const double s = lm_score(keys, pos);
                if (s > lo) lo = s;
            }
        }
        thr_low[c] = lo;
        status[c] = st;
    }

    LmMix p = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    int n_iter = 0;
    double high = n > 0 ? 0.0 : ignore_high;                                    // given_gt_thr = 0.0 (:229)
    if (n >= LM_MIN_FIT) {                                                      // workgroup-uniform, as is every branch below
        const double dn = (double)n;
        p.w[0] = p.w[1] = 0.5;
        p.mu[0] = lm_score(keys, n - 1);                                        // min: the segment is sorted descending
        p.mu[1] = lm_score(keys, 0);
        p.var[0] = p.var[1] = 1.0;
        double prev_bound = -INFINITY;
        bool converged = false;
        for (n_iter = 1; n_iter <= LM_MAX_ITER; ++n_iter) {
            const LmTerms t = lm_terms(p);
            double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                             // sum norm, sum r_k, sum r_k x
            for (long long i = tid; i < n; i += LM_EM_THREADS) {
                const double x = lm_score(keys, i);
                double lr[2];
                a[0] += lm_estep(x, p, t, lr);
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const double r = exp(lr[k]);
                    a[1 + k] += r;
                    a[3 + k] += r * x;
                }
            }
            lm_block_sum<5>(a, s_part);
            const double bound = a[0] / dn;
            double nk[2], mu_new[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                nk[k] = a[1 + k] + 10.0 * DBL_EPSILON;
                mu_new[k] = a[3 + k] / nk[k];
            }
            double b[2] = {0.0, 0.0};                                           // sum r_k (x - mu_new_k)^2, r recomputed from the old parameters
            for (long long i = tid; i < n; i += LM_EM_THREADS) {
                const double x = lm_score(keys, i);
                double lr[2];
                lm_estep(x, p, t, lr);
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const double d = x - mu_new[k];
                    b[k] += exp(lr[k]) * (d * d);
                }
            }
            lm_block_sum<2>(b, s_part);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                p.mu[k] = mu_new[k];
                p.var[k] = b[k] / nk[k] + LM_REG_COVAR;
                p.w[k] = nk[k] / dn;
            }
            const double wsum = p.w[0] + p.w[1];
            p.w[0] = p.w[0] / wsum;
            p.w[1] = p.w[1] / wsum;
            const double change = bound - prev_bound;
            prev_bound = bound;
            if (fabs(change) < LM_TOL) { converged = true; break; }
        }
        if (!converged) n_iter = LM_MAX_ITER;

        // ---- Policy: the final E-step
        const LmTerms t = lm_terms(p);
        int cnt = 0;
        double best_norm = -INFINITY, best_x = -INFINITY;
        for (long long i = tid; i < n; i += LM_EM_THREADS) {
            const double x = lm_score(keys, i);
            double lr[2];
            const double norm = lm_estep(x, p, t, lr);
            if (lr[1] > lr[0]) {                                                // a tie goes to component 0 (argmax)
                ++cnt;
                if (norm > best_norm || (norm == best_norm && x > best_x)) { best_norm = norm; best_x = x; }
            }
        }
        cnt = et_wave_sum_i(cnt);
#pragma unroll
        for (int m = ET_WAVE / 2; m >= 1; m >>= 1) {
            const double on = __shfl_xor(best_norm, m), ox = __shfl_xor(best_x, m);
            if (on > best_norm || (on == best_norm && ox > best_x)) { best_norm = on; best_x = ox; }
        }
        if (lane == 0) { s_cnt[wave] = cnt; s_best[wave][0] = best_norm; s_best[wave][1] = best_x; }
        __syncthreads();
        if (tid == 0) {
            int total = 0;
            double bn = -INFINITY, bx = -INFINITY;
            for (int w = 0; w < LM_EM_WAVES; ++w) {
                total += s_cnt[w];
                if (s_best[w][0] > bn || (s_best[w][0] == bn && s_best[w][1] > bx)) { bn = s_best[w][0]; bx = s_best[w][1]; }
            }
            if (total > 0 && bx > high) high = bx;                              // max(given_gt_thr, x_top)
        }
    }
    if (tid == 0) {
        thr_high[c] = high;
        n_iter_out[c] = n_iter;
        double* g = gmm + (size_t)c * 6;
        g[0] = p.w[0]; g[1] = p.w[1]; g[2] = p.mu[0]; g[3] = p.mu[1]; g[4] = p.var[0]; g[5] = p.var[1];
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
static inline size_t lm_align(size_t b) { return (b + 255) / 256 * 256; }

struct LmLayout { size_t column, hist, seg, total; long long tiles; };

static int lm_layout(int64_t cap, int nc, LmLayout* l) {
    if (cap <= 0 || cap > 0x7fffffffLL || nc <= 0 || nc >= 65535) return -2;   // positions are 32-bit, the class has two digits
    l->tiles = (cap + LM_TILE - 1) / LM_TILE;
    l->column = lm_align((size_t)cap * sizeof(unsigned));
    l->hist = lm_align((size_t)l->tiles * LM_RADIX * sizeof(unsigned));
    l->seg = lm_align(((size_t)nc + 1) * sizeof(long long));
    l->total = 4 * l->column + l->hist + l->seg;
    return 0;
}

extern "C" int et_labelmatch_thresholds_workspace_bytes(int64_t cap, int nc, size_t* bytes) {
    LmLayout l;
    if (!bytes) return -1;
    if (lm_layout(cap, nc, &l)) return -2;
    *bytes = l.total;
    return 0;
}

extern "C" int et_labelmatch_thresholds(const float* conf_log, const int* cls_log, const uint64_t* log_count, int64_t cap, int nc,
                                        int epoch, double ignore_thres_low, double ignore_thres_high, double resample_low_percent,
                                        int64_t* cls_num_total, double* thr_high, double* thr_low, int64_t* n_per_class, int* n_iter,
                                        int* status, double* gmm, float* sorted_conf, int64_t* seg_offset, void* ws, size_t ws_bytes,
                                        et_stream_t stream) {
    if (!conf_log || !cls_log || !log_count || !cls_num_total || !thr_high || !thr_low || !n_per_class || !n_iter || !status ||
        !gmm || !ws)
        return -1;
    LmLayout l;
    if (lm_layout(cap, nc, &l) || epoch < 0) return -2;
    if (ws_bytes < l.total) return -3;
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    unsigned* key[2] = {(unsigned*)w, (unsigned*)(w + 2 * l.column)};
    unsigned* cls[2] = {(unsigned*)(w + l.column), (unsigned*)(w + 3 * l.column)};
    unsigned* hist = (unsigned*)(w + 4 * l.column);
    long long* seg = seg_offset ? (long long*)seg_offset : (long long*)(w + 4 * l.column + l.hist);
    const unsigned long long* count = (const unsigned long long*)log_count;
    const int passes = 4 + (nc < 256 ? 1 : 2);
    int src = 1;                                                                // pass 0 reads the log and writes pair 0
    for (int pass = 0; pass < passes; ++pass) {
        const int dst = src ^ 1;
        hipLaunchKernelGGL(lm_hist_kernel, dim3((unsigned)l.tiles), dim3(LM_SORT_THREADS), 0, s, conf_log, cls_log, key[src], cls[src],
                           count, (long long)cap, nc, pass, hist);
        hipLaunchKernelGGL(lm_scan_kernel, dim3(1), dim3(LM_SCAN_THREADS), 0, s, count, (long long)cap, hist);
        hipLaunchKernelGGL(lm_scatter_kernel, dim3((unsigned)l.tiles), dim3(LM_SORT_THREADS), 0, s, conf_log, cls_log, key[src],
                           cls[src], count, (long long)cap, nc, pass, hist, key[dst], cls[dst]);
        src = dst;
    }
    hipLaunchKernelGGL(lm_segment_kernel, dim3((unsigned)((nc + 1 + 255) / 256)), dim3(256), 0, s, cls[src], count, (long long)cap, nc,
                       seg);
    hipLaunchKernelGGL(lm_threshold_kernel, dim3((unsigned)(nc + 1)), dim3(LM_EM_THREADS), 0, s, key[src], seg, nc, (long long)cap,
                       epoch, ignore_thres_low, ignore_thres_high, resample_low_percent, (long long*)cls_num_total, thr_high, thr_low,
                       (long long*)n_per_class, n_iter, status, gmm, sorted_conf);
    ET_CHECK_LAUNCH();
    return 0;
}
