// The matching step of the sweep mAP (the reference's second vendored box-metric tool, tarlen5-calculate-mean-ap/calculate.py:
// calc_iou_individual, get_single_image_results), for every problem of a test set in one launch.
//   ap_sweep_kernel   per problem (the detections of one image in ascending-score order against its ground truths) and per IoU
//                     threshold t the suffix table tp[t][k], k = 0 .. P: the number of matches the tool finds when only
//                     detections k .. P - 1 are kept.  A model-score threshold keeps a suffix of the ascending order, so these
//                     P + 1 numbers are every outcome the tool's loop over score thresholds can see for the image.
// The tool's matching: the pairs with iou > thr, walked in descending IoU (among bit-equal IoUs the later-enumerated pair first:
// np.argsort(kind="stable")[::-1] on the detection-major, ground-truth-minor list); a pair is a match when neither side is
// matched yet.  float64, the tool's operations in the tool's order (the build has -ffp-contract=off).  One workgroup per problem:
//   (a, b) all P x G IoUs, the pairs above the smallest threshold collected in LDS (slots taken with an LDS counter: arrival order
//          varies from run to run, nothing below depends on it);
//   (c)    a bitonic sort by the key (IoU descending, (detection, ground truth) descending): the key is unique;
//   (d)    one lane per (threshold, suffix) walks the ordered list with its own matched-detection / matched-ground-truth bit sets
//          (LDS words, lane-interleaved) and stops at the first pair that is not above its threshold.
// No atomics on global memory, the same bits on every run.
#include "common.h"

#define APS_P_CAP MRCNN_AP_SWEEP_MAX_DET        // detections of one problem (4 words of 32 bits per lane)
#define APS_G_CAP MRCNN_AP_SWEEP_MAX_GT         // ground truths of one problem (10 words)
#define APS_T_CAP MRCNN_AP_SWEEP_MAX_THR
#define APS_C_CAP MRCNN_AP_SWEEP_MAX_CAND       // candidate pairs of one problem: 32 KiB of IoUs + 16 KiB of (d << 16 | g)
#define APS_THREADS 256
#define APS_P_WORDS (APS_P_CAP / 32)
#define APS_WORDS (APS_P_CAP / 32 + APS_G_CAP / 32)   // 14 words x 256 lanes: 14 KiB; 62 KiB of LDS in all, two workgroups per CU

static_assert(APS_P_CAP % 32 == 0 && APS_G_CAP % 32 == 0 && APS_G_CAP <= 0xFFFF && APS_P_CAP <= 0x7FFF, "bit sets and packed pair index");
static_assert((APS_C_CAP & (APS_C_CAP - 1)) == 0, "the sort pads to a power of two");
static_assert(APS_C_CAP * 12 + APS_WORDS * APS_THREADS * 4 + APS_T_CAP * 8 + 16 <= 64 * 1024, "static LDS of one workgroup");

// calc_iou_individual (:55-77): p the predicted box, t the true one, (c0, c1, c2, c3) = the tool's (x1, y1, x2, y2).
__device__ __forceinline__ double aps_iou(double p0, double p1, double p2, double p3, double t0, double t1, double t2, double t3) {
    if (t2 < p0 || p2 < t0 || t3 < p1 || p3 < t1) return 0.0;
    const double far_x = t2 < p2 ? t2 : p2, near_x = t0 > p0 ? t0 : p0;
    const double far_y = t3 < p3 ? t3 : p3, near_y = t1 > p1 ? t1 : p1;
    const double inter = (far_x - near_x + 1.0) * (far_y - near_y + 1.0);
    const double area_t = (t2 - t0 + 1.0) * (t3 - t1 + 1.0);
    const double area_p = (p2 - p0 + 1.0) * (p3 - p1 + 1.0);
    return inter / (area_t + area_p - inter);
}

// a comes before b in the walk: the greater IoU (positive doubles order as their bit patterns), then the later pair
__device__ __forceinline__ bool aps_before(unsigned long long ka, unsigned ia, unsigned long long kb, unsigned ib) {
    return ka > kb || (ka == kb && ia > ib);
}

__global__ __launch_bounds__(APS_THREADS) void ap_sweep_kernel(const double* __restrict__ det_box, const int* __restrict__ det_off, int D,
                                                               const double* __restrict__ gt_box, const int* __restrict__ gt_off, int G,
                                                               const double* __restrict__ thr, int T, int* __restrict__ tp,
                                                               int* __restrict__ status) {
    __shared__ unsigned long long s_key[APS_C_CAP];
    __shared__ unsigned s_pair[APS_C_CAP];
    __shared__ unsigned s_bits[APS_WORDS * APS_THREADS];
    __shared__ double s_thr[APS_T_CAP];
    __shared__ int s_count;
    const int prob = blockIdx.x, tid = threadIdx.x;
    // the problem's rows, inside the tables whatever the offsets hold
    const int d0 = min(max(det_off[prob], 0), D), d1 = min(max(det_off[prob + 1], d0), D);
    const int g0 = min(max(gt_off[prob], 0), G), g1 = min(max(gt_off[prob + 1], g0), G);
    const int P = d1 - d0, Gn = g1 - g0;
    // problem p owns tp[T * (det_off[p] + p) ..), T rows of P + 1: ends at T * (d1 + p + 1) <= T * (D + N)
    int* out = tp + (size_t)T * ((size_t)d0 + (size_t)prob);
    if (P > APS_P_CAP || Gn > APS_G_CAP) {                                       // uniform over the workgroup; the host never sends one
        for (int e = tid; e < T * (P + 1); e += APS_THREADS) out[e] = 0;
        if (tid == 0) status[prob] = MRCNN_AP_SWEEP_OVER_ROWS;
        return;
    }
    if (tid == 0) s_count = 0;
    if (tid < T) s_thr[tid] = thr[tid];
    __syncthreads();
    double tmin = s_thr[0];
    for (int t = 1; t < T; ++t) tmin = s_thr[t] < tmin ? s_thr[t] : tmin;
    const double* pb = det_box + 4 * (size_t)d0;
    const double* tb = gt_box + 4 * (size_t)g0;
    for (int e = tid; e < P * Gn; e += APS_THREADS) {
        const int d = e / Gn, g = e - d * Gn;
        const double v = aps_iou(pb[4 * d], pb[4 * d + 1], pb[4 * d + 2], pb[4 * d + 3], tb[4 * g], tb[4 * g + 1], tb[4 * g + 2], tb[4 * g + 3]);
        if (v > tmin) {
            const int slot = atomicAdd(&s_count, 1);                             // LDS
            if (slot < APS_C_CAP) {
                s_key[slot] = (unsigned long long)__double_as_longlong(v);
                s_pair[slot] = ((unsigned)d << 16) | (unsigned)g;
            }
        }
    }
    __syncthreads();
    const int n = s_count;
    if (n > APS_C_CAP) {                                                         // uniform: the host statement computes this problem
        for (int e = tid; e < T * (P + 1); e += APS_THREADS) out[e] = 0;
        if (tid == 0) status[prob] = MRCNN_AP_SWEEP_OVER_CANDIDATES;
        return;
    }
    int m = 1;
    while (m < n) m <<= 1;                                                       // m <= APS_C_CAP
    for (int i = n + tid; i < m; i += APS_THREADS) { s_key[i] = 0ull; s_pair[i] = 0u; }   // an IoU above a threshold > 0 has a key > 0
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < m; i += APS_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long ka = s_key[i], kb = s_key[l];
                    const unsigned ia = s_pair[i], ib = s_pair[l];
                    const bool swap = (i & k) == 0 ? aps_before(kb, ib, ka, ia) : aps_before(ka, ia, kb, ib);
                    if (swap) { s_key[i] = kb; s_key[l] = ka; s_pair[i] = ib; s_pair[l] = ia; }
                }
            }
            __syncthreads();
        }
    }
    unsigned* bits = s_bits + tid;                                               // word w of this lane: bits[w * APS_THREADS]
    const int pw = (P + 31) >> 5, gw = (Gn + 31) >> 5;
    for (int e = tid; e < T * P; e += APS_THREADS) {
        const int t = e / P, k = e - t * P;
        for (int w = 0; w < pw; ++w) bits[w * APS_THREADS] = 0u;
        for (int w = 0; w < gw; ++w) bits[(APS_P_WORDS + w) * APS_THREADS] = 0u;
        const double th = s_thr[t];
        const int most = min(P - k, Gn);                                         // no more matches than kept detections or ground truths
        int cnt = 0;
        for (int c = 0; c < n && cnt < most; ++c) {
            if (!(__longlong_as_double((long long)s_key[c]) > th)) break;
            const unsigned pair = s_pair[c];
            const int d = (int)(pair >> 16), g = (int)(pair & 0xFFFFu);
            if (d < k) continue;
            unsigned* wd = bits + (d >> 5) * APS_THREADS;
            unsigned* wg = bits + (APS_P_WORDS + (g >> 5)) * APS_THREADS;
            const unsigned vd = *wd, vg = *wg, bd = 1u << (d & 31), bg = 1u << (g & 31);
            if ((vd & bd) || (vg & bg)) continue;
            *wd = vd | bd;
            *wg = vg | bg;
            ++cnt;
        }
        out[(size_t)t * (P + 1) + k] = cnt;
    }
    for (int t = tid; t < T; t += APS_THREADS) out[(size_t)t * (P + 1) + P] = 0;  // nothing kept
    if (tid == 0) status[prob] = MRCNN_AP_SWEEP_OK;
}

extern "C" int mrcnn_ap_sweep_caps(int32_t* caps) {
    if (!caps) return MRCNN_ERR_ARG;
    caps[0] = APS_P_CAP; caps[1] = APS_G_CAP; caps[2] = APS_T_CAP; caps[3] = APS_C_CAP;
    return MRCNN_OK;
}

extern "C" int mrcnn_ap_sweep(const double* det_box, const int32_t* det_off, int D, const double* gt_box, const int32_t* gt_off, int G,
                              int N, const double* thr, int T, int32_t* tp, int32_t* status, void* stream) {
    if (N <= 0 || D < 0 || G < 0 || T <= 0) return MRCNN_ERR_ARG;
    if (!det_off || !gt_off || !thr || !tp || !status || (D > 0 && !det_box) || (G > 0 && !gt_box)) return MRCNN_ERR_ARG;
    if (T > APS_T_CAP) return MRCNN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ap_sweep_kernel, dim3((unsigned)N), dim3(APS_THREADS), 0, (hipStream_t)stream, det_box, (const int*)det_off, D,
                       gt_box, (const int*)gt_off, G, thr, T, (int*)tp, (int*)status);
    return mrcnn_launch_status();
}
