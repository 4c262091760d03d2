// The matching step of the Pascal-VOC box metrics (the vendored Object-Detection-Metrics tool of the reference,
// lib/Evaluator.py:99-122 with the IoU of :382-426), for the detections of a whole test set in one launch.
//   voc_match_kernel   per detection: the ground truth of its image and class with the greatest IoU (first one on a tie, -1 when
//                      every IoU is 0), that IoU, and per threshold whether the detection is a true positive -- its IoU reaches
//                      the threshold and no detection that precedes it (higher score, or equal score and earlier row: the tool's
//                      stable descending sort) claimed the same ground truth at that threshold (the tool's "seen" flag).
// float64 throughout, the tool's operations in the tool's order (the build has -ffp-contract=off: no fused multiply-add).  Every
// competitor for a ground truth lies in the same image, an image is one workgroup: no atomics, the same bits on every run.
#include "common.h"
#include <cfloat>

#define APM_GT_CAP 256            // ground truths of one image staged in LDS (9 KiB); above it they are read from global memory

__device__ __forceinline__ double apm_iou(double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3) {
    if (a0 > b2 || b0 > a2 || a3 < b1 || a1 > b3) return 0.0;
    const double lo0 = a0 > b0 ? a0 : b0, lo1 = a1 > b1 ? a1 : b1;
    const double hi2 = a2 < b2 ? a2 : b2, hi3 = a3 < b3 ? a3 : b3;
    const double inter = (hi2 - lo0 + 1.0) * (hi3 - lo1 + 1.0);
    const double area_a = (a2 - a0 + 1.0) * (a3 - a1 + 1.0);
    const double area_b = (b2 - b0 + 1.0) * (b3 - b1 + 1.0);
    return inter / (area_a + area_b - inter);
}

// The tool's loop over the image's ground truths of the detection's class, in row order: `iou > iouMax` from
// iouMax = sys.float_info.min, so the first strictly greatest IoU wins and an IoU of 0 never does.
__device__ __forceinline__ void apm_best(const double* box, const int* cls, int ng, int c, double a0, double a1, double a2, double a3,
                                         int& arg, double& best) {
    for (int j = 0; j < ng; ++j) {
        if (cls[j] != c) continue;
        const double v = apm_iou(a0, a1, a2, a3, box[4 * j], box[4 * j + 1], box[4 * j + 2], box[4 * j + 3]);
        if (v > best) { best = v; arg = j; }
    }
}

// One wavefront = one workgroup per image; a lane takes one detection of the image, striding.
__global__ __launch_bounds__(64) void voc_match_kernel(const double* __restrict__ det_box, const int* __restrict__ det_cls,
                                                       const double* __restrict__ det_score, const int* __restrict__ det_off,
                                                       const double* __restrict__ gt_box, const int* __restrict__ gt_cls,
                                                       const int* __restrict__ gt_off, int D, int G, const double* __restrict__ thr, int T,
                                                       int* best_gt, double* best_iou, unsigned char* __restrict__ tp) {
    __shared__ double s_box[4 * APM_GT_CAP];
    __shared__ int s_cls[APM_GT_CAP];
    const int img = blockIdx.x, lane = threadIdx.x;
    // the image's rows, inside the tables whatever the offsets hold
    const int d0 = min(max(det_off[img], 0), D), d1 = min(max(det_off[img + 1], d0), D);
    const int g0 = min(max(gt_off[img], 0), G), g1 = min(max(gt_off[img + 1], g0), G);
    const int ng = g1 - g0;
    const bool staged = ng <= APM_GT_CAP;                                        // uniform over the workgroup
    if (staged) {
        for (int k = lane; k < 4 * ng; k += 64) s_box[k] = gt_box[4 * (size_t)g0 + k];
        for (int k = lane; k < ng; k += 64) s_cls[k] = gt_cls[g0 + k];
    }
    __syncthreads();
    for (int d = d0 + lane; d < d1; d += 64) {
        const double a0 = det_box[4 * (size_t)d], a1 = det_box[4 * (size_t)d + 1], a2 = det_box[4 * (size_t)d + 2], a3 = det_box[4 * (size_t)d + 3];
        int arg = -1;
        double best = DBL_MIN;
        if (staged) apm_best(s_box, s_cls, ng, det_cls[d], a0, a1, a2, a3, arg, best);
        else apm_best(gt_box + 4 * (size_t)g0, gt_cls + g0, ng, det_cls[d], a0, a1, a2, a3, arg, best);
        best_gt[d] = arg < 0 ? -1 : g0 + arg;
        best_iou[d] = arg < 0 ? 0.0 : best;
    }
    __threadfence_block();
    __syncthreads();                                                             // the image's best_gt / best_iou are complete
    for (int d = d0 + lane; d < d1; d += 64) {
        const int g = best_gt[d];
        const double v = best_iou[d], s = det_score[d];
        // the greatest IoU among the detections that precede d and chose the same ground truth: one of them reached a threshold
        // (and set the tool's "seen" flag before d was looked at) exactly when this maximum reaches it
        double claimed = -1.0;
        if (g >= 0) {
            for (int e = d0; e < d1; ++e) {
                if (e == d || best_gt[e] != g) continue;
                const double se = det_score[e];
                if (se > s || (se == s && e < d)) claimed = fmax(claimed, best_iou[e]);
            }
        }
        for (int t = 0; t < T; ++t) {
            const double th = thr[t];
            tp[(size_t)t * D + d] = (g >= 0 && v >= th && !(claimed >= th)) ? 1 : 0;
        }
    }
}

extern "C" int mrcnn_voc_match(const double* det_box, const int32_t* det_cls, const double* det_score, const int32_t* det_off, int D,
                               const double* gt_box, const int32_t* gt_cls, const int32_t* gt_off, int G, int I, const double* thr, int T,
                               int32_t* best_gt, double* best_iou, uint8_t* tp, void* stream) {
    if (D <= 0 || I <= 0 || G < 0 || T <= 0) return MRCNN_ERR_ARG;
    if (!det_box || !det_cls || !det_score || !det_off || !gt_off || !thr || !best_gt || !best_iou || !tp) return MRCNN_ERR_ARG;
    if (G > 0 && (!gt_box || !gt_cls)) return MRCNN_ERR_ARG;
    hipLaunchKernelGGL(voc_match_kernel, dim3((unsigned)I), dim3(64), 0, (hipStream_t)stream, det_box, (const int*)det_cls, det_score,
                       (const int*)det_off, gt_box, (const int*)gt_cls, (const int*)gt_off, D, G, thr, T, (int*)best_gt, best_iou,
                       (unsigned char*)tp);
    return mrcnn_launch_status();
}
