// The pixel work of the tester (Analyzer.compute_performances and compute_det_mask_pars, mrcnn/analyze.py:1502-1861) on the bit
// planes of the mask graph (maskgraph.hip: planes[n][H][wpr] 32-bit words, wpr = ceil(W / 32), pixel x = bit x & 31 of word
// x >> 5, least significant bit first, zero bits past W; a box is (y1, x1, y2, x2) with an exclusive end, zeros for an empty plane).
//   mask_cross_stats_kernel   inter[i][j] = popcount(a_i & b_j) for every plane a_i of one set against every plane b_j of another
//                             set of the same frame: the intersections behind the G x D (and D x G) jaccard_score calls of
//                             compute_performances.  The union is count_a + count_b - inter, on the host.
//   mask_plane_sums_kernel    sum[p] = float64 sum of the non-NaN image values under plane p: np.nansum(data[mask == 1]) of
//                             compute_det_mask_pars.
// Integer-exact, or float64 in a fixed order; no atomics, no LDS beyond four partial sums, nothing allocated.
#include "common.h"

// One wavefront per cell (i, j), four cells per workgroup; a lane takes one word of the two boxes' intersection, striding.  Words
// of the intersection's columns may hold bits outside it: those are outside one plane's box, hence zero in that plane.
__global__ __launch_bounds__(256) void mask_cross_stats_kernel(const unsigned* __restrict__ planes_a, const int* __restrict__ box_a, int na,
                                                               const unsigned* __restrict__ planes_b, const int* __restrict__ box_b, int nb,
                                                               int H, int W, int wpr, int* __restrict__ inter) {
    const int lane = threadIdx.x & 63;
    const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);      // wave-uniform
    if (cell >= (long long)na * nb) return;
    const int i = (int)(cell / nb), j = (int)(cell % nb);
    // exclusive window, inside the frame whatever the boxes hold; empty when either box is
    const int y0 = max(max(box_a[4 * i], box_b[4 * j]), 0), y1 = min(min(box_a[4 * i + 2], box_b[4 * j + 2]), H);
    const int x0 = max(max(box_a[4 * i + 1], box_b[4 * j + 1]), 0), x1 = min(min(box_a[4 * i + 3], box_b[4 * j + 3]), W);
    int cnt = 0;
    if (y0 < y1 && x0 < x1) {
        const long long plane_words = (long long)H * wpr;
        const unsigned* A = planes_a + (long long)i * plane_words;
        const unsigned* B = planes_b + (long long)j * plane_words;
        const int k0 = x0 >> 5, nk = ((x1 - 1) >> 5) - k0 + 1;
        const int total = (y1 - y0) * nk;                                       // <= H * wpr
        for (int idx = lane; idx < total; idx += 64) {
            const long long at = (long long)(y0 + idx / nk) * wpr + k0 + idx % nk;
            cnt += __popc(A[at] & B[at]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) inter[cell] = cnt;
}

__device__ __forceinline__ float me_pixel(const unsigned* __restrict__ img, int big_endian, long long idx) {
    unsigned u = img[idx];
    if (big_endian) u = __builtin_bswap32(u);
    return __uint_as_float(u);
}

// One workgroup per plane; a thread takes one word of the plane's box, striding, and adds the image values at its set bits in
// bit order.  The 256 partial sums are combined in a fixed order -- the xor tree inside each wavefront, then wavefront 0 to 3 --
// so the result does not change from run to run.
__global__ __launch_bounds__(256) void mask_plane_sums_kernel(const unsigned* __restrict__ img, int big_endian, const unsigned* __restrict__ planes,
                                                              const int* __restrict__ box, int H, int W, int wpr, double* __restrict__ sum) {
    __shared__ double s_part[4];
    const int p = blockIdx.x;
    const int y0 = max(box[4 * p], 0), y1 = min(box[4 * p + 2], H);
    const int x0 = max(box[4 * p + 1], 0), x1 = min(box[4 * p + 3], W);
    double acc = 0.0;
    if (y0 < y1 && x0 < x1) {
        const unsigned* pl = planes + (long long)p * H * wpr;
        const int k0 = x0 >> 5, nk = ((x1 - 1) >> 5) - k0 + 1;
        const int total = (y1 - y0) * nk;
        for (int idx = threadIdx.x; idx < total; idx += 256) {
            const int y = y0 + idx / nk, k = k0 + idx % nk;
            unsigned u = pl[(long long)y * wpr + k];
            while (u) {
                const int x = 32 * k + __ffs((int)u) - 1;
                u &= u - 1u;
                if (x < W) {                                                     // bits past W are zero by contract; never index past the row
                    const float v = me_pixel(img, big_endian, (long long)y * W + x);
                    if (v == v) acc += (double)v;
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) sum[p] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

extern "C" int mrcnn_mask_cross_stats(const void* planes_a, const int32_t* box_a, int na, const void* planes_b, const int32_t* box_b, int nb,
                                      int H, int W, int32_t* inter, void* stream) {
    if (na <= 0 || nb <= 0 || H <= 0 || W <= 0) return MRCNN_ERR_ARG;
    if (!planes_a || !box_a || !planes_b || !box_b || !inter) return MRCNN_ERR_ARG;
    const int wpr = (W + 31) >> 5;
    const int64_t cells = (int64_t)na * nb;
    if ((int64_t)H * wpr > 0x7FFFFFFFll || cells > 0x7FFFFFFFll) return MRCNN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mask_cross_stats_kernel, dim3((unsigned)cdiv64(cells, 4)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned*)planes_a, (const int*)box_a, na, (const unsigned*)planes_b, (const int*)box_b, nb, H, W, wpr,
                       (int*)inter);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_mask_plane_sums(const void* img, int big_endian, const void* planes, const int32_t* box, int n, int H, int W, double* sum,
                                     void* stream) {
    if (n <= 0 || H <= 0 || W <= 0) return MRCNN_ERR_ARG;
    if (!img || !planes || !box || !sum) return MRCNN_ERR_ARG;
    const int wpr = (W + 31) >> 5;
    if ((int64_t)H * wpr > 0x7FFFFFFFll) return MRCNN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mask_plane_sums_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, (const unsigned*)img, big_endian,
                       (const unsigned*)planes, (const int*)box, H, W, wpr, (double*)sum);
    return mrcnn_launch_status();
}
