// Ground truth of a training sample, prepared where the sample already is: the two reductions / selections load_image_gt and
// data_generator run on the host over the [H, W, N] instance masks (mrcnn/model.py:1361-1367 and 1831-1870):
//   * _ = np.sum(mask, axis=(0, 1)) > 0 and utils.extract_bboxes(mask) (mrcnn/utils.py:49-77)     -> mrcnn_mask_bits_stats
//   * mask[:, :, _idx], gt_masks[:, :, ids] and the copy into the zero [H, W, MAX_GT_INSTANCES] batch planes
//                                                                                                  -> mrcnn_mask_bits_gather
// and, for an image resize_image scales, utils.resize_mask before them (mrcnn/utils.py:564-583)   -> mrcnn_mask_bits_zoom
// All read the loader's bit-packed layout [H, W, nb] (numpy.packbits(mask != 0, axis=-1, bitorder="little"), nb a whole number of
// 32-bit words: what mrcnn_augment_warp_mask_bits reads and writes), so the planes never exist unpacked before the batch tensor.
// Integer arithmetic throughout: the results do not depend on the order the partial results arrive in.
#include "common.h"
#include <limits.h>

#define GTPREP_ROWS 16            // rows of one wave's strip
#define GTPREP_WAVES 4            // waves of a workgroup: four consecutive words of the same pixels (they share cache lines)

// table[i] = {count, ymin, xmin, ymax, xmax} of instance i, in the workspace
__global__ __launch_bounds__(256) void gtprep_stats_init_kernel(int* __restrict__ table, int slots) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= slots) return;
    int* t = table + 5ll * i;
    t[0] = 0;
    t[1] = INT_MAX;
    t[2] = INT_MAX;
    t[3] = -1;
    t[4] = -1;
}

// A lane owns one pixel of a 64-pixel row segment, a wave one 32-bit word (32 instances) of that segment over GTPREP_ROWS rows.
// Per row and bit one ballot gives the 64 pixels of that instance: its popcount is the pixel count, its lowest / highest set
// lane the x-extent, its non-emptiness the y-extent.  Lane b keeps the accumulators of bit b; lanes 32 .. 63 keep none.
__global__ __launch_bounds__(64 * GTPREP_WAVES) void gtprep_stats_kernel(const unsigned* __restrict__ words, int H, int W, int nw,
                                                                         int segs, int* __restrict__ table) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.y * GTPREP_WAVES + wave;                 // wave-uniform
    if (k >= nw) return;
    const int seg = blockIdx.x % segs, strip = blockIdx.x / segs;
    const int x = seg * 64 + lane;
    const int y0 = strip * GTPREP_ROWS;
    const int y1 = y0 + GTPREP_ROWS < H ? y0 + GTPREP_ROWS : H;
    int cnt = 0, ymin = INT_MAX, ymax = -1, xmin = INT_MAX, xmax = -1;
    for (int y = y0; y < y1; ++y) {
        const unsigned w = x < W ? words[((long long)y * W + x) * nw + k] : 0u;
        if (__ballot(w != 0u) == 0ull) continue;                    // wave-uniform: nothing of these 32 instances in this row segment
#pragma unroll
        for (int b = 0; b < 32; ++b) {
            const unsigned long long m = __ballot((w >> b) & 1u);
            if (m != 0ull && lane == b) {
                cnt += __popcll(m);
                const int lo = seg * 64 + (__ffsll((long long)m) - 1), hi = seg * 64 + 63 - __clzll((long long)m);
                xmin = lo < xmin ? lo : xmin;
                xmax = hi > xmax ? hi : xmax;
                ymin = y < ymin ? y : ymin;
                ymax = y;
            }
        }
    }
    if (lane < 32 && cnt > 0) {
        int* t = table + 5ll * (k * 32 + lane);
        atomicAdd(t, cnt);
        atomicMin(t + 1, ymin);
        atomicMin(t + 2, xmin);
        atomicMax(t + 3, ymax);
        atomicMax(t + 4, xmax);
    }
}

// utils.extract_bboxes's convention: (y1, x1, y2 + 1, x2 + 1), zeros for an instance without a pixel; instances >= n stay unread
__global__ __launch_bounds__(256) void gtprep_stats_final_kernel(const int* __restrict__ table, int n, int* __restrict__ count,
                                                                 int* __restrict__ box) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int* t = table + 5ll * i;
    const int c = t[0];
    count[i] = c;
    int* o = box + 4ll * i;
    o[0] = c ? t[1] : 0;
    o[1] = c ? t[2] : 0;
    o[2] = c ? t[3] + 1 : 0;
    o[3] = c ? t[4] + 1 : 0;
}

__device__ __forceinline__ unsigned gtprep_bit(const unsigned* __restrict__ px, const int* __restrict__ sel, int j, int k, int nbits) {
    if (j >= k) return 0u;
    const int s = sel[j];
    if ((unsigned)s >= (unsigned)nbits) return 0u;                 // (the wrapper refuses such a table; never read outside the pixel)
    return (px[s >> 5] >> (s & 31)) & 1u;
}

// WORDS: a thread writes planes 4q .. 4q + 3 of one pixel as one 32-bit word (G % 4 == 0, out 4-byte aligned); else one byte.
template <bool WORDS>
__global__ __launch_bounds__(256) void gtprep_gather_kernel(const unsigned* __restrict__ words, long long npix, int nw,
                                                            const int* __restrict__ sel, int k, int G, unsigned char* __restrict__ out) {
    const int per = WORDS ? G >> 2 : G;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= npix * per) return;
    const long long pix = t / per;
    const int q = (int)(t - pix * per);
    const unsigned* px = words + pix * nw;
    const int nbits = nw * 32;
    if (WORDS) {
        unsigned v = 0u;
        if (4 * q < k) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v |= gtprep_bit(px, sel, 4 * q + i, k, nbits) << (8 * i);
        }
        ((unsigned*)out)[t] = v;
    } else {
        out[t] = (unsigned char)gtprep_bit(px, sel, q, k, nbits);
    }
}

// utils.resize_mask on the packed layout: scipy.ndimage.zoom(mask, [s, s, 1], order=0) copies, per output pixel, one input pixel
// or the constant 0, the row chosen by the output row alone and the column by the output column alone (iy / ix: scipy's own
// choices, gtprep.zoom_index_tables; an entry outside [0, h) / [0, w), -1 by convention, is the constant), and np.pad puts the
// result at (top, left) of the zero canvas.  A thread owns one 32-bit word (32 instances) of one canvas pixel: consecutive threads
// store consecutive words.
__global__ __launch_bounds__(256) void gtprep_zoom_kernel(const unsigned* __restrict__ words, int h, int w, int nw,
                                                          const int* __restrict__ iy, int oh, const int* __restrict__ ix, int ow, int top,
                                                          int left, int OW, long long total, unsigned* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long pix = t / nw;
    const int k = (int)(t - pix * nw);
    const int X = (int)(pix % OW), Y = (int)(pix / OW);
    const int oy = Y - top, ox = X - left;
    unsigned v = 0u;                                               // np.pad(..., constant_values=0), zoom's cval
    if (oy >= 0 && oy < oh && ox >= 0 && ox < ow) {
        const int sy = iy[oy], sx = ix[ox];
        if ((unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w) v = words[((long long)sy * w + sx) * nw + k];
    }
    out[t] = v;
}

static int gtprep_frame_status(int H, int W, int nb) {
    if (H <= 0 || W <= 0 || nb <= 0 || nb % 4 != 0) return MRCNN_ERR_ARG;
    if (H > MRCNN_GTPREP_MAX_SIDE || W > MRCNN_GTPREP_MAX_SIDE || nb > MRCNN_GTPREP_MAX_INSTANCES / 8) return MRCNN_ERR_UNSUPPORTED;
    return MRCNN_OK;
}

extern "C" int mrcnn_mask_bits_stats_check(int H, int W, int nb, int n) {
    if (n <= 0) return MRCNN_ERR_ARG;
    const int rc = gtprep_frame_status(H, W, nb);
    if (rc == MRCNN_ERR_ARG) return rc;
    if (n > MRCNN_GTPREP_MAX_INSTANCES) return MRCNN_ERR_UNSUPPORTED;
    if (rc) return rc;
    return (long long)n > 8ll * nb ? MRCNN_ERR_ARG : MRCNN_OK;
}

extern "C" size_t mrcnn_mask_bits_stats_workspace(int nb) {
    if (nb <= 0 || nb % 4 != 0 || nb > MRCNN_GTPREP_MAX_INSTANCES / 8) return 0;
    return (size_t)nb * 8 * 5 * sizeof(int);
}

extern "C" int mrcnn_mask_bits_stats(const void* packed, int H, int W, int nb, int n, int* count, int* box, void* ws, size_t ws_bytes,
                                     void* stream) {
    const int rc = mrcnn_mask_bits_stats_check(H, W, nb, n);
    if (rc) return rc;
    if (!packed || !count || !box || !ws || ((uintptr_t)packed & 3) || ((uintptr_t)ws & 3)) return MRCNN_ERR_ARG;
    if (ws_bytes < mrcnn_mask_bits_stats_workspace(nb)) return MRCNN_ERR_WORKSPACE;
    const int nw = nb / 4, slots = nw * 32;
    const int segs = (W + 63) / 64, strips = (H + GTPREP_ROWS - 1) / GTPREP_ROWS;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gtprep_stats_init_kernel, dim3((slots + 255) / 256), dim3(256), 0, st, (int*)ws, slots);
    hipLaunchKernelGGL(gtprep_stats_kernel, dim3((unsigned)(segs * strips), (unsigned)((nw + GTPREP_WAVES - 1) / GTPREP_WAVES)),
                       dim3(64 * GTPREP_WAVES), 0, st, (const unsigned*)packed, H, W, nw, segs, (int*)ws);
    hipLaunchKernelGGL(gtprep_stats_final_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const int*)ws, n, count, box);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_mask_bits_gather_check(int H, int W, int nb, int k, int G) {
    if (k < 0 || G <= 0 || k > G) return MRCNN_ERR_ARG;
    const int rc = gtprep_frame_status(H, W, nb);
    if (rc == MRCNN_ERR_ARG) return rc;
    if (G > MRCNN_GTPREP_MAX_INSTANCES) return MRCNN_ERR_UNSUPPORTED;
    return rc;
}

extern "C" int mrcnn_mask_bits_gather(const void* packed, int H, int W, int nb, const int* sel, int k, int G, void* out, void* stream) {
    const int rc = mrcnn_mask_bits_gather_check(H, W, nb, k, G);
    if (rc) return rc;
    if (!packed || !out || (k > 0 && !sel) || ((uintptr_t)packed & 3)) return MRCNN_ERR_ARG;
    const long long npix = (long long)H * W;
    const bool wordsout = G % 4 == 0 && ((uintptr_t)out & 3) == 0;
    const long long threads = npix * (wordsout ? G / 4 : G);           // <= 2^26 * 2^12
    const dim3 grid((unsigned)cdiv64(threads, 256)), block(256);
    if (wordsout)
        hipLaunchKernelGGL(gtprep_gather_kernel<true>, grid, block, 0, (hipStream_t)stream, (const unsigned*)packed, npix, nb / 4, sel, k,
                           G, (unsigned char*)out);
    else
        hipLaunchKernelGGL(gtprep_gather_kernel<false>, grid, block, 0, (hipStream_t)stream, (const unsigned*)packed, npix, nb / 4, sel, k,
                           G, (unsigned char*)out);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_mask_bits_zoom_check(int h, int w, int nb, int oh, int ow, int top, int left, int OH, int OW) {
    const int src = gtprep_frame_status(h, w, nb), dst = gtprep_frame_status(OH, OW, nb);
    if (src == MRCNN_ERR_ARG || dst == MRCNN_ERR_ARG) return MRCNN_ERR_ARG;
    if (oh <= 0 || ow <= 0 || top < 0 || left < 0 || oh > OH - top || ow > OW - left) return MRCNN_ERR_ARG;
    return src ? src : dst;
}

extern "C" int mrcnn_mask_bits_zoom(const void* packed, int h, int w, int nb, const int* iy, int oh, const int* ix, int ow, int top,
                                    int left, int OH, int OW, void* out, void* stream) {
    const int rc = mrcnn_mask_bits_zoom_check(h, w, nb, oh, ow, top, left, OH, OW);
    if (rc) return rc;
    if (!packed || !iy || !ix || !out || ((uintptr_t)packed & 3) || ((uintptr_t)out & 3)) return MRCNN_ERR_ARG;
    const int nw = nb / 4;
    const long long total = (long long)OH * OW * nw;                   // <= 2^26 * 2^7
    hipLaunchKernelGGL(gtprep_zoom_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned*)packed, h,
                       w, nw, iy, oh, ix, ow, top, left, OW, total, (unsigned*)out);
    return mrcnn_launch_status();
}
