// The mask graph of Analyzer.extract_det_masks (mrcnn/analyze.py:1162-1496) on bit planes: which detection masks overlap or
// touch, and the unions of the ones that are merged.  The masks of one frame are planes[n][H][wpr] 32-bit words, wpr =
// ceil(W / 32); pixel x of a row is bit x & 31 of word x >> 5, least significant bit first (numpy.packbits(...,
// bitorder="little"), the convention of mrcnn_unpack_mask_bits); the bits past W in a row's last word are always zero -- every
// kernel here writes them as zero and may rely on reading them as zero.  Three entry points:
//   mask_pack_kernel + mask_stats_kernel   [H, W, n] bytes -> planes, and per plane its pixel count and box (utils.extract_bboxes);
//   mask_pair_stats_kernel                 per pair of planes: popcount(a & b) -- mask_iou's intersection; the union is count_a +
//                                          count_b - inter on the host -- and the 4-neighbour predicate analyze.masks_touch4,
//                                          which equals Analyzer.are_mask_connected (the component count of a | b drops below
//                                          n_a + n_b iff some pixel of a equals or is a 4-neighbour of some pixel of b);
//   mask_union_kernel                      OR of the members of each component (merge_masks chains), with count and box;
//   source_planes_kernel + mask_stats_kernel   the bit-mask sources of a mosaic (mrcnn_tile_source) -> planes of a frame shrunk by
//                                          k: a bit is set when the source has a pixel in its k x k block.
// Integer kernels, latency-bound: no MFMA; LDS only to turn the (x, d)-contiguous bytes into per-detection ballots and for the
// per-plane reductions.
#include "common.h"
#include "tile_source.h"
#include <climits>

#define MG_DC 64        // detections per staging pass of the pack kernel

// Count and box of the set bits seen by this workgroup (256 threads), from per-thread partial results; thread 0 writes
// count[c] and box[c] = (y1, x1, y2, x2), y2 / x2 exclusive, zeros when nothing is set.
__device__ __forceinline__ void mg_block_stats(int cnt, int bx0, int by0, int bx1, int by1, int* s, int c, int* __restrict__ count,
                                               int* __restrict__ box) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        s[0] = 0; s[1] = INT_MAX; s[2] = INT_MAX; s[3] = -1; s[4] = -1;
    }
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        bx0 = min(bx0, __shfl_xor(bx0, o, 64)); by0 = min(by0, __shfl_xor(by0, o, 64));
        bx1 = max(bx1, __shfl_xor(bx1, o, 64)); by1 = max(by1, __shfl_xor(by1, o, 64));
    }
    if ((tid & 63) == 0 && cnt) {
        atomicAdd(&s[0], cnt);
        atomicMin(&s[1], bx0); atomicMin(&s[2], by0);
        atomicMax(&s[3], bx1); atomicMax(&s[4], by1);
    }
    __syncthreads();
    if (tid == 0) {
        const bool any = s[0] > 0;
        count[c] = s[0];
        box[4 * c + 0] = any ? s[2] : 0;
        box[4 * c + 1] = any ? s[1] : 0;
        box[4 * c + 2] = any ? s[4] + 1 : 0;
        box[4 * c + 3] = any ? s[3] + 1 : 0;
    }
}

__device__ __forceinline__ void mg_accumulate(unsigned u, int y, int k, int& cnt, int& bx0, int& by0, int& bx1, int& by1) {
    if (u) {
        cnt += __popc(u);
        bx0 = min(bx0, 32 * k + __ffs((int)u) - 1);
        bx1 = max(bx1, 32 * k + 31 - __clz((int)u));
        by0 = min(by0, y);
        by1 = max(by1, y);
    }
}

// One wavefront per 64 consecutive pixels of a row, four per workgroup.  Per pass of up to MG_DC detections the wavefront
// reads its pixels' bytes in address order (one contiguous run when n <= MG_DC, runs of MG_DC bytes otherwise), stages the
// "set" flags transposed in LDS and takes one __ballot per detection: the two words of that detection's plane.
__global__ __launch_bounds__(256) void mask_pack_kernel(const unsigned char* __restrict__ masks, int H, int W, int n, int wpr,
                                                        unsigned* __restrict__ planes) {
    __shared__ unsigned char s_flag[4][MG_DC][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int segs = (W + 63) >> 6;
    const long long task = (long long)blockIdx.x * 4 + wv;          // wave-uniform
    const bool active = task < (long long)H * segs;
    const int y = active ? (int)(task / segs) : 0, seg = active ? (int)(task % segs) : 0;
    const int x0 = seg << 6;
    const int npix = active ? min(64, W - x0) : 0;                   // pixels of this wavefront inside the row
    const long long pix0 = (long long)y * W + x0;
    const long long plane_words = (long long)H * wpr;
    for (int d0 = 0; d0 < n; d0 += MG_DC) {                          // the same trip count for every wavefront
        const int dc = min(MG_DC, n - d0);
        for (int idx = lane; idx < 64 * dc; idx += 64) {
            const int p = idx / dc, dd = idx - p * dc;
            unsigned char v = 0;
            if (p < npix) v = masks[(pix0 + p) * n + d0 + dd] != 0;
            s_flag[wv][dd][p] = v;
        }
        __syncthreads();
        unsigned lo = 0u, hi = 0u;                                   // lane dd keeps the words of detection d0 + dd
        for (int dd = 0; dd < dc; ++dd) {
            const unsigned long long b = __ballot(s_flag[wv][dd][lane] != 0);
            if (lane == dd) {
                lo = (unsigned)b;
                hi = (unsigned)(b >> 32);
            }
        }
        if (active && lane < dc) {
            unsigned* row = planes + (long long)(d0 + lane) * plane_words + (long long)y * wpr;
            row[2 * seg] = lo;
            if (2 * seg + 1 < wpr) row[2 * seg + 1] = hi;
        }
        __syncthreads();
    }
}

// One workgroup per plane: pixel count and box.
__global__ __launch_bounds__(256) void mask_stats_kernel(const unsigned* __restrict__ planes, int H, int wpr, int* __restrict__ count,
                                                         int* __restrict__ box) {
    __shared__ int s[5];
    const int c = blockIdx.x;
    const long long total = (long long)H * wpr;
    const unsigned* pl = planes + (long long)c * total;
    int cnt = 0, bx0 = INT_MAX, by0 = INT_MAX, bx1 = -1, by1 = -1;
    for (long long idx = threadIdx.x; idx < total; idx += 256)
        mg_accumulate(pl[idx], (int)(idx / wpr), (int)(idx % wpr), cnt, bx0, by0, bx1, by1);
    mg_block_stats(cnt, bx0, by0, bx1, by1, s, c, count, box);
}

// One wavefront per pair, four pairs per workgroup.  Window = b's box intersected with a's box grown by one pixel, clipped to
// the frame; a lane takes one word of b in the window, and the words of a at the same place, left and right of it (for the
// carry across x = 31 | 32) and in the rows above and below (zero outside the frame).
__global__ __launch_bounds__(256) void mask_pair_stats_kernel(const unsigned* __restrict__ planes, const int* __restrict__ box, int n, int H,
                                                              int W, int wpr, const int* __restrict__ pairs, int P, int* __restrict__ inter,
                                                              int* __restrict__ touch) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);       // wave-uniform
    if (p >= P) return;
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    int cnt = 0;
    bool hit = false;
    if ((unsigned)i < (unsigned)n && (unsigned)j < (unsigned)n) {
        const int ay1 = box[4 * i], ax1 = box[4 * i + 1], ay2 = box[4 * i + 2], ax2 = box[4 * i + 3];
        const int by1 = box[4 * j], bx1 = box[4 * j + 1], by2 = box[4 * j + 2], bx2 = box[4 * j + 3];
        if (ay2 > ay1 && ax2 > ax1 && by2 > by1 && bx2 > bx1) {
            // inclusive window, inside the frame whatever the boxes hold
            const int gy0 = max(max(by1, ay1 - 1), 0), gy1 = min(min(by2 - 1, ay2), H - 1);
            const int gx0 = max(max(bx1, ax1 - 1), 0), gx1 = min(min(bx2 - 1, ax2), W - 1);
            if (gy0 <= gy1 && gx0 <= gx1) {
                const long long plane_words = (long long)H * wpr;
                const unsigned* A = planes + (long long)i * plane_words;
                const unsigned* B = planes + (long long)j * plane_words;
                const int k0 = gx0 >> 5, nk = (gx1 >> 5) - k0 + 1;
                const int total = (gy1 - gy0 + 1) * nk;              // <= H * wpr
                for (int idx = lane; idx < total; idx += 64) {
                    const int r = gy0 + idx / nk, k = k0 + idx % nk;
                    const unsigned wb = B[(long long)r * wpr + k];
                    if (wb) {
                        const unsigned* ar = A + (long long)r * wpr;
                        const unsigned wa = ar[k];
                        cnt += __popc(wa & wb);
                        unsigned dil = wa | (wa << 1) | (wa >> 1);
                        if (k > 0) dil |= ar[k - 1] >> 31;
                        if (k + 1 < wpr) dil |= ar[k + 1] << 31;
                        if (r > 0) dil |= ar[k - wpr];
                        if (r + 1 < H) dil |= ar[k + wpr];
                        hit = hit || (dil & wb) != 0u;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    const unsigned long long any = __ballot(hit);
    if (lane == 0) {
        inter[p] = cnt;
        touch[p] = any != 0ull ? 1 : 0;
    }
}

// One workgroup per component: OR of the members' planes, written in full (zero where no member has a bit), count and box.
__global__ __launch_bounds__(256) void mask_union_kernel(const unsigned* __restrict__ planes, int n, int H, int wpr,
                                                         const int* __restrict__ comp_offsets, const int* __restrict__ member_ids, int M,
                                                         unsigned* __restrict__ out, int* __restrict__ count, int* __restrict__ box) {
    __shared__ int s[5];
    const int c = blockIdx.x;
    int m0 = comp_offsets[c], m1 = comp_offsets[c + 1];
    m0 = max(0, min(m0, M));
    m1 = max(m0, min(m1, M));
    const long long total = (long long)H * wpr;
    unsigned* o = out + (long long)c * total;
    int cnt = 0, bx0 = INT_MAX, by0 = INT_MAX, bx1 = -1, by1 = -1;
    for (long long idx = threadIdx.x; idx < total; idx += 256) {
        unsigned u = 0u;
        for (int q = m0; q < m1; ++q) {
            const int id = member_ids[q];
            if ((unsigned)id < (unsigned)n) u |= planes[(long long)id * total + idx];
        }
        o[idx] = u;
        mg_accumulate(u, (int)(idx / wpr), (int)(idx % wpr), cnt, bx0, by0, bx1, by1);
    }
    mg_block_stats(cnt, bx0, by0, bx1, by1, s, c, count, box);
}

static inline bool mg_frame_ok(int n, int H, int W) { return n > 0 && H > 0 && W > 0; }

extern "C" int mrcnn_mask_planes_pack(const void* masks, int H, int W, int n, void* planes, int32_t* count, int32_t* box, void* stream) {
    if (!mg_frame_ok(n, H, W) || !masks || !planes || !count || !box) return MRCNN_ERR_ARG;
    const int wpr = (W + 31) >> 5;
    const int64_t tasks = (int64_t)H * ((W + 63) >> 6);
    if (tasks > 0x7FFFFFFFll || (int64_t)H * wpr > 0x7FFFFFFFll) return MRCNN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)cdiv64(tasks, 4)), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)masks, H,
                       W, n, wpr, (unsigned*)planes);
    hipLaunchKernelGGL(mask_stats_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, (const unsigned*)planes, H, wpr, (int*)count,
                       (int*)box);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_mask_pair_stats(const void* planes, const int32_t* box, int n, int H, int W, const int32_t* pairs, int P, int32_t* inter,
                                     int32_t* touch, void* stream) {
    if (!mg_frame_ok(n, H, W) || P < 0) return MRCNN_ERR_ARG;
    if (P == 0) return MRCNN_OK;
    if (!planes || !box || !pairs || !inter || !touch) return MRCNN_ERR_ARG;
    const int wpr = (W + 31) >> 5;
    if ((int64_t)H * wpr > 0x7FFFFFFFll) return MRCNN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mask_pair_stats_kernel, dim3((unsigned)cdiv64(P, 4)), dim3(256), 0, (hipStream_t)stream, (const unsigned*)planes,
                       (const int*)box, n, H, W, wpr, (const int*)pairs, P, (int*)inter, (int*)touch);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_mask_union(const void* planes, int n, int H, int W, const int32_t* comp_offsets, const int32_t* member_ids, int C, int M,
                                void* out_planes, int32_t* out_count, int32_t* out_box, void* stream) {
    if (!mg_frame_ok(n, H, W) || C < 0 || M < 0) return MRCNN_ERR_ARG;
    if (C == 0) return MRCNN_OK;
    if (!planes || !comp_offsets || !member_ids || !out_planes || !out_count || !out_box || out_planes == planes) return MRCNN_ERR_ARG;
    const int wpr = (W + 31) >> 5;
    if ((int64_t)H * wpr > 0x7FFFFFFFll) return MRCNN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mask_union_kernel, dim3((unsigned)C), dim3(256), 0, (hipStream_t)stream, (const unsigned*)planes, n, H, wpr,
                       (const int*)comp_offsets, (const int*)member_ids, M, (unsigned*)out_planes, (int*)out_count, (int*)out_box);
    return mrcnn_launch_status();
}

// One thread per output word (i, Y, Kw): it covers the plane pixels [k Y, k (Y + 1)) x [32 k Kw, 32 k (Kw + 1)), clipped to the
// frame's w columns and to source i's box.  The thread ORs the source's words over those rows and moves every set bit to the
// output column (x0 + local column) / k: a gather, no atomics; words outside the box and the bits past w come out zero.
__global__ __launch_bounds__(256) void source_planes_kernel(const unsigned* __restrict__ pool, long long pool_words,
                                                            const TmSrc* __restrict__ desc, int n, int k, int h, int w, int wpr,
                                                            unsigned* __restrict__ planes) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * h * wpr) return;
    const int Kw = (int)(idx % wpr);
    const long long t = idx / wpr;
    const int Y = (int)(t % h), i = (int)(t / h);
    const TmSrc d = desc[i];
    unsigned out = 0u;
    if (tm_valid(d)) {
        const int nbits = min(32, w - 32 * Kw);
        const long long ry0 = max((long long)Y * k - d.y0, 0ll), ry1 = min(((long long)Y + 1) * k - d.y0, (long long)d.h);
        const long long cx0 = max(32ll * Kw * k - d.x0, 0ll), cx1 = min((32ll * Kw + nbits) * k - d.x0, (long long)d.w);
        if (ry0 < ry1 && cx0 < cx1) {
            for (long long p = cx0 & ~31ll; p < cx1; p += 32) {           // the words of the source's rows under this output word
                unsigned acc = 0u;
                for (long long r = ry0; r < ry1; ++r) acc |= tm_word(pool, pool_words, d, (int)r, (int)(p >> 5));
                if (p < cx0) acc &= 0xFFFFFFFFu << (int)(cx0 - p);
                if (cx1 - p < 32) acc &= 0xFFFFFFFFu >> (int)(32 - (cx1 - p));
                while (acc) {
                    const int j = __ffs((int)acc) - 1;
                    acc &= acc - 1u;
                    out |= 1u << (int)(((long long)d.x0 + p + j) / k - 32ll * Kw);
                }
            }
        }
    }
    planes[idx] = out;
}

extern "C" int mrcnn_sources_to_planes_check(int n, int shrink, int h, int w) {
    if (n <= 0 || shrink <= 0 || h <= 0 || w <= 0) return MRCNN_ERR_ARG;
    const int64_t wpr = ((int64_t)w + 31) >> 5;
    if ((int64_t)n * h * wpr > 0x7FFFFFFFll || (int64_t)shrink * h > 0x7FFFFFFFll || (int64_t)shrink * wpr * 32 > 0x7FFFFFFFll)
        return MRCNN_ERR_UNSUPPORTED;
    return MRCNN_OK;
}

extern "C" int mrcnn_sources_to_planes(const void* pool, int64_t pool_words, const mrcnn_tile_source* desc, int n, int shrink, int h, int w,
                                       void* planes, int32_t* count, int32_t* box, void* stream) {
    const int rc = mrcnn_sources_to_planes_check(n, shrink, h, w);
    if (rc != MRCNN_OK) return rc;
    if (!pool || pool_words < 0 || !desc || !planes || !count || !box) return MRCNN_ERR_ARG;
    const int wpr = (w + 31) >> 5;
    const int64_t words = (int64_t)n * h * wpr;
    hipLaunchKernelGGL(source_planes_kernel, dim3((unsigned)cdiv64(words, 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned*)pool,
                       (long long)pool_words, desc, n, shrink, h, w, wpr, (unsigned*)planes);
    hipLaunchKernelGGL(mask_stats_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, (const unsigned*)planes, h, wpr, (int*)count,
                       (int*)box);
    return mrcnn_launch_status();
}
