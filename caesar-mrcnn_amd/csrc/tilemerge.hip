// Stitching of sources across tile borders (SFinder.merge_edge_sources, mrcnn/sfinder.py:711-935) on bit masks.
// A source is the row-major bitmap of its bounding box in mosaic coordinates: bit (x - x0) of row (y - y0), 32-bit words,
// least significant bit first (numpy.packbits(..., bitorder="little"), the convention of mrcnn_unpack_mask_bits), all sources
// in one pool of words, one mrcnn_tile_source descriptor each.  Two kernels, one launch each for the whole mosaic:
//   tile_adjacency_kernel  the pixel-pair loops :787-810 (any pixel of i within |dx| <= 1 and |dy| <= 1 of a pixel of j) as
//                          "i dilated by one pixel" AND j, word by word;
//   tile_union_kernel      the list-membership union :848-862 and the pixel min / max box :873-884 as ORs, plus the
//                          "fresh" bitmaps member_k AND NOT (member_0 | ... | member_{k-1}) whose set bits, member after
//                          member, are the reference's first-seen pixel order.
// Every read goes through tm_word: rows / words outside a source, padding bits past its width and addresses past the pool
// read as zero.  Integer kernels, latency-bound: no LDS tiles, no MFMA.
#include "common.h"
#include "tile_source.h"
#include <climits>

// One wavefront per pair, four pairs per workgroup.
__global__ __launch_bounds__(256) void tile_adjacency_kernel(const unsigned* __restrict__ pool, long long pool_words,
                                                             const TmSrc* __restrict__ desc, int n, const int* __restrict__ pairs, int P,
                                                             int* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);       // wave-uniform
    if (p >= P) return;
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    int found = 0;
    if ((unsigned)i < (unsigned)n && (unsigned)j < (unsigned)n) {
        const TmSrc a = desc[i], b = desc[j];
        if (tm_valid(a) && tm_valid(b)) {
            // window = j's box intersected with i's box grown by one pixel, in j's local coordinates (inclusive)
            const int gx0 = max(b.x0, a.x0 - 1), gx1 = min(b.x0 + b.w - 1, a.x0 + a.w);
            const int gy0 = max(b.y0, a.y0 - 1), gy1 = min(b.y0 + b.h - 1, a.y0 + a.h);
            if (gx0 <= gx1 && gy0 <= gy1) {
                const int k0 = (gx0 - b.x0) >> 5, nk = ((gx1 - b.x0) >> 5) - k0 + 1;
                const int r0 = gy0 - b.y0, nr = gy1 - gy0 + 1;
                const long long total = (long long)nr * nk;
                for (long long base = 0; base < total; base += 64) {        // wave-uniform trip count
                    const long long idx = base + lane;
                    bool hit = false;
                    if (idx < total) {
                        const int r = r0 + (int)(idx / nk), k = k0 + (int)(idx % nk);
                        const unsigned wj = tm_word(pool, pool_words, b, r, k);
                        if (wj) {
                            const int ya = b.y0 + r - a.y0;                 // i's local row of the same mosaic row
                            const int xs = b.x0 + 32 * k - a.x0 - 1;        // i's local bit of the pixel left of j's bit 0
                            // i's rows ya-1, ya, ya+1 OR-ed, as the 34 bits xs .. xs+33 (re-aligned to j's bit origin - 1)
                            unsigned lo = 0u, hi = 0u;
                            for (int dy = -1; dy <= 1; ++dy) {
                                lo |= tm_bits(pool, pool_words, a, ya + dy, xs);
                                hi |= tm_bits(pool, pool_words, a, ya + dy, xs + 32);
                            }
                            const unsigned long long e = ((unsigned long long)(hi & 3u) << 32) | lo;
                            // bit b of: e = left neighbour, e >> 1 = same column, e >> 2 = right neighbour of j's pixel b
                            const unsigned dil = (unsigned)(e | (e >> 1) | (e >> 2));
                            hit = (dil & wj) != 0u;
                        }
                    }
                    if (__ballot(hit) != 0ull) {
                        found = 1;
                        break;
                    }
                }
            }
        }
    }
    if (lane == 0) out[p] = found;
}

// One workgroup per component.
__global__ __launch_bounds__(256) void tile_union_kernel(const unsigned* __restrict__ pool, long long pool_words,
                                                         const TmSrc* __restrict__ desc, int n, const int* __restrict__ comp_offsets,
                                                         const int* __restrict__ member_ids, int M, const long long* __restrict__ out_offsets,
                                                         const long long* __restrict__ fresh_offsets, TmSrc* __restrict__ out_desc,
                                                         int* __restrict__ out_count, unsigned* __restrict__ out_pool, long long out_pool_words,
                                                         unsigned* __restrict__ fresh_pool, long long fresh_pool_words) {
    __shared__ int s_box[4];        // x min, y min, x max, y max (inclusive) of the set bits
    __shared__ int s_count;
    const int c = blockIdx.x, tid = threadIdx.x;
    int m0 = comp_offsets[c], m1 = comp_offsets[c + 1];
    m0 = max(0, min(m0, M));
    m1 = max(m0, min(m1, M));
    // the members' box (every thread computes it: a handful of descriptors, cached)
    int lx0 = INT_MAX, ly0 = INT_MAX, lx1 = INT_MIN, ly1 = INT_MIN;
    for (int q = m0; q < m1; ++q) {
        const int id = member_ids[q];
        if ((unsigned)id >= (unsigned)n) continue;
        const TmSrc d = desc[id];
        if (!tm_valid(d)) continue;
        lx0 = min(lx0, d.x0); ly0 = min(ly0, d.y0);
        lx1 = max(lx1, d.x0 + d.w - 1); ly1 = max(ly1, d.y0 + d.h - 1);
    }
    if (tid == 0) {
        s_box[0] = INT_MAX; s_box[1] = INT_MAX; s_box[2] = INT_MIN; s_box[3] = INT_MIN;
        s_count = 0;
    }
    __syncthreads();
    // pass 1: tighten to the set bits (the reference's pixel min / max, :873-882)
    if (lx0 <= lx1) {
        const int nk = ((lx1 - lx0) >> 5) + 1;
        const long long total = (long long)(ly1 - ly0 + 1) * nk;
        int bx0 = INT_MAX, by0 = INT_MAX, bx1 = INT_MIN, by1 = INT_MIN;
        for (long long idx = tid; idx < total; idx += 256) {
            const int y = ly0 + (int)(idx / nk), x = lx0 + 32 * (int)(idx % nk);
            unsigned u = 0u;
            for (int q = m0; q < m1; ++q) {
                const int id = member_ids[q];
                if ((unsigned)id >= (unsigned)n) continue;
                const TmSrc d = desc[id];
                if (tm_valid(d)) u |= tm_bits(pool, pool_words, d, y - d.y0, x - d.x0);
            }
            if (u) {
                bx0 = min(bx0, x + __ffs((int)u) - 1);
                bx1 = max(bx1, x + 31 - __clz((int)u));
                by0 = min(by0, y);
                by1 = max(by1, y);
            }
        }
        if (bx0 <= bx1) {
            atomicMin(&s_box[0], bx0); atomicMin(&s_box[1], by0);
            atomicMax(&s_box[2], bx1); atomicMax(&s_box[3], by1);
        }
    }
    __syncthreads();
    const int tx0 = s_box[0], ty0 = s_box[1], tx1 = s_box[2], ty1 = s_box[3];
    const bool any = tx0 <= tx1;
    const int tw = any ? tx1 - tx0 + 1 : 0, th = any ? ty1 - ty0 + 1 : 0, twpr = (tw + 31) >> 5;
    // pass 2: the union bitmap in the tight box, and its pixel count
    const long long ooff = out_offsets[c];
    int cnt = 0;
    for (long long idx = tid; idx < (long long)th * twpr; idx += 256) {
        const int r = (int)(idx / twpr), k = (int)(idx % twpr);
        unsigned u = 0u;
        for (int q = m0; q < m1; ++q) {
            const int id = member_ids[q];
            if ((unsigned)id >= (unsigned)n) continue;
            const TmSrc d = desc[id];
            if (tm_valid(d)) u |= tm_bits(pool, pool_words, d, ty0 + r - d.y0, tx0 + 32 * k - d.x0);
        }
        const int valid = tw - 32 * k;
        if (valid < 32) u &= 0xFFFFFFFFu >> (32 - valid);           // valid >= 1 here
        cnt += __popc(u);
        if (ooff >= 0 && ooff + idx < out_pool_words) out_pool[ooff + idx] = u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0 && cnt) atomicAdd(&s_count, cnt);
    // fresh bitmaps: member q's own words minus everything the members before it already hold, in member q's box
    for (int q = m0; q < m1; ++q) {
        const int id = member_ids[q];
        if ((unsigned)id >= (unsigned)n) continue;
        const TmSrc d = desc[id];
        if (!tm_valid(d)) continue;
        const long long foff = fresh_offsets[q];
        const long long total = (long long)d.h * d.words_per_row;
        for (long long idx = tid; idx < total; idx += 256) {
            const int r = (int)(idx / d.words_per_row), k = (int)(idx % d.words_per_row);
            unsigned own = tm_word(pool, pool_words, d, r, k);
            for (int t = m0; t < q && own; ++t) {
                const int it = member_ids[t];
                if ((unsigned)it >= (unsigned)n) continue;
                const TmSrc e = desc[it];
                if (tm_valid(e)) own &= ~tm_bits(pool, pool_words, e, d.y0 + r - e.y0, d.x0 + 32 * k - e.x0);
            }
            if (foff >= 0 && foff + idx < fresh_pool_words) fresh_pool[foff + idx] = own;
        }
    }
    __syncthreads();
    if (tid == 0) {
        TmSrc o;
        o.x0 = any ? tx0 : 0; o.y0 = any ? ty0 : 0; o.w = tw; o.h = th;
        o.word_offset = (int)ooff; o.words_per_row = twpr;
        out_desc[c] = o;
        out_count[c] = s_count;
    }
}

extern "C" int mrcnn_tile_adjacency(const void* pool, int64_t pool_words, const mrcnn_tile_source* desc, int n, const int32_t* pairs,
                                    int P, int32_t* out, void* stream) {
    if (P < 0 || n < 0 || pool_words < 0) return MRCNN_ERR_ARG;
    if (P == 0) return MRCNN_OK;
    if (!pool || !desc || !pairs || !out || n == 0) return MRCNN_ERR_ARG;
    if (pool_words > 0x7FFFFFFFll) return MRCNN_ERR_UNSUPPORTED;        // word_offset is 32-bit
    hipLaunchKernelGGL(tile_adjacency_kernel, dim3((unsigned)cdiv64(P, 4)), dim3(256), 0, (hipStream_t)stream, (const unsigned*)pool,
                       (long long)pool_words, desc, n, (const int*)pairs, P, (int*)out);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_tile_union(const void* pool, int64_t pool_words, const mrcnn_tile_source* desc, int n, const int32_t* comp_offsets,
                                const int32_t* member_ids, int C, int M, const int64_t* out_offsets, const int64_t* fresh_offsets,
                                mrcnn_tile_source* out_desc, int32_t* out_count, void* out_pool, int64_t out_pool_words, void* fresh_pool,
                                int64_t fresh_pool_words, void* stream) {
    if (C < 0 || M < 0 || n < 0 || pool_words < 0 || out_pool_words < 0 || fresh_pool_words < 0) return MRCNN_ERR_ARG;
    if (C == 0) return MRCNN_OK;
    if (!pool || !desc || !comp_offsets || !member_ids || !out_offsets || !fresh_offsets || !out_desc || !out_count || !out_pool ||
        !fresh_pool || n == 0)
        return MRCNN_ERR_ARG;
    if (pool_words > 0x7FFFFFFFll || out_pool_words > 0x7FFFFFFFll) return MRCNN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tile_union_kernel, dim3((unsigned)C), dim3(256), 0, (hipStream_t)stream, (const unsigned*)pool, (long long)pool_words,
                       desc, n, (const int*)comp_offsets, (const int*)member_ids, M, (const long long*)out_offsets,
                       (const long long*)fresh_offsets, out_desc, (int*)out_count, (unsigned*)out_pool, (long long)out_pool_words,
                       (unsigned*)fresh_pool, (long long)fresh_pool_words);
    return mrcnn_launch_status();
}
