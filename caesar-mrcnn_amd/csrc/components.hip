// Connected components of the bit planes of the mask graph (maskgraph.hip: planes[n][H][wpr], least significant bit first, bits
// past W zero; boxes (y1, x1, y2, x2) as _pack / _union give them), numbered as analyze.label_components numbers them: 1..k in
// raster order of each component's first pixel.  One workgroup of 256 threads per plane, inside the plane's box:
//   runs     a row's maximal stretches of set bits, taken from the words by bit tricks (a start is a set bit whose left
//            neighbour is clear, an end one whose right neighbour is clear; the j-th start pairs with the j-th end).  A run's id is
//            its rank in raster order (row, then start): a prefix sum of the rows' run counts, then one thread per row;
//   unions   adjacent rows are merged by two pointers, one thread per row pair: runs [s, e] and [s', e'] are joined when
//            s <= e' + c and s' <= e + c, c = 0 for 4- and 1 for 8-connectivity.  Union-find with the SMALLER id as parent:
//            parent[] only ever decreases, hooks are atomicMin on a root (retried from the value found when it no longer was one),
//            so whatever order the hooks land in, a component's root is its smallest id -- the run of its first pixel;
//   labels   label[root] = 1 + the number of roots below it (a prefix sum over the ids), label[run] = label[root].
// parent[] lives in LDS (48 KiB, ds_min_rtn_u32) for up to MC_LDS_RUNS runs, else in the caller's workspace (global_atomic_smin,
// read back with agent-scope loads so that no stale L1 line is seen; any value ever stored is an ancestor, so a stale read
// would only cost a retry).  No float, no cross-workgroup traffic, no loop that waits for another workgroup; everything that
// reaches the outputs is independent of the order of the atomics, so two runs give the same bytes.
// The emit kernel turns the run table into one plane per component (the layout of mask_union_kernel's outputs), the row-extent
// kernel is a bit scan per row and has no labelling.
#include "common.h"
#include <climits>

#define MC_THREADS 256
#define MC_LDS_RUNS 12288            // parent[] entries kept in LDS: 48 KiB of a workgroup's static 64 KiB
#define MC_MAX_SIDE 8192             // starts and ends are 16-bit
#define MC_MAX_PLANES 4096           // every workgroup sums the boxes before its own
#define MC_MAX_RUNS (1 << 22)        // run capacity of one plane's box: rows * ceil(columns / 2)
#define MC_MAX_PIECES (1 << 24)

struct mc_box { int y1, x1, bh, bw; };

// A box cut to the frame; bh = bw = 0 when nothing is left.  The host sizes the workspace with this and the kernels place their
// tables with it, from the host and the device copy of one table.
__host__ __device__ static inline mc_box mc_clip(const int32_t* b, int H, int W) {
    mc_box r;
    r.y1 = b[0] < 0 ? 0 : (b[0] > H ? H : b[0]);                    // all four inside [0, H] / [0, W]: no difference overflows
    r.x1 = b[1] < 0 ? 0 : (b[1] > W ? W : b[1]);
    const int y2 = b[2] < 0 ? 0 : (b[2] > H ? H : b[2]), x2 = b[3] < 0 ? 0 : (b[3] > W ? W : b[3]);
    r.bh = y2 - r.y1;
    r.bw = x2 - r.x1;
    if (r.bh <= 0 || r.bw <= 0) r.bh = r.bw = r.y1 = r.x1 = 0;
    return r;
}
__host__ __device__ static inline long long mc_cap(const mc_box& b) { return (long long)b.bh * ((b.bw + 1) >> 1); }
// Workspace words of one plane: row_off[bh + 1], start / end [cap] (two 16-bit halves), label[cap], and parent[cap] when the
// box can hold more runs than the LDS table.
__host__ __device__ static inline long long mc_words(const mc_box& b) {
    const long long cap = mc_cap(b);
    return (long long)b.bh + 1 + (cap > MC_LDS_RUNS ? 3 : 2) * cap;
}

// Word k of a row with the bits outside columns [x1, x2) cleared; k in [x1 >> 5, (x2 - 1) >> 5].
__device__ __forceinline__ unsigned mc_word(const unsigned* __restrict__ row, int k, int x1, int x2) {
    unsigned w = row[k];
    const int lo = x1 - 32 * k, hi = x2 - 32 * k;
    if (lo > 0) w &= ~0u << lo;
    if (hi < 32) w &= (1u << hi) - 1u;
    return w;
}

// Exclusive prefix sum of v over the 256 threads, and the total.  s_w: 4 ints, free again on return.
__device__ __forceinline__ int mc_block_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < MC_THREADS / 64; ++q) {
        const int t = s_w[q];
        if (q < wv) before += t;
        all += t;
    }
    __syncthreads();
    total = all;
    return before + inc - v;
}

// Sum of the workspace words of the planes before plane p (block-wide; every thread gets it).  s_ll: one long long.
__device__ __forceinline__ long long mc_offset_of(const int32_t* __restrict__ box, int p, int H, int W, long long* s_ll) {
    long long part = 0;
    for (int q = threadIdx.x; q < p; q += MC_THREADS) part += mc_words(mc_clip(box + 4 * q, H, W));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (threadIdx.x == 0) *s_ll = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && part) atomicAdd((unsigned long long*)s_ll, (unsigned long long)part);      // integer: any order
    __syncthreads();
    const long long off = *s_ll;
    __syncthreads();
    return off;
}

template <bool LDS>
__device__ __forceinline__ int mc_load(const int* p) {
    if (LDS) return *(const volatile int*)p;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ void mc_store(int* p, int v) {
    if (LDS) *(volatile int*)p = v;
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ int mc_find(const int* parent, int a) {
    for (;;) {                                                       // parent[x] <= x: strictly down to the root
        const int q = mc_load<LDS>(parent + a);
        if (q == a) return a;
        a = q;
    }
}
template <bool LDS>
__device__ __forceinline__ void mc_union(int* parent, int a, int b) {
    for (;;) {
        a = mc_find<LDS>(parent, a);
        b = mc_find<LDS>(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);                    // hook the larger root under the smaller
        if (old == a) return;
        a = old;                                                     // a had a parent by then (now min(old, b)): join that with b
    }
}

// Unions, roots and labels of the nruns runs whose rows are row_off[0 .. bh]; returns the component count to every thread.
template <bool LDS>
__device__ __forceinline__ int mc_label(int* parent, const int* __restrict__ row_off, const unsigned short* __restrict__ st,
                                        const unsigned short* __restrict__ en, int* __restrict__ label, int bh, int nruns, int c, int* s_w) {
    const int tid = threadIdx.x;
    for (int id = tid; id < nruns; id += MC_THREADS) mc_store<LDS>(parent + id, id);
    __syncthreads();
    for (int r = 1 + tid; r < bh; r += MC_THREADS) {
        int i = row_off[r - 1], j = row_off[r];
        const int i1 = j, j1 = row_off[r + 1];
        while (i < i1 && j < j1) {
            const int si = st[i], ei = en[i], sj = st[j], ej = en[j];
            if (si <= ej + c && sj <= ei + c) mc_union<LDS>(parent, i, j);
            if (ei < ej) ++i; else ++j;
        }
    }
    __syncthreads();
    for (int id = tid; id < nruns; id += MC_THREADS) mc_store<LDS>(parent + id, mc_find<LDS>(parent, id));
    __syncthreads();
    int carry = 0;
    for (int base = 0; base < nruns; base += MC_THREADS) {           // the same trip count for every thread
        const int id = base + tid;
        const int root = id < nruns && mc_load<LDS>(parent + id) == id;
        int total;
        const int below = mc_block_scan(root, s_w, total);
        if (root) label[id] = carry + below + 1;
        carry += total;
    }
    __syncthreads();
    for (int id = tid; id < nruns; id += MC_THREADS) {
        const int root = mc_load<LDS>(parent + id);
        if (root != id) label[id] = label[root];                     // a root's label is written above and never again
    }
    return carry;
}

__global__ __launch_bounds__(MC_THREADS) void mask_components_count_kernel(const unsigned* __restrict__ planes, const int32_t* __restrict__ box,
                                                                           int n, int H, int W, int wpr, int c, int* __restrict__ ws,
                                                                           long long ws_words, int* __restrict__ ncomp) {
    __shared__ int s_parent[MC_LDS_RUNS];
    __shared__ int s_w[MC_THREADS / 64];
    __shared__ long long s_ll;
    const int p = blockIdx.x, tid = threadIdx.x;
    const long long off = mc_offset_of(box, p, H, W, &s_ll);
    const mc_box b = mc_clip(box + 4 * p, H, W);
    const long long cap = mc_cap(b);
    if (cap > MC_MAX_RUNS || off + mc_words(b) > ws_words) {         // not the table the workspace was sized for: nothing is touched
        if (tid == 0) ncomp[p] = 0;
        return;
    }
    int* row_off = ws + off;
    unsigned short* st = (unsigned short*)(row_off + b.bh + 1);
    unsigned short* en = st + cap;
    int* label = row_off + b.bh + 1 + cap;
    int* g_parent = label + cap;                                     // there only when cap > MC_LDS_RUNS
    const unsigned* pl = planes + (long long)p * H * wpr;
    const int x1 = b.x1, x2 = b.x1 + b.bw;
    const int k0 = x1 >> 5, k1 = b.bw > 0 ? (x2 - 1) >> 5 : k0 - 1;

    int carry = 0;
    for (int base = 0; base < b.bh; base += MC_THREADS) {            // runs per row, and their prefix sum
        const int r = base + tid;
        int cnt = 0;
        if (r < b.bh) {
            const unsigned* row = pl + (long long)(b.y1 + r) * wpr;
            unsigned prev = 0u;
            for (int k = k0; k <= k1; ++k) {
                const unsigned w = mc_word(row, k, x1, x2);
                cnt += __popc(w & ~((w << 1) | prev));
                prev = w >> 31;
            }
        }
        int total;
        const int below = mc_block_scan(cnt, s_w, total);
        if (r < b.bh) row_off[r] = carry + below;
        carry += total;
    }
    const int nruns = carry;                                         // <= cap: a run needs a clear bit before the next
    if (tid == 0) row_off[b.bh] = nruns;
    __syncthreads();
    for (int r = tid; r < b.bh; r += MC_THREADS) {                   // the runs of a row, in order
        const unsigned* row = pl + (long long)(b.y1 + r) * wpr;
        int is = row_off[r], ie = is;
        unsigned prev = 0u, w = k0 <= k1 ? mc_word(row, k0, x1, x2) : 0u;
        for (int k = k0; k <= k1; ++k) {
            const unsigned next = k < k1 ? mc_word(row, k + 1, x1, x2) : 0u;
            unsigned starts = w & ~((w << 1) | prev), ends = w & ~((w >> 1) | (next << 31));
            while (starts) {
                st[is++] = (unsigned short)(32 * k + __ffs((int)starts) - 1);
                starts &= starts - 1u;
            }
            while (ends) {
                en[ie++] = (unsigned short)(32 * k + __ffs((int)ends) - 1);
                ends &= ends - 1u;
            }
            prev = w >> 31;
            w = next;
        }
    }
    __syncthreads();
    int k;
    if (nruns <= MC_LDS_RUNS) k = mc_label<true>(s_parent, row_off, st, en, label, b.bh, nruns, c, s_w);
    else k = mc_label<false>(g_parent, row_off, st, en, label, b.bh, nruns, c, s_w);
    if (tid == 0) ncomp[p] = k;
}

// Count and box of the bits this workgroup set, as mask_union_kernel reports them.  s: 5 ints.
__device__ __forceinline__ void mc_block_stats(int cnt, int bx0, int by0, int bx1, int by1, int* s, int* __restrict__ count, int* __restrict__ box) {
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
        count[0] = s[0];
        box[0] = any ? s[2] : 0;
        box[1] = any ? s[1] : 0;
        box[2] = any ? s[4] + 1 : 0;
        box[3] = any ? s[3] + 1 : 0;
    }
}

// One workgroup per piece: the plane piece_offsets places it in, component = its rank there + 1.  The whole output plane is
// written: zeros first, then one thread per row ORs that row's runs of the component into the words it alone owns.
__global__ __launch_bounds__(MC_THREADS) void mask_components_emit_kernel(const int32_t* __restrict__ box, int n, int H, int W, int wpr,
                                                                          const int* __restrict__ ws, long long ws_words,
                                                                          const int* __restrict__ ncomp, const int32_t* __restrict__ piece_offsets,
                                                                          int P, int first_only, unsigned* __restrict__ out,
                                                                          int* __restrict__ out_count, int* __restrict__ out_box) {
    __shared__ int s[5];
    __shared__ long long s_ll;
    const int piece = blockIdx.x, tid = threadIdx.x;
    int lo = 0, hi = n;                                              // the last plane with piece_offsets[p] <= piece
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (piece_offsets[mid] <= piece) lo = mid; else hi = mid;
    }
    const int p = lo, comp = piece - piece_offsets[p] + 1;
    const long long off = mc_offset_of(box, p, H, W, &s_ll);
    const mc_box b = mc_clip(box + 4 * p, H, W);
    const long long cap = mc_cap(b);
    const long long total = (long long)H * wpr;
    unsigned* o = out + (long long)piece * total;
    for (long long idx = tid; idx < total; idx += MC_THREADS) o[idx] = 0u;
    __syncthreads();
    int cnt = 0, bx0 = INT_MAX, by0 = INT_MAX, bx1 = -1, by1 = -1;
    const bool ok = comp >= 1 && piece < piece_offsets[p + 1] && cap <= MC_MAX_RUNS && off + mc_words(b) <= ws_words &&
                    comp <= ncomp[p] && (!first_only || comp == 1);
    if (ok) {
        const int* row_off = ws + off;
        const unsigned short* st = (const unsigned short*)(row_off + b.bh + 1);
        const unsigned short* en = st + cap;
        const int* label = row_off + b.bh + 1 + cap;
        for (int r = tid; r < b.bh; r += MC_THREADS) {
            unsigned* orow = o + (long long)(b.y1 + r) * wpr;
            const int j1 = min(row_off[r + 1], (int)cap);
            for (int j = max(row_off[r], 0); j < j1; ++j) {
                if (label[j] != comp) continue;
                const int sx = st[j], ex = min((int)en[j], W - 1);
                if (sx > ex) continue;
                for (int k = sx >> 5; k <= (ex >> 5); ++k) {
                    unsigned m = ~0u;
                    if (k == (sx >> 5)) m &= ~0u << (sx & 31);
                    if (k == (ex >> 5)) m &= ~0u >> (31 - (ex & 31));
                    orow[k] |= m;
                }
                cnt += ex - sx + 1;
                bx0 = min(bx0, sx); bx1 = max(bx1, ex);
                by0 = min(by0, b.y1 + r); by1 = max(by1, b.y1 + r);
            }
        }
    }
    mc_block_stats(cnt, bx0, by0, bx1, by1, s, out_count + piece, out_box + 4 * piece);
}

// One thread per row of every plane's box: the columns of its first and last set bit inside the box, (-1, -1) when there is none.
__global__ __launch_bounds__(MC_THREADS) void mask_row_extents_kernel(const unsigned* __restrict__ planes, const int32_t* __restrict__ box, int H,
                                                                      int W, int wpr, const int32_t* __restrict__ row_offsets, int R,
                                                                      int* __restrict__ extents) {
    const int p = blockIdx.x;
    const mc_box b = mc_clip(box + 4 * p, H, W);
    const int r0 = row_offsets[p];
    if (r0 < 0 || (long long)r0 + b.bh > R) return;                   // not the table the pool was sized for
    const unsigned* pl = planes + (long long)p * H * wpr;
    const int x1 = b.x1, x2 = b.x1 + b.bw;
    const int k0 = x1 >> 5, k1 = b.bw > 0 ? (x2 - 1) >> 5 : k0 - 1;
    for (int r = threadIdx.x; r < b.bh; r += MC_THREADS) {
        const unsigned* row = pl + (long long)(b.y1 + r) * wpr;
        int first = -1, last = -1;
        for (int k = k0; k <= k1; ++k) {
            const unsigned w = mc_word(row, k, x1, x2);
            if (w) {
                if (first < 0) first = 32 * k + __ffs((int)w) - 1;
                last = 32 * k + 31 - __clz((int)w);
            }
        }
        extents[2 * (long long)(r0 + r)] = first;
        extents[2 * (long long)(r0 + r) + 1] = last;
    }
}

// The status for a frame, a connectivity and a host box table; *words = workspace words of the table.
static int mc_table_status(int n, int H, int W, int connectivity, const int32_t* box_host, long long* words) {
    *words = 0;
    if (n <= 0 || H <= 0 || W <= 0 || (connectivity != 4 && connectivity != 8) || !box_host) return MRCNN_ERR_ARG;
    if (H > MC_MAX_SIDE || W > MC_MAX_SIDE || n > MC_MAX_PLANES) return MRCNN_ERR_UNSUPPORTED;
    long long sum = 0;
    for (int p = 0; p < n; ++p) {
        const mc_box b = mc_clip(box_host + 4 * p, H, W);
        if (mc_cap(b) > MC_MAX_RUNS) return MRCNN_ERR_UNSUPPORTED;
        sum += mc_words(b);
        if (sum > 0x7FFFFFFFll) return MRCNN_ERR_UNSUPPORTED;
    }
    *words = sum;
    return MRCNN_OK;
}

extern "C" int mrcnn_mask_components_check(int n, int H, int W, int connectivity, const int32_t* box_host, size_t ws_bytes) {
    long long words;
    const int rc = mc_table_status(n, H, W, connectivity, box_host, &words);
    if (rc) return rc;
    return ws_bytes / 4 >= (size_t)words ? MRCNN_OK : MRCNN_ERR_WORKSPACE;
}

extern "C" size_t mrcnn_mask_components_workspace(int n, int H, int W, const int32_t* box_host) {
    long long words;
    return mc_table_status(n, H, W, 4, box_host, &words) ? 0 : (size_t)words * 4;
}

extern "C" int mrcnn_mask_components_count(const void* planes, const int32_t* box_host, const int32_t* box, int n, int H, int W, int connectivity,
                                           void* ws, size_t ws_bytes, int32_t* ncomp, void* stream) {
    const int rc = mrcnn_mask_components_check(n, H, W, connectivity, box_host, ws_bytes);
    if (rc) return rc;
    if (!planes || !box || !ws || !ncomp) return MRCNN_ERR_ARG;
    hipLaunchKernelGGL(mask_components_count_kernel, dim3((unsigned)n), dim3(MC_THREADS), 0, (hipStream_t)stream, (const unsigned*)planes, box, n,
                       H, W, (W + 31) >> 5, connectivity == 8 ? 1 : 0, (int*)ws, (long long)(ws_bytes / 4), (int*)ncomp);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_mask_components_emit(const int32_t* box_host, const int32_t* box, int n, int H, int W, const void* ws, size_t ws_bytes,
                                          const int32_t* ncomp, const int32_t* piece_offsets_host, const int32_t* piece_offsets, int mode,
                                          void* out_planes, int32_t* out_count, int32_t* out_box, void* stream) {
    const int rc = mrcnn_mask_components_check(n, H, W, 4, box_host, ws_bytes);
    if (rc) return rc;
    if (!piece_offsets_host || (mode != MRCNN_COMPONENTS_ALL && mode != MRCNN_COMPONENTS_FIRST) || piece_offsets_host[0] != 0)
        return MRCNN_ERR_ARG;
    for (int p = 0; p < n; ++p) {
        const int64_t d = (int64_t)piece_offsets_host[p + 1] - piece_offsets_host[p];
        if (d < 0 || (mode == MRCNN_COMPONENTS_FIRST && d > 1)) return MRCNN_ERR_ARG;
    }
    const int P = piece_offsets_host[n];
    if (P > MC_MAX_PIECES) return MRCNN_ERR_UNSUPPORTED;
    if (P == 0) return MRCNN_OK;
    if (!box || !ws || !ncomp || !piece_offsets || !out_planes || !out_count || !out_box) return MRCNN_ERR_ARG;
    hipLaunchKernelGGL(mask_components_emit_kernel, dim3((unsigned)P), dim3(MC_THREADS), 0, (hipStream_t)stream, box, n, H, W, (W + 31) >> 5,
                       (const int*)ws, (long long)(ws_bytes / 4), (const int*)ncomp, piece_offsets, P, mode == MRCNN_COMPONENTS_FIRST ? 1 : 0,
                       (unsigned*)out_planes, (int*)out_count, (int*)out_box);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_mask_row_extents(const void* planes, const int32_t* box_host, const int32_t* box, int n, int H, int W,
                                      const int32_t* row_offsets, int R, int32_t* extents, void* stream) {
    if (n <= 0 || H <= 0 || W <= 0 || !box_host || R < 0) return MRCNN_ERR_ARG;
    if ((int64_t)H * ((W + 31) >> 5) > 0x7FFFFFFFll) return MRCNN_ERR_UNSUPPORTED;
    int64_t rows = 0;
    for (int p = 0; p < n; ++p) rows += mc_clip(box_host + 4 * p, H, W).bh;
    if (rows != R) return MRCNN_ERR_ARG;
    if (R == 0) return MRCNN_OK;
    if (!planes || !box || !row_offsets || !extents) return MRCNN_ERR_ARG;
    hipLaunchKernelGGL(mask_row_extents_kernel, dim3((unsigned)n), dim3(MC_THREADS), 0, (hipStream_t)stream, (const unsigned*)planes, box, H, W,
                       (W + 31) >> 5, row_offsets, R, (int*)extents);
    return mrcnn_launch_status();
}
