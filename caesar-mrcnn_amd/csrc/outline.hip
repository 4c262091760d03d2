// Contours and pixel lists of bit masks (Analyzer.make_json_results, mrcnn/analyze.py:1902-1927, and the merged sources of
// SFinder.merge_edge_sources, mrcnn/sfinder.py:887-909): what skimage.measure.find_contours(level = 0.5) gives for the
// zero-padded 0 / 1 mask -- restated here as in analyze.find_contours, parity with skimage itself stays UNPINNED -- and what
// np.argwhere gives, for all n sources of one call.  Sources are the bit masks of tile_source.h (one pool of 32-bit words, a
// mrcnn_tile_source each); every read goes through tm_word / tm_bits: padding bits, rows outside a source and addresses past
// the pool read as zero.  analyze.outline_statement is the NumPy statement of the rule:
//   * cell (r, c), 0 <= r <= h, 0 <= c <= w, has the corners mask[r - 1 .. r][c - 1 .. c]; its segments follow find_contours'
//     table (a saddle has two); segments are numbered in raster order of their cells;
//   * a crossing point lies on one grid edge between two cells: it ends one segment and starts one, succ(s) is the segment
//     of the neighbouring cell that starts on the edge where s ends; every contour is a cycle of succ;
//   * contours are ordered by the smallest segment of their cycle; with `last` the largest, the contour is
//     p(succ(last)), ..., p(last), q(last); every coordinate is a multiple of 0.5.
// An "entry" is 32 cells of one cell row: entry (r, j) of a source holds the cells 32 j .. 32 j + 31 of cell row r, and the
// pixel word j of pixel row r.  Kernels (workgroup barriers only; nothing depends on the order of atomics -- there are none):
//   ol_scan_kernel    one workgroup: exclusive scans over the n sources (entries, segments, pixels, contours);
//   ol_count_kernel   one workgroup per source: segments and pixels per entry, scanned in raster order;
//   ol_emit_kernel    one thread per entry: p and succ of its segments (succ from the neighbouring entry's scanned offset
//                     and the popcounts below the neighbouring cell), and the entry's pixels at their argwhere rank;
//   ol_rank_kernel    one workgroup per source: pointer doubling over succ, read one buffer / write the other, a barrier
//                     per round.  A window of 2^k successors carries its smallest index, its largest index and the distance
//                     to the first occurrence of the largest; windows that wrap round a cycle keep all three right, so
//                     ceil(log2 S) rounds give every segment its cycle's leader, its `last` and its distance to `last`.
//                     Two forms: the buffers in LDS (S <= outline_lds_segs, at most 1536) or in a global workspace;
//   ol_write_kernel   one thread per segment: its point at the contour's offset + its position, the closing point, the
//                     contour offsets.
#include "common.h"
#include "tile_source.h"

#define OL_MAX_DIM 8192                  // MRCNN_OUTLINE_MAX_DIM: coordinates are kept doubled in 16 bits
#define OL_MAX_SEGS (1 << 22)            // MRCNN_OUTLINE_MAX_SEGMENTS per source
#define OL_MAX_N 65535                   // sources per call (a grid dimension)
#define OL_LDS_SEGS 1536                 // 8 arrays of int: 48 KiB of LDS
#define OL_T 512                         // threads of the per-source workgroups

int g_mrcnn_outline_lds_segs = OL_LDS_SEGS;

enum { OL_TOP = 0, OL_LEFT = 1, OL_BOTTOM = 2, OL_RIGHT = 3 };

__host__ __device__ static inline int ol_nwc(int w) { return (w + 32) >> 5; }                  // words of cell columns 0 .. w
__host__ __device__ static inline long long ol_entries(int w, int h) { return (w <= 0 || h <= 0) ? 0ll : (long long)(h + 1) * ol_nwc(w); }

// start / end edge of the first segment of case k (find_contours' table), two bits per case
__device__ __forceinline__ int ol_p0(int k) {
    // 1 T, 2 R, 3 R, 4 L, 5 T, 6 R, 7 R, 8 B, 9 T, 10 B, 11 B, 12 L, 13 T, 14 L
    const unsigned long long t = 0ull | (0ull << 2) | (3ull << 4) | (3ull << 6) | (1ull << 8) | (0ull << 10) | (3ull << 12) | (3ull << 14) |
                                 (2ull << 16) | (0ull << 18) | (2ull << 20) | (2ull << 22) | (1ull << 24) | (0ull << 26) | (1ull << 28);
    return (int)((t >> (2 * k)) & 3ull);
}
__device__ __forceinline__ int ol_q0(int k) {
    // 1 L, 2 T, 3 L, 4 B, 5 B, 6 T, 7 B, 8 R, 9 L, 10 T, 11 L, 12 R, 13 R, 14 T
    const unsigned long long t = 0ull | (1ull << 2) | (0ull << 4) | (1ull << 6) | (2ull << 8) | (2ull << 10) | (0ull << 12) | (2ull << 14) |
                                 (3ull << 16) | (1ull << 18) | (0ull << 20) | (1ull << 22) | (3ull << 24) | (3ull << 26) | (0ull << 28);
    return (int)((t >> (2 * k)) & 3ull);
}

// The 32 cells of entry (r, j): corner bits, boundary cells (1 .. 14), saddles of case 6 and of case 9.  Anything outside the
// source reads as zero, so an entry outside the table is all background.
struct OlCells { unsigned ul, ur, ll, lr, bnd, s6, s9; };
__device__ __forceinline__ OlCells ol_cells(const unsigned* __restrict__ pool, long long pool_words, const TmSrc& d, int r, int j) {
    OlCells c;
    c.ul = tm_bits(pool, pool_words, d, r - 1, 32 * j - 1);
    c.ur = tm_bits(pool, pool_words, d, r - 1, 32 * j);
    c.ll = tm_bits(pool, pool_words, d, r, 32 * j - 1);
    c.lr = tm_bits(pool, pool_words, d, r, 32 * j);
    c.bnd = (c.ul | c.ur | c.ll | c.lr) & ~(c.ul & c.ur & c.ll & c.lr);
    c.s6 = c.ur & c.ll & ~c.ul & ~c.lr;
    c.s9 = c.ul & c.lr & ~c.ur & ~c.ll;
    return c;
}
// segments of the entry's cells below bit b
__device__ __forceinline__ int ol_rank(const OlCells& c, int b) {
    const unsigned low = (1u << b) - 1u;
    return __popc(c.bnd & low) + __popc((c.s6 | c.s9) & low);
}

// Exclusive scan of v over the OL_T threads of a workgroup (thread order); total = the sum.  Called by all threads.
__device__ __forceinline__ int ol_block_scan(int v, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                         // the previous call's readers are done with s_wave
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < OL_T / 64; ++k) {
        const int t = s_wave[k];
        if (k < wv) base += t;
        tot += t;
    }
    total = tot;
    return base + inc - v;
}

// out[0 .. n] = exclusive scan of: the sources' entry counts (desc given) or in[stride * i].
__global__ __launch_bounds__(OL_T) void ol_scan_kernel(const TmSrc* __restrict__ desc, const int* __restrict__ in, int stride, int n,
                                                       int* __restrict__ out) {
    __shared__ int s_wave[OL_T / 64];
    int carry = 0;
    for (int base = 0; base < n; base += OL_T) {             // uniform trip count
        const int i = base + threadIdx.x;
        int v = 0;
        if (i < n) v = desc ? (int)ol_entries(desc[i].w, desc[i].h) : max(in[(long long)stride * i], 0);
        int total;
        const int ex = ol_block_scan(v, s_wave, total);
        if (i < n) out[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) out[n] = carry;
}

__global__ __launch_bounds__(OL_T) void ol_count_kernel(const unsigned* __restrict__ pool, long long pool_words, const TmSrc* __restrict__ desc,
                                                        const int* __restrict__ ent_off, int* __restrict__ seg_off, int* __restrict__ pix_off,
                                                        int* __restrict__ totals) {
    __shared__ int s_wave[OL_T / 64];
    const int i = blockIdx.x;
    const TmSrc d = desc[i];
    const int e0 = ent_off[i], E = ent_off[i + 1] - e0, nwc = ol_nwc(d.w);
    int carry_s = 0, carry_k = 0;
    for (int base = 0; base < E; base += OL_T) {             // uniform trip count
        const int e = base + threadIdx.x;
        int sc = 0, pc = 0;
        if (e < E) {
            const int r = e / nwc, j = e - r * nwc;
            const OlCells c = ol_cells(pool, pool_words, d, r, j);
            sc = __popc(c.bnd) + __popc(c.s6 | c.s9);
            pc = __popc(tm_word(pool, pool_words, d, r, j));
        }
        int tot_s, tot_k;
        const int ex_s = ol_block_scan(sc, s_wave, tot_s);
        const int ex_k = ol_block_scan(pc, s_wave, tot_k);
        if (e < E) {
            seg_off[e0 + e] = carry_s + ex_s;
            pix_off[e0 + e] = carry_k + ex_k;
        }
        carry_s += tot_s;
        carry_k += tot_k;
    }
    if (threadIdx.x == 0) {
        totals[2 * i] = carry_s;
        totals[2 * i + 1] = carry_k;
    }
}

// The segment range of source i inside the arrays of s_cap segments the caller sized from the totals it read: [g0, g0 + S).
__device__ __forceinline__ int ol_seg_range(const int* __restrict__ seg_base, int i, int s_cap, int& g0) {
    g0 = seg_base[i];
    const int S = seg_base[i + 1] - g0;
    return (g0 < 0 || S < 0 || (long long)g0 + S > s_cap) ? 0 : S;
}

__global__ __launch_bounds__(256) void ol_emit_kernel(const unsigned* __restrict__ pool, long long pool_words, const TmSrc* __restrict__ desc,
                                                      const int* __restrict__ ent_off, const int* __restrict__ seg_off,
                                                      const int* __restrict__ pix_off, const int* __restrict__ seg_base, int s_cap,
                                                      const int* __restrict__ pix_base, unsigned* __restrict__ pq, int* __restrict__ succ,
                                                      int* __restrict__ pixels, int pixels_cap) {
    const int i = blockIdx.y;
    const int e0 = ent_off[i], E = ent_off[i + 1] - e0;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const TmSrc d = desc[i];
    const int nwc = ol_nwc(d.w);
    const int r = e / nwc, j = e - r * nwc;
    // pixels (y, x) of pixel word j of row r, at their rank in raster order
    unsigned word = tm_word(pool, pool_words, d, r, j);
    if (word) {
        const int k1 = min(pix_base[i + 1], pixels_cap);
        int o = pix_base[i] + pix_off[e0 + e];
        while (word) {
            const int b = __ffs((int)word) - 1;
            word &= word - 1u;
            if (o >= 0 && o < k1) {
                pixels[2ll * o] = r;
                pixels[2ll * o + 1] = 32 * j + b;
            }
            ++o;
        }
    }
    const OlCells cur = ol_cells(pool, pool_words, d, r, j);
    if (!cur.bnd) return;
    int g0;
    const int S = ol_seg_range(seg_base, i, s_cap, g0);
    const OlCells up = ol_cells(pool, pool_words, d, r - 1, j), dn = ol_cells(pool, pool_words, d, r + 1, j);
    const int sbase = seg_off[e0 + e];
    unsigned todo = cur.bnd;
    while (todo) {
        const int b = __ffs((int)todo) - 1;
        todo &= todo - 1u;
        const int k = (int)((cur.ul >> b) & 1u) | (int)((cur.ur >> b) & 1u) << 1 | (int)((cur.ll >> b) & 1u) << 2 | (int)((cur.lr >> b) & 1u) << 3;
        const int nseg = (k == 6 || k == 9) ? 2 : 1;
        const int s0 = sbase + ol_rank(cur, b);
        const int c = 32 * j + b;
        for (int t = 0; t < nseg; ++t) {
            const int s = s0 + t;
            if (s < 0 || s >= S) continue;
            const int pe = t ? (k == 6 ? OL_LEFT : OL_BOTTOM) : ol_p0(k);
            const int qe = t ? (k == 6 ? OL_BOTTOM : OL_RIGHT) : ol_q0(k);
            // p, doubled and shifted by one: top (2c - 1, 2r - 2), left (2c - 2, 2r - 1), bottom (2c - 1, 2r), right (2c, 2r - 1)
            const int px = 2 * c + (pe == OL_LEFT ? -2 : pe == OL_RIGHT ? 0 : -1) + 1;
            const int py = 2 * r + (pe == OL_TOP ? -2 : pe == OL_BOTTOM ? 0 : -1) + 1;
            pq[g0 + s] = ((unsigned)py << 16) | ((unsigned)px & 0xFFFFu);
            // succ: the segment of the cell across edge qe that starts on that edge
            int eb = e, bb = b, extra = 0;
            OlCells nb = cur;
            if (qe == OL_TOP) {
                nb = up; eb = e - nwc;
                extra = (int)((nb.s9 >> bb) & 1u);             // case 9: (top, left), (bottom, right)
            } else if (qe == OL_BOTTOM) {
                nb = dn; eb = e + nwc;
            } else if (qe == OL_LEFT) {
                if (b > 0) bb = b - 1;
                else { nb = ol_cells(pool, pool_words, d, r, j - 1); eb = e - 1; bb = 31; }
            } else {
                if (b < 31) bb = b + 1;
                else { nb = ol_cells(pool, pool_words, d, r, j + 1); eb = e + 1; bb = 0; }
                extra = (int)((nb.s6 >> bb) & 1u);             // case 6: (right, top), (left, bottom)
            }
            if (eb < 0 || eb >= E) eb = e;                      // never for a consistent table
            succ[g0 + s] = seg_off[e0 + eb] + ol_rank(nb, bb) + extra;
        }
    }
}

// dst[s]: the point index of p(s) among the source's points; aux_a[s]: the contour's ordinal for a leader, -2 for a cycle's
// `last`, else -1; aux_b[s]: for a leader, the contour's first point index.  ncont[i]: contours of the source.
template <bool LDS>
__global__ __launch_bounds__(OL_T) void ol_rank_kernel(const int* __restrict__ seg_base, int s_cap, int lds_segs, const int* __restrict__ succ,
                                                       int* rank_ws, int* __restrict__ dst, int* __restrict__ aux_a, int* __restrict__ aux_b,
                                                       int* __restrict__ ncont) {
    __shared__ int s_wave[OL_T / 64];
    const int i = blockIdx.x, tid = threadIdx.x;
    int g0;
    const int S = ol_seg_range(seg_base, i, s_cap, g0);
    if ((S <= lds_segs) != LDS) return;                          // the other form's launch takes this source
    if (S <= 0) {
        if (tid == 0) ncont[i] = 0;
        return;
    }
    int *nx[2], *mn[2], *mx[2], *ds[2];
    if constexpr (LDS) {
        __shared__ int s_buf[8][OL_LDS_SEGS];
        for (int k = 0; k < 2; ++k) { nx[k] = s_buf[k]; mn[k] = s_buf[2 + k]; mx[k] = s_buf[4 + k]; ds[k] = s_buf[6 + k]; }
    } else {
        int* base = rank_ws + 8ll * g0;
        for (int k = 0; k < 2; ++k) { nx[k] = base + (long long)k * S; mn[k] = base + (2ll + k) * S; mx[k] = base + (4ll + k) * S; ds[k] = base + (6ll + k) * S; }
    }
    const int* succ0 = succ + g0;
    for (int s = tid; s < S; s += OL_T) {
        nx[0][s] = min(max(succ0[s], 0), S - 1);
        mn[0][s] = s; mx[0][s] = s; ds[0][s] = 0;
    }
    __syncthreads();
    int cur = 0;
    for (int len = 1; len < S; len <<= 1) {                      // windows of len successors -> 2 len
        const int o = cur ^ 1;
        for (int s = tid; s < S; s += OL_T) {
            const int t = nx[cur][s];
            mn[o][s] = min(mn[cur][s], mn[cur][t]);
            const int m1 = mx[cur][s], m2 = mx[cur][t];
            if (m2 > m1) { mx[o][s] = m2; ds[o][s] = len + ds[cur][t]; }
            else { mx[o][s] = m1; ds[o][s] = ds[cur][s]; }
            nx[o][s] = nx[cur][t];
        }
        __syncthreads();
        cur = o;
    }
    // leaders in index order: ordinal, first point and length of their contour (into the free buffers)
    const int o = cur ^ 1;
    int carry_c = 0, carry_p = 0;
    for (int base = 0; base < S; base += OL_T) {                 // uniform trip count
        const int s = base + tid;
        const bool lead = s < S && mn[cur][s] == s;
        int L = 0;
        if (lead) L = ds[cur][min(max(succ0[mx[cur][s]], 0), S - 1)] + 1;
        int tot_c, tot_p;
        const int ex_c = ol_block_scan(lead ? 1 : 0, s_wave, tot_c);
        const int ex_p = ol_block_scan(lead ? L + 1 : 0, s_wave, tot_p);
        if (lead) { mn[o][s] = carry_c + ex_c; mx[o][s] = carry_p + ex_p; ds[o][s] = L; }
        carry_c += tot_c;
        carry_p += tot_p;
    }
    __syncthreads();
    for (int s = tid; s < S; s += OL_T) {
        const int ld = mn[cur][s];
        const int po = mx[o][ld], L = ds[o][ld];
        dst[g0 + s] = po + L - 1 - ds[cur][s];
        aux_a[g0 + s] = s == ld ? mn[o][s] : (s == mx[cur][s] ? -2 : -1);
        aux_b[g0 + s] = po;
    }
    if (tid == 0) ncont[i] = carry_c;
}

__global__ __launch_bounds__(256) void ol_write_kernel(const int* __restrict__ seg_base, int s_cap, const int* __restrict__ cbase,
                                                       const unsigned* __restrict__ pq, const int* __restrict__ succ,
                                                       const int* __restrict__ dst, const int* __restrict__ aux_a,
                                                       const int* __restrict__ aux_b, int n, float* __restrict__ points, int points_cap,
                                                       int* __restrict__ contour_offsets, int contours_cap) {
    const int i = blockIdx.y;
    if (i == 0 && blockIdx.x == 0 && threadIdx.x == 0) {        // the end of the last contour
        const int C = cbase[n];
        if (C >= 0 && C <= contours_cap) contour_offsets[C] = seg_base[n] + C;
    }
    int g0;
    const int S = ol_seg_range(seg_base, i, s_cap, g0);
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const int cb = cbase[i], Ci = cbase[i + 1] - cb;
    if (cb < 0 || Ci < 0) return;
    const int pb = g0 + cb;                                      // points of the sources before this one
    const int d = dst[g0 + s], a = aux_a[g0 + s];
    const int np = S + Ci;
    const unsigned v = pq[g0 + s];
    if (d >= 0 && d < np && pb + d < points_cap) {
        points[2ll * (pb + d)] = 0.5f * (float)((int)(v & 0xFFFFu) - 1);
        points[2ll * (pb + d) + 1] = 0.5f * (float)((int)(v >> 16) - 1);
    }
    if (a >= 0) {
        if (a < Ci && cb + a < contours_cap) contour_offsets[cb + a] = pb + aux_b[g0 + s];
    } else if (a == -2 && d + 1 >= 0 && d + 1 < np && pb + d + 1 < points_cap) {
        const unsigned u = pq[g0 + min(max(succ[g0 + s], 0), S - 1)];         // q(last) = p(succ(last))
        points[2ll * (pb + d + 1)] = 0.5f * (float)((int)(u & 0xFFFFu) - 1);
        points[2ll * (pb + d + 1) + 1] = 0.5f * (float)((int)(u >> 16) - 1);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct OlPlan {
    long long E, S, K;      // entries, segments, pixels of the call
    int max_E, max_S;       // of one source
    bool global_form;       // some source ranks in the global workspace
};

// The status of a call for this table (and these totals, when given), and its sizes.
static int ol_plan(const mrcnn_tile_source* dh, int n, int64_t pool_words, const int32_t* totals, OlPlan* plan) {
    if (n <= 0 || !dh || pool_words < 0) return MRCNN_ERR_ARG;
    OlPlan p = {0, 0, 0, 0, 0, false};
    bool past = n > OL_MAX_N || pool_words > 0x7FFFFFFFll;
    for (int i = 0; i < n; ++i) {
        const mrcnn_tile_source& d = dh[i];
        if (totals && (totals[2 * i] < 0 || totals[2 * i + 1] < 0)) return MRCNN_ERR_ARG;
        if (d.w <= 0 || d.h <= 0) {
            if (totals && (totals[2 * i] || totals[2 * i + 1])) return MRCNN_ERR_ARG;
            continue;
        }
        if (d.word_offset < 0 || (long long)d.words_per_row < ((long long)d.w + 31) / 32 ||
            (long long)d.word_offset + (long long)d.h * d.words_per_row > pool_words)
            return MRCNN_ERR_ARG;
        if (d.w > OL_MAX_DIM || d.h > OL_MAX_DIM) {
            past = true;
            continue;
        }
        const long long e = ol_entries(d.w, d.h);
        p.E += e;
        if (e > p.max_E) p.max_E = (int)e;
        if (totals) {
            const int s = totals[2 * i];
            if (s > OL_MAX_SEGS) past = true;
            p.S += s;
            p.K += totals[2 * i + 1];
            if (s > p.max_S) p.max_S = s;
            if (s > g_mrcnn_outline_lds_segs) p.global_form = true;
        }
    }
    if (past || p.E > 0x7FFFFFFFll || p.S + p.S / 4 > 0x7FFFFFFFll || p.K > 0x7FFFFFFFll) return MRCNN_ERR_UNSUPPORTED;
    if (plan) *plan = p;
    return MRCNN_OK;
}

static inline size_t ol_align(size_t v) { return (v + 63) & ~(size_t)63; }
// count workspace: ent_off [n + 1], seg_base [n + 1], seg_off [E], pix_off [E]
static size_t ol_count_bytes(const OlPlan& p, int n) { return 2 * ol_align(4 * ((size_t)n + 1)) + 2 * ol_align(4 * (size_t)p.E); }
// emit workspace: ncont [n], pq, succ, dst, aux_a, aux_b [S], and 8 S for the global form of the ranking
static size_t ol_emit_bytes(const OlPlan& p, int n) {
    return ol_align(4 * (size_t)n) + 5 * ol_align(4 * (size_t)p.S) + (p.global_form ? ol_align(32 * (size_t)p.S) : 0);
}

extern "C" int mrcnn_outline_check(const mrcnn_tile_source* desc_host, int n, int64_t pool_words, const int32_t* totals_host) {
    return ol_plan(desc_host, n, pool_words, totals_host, nullptr);
}

extern "C" size_t mrcnn_outline_workspace(const mrcnn_tile_source* desc_host, int n, int64_t pool_words, const int32_t* totals_host) {
    OlPlan p;
    if (ol_plan(desc_host, n, pool_words, totals_host, &p) != MRCNN_OK) return 0;
    return (totals_host ? ol_emit_bytes(p, n) : ol_count_bytes(p, n)) + 64;
}

struct OlCountWs { int *ent_off, *seg_base, *seg_off, *pix_off; };
static OlCountWs ol_count_ws(void* ws, const OlPlan& p, int n) {
    char* b = (char*)ws;
    OlCountWs w;
    w.ent_off = (int*)b; b += ol_align(4 * ((size_t)n + 1));
    w.seg_base = (int*)b; b += ol_align(4 * ((size_t)n + 1));
    w.seg_off = (int*)b; b += ol_align(4 * (size_t)p.E);
    w.pix_off = (int*)b;
    return w;
}

extern "C" int mrcnn_outline_count(const void* pool, int64_t pool_words, const mrcnn_tile_source* desc_host, const mrcnn_tile_source* desc,
                                   int n, void* count_ws, size_t count_ws_bytes, int32_t* totals, int32_t* pixel_offsets, void* stream) {
    OlPlan p;
    const int rc = ol_plan(desc_host, n, pool_words, nullptr, &p);
    if (rc != MRCNN_OK) return rc;
    if (!pool || !desc || !count_ws || !totals || !pixel_offsets) return MRCNN_ERR_ARG;
    if (count_ws_bytes < ol_count_bytes(p, n)) return MRCNN_ERR_WORKSPACE;
    const OlCountWs w = ol_count_ws(count_ws, p, n);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ol_scan_kernel, dim3(1), dim3(OL_T), 0, st, desc, (const int*)nullptr, 0, n, w.ent_off);
    hipLaunchKernelGGL(ol_count_kernel, dim3((unsigned)n), dim3(OL_T), 0, st, (const unsigned*)pool, (long long)pool_words, desc,
                       (const int*)w.ent_off, w.seg_off, w.pix_off, (int*)totals);
    hipLaunchKernelGGL(ol_scan_kernel, dim3(1), dim3(OL_T), 0, st, (const TmSrc*)nullptr, (const int*)totals, 2, n, w.seg_base);
    hipLaunchKernelGGL(ol_scan_kernel, dim3(1), dim3(OL_T), 0, st, (const TmSrc*)nullptr, (const int*)totals + 1, 2, n, (int*)pixel_offsets);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_outline_emit(const void* pool, int64_t pool_words, const mrcnn_tile_source* desc_host, const mrcnn_tile_source* desc,
                                  int n, const int32_t* totals_host, const void* count_ws, size_t count_ws_bytes, void* emit_ws,
                                  size_t emit_ws_bytes, const int32_t* pixel_offsets, float* points, int64_t points_cap,
                                  int32_t* contour_offsets, int64_t contours_cap, int32_t* source_contours, int32_t* pixels,
                                  int64_t pixels_cap, void* stream) {
    OlPlan p;
    const int rc = ol_plan(desc_host, n, pool_words, totals_host, &p);
    if (rc != MRCNN_OK) return rc;
    if (!totals_host || points_cap < 0 || contours_cap < 0 || pixels_cap < 0) return MRCNN_ERR_ARG;
    if (!pool || !desc || !count_ws || !emit_ws || !pixel_offsets || !points || !contour_offsets || !source_contours || !pixels)
        return MRCNN_ERR_ARG;
    if (points_cap < p.S + p.S / 4 || contours_cap < p.S / 4 || pixels_cap < p.K) return MRCNN_ERR_ARG;
    if (count_ws_bytes < ol_count_bytes(p, n) || emit_ws_bytes < ol_emit_bytes(p, n)) return MRCNN_ERR_WORKSPACE;
    const OlCountWs w = ol_count_ws((void*)count_ws, p, n);
    char* b = (char*)emit_ws;
    int* ncont = (int*)b; b += ol_align(4 * (size_t)n);
    const size_t seg_bytes = ol_align(4 * (size_t)p.S);
    unsigned* pq = (unsigned*)b; b += seg_bytes;
    int* succ = (int*)b; b += seg_bytes;
    int* dst = (int*)b; b += seg_bytes;
    int* aux_a = (int*)b; b += seg_bytes;
    int* aux_b = (int*)b; b += seg_bytes;
    int* rank_ws = (int*)b;
    const int s_cap = (int)p.S, lds_segs = g_mrcnn_outline_lds_segs;
    const int cap_p = (int)(points_cap > 0x7FFFFFFFll ? 0x7FFFFFFFll : points_cap);
    const int cap_c = (int)(contours_cap > 0x7FFFFFFFll ? 0x7FFFFFFFll : contours_cap);
    const int cap_k = (int)(pixels_cap > 0x7FFFFFFFll ? 0x7FFFFFFFll : pixels_cap);
    hipStream_t st = (hipStream_t)stream;
    if (p.max_E > 0)
        hipLaunchKernelGGL(ol_emit_kernel, dim3((unsigned)cdiv64(p.max_E, 256), (unsigned)n), dim3(256), 0, st, (const unsigned*)pool,
                           (long long)pool_words, desc, (const int*)w.ent_off, (const int*)w.seg_off, (const int*)w.pix_off,
                           (const int*)w.seg_base, s_cap, (const int*)pixel_offsets, pq, succ, (int*)pixels, cap_k);
    // the LDS form always runs: it also owns the sources without segments (ncont = 0)
    hipLaunchKernelGGL(ol_rank_kernel<true>, dim3((unsigned)n), dim3(OL_T), 0, st, (const int*)w.seg_base, s_cap, lds_segs,
                           (const int*)succ, (int*)nullptr, dst, aux_a, aux_b, ncont);
    if (p.global_form)
        hipLaunchKernelGGL(ol_rank_kernel<false>, dim3((unsigned)n), dim3(OL_T), 0, st, (const int*)w.seg_base, s_cap, lds_segs,
                           (const int*)succ, rank_ws, dst, aux_a, aux_b, ncont);
    hipLaunchKernelGGL(ol_scan_kernel, dim3(1), dim3(OL_T), 0, st, (const TmSrc*)nullptr, (const int*)ncont, 1, n, (int*)source_contours);
    hipLaunchKernelGGL(ol_write_kernel, dim3((unsigned)cdiv64(p.max_S > 0 ? p.max_S : 1, 256), (unsigned)n), dim3(256), 0, st,
                       (const int*)w.seg_base, s_cap, (const int*)source_contours, (const unsigned*)pq, (const int*)succ, (const int*)dst,
                       (const int*)aux_a, (const int*)aux_b, n, points, cap_p, (int*)contour_offsets, cap_c);
    return mrcnn_launch_status();
}
