// Source parameters of a tiled run (SFinder.compute_source_params, mrcnn/sfinder.py:994-1211) for all sources of a mosaic in
// one launch: the masked reductions behind nPix, S, Smin, Smax, the mask and flux-weighted moments and the sigma-clipped
// mean / median / std.  The image plane is uploaded once ([H, W] float32, native or the file's big-endian bytes); a source is
// the bit mask of include/mrcnn_hip.h (mrcnn_tile_source) plus its cut-out rectangle.  One workgroup per source:
//   phase A  nanmin of the cut-out (clipped to the image): the value NaN pixels are replaced by (utils.py:1090-1091);
//   phase B  one pass over the mask words (a lane takes one word, its set bits index the image): counts, min, max, the
//            float64 sums, and the filled values gathered, in raster order, into the source's slice of the workspace;
//   phase C  the clipping loop on that slice.  After every iteration the kept set is a value interval [lo, hi], so nothing is
//            compacted: every pass re-reads the slice under the predicate "finite and lo <= x <= hi".  The median is exact:
//            a radix select over order-preserving 32-bit keys (4 passes of 8 bits, LDS histogram, parallel scan of the
//            256 bins) and, for an even count, one more pass for the next larger kept value; mean and sum of squared
//            deviations are two passes in float64.
// Every reduction has a fixed order (per-thread strided partials, xor butterfly within a wave, the four wave totals added in
// wave order), LDS atomics are integer only: results are bitwise reproducible.  Image reads are clipped to [0, H) x [0, W),
// mask reads go through tm_word, slice accesses are bounded by the slice; every loop bound is known at launch.
#include "common.h"
#include "tile_source.h"
#include <math.h>

#define SP_THREADS 256
#define SP_WAVES (SP_THREADS / 64)

struct SpShared {
    int hist[256];
    double red_d[4][SP_WAVES];
    long long red_l[3][SP_WAVES];
    float red_f[2][SP_WAVES];
    int red_i[2][SP_WAVES];
    unsigned sel_prefix;
    int sel_rank;
    int cnt_le;
    unsigned min_gt;
};

__device__ __forceinline__ double sp_shfl_xor_d(double v, int o) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(u & 0xFFFFFFFFull), o, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(u >> 32), o, 64);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ long long sp_shfl_xor_l(long long v, int o) {
    const unsigned long long u = (unsigned long long)v;
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(u & 0xFFFFFFFFull), o, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(u >> 32), o, 64);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// Workgroup sum of one double per thread, same value (bitwise) in every thread.  Two barriers: `slot` may be reused at once.
__device__ __forceinline__ double sp_block_sum(double v, double* slot) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += sp_shfl_xor_d(v, o);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = slot[0];
#pragma unroll
    for (int w = 1; w < SP_WAVES; ++w) r += slot[w];
    __syncthreads();
    return r;
}
__device__ __forceinline__ int sp_block_sum_i(int v, int* slot) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = slot[0];
#pragma unroll
    for (int w = 1; w < SP_WAVES; ++w) r += slot[w];
    __syncthreads();
    return r;
}
// Inclusive prefix sum over the workgroup's threads (thread order); *total = the sum.
__device__ __forceinline__ int sp_block_scan(int v, int* slot, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(s, o, 64);
        if (lane >= o) s += t;
    }
    if (lane == 63) slot[wave] = s;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SP_WAVES; ++w) {
        const int t = slot[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();
    *total = all;
    return s + before;
}

__device__ __forceinline__ float sp_pixel(const unsigned* __restrict__ img, int big_endian, long long idx) {
    unsigned u = img[idx];
    if (big_endian) u = __builtin_bswap32(u);
    return __uint_as_float(u);
}
// Order-preserving key of a float: a < b (as floats, -0 < +0) <=> key(a) < key(b).
__device__ __forceinline__ unsigned sp_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sp_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ bool sp_kept(float x, double lo, double hi) {
    const double d = (double)x;
    return isfinite(x) && d >= lo && d <= hi;
}

// Key of rank `rank` (0-based, ascending) among the kept values of vals[0, n).  rank < kept count.
__device__ unsigned sp_select(const float* vals, long long n, double lo, double hi, int rank, SpShared& sh) {
    unsigned prefix = 0u, pmask = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        sh.hist[threadIdx.x] = 0;                                      // SP_THREADS == 256 bins
        __syncthreads();
        for (long long i = threadIdx.x; i < n; i += SP_THREADS) {
            const float x = vals[i];
            if (sp_kept(x, lo, hi)) {
                const unsigned k = sp_key(x);
                if ((k & pmask) == prefix) atomicAdd(&sh.hist[(k >> shift) & 255u], 1);
            }
        }
        __syncthreads();
        const int mine = sh.hist[threadIdx.x];
        int total;
        const int incl = sp_block_scan(mine, sh.red_i[0], &total);
        if (rank >= incl - mine && rank < incl) {                      // exactly one thread (rank < total)
            sh.sel_prefix = prefix | ((unsigned)threadIdx.x << shift);
            sh.sel_rank = rank - (incl - mine);
        }
        __syncthreads();
        prefix = sh.sel_prefix;
        rank = sh.sel_rank;
        pmask |= 255u << shift;
        __syncthreads();
    }
    return prefix;
}

// Median of the `kept` (> 0) kept values, as NumPy takes it: the middle value, or the mean of the two middle values.
__device__ double sp_median(const float* vals, long long n, double lo, double hi, int kept, SpShared& sh) {
    const unsigned klo = sp_select(vals, n, lo, hi, (kept - 1) >> 1, sh);
    const float a = sp_unkey(klo);
    if (kept & 1) return (double)a;
    // even: the value of rank kept / 2 is `a` again if enough kept values are <= a, else the smallest kept value above it
    if (threadIdx.x == 0) { sh.cnt_le = 0; sh.min_gt = 0xFFFFFFFFu; }
    __syncthreads();
    int le = 0;
    unsigned mg = 0xFFFFFFFFu;
    for (long long i = threadIdx.x; i < n; i += SP_THREADS) {
        const float x = vals[i];
        if (sp_kept(x, lo, hi)) {
            const unsigned k = sp_key(x);
            if (k <= klo) ++le; else mg = min(mg, k);
        }
    }
    if (le) atomicAdd(&sh.cnt_le, le);
    if (mg != 0xFFFFFFFFu) atomicMin(&sh.min_gt, mg);
    __syncthreads();
    const float b = sh.cnt_le > (kept >> 1) ? a : sp_unkey(sh.min_gt);
    __syncthreads();
    return ((double)a + (double)b) / 2.0;
}

__global__ __launch_bounds__(SP_THREADS) void source_params_kernel(const unsigned* __restrict__ img, int big_endian, int H, int W,
                                                                   const unsigned* __restrict__ pool, long long pool_words,
                                                                   const TmSrc* __restrict__ desc, int n,
                                                                   const int* __restrict__ cutouts, const long long* __restrict__ val_offsets,
                                                                   float* values, long long values_len, double sigma,
                                                                   int maxiters, mrcnn_source_record* __restrict__ out) {
    __shared__ SpShared sh;
    const int s = blockIdx.x, tid = threadIdx.x;
    if (s >= n) return;
    const TmSrc d = desc[s];
    const int cx0 = cutouts[4 * s], cy0 = cutouts[4 * s + 1], cx1 = cutouts[4 * s + 2], cy1 = cutouts[4 * s + 3];
    // the cut-out inside the image (NumPy's slice clipping); empty when it lies outside
    const int rx0 = max(cx0, 0), ry0 = max(cy0, 0), rx1 = min(cx1, W), ry1 = min(cy1, H);
    const int rw = max(rx1 - rx0, 0), rh = max(ry1 - ry0, 0);

    // ---- phase A: nanmin of the cut-out -------------------------------------------------------------------------
    float mn = INFINITY;
    int seen = 0;
    {
        const long long total = (long long)rw * rh;
        for (long long i = tid; i < total; i += SP_THREADS) {
            const int r = (int)(i / rw), c = (int)(i - (long long)r * rw);
            const float v = sp_pixel(img, big_endian, (long long)(ry0 + r) * W + (rx0 + c));
            if (v == v) { mn = fminf(mn, v); seen = 1; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, o, 64));
            seen |= __shfl_xor(seen, o, 64);
        }
        if ((tid & 63) == 0) { sh.red_f[0][tid >> 6] = mn; sh.red_i[0][tid >> 6] = seen; }
        __syncthreads();
        mn = sh.red_f[0][0];
        seen = sh.red_i[0][0];
#pragma unroll
        for (int w = 1; w < SP_WAVES; ++w) { mn = fminf(mn, sh.red_f[0][w]); seen |= sh.red_i[0][w]; }
        __syncthreads();
    }
    const float fill = seen ? mn : __uint_as_float(0x7FC00000u);        // all NaN (or empty): np.nanmin gives NaN

    // ---- phase B: the masked pass ---------------------------------------------------------------------------------
    long long voff = val_offsets[s], vcap = val_offsets[s + 1] - voff;
    if (voff < 0 || vcap < 0 || voff + vcap > values_len) { voff = 0; vcap = 0; }
    float* vals = values + voff;                                         // (written and re-read by this workgroup: no restrict)
    int npix = 0;
    float smin = INFINITY, smax = -INFINITY;
    double s64 = 0.0, w00 = 0.0, w10 = 0.0, w01 = 0.0;
    long long m00 = 0, m10 = 0, m01 = 0;
    long long n_mask = 0;                                                // uniform: pixels gathered so far
    if (tm_valid(d) && rw > 0 && rh > 0) {
        const long long words = (long long)d.h * d.words_per_row;
        for (long long base = 0; base < words; base += SP_THREADS) {    // uniform trip count
            const long long idx = base + tid;
            unsigned wv = 0u;
            int y = 0, xb = 0;
            if (idx < words) {
                const int r = (int)(idx / d.words_per_row), k = (int)(idx - (long long)r * d.words_per_row);
                y = d.y0 + r;
                xb = d.x0 + 32 * k;
                if (y >= ry0 && y < ry1) {
                    wv = tm_word(pool, pool_words, d, r, k);
                    // bits whose pixel lies inside the clipped cut-out: rx0 <= xb + b < rx1
                    const long long b0 = (long long)rx0 - xb, b1 = (long long)rx1 - xb;
                    if (b1 <= 0 || b0 >= 32) wv = 0u;
                    else {
                        if (b0 > 0) wv &= 0xFFFFFFFFu << (int)b0;
                        if (b1 < 32) wv &= 0xFFFFFFFFu >> (32 - (int)b1);
                    }
                }
            }
            const int cnt = __popc(wv);
            int total;
            long long pos = n_mask + sp_block_scan(cnt, sh.red_i[0], &total) - cnt;
            while (wv) {
                const int b = __ffs((int)wv) - 1;
                wv &= wv - 1u;
                const int x = xb + b;
                float v = sp_pixel(img, big_endian, (long long)y * W + x);
                if (v != v) v = fill;
                if (pos < vcap) vals[pos] = v;
                ++pos;
                const double dv = (double)v;
                const int lx = x - cx0, ly = y - cy0;
                if (v == v) { ++npix; smin = fminf(smin, v); smax = fmaxf(smax, v); s64 += dv; }
                m00 += 1; m10 += lx; m01 += ly;
                w00 += dv; w10 += (double)lx * dv; w01 += (double)ly * dv;
            }
            n_mask += total;
        }
    }
    // workgroup totals, fixed order
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            npix += __shfl_xor(npix, o, 64);
            smin = fminf(smin, __shfl_xor(smin, o, 64));
            smax = fmaxf(smax, __shfl_xor(smax, o, 64));
            s64 += sp_shfl_xor_d(s64, o); w00 += sp_shfl_xor_d(w00, o); w10 += sp_shfl_xor_d(w10, o); w01 += sp_shfl_xor_d(w01, o);
            m00 += sp_shfl_xor_l(m00, o); m10 += sp_shfl_xor_l(m10, o); m01 += sp_shfl_xor_l(m01, o);
        }
        const int wave = tid >> 6;
        if ((tid & 63) == 0) {
            sh.red_i[1][wave] = npix; sh.red_f[0][wave] = smin; sh.red_f[1][wave] = smax;
            sh.red_d[0][wave] = s64; sh.red_d[1][wave] = w00; sh.red_d[2][wave] = w10; sh.red_d[3][wave] = w01;
            sh.red_l[0][wave] = m00; sh.red_l[1][wave] = m10; sh.red_l[2][wave] = m01;
        }
        __syncthreads();                                                 // (also: the gathered values are visible to the workgroup)
        npix = sh.red_i[1][0]; smin = sh.red_f[0][0]; smax = sh.red_f[1][0];
        s64 = sh.red_d[0][0]; w00 = sh.red_d[1][0]; w10 = sh.red_d[2][0]; w01 = sh.red_d[3][0];
        m00 = sh.red_l[0][0]; m10 = sh.red_l[1][0]; m01 = sh.red_l[2][0];
#pragma unroll
        for (int w = 1; w < SP_WAVES; ++w) {
            npix += sh.red_i[1][w]; smin = fminf(smin, sh.red_f[0][w]); smax = fmaxf(smax, sh.red_f[1][w]);
            s64 += sh.red_d[0][w]; w00 += sh.red_d[1][w]; w10 += sh.red_d[2][w]; w01 += sh.red_d[3][w];
            m00 += sh.red_l[0][w]; m10 += sh.red_l[1][w]; m01 += sh.red_l[2][w];
        }
        __syncthreads();
    }

    // ---- phase C: sigma clipping on the gathered values ---------------------------------------------------------
    const long long nv = n_mask < vcap ? n_mask : vcap;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    double lo = -INFINITY, hi = INFINITY;
    int kept;
    {
        int c = 0;
        for (long long i = tid; i < nv; i += SP_THREADS) c += isfinite(vals[i]) ? 1 : 0;
        kept = sp_block_sum_i(c, sh.red_i[0]);
    }
    double mean = qnan, median = qnan, sd = qnan;
    int iters = 0;
    bool fresh = false;                                                  // mean / median / sd describe the current kept set
    while (iters < maxiters && kept > 0) {                               // uniform
        median = sp_median(vals, nv, lo, hi, kept, sh);
        double a = 0.0;
        for (long long i = tid; i < nv; i += SP_THREADS) { const float x = vals[i]; if (sp_kept(x, lo, hi)) a += (double)x; }
        mean = sp_block_sum(a, sh.red_d[0]) / (double)kept;
        a = 0.0;
        for (long long i = tid; i < nv; i += SP_THREADS) {
            const float x = vals[i];
            if (sp_kept(x, lo, hi)) { const double t = (double)x - mean; a += t * t; }
        }
        sd = sqrt(sp_block_sum(a, sh.red_d[0]) / (double)kept);
        // (product, then sum, as the host statement: the library is built with -ffp-contract=off, nothing is fused)
        const double nlo = median - sigma * sd, nhi = median + sigma * sd;
        lo = nlo > lo ? nlo : lo;
        hi = nhi < hi ? nhi : hi;
        int c = 0;
        for (long long i = tid; i < nv; i += SP_THREADS) c += sp_kept(vals[i], lo, hi) ? 1 : 0;
        const int now = sp_block_sum_i(c, sh.red_i[0]);
        ++iters;
        fresh = now == kept;
        kept = now;
        if (fresh) break;
    }
    if (!fresh) {                                                        // the cap was hit (or nothing is left): statistics of what is kept
        mean = median = sd = qnan;
        if (kept > 0) {
            median = sp_median(vals, nv, lo, hi, kept, sh);
            double a = 0.0;
            for (long long i = tid; i < nv; i += SP_THREADS) { const float x = vals[i]; if (sp_kept(x, lo, hi)) a += (double)x; }
            mean = sp_block_sum(a, sh.red_d[0]) / (double)kept;
            a = 0.0;
            for (long long i = tid; i < nv; i += SP_THREADS) {
                const float x = vals[i];
                if (sp_kept(x, lo, hi)) { const double t = (double)x - mean; a += t * t; }
            }
            sd = sqrt(sp_block_sum(a, sh.red_d[0]) / (double)kept);
        }
    }

    if (tid == 0) {
        mrcnn_source_record r;
        r.s64 = s64; r.w00 = w00; r.w10 = w10; r.w01 = w01;
        r.clip_mean = mean; r.clip_median = median; r.clip_std = sd;
        r.m00 = m00; r.m10 = m10; r.m01 = m01;
        r.fill = fill;
        r.smin = npix ? smin : __uint_as_float(0x7FC00000u);
        r.smax = npix ? smax : __uint_as_float(0x7FC00000u);
        r.n_mask = (int)(n_mask > 0x7FFFFFFFll ? 0x7FFFFFFFll : n_mask);
        r.npix = npix;
        r.clip_kept = kept;
        r.clip_iters = iters;
        r.n_gathered = (int)(nv > 0x7FFFFFFFll ? 0x7FFFFFFFll : nv);
        out[s] = r;
    }
}

extern "C" int mrcnn_source_params(const void* img, int big_endian, int H, int W, const void* pool, int64_t pool_words,
                                   const mrcnn_tile_source* desc, int n, const int32_t* cutouts, const int64_t* val_offsets,
                                   void* values, int64_t values_len, double sigma, int maxiters, mrcnn_source_record* out, void* stream) {
    if (n < 0 || H < 0 || W < 0 || pool_words < 0 || values_len < 0 || maxiters < 0 || !(sigma >= 0.0)) return MRCNN_ERR_ARG;
    if (n == 0) return MRCNN_OK;
    if (!img || !pool || !desc || !cutouts || !val_offsets || !values || !out || H == 0 || W == 0) return MRCNN_ERR_ARG;
    if (pool_words > 0x7FFFFFFFll) return MRCNN_ERR_UNSUPPORTED;        // word_offset is 32-bit
    hipLaunchKernelGGL(source_params_kernel, dim3((unsigned)n), dim3(SP_THREADS), 0, (hipStream_t)stream, (const unsigned*)img, big_endian,
                       H, W, (const unsigned*)pool, (long long)pool_words, desc, n, (const int*)cutouts, (const long long*)val_offsets,
                       (float*)values, (long long)values_len, sigma, maxiters, out);
    return mrcnn_launch_status();
}
