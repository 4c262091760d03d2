// Source catalogue on the device: the geometry and the pixel bookkeeping of the source classifier for a whole catalogue at once
// (mrcnn/classifier.py:167-260 classify_source, mrcnn/utils.py:1211-1227 crop_img; caesar-mrcnn_amd/classifier.py is the host
// statement every kernel here equals value for value).
//
//   catalog_scan_kernel<FILL>   windows of a block of 64 sources i, and for each the sources j whose centre lies strictly inside:
//                               counted (FILL = false) or written as a CSR row in ascending j (FILL = true).  A workgroup of four
//                               wavefronts owns 64 sources, 16 per wavefront; the catalogue's centres pass through LDS in tiles of
//                               256, so a workgroup reads them once per block of i, not once per i.  A wavefront tests 64 j at a time
//                               against one window; __ballot gives the members as a mask, the prefix popcount of a lane's lower
//                               neighbours its slot in the row: ascending j without an atomic and without a sort.  The box columns
//                               are read from global memory for members only (the cut flag).  At 10^5 sources: 10^10 tests of four
//                               float64 comparisons against 1563 workgroups x 1.6 MB of centres that stay in the L2 -- the
//                               comparisons bound it, not the traffic.
//   catalog_flags_kernel        finite and NaN pixels of every window of a resident plane, one workgroup per window.
//   catalog_fill_walk_kernel    crop_img's in-place NaN fill, window after window in table order, by ONE workgroup: minimum of the
//   catalog_fill_one_kernel     window as the plane is then, barrier, write it into the NaN pixels, barrier.  Or one launch per
//                               window in stream order.  min is exact in any order, so both forms leave the same plane.
// Plain C++ throughout; every store is a vector store.
#include "common.h"
#include <math.h>

#define CAT_IB 64                // sources i per workgroup
#define CAT_IPW 16               // ... per wavefront
#define CAT_JT 256               // centres j per LDS tile

int g_mrcnn_catalog_max_sources = MRCNN_CATALOG_MAX_SOURCES;

__device__ __forceinline__ int cat_lower_lanes(unsigned long long mask) {      // set bits of `mask` below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

template <bool FILL>
__global__ __launch_bounds__(256) void catalog_scan_kernel(const double* __restrict__ x0, const double* __restrict__ y0,
                                                           const double* __restrict__ bxmin, const double* __restrict__ bxmax,
                                                           const double* __restrict__ bymin, const double* __restrict__ bymax, int S,
                                                           double hx, double hy, int* __restrict__ windows, int* __restrict__ counts,
                                                           const long long* __restrict__ offsets, int* __restrict__ members,
                                                           unsigned char* __restrict__ cut) {
    __shared__ double s_win[CAT_IB][4];                  // xmin, xmax, ymin, ymax of the block's windows, as float64
    __shared__ double s_x[CAT_JT], s_y[CAT_JT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i_base = blockIdx.x * CAT_IB;
    if (tid < CAT_IB) {
        const int i = i_base + tid;
        double w0 = INFINITY, w1 = -INFINITY, w2 = INFINITY, w3 = -INFINITY;        // past the catalogue: a window nothing is inside
        if (i < S) {
            const double cx = x0[i], cy = y0[i];
            const int xmin = (int)(cx - hx), xmax = (int)(cx + hx), ymin = (int)(cy - hy), ymax = (int)(cy + hy);
            w0 = (double)xmin; w1 = (double)xmax; w2 = (double)ymin; w3 = (double)ymax;
            if (!FILL) {
                windows[4 * i + 0] = xmin; windows[4 * i + 1] = xmax; windows[4 * i + 2] = ymin; windows[4 * i + 3] = ymax;
            }
        }
        s_win[tid][0] = w0; s_win[tid][1] = w1; s_win[tid][2] = w2; s_win[tid][3] = w3;
    }
    int cnt[CAT_IPW];                                     // members found so far, per source of this wavefront (wave-uniform)
#pragma unroll
    for (int k = 0; k < CAT_IPW; ++k) cnt[k] = 0;
    for (int j0 = 0; j0 < S; j0 += CAT_JT) {
        __syncthreads();                                  // the windows are there / the last tile has been read
        {
            const int j = j0 + tid;
            s_x[tid] = j < S ? x0[j] : NAN;               // NaN is inside no window
            s_y[tid] = j < S ? y0[j] : NAN;
        }
        __syncthreads();
        for (int c = 0; c < CAT_JT; c += 64) {
            if (j0 + c >= S) break;                       // uniform
            const int j = j0 + c + lane;
            const double xj = s_x[c + lane], yj = s_y[c + lane];
#pragma unroll
            for (int k = 0; k < CAT_IPW; ++k) {
                const int il = wave * CAT_IPW + k, i = i_base + il;
                const double w0 = s_win[il][0], w1 = s_win[il][1], w2 = s_win[il][2], w3 = s_win[il][3];
                const bool in = xj > w0 && xj < w1 && yj > w2 && yj < w3 && j != i;
                const unsigned long long mask = __ballot(in);
                if (FILL) {
                    if (in) {
                        const long long pos = offsets[i] + cnt[k] + cat_lower_lanes(mask);
                        if (pos < offsets[i + 1]) {       // (a scan that does not belong to these counts writes nothing past its row)
                            members[pos] = j;
                            cut[pos] = (bxmin[j] <= w0 || bxmax[j] >= w1 || bymin[j] <= w2 || bymax[j] >= w3) ? 1 : 0;
                        }
                    }
                }
                cnt[k] += __popcll(mask);
            }
        }
    }
    if (!FILL && lane == 0) {
#pragma unroll
        for (int k = 0; k < CAT_IPW; ++k) {
            const int i = i_base + wave * CAT_IPW + k;
            if (i < S) counts[i] = cnt[k];
        }
    }
}

// ---- windows of a resident plane ----------------------------------------------------------------------------------------------
struct CatRect { int x0, y0, w, h; };                     // the window clipped as NumPy slicing clips; w = 0: nothing to do

__device__ __forceinline__ CatRect cat_clip(const int* __restrict__ win, int NY, int NX) {
    const int xmin = win[0], xmax = win[1], ymin = win[2], ymax = win[3];
    CatRect r = {0, 0, 0, 0};
    if (xmin < 0 || xmax < 0 || ymin < 0 || ymax < 0) return r;
    const int x1 = xmax < NX ? xmax : NX, y1 = ymax < NY ? ymax : NY;
    if (x1 <= xmin || y1 <= ymin) return r;
    r.x0 = xmin; r.y0 = ymin; r.w = x1 - xmin; r.h = y1 - ymin;
    return r;
}

__device__ __forceinline__ int cat_block_sum(int v, int* red, int tid, int nthreads) {
    red[tid] = v;
    __syncthreads();
    for (int s = nthreads >> 1; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const int r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void catalog_flags_kernel(const float* __restrict__ plane, int NY, int NX, const int* __restrict__ windows,
                                                            int* __restrict__ flags) {
    __shared__ int s_red[256];
    const int t = blockIdx.x, tid = threadIdx.x;
    const CatRect r = cat_clip(windows + 4 * (long long)t, NY, NX);
    const long long n = (long long)r.w * r.h;
    int fin = 0, nan = 0;
    for (long long p = tid; p < n; p += 256) {
        const long long y = p / r.w;
        const float v = plane[(r.y0 + y) * (long long)NX + r.x0 + (p - y * r.w)];
        if (v != v) ++nan;
        else if (!isinf(v)) ++fin;
    }
    fin = cat_block_sum(fin, s_red, tid, 256);
    nan = cat_block_sum(nan, s_red, tid, 256);
    if (tid == 0) { flags[2 * (long long)t] = fin; flags[2 * (long long)t + 1] = nan; }
}

// One window's turn of the fill, by the whole workgroup (1024 threads).  The plane is read and written by this workgroup alone.
__device__ __forceinline__ void cat_fill_turn(float* plane, int NY, int NX, const int* __restrict__ win, int* __restrict__ alive,
                                              float* s_mn, int* s_red) {
    const int tid = threadIdx.x;
    const CatRect r = cat_clip(win, NY, NX);
    const long long n = (long long)r.w * r.h;
    float mn = INFINITY;
    int fin = 0;
    for (long long p = tid; p < n; p += 1024) {
        const long long y = p / r.w;
        const float v = plane[(r.y0 + y) * (long long)NX + r.x0 + (p - y * r.w)];
        if (v != v) continue;
        mn = fminf(mn, v);                                // np.nanmin: infinities take part
        if (!isinf(v)) ++fin;
    }
    s_mn[tid] = mn;
    fin = cat_block_sum(fin, s_red, tid, 1024);           // (its barriers also publish s_mn)
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) s_mn[tid] = fminf(s_mn[tid], s_mn[tid + s]);
        __syncthreads();
    }
    mn = s_mn[0];
    if (tid == 0) *alive = fin > 0 ? 1 : 0;
    if (fin > 0) {                                        // uniform
        for (long long p = tid; p < n; p += 1024) {
            const long long y = p / r.w;
            float* q = plane + (r.y0 + y) * (long long)NX + r.x0 + (p - y * r.w);
            const float v = *q;
            if (v != v) *q = mn;
        }
    }
    __threadfence();
    __syncthreads();                                      // the next turn reads what this one wrote (and s_mn is free again)
}

__global__ __launch_bounds__(1024) void catalog_fill_walk_kernel(float* plane, int NY, int NX, const int* __restrict__ windows, int K,
                                                                 int* __restrict__ alive) {
    __shared__ float s_mn[1024];
    __shared__ int s_red[1024];
    for (int k = 0; k < K; ++k) cat_fill_turn(plane, NY, NX, windows + 4 * (long long)k, alive + k, s_mn, s_red);
}

__global__ __launch_bounds__(1024) void catalog_fill_one_kernel(float* plane, int NY, int NX, const int* __restrict__ windows, int k,
                                                                int* __restrict__ alive) {
    __shared__ float s_mn[1024];
    __shared__ int s_red[1024];
    cat_fill_turn(plane, NY, NX, windows + 4 * (long long)k, alive + k, s_mn, s_red);
}

// ---- entry points --------------------------------------------------------------------------------------------------------------
extern "C" int mrcnn_catalog_check(int S) {
    if (S <= 0) return MRCNN_ERR_ARG;
    if (S > g_mrcnn_catalog_max_sources) return MRCNN_ERR_UNSUPPORTED;
    return MRCNN_OK;
}

static bool cat_size_ok(double d) { return d > 0.0 && d < 2147483648.0; }      // (false for NaN)

extern "C" int mrcnn_catalog_count(const double* x0, const double* y0, int S, double dx, double dy, int* windows, int* counts,
                                   void* stream) {
    if (!x0 || !y0 || !windows || !counts || !cat_size_ok(dx) || !cat_size_ok(dy)) return MRCNN_ERR_ARG;
    const int rc = mrcnn_catalog_check(S);
    if (rc != MRCNN_OK) return rc;
    hipLaunchKernelGGL(catalog_scan_kernel<false>, dim3((unsigned)cdiv64(S, CAT_IB)), dim3(256), 0, (hipStream_t)stream, x0, y0,
                       (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, S, dx / 2, dy / 2,
                       windows, counts, (const long long*)nullptr, (int*)nullptr, (unsigned char*)nullptr);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_catalog_fill(const double* x0, const double* y0, const double* xmin, const double* xmax, const double* ymin,
                                  const double* ymax, int S, double dx, double dy, const long long* offsets, long long total, int* members,
                                  unsigned char* cut, void* stream) {
    if (!x0 || !y0 || !xmin || !xmax || !ymin || !ymax || !offsets || total < 0 || !cat_size_ok(dx) || !cat_size_ok(dy)) return MRCNN_ERR_ARG;
    const int rc = mrcnn_catalog_check(S);
    if (rc != MRCNN_OK) return rc;
    if (total > 2147483647ll) return MRCNN_ERR_UNSUPPORTED;
    if (total == 0) return MRCNN_OK;
    if (!members || !cut) return MRCNN_ERR_ARG;
    hipLaunchKernelGGL(catalog_scan_kernel<true>, dim3((unsigned)cdiv64(S, CAT_IB)), dim3(256), 0, (hipStream_t)stream, x0, y0, xmin, xmax,
                       ymin, ymax, S, dx / 2, dy / 2, (int*)nullptr, (int*)nullptr, offsets, members, cut);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_catalog_window_flags(const float* plane, int NY, int NX, const int* windows, int T, int* flags, void* stream) {
    if (!plane || !windows || !flags || T <= 0 || NY <= 0 || NX <= 0) return MRCNN_ERR_ARG;
    hipLaunchKernelGGL(catalog_flags_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, plane, NY, NX, windows, flags);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_catalog_nan_fill(float* plane, int NY, int NX, const int* windows, int K, int form, int* alive, void* stream) {
    if (K < 0 || NY <= 0 || NX <= 0 || (form != 0 && form != 1)) return MRCNN_ERR_ARG;
    if (K == 0) return MRCNN_OK;
    if (!plane || !windows || !alive) return MRCNN_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (form == 0) {
        hipLaunchKernelGGL(catalog_fill_walk_kernel, dim3(1), dim3(1024), 0, s, plane, NY, NX, windows, K, alive);
    } else {
        for (int k = 0; k < K; ++k)
            hipLaunchKernelGGL(catalog_fill_one_kernel, dim3(1), dim3(1024), 0, s, plane, NY, NX, windows, k, alive);
    }
    return mrcnn_launch_status();
}
