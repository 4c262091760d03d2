// detect() pre-processing on the device: MaskRCNN.mold_inputs (mrcnn/model.py:2519-2556) for uint8 images --
// utils.resize_image (mrcnn/utils.py:456-561: up-scaling with skimage.transform.resize(order=1, mode='constant', cval=0,
// clip=True, preserve_range=True) [3P], zero padding to the network's canvas, cast back to uint8) followed by mold_image
// (mrcnn/model.py:2964-2969: float32 minus MEAN_PIXEL).  The caller keeps the scalar logic (scale, output size, window,
// padding); a thread owns one canvas pixel x channel and evaluates the host restatement's float64 expression
// (caesar-mrcnn_amd/utils.py:resize) in the same order, so the molded image is identical to the host path's.
// The training loader stops after resize_image (load_image_gt augments between the two, mrcnn/model.py:1300-1359): the same
// expression with the uint8 canvas as its result, mrcnn_resize_image_u8.
#include "common.h"

// min / max over all bytes of the source image: the bounds skimage's clip=True clamps the interpolated values to
__global__ __launch_bounds__(1024) void mold_minmax_kernel(const unsigned char* __restrict__ src, long long n, int* __restrict__ mm) {
    __shared__ int s_mn[1024], s_mx[1024];
    const int tid = threadIdx.x;
    int mn = 255, mx = 0;
    for (long long i = tid; i < n; i += 1024) {
        const int v = src[i];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    s_mn[tid] = mn; s_mx[tid] = mx;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) {
            s_mn[tid] = s_mn[tid] < s_mn[tid + s] ? s_mn[tid] : s_mn[tid + s];
            s_mx[tid] = s_mx[tid] > s_mx[tid + s] ? s_mx[tid] : s_mx[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) { mm[0] = s_mn[0]; mm[1] = s_mx[0]; }
}

struct MoldMean { double m[4]; };

// One value of utils.resize_image before the padding: channel c of pixel (oy, ox) of the image resized from h x w to oh x ow
// (oh == h && ow == w: copied) -- utils.resize's float64 bilinear in its order, clipped to the source's min / max (mm), truncated
// to a byte as image.astype(uint8) does (0 <= o <= 255)
__device__ __forceinline__ int mold_resize_value(const unsigned char* __restrict__ src, int h, int w, int C, int oh, int ow, int oy, int ox,
                                                 int c, const int* __restrict__ mm) {
    if (oh == h && ow == w) return src[((long long)oy * w + ox) * C + c];
    const double ry = ((double)oy + 0.5) * ((double)h / (double)oh) - 0.5;
    const double rx = ((double)ox + 0.5) * ((double)w / (double)ow) - 0.5;
    const double fy0 = floor(ry), fx0 = floor(rx);
    const int y0 = (int)fy0, x0 = (int)fx0;
    const double fy = ry - fy0, fx = rx - fx0;
    const bool yt = y0 >= 0 && y0 < h, yb = y0 + 1 >= 0 && y0 + 1 < h;
    const bool xl = x0 >= 0 && x0 < w, xr = x0 + 1 >= 0 && x0 + 1 < w;
    const double tl = (yt && xl) ? (double)src[((long long)y0 * w + x0) * C + c] : 0.0;
    const double tr = (yt && xr) ? (double)src[((long long)y0 * w + x0 + 1) * C + c] : 0.0;
    const double bl = (yb && xl) ? (double)src[((long long)(y0 + 1) * w + x0) * C + c] : 0.0;
    const double br = (yb && xr) ? (double)src[((long long)(y0 + 1) * w + x0 + 1) * C + c] : 0.0;
    double o = (tl * (1.0 - fx) + tr * fx) * (1.0 - fy) + (bl * (1.0 - fx) + br * fx) * fy;
    const double mn = (double)mm[0], mx = (double)mm[1];
    o = o < mn ? mn : o;
    o = o > mx ? mx : o;
    return (int)o;
}

// channel c of canvas pixel i / C: rows [top, top + oh) x columns [left, left + ow) hold the resized image, everything else the
// padding value 0 (np.pad(..., constant_values=0))
__device__ __forceinline__ int mold_canvas_value(const unsigned char* __restrict__ src, int h, int w, int C, int oh, int ow, int top, int left,
                                                 int OW, const int* __restrict__ mm, long long i) {
    const int c = (int)(i % C);
    const long long pix = i / C;
    const int X = (int)(pix % OW), Y = (int)(pix / OW);
    const int oy = Y - top, ox = X - left;
    if (oy < 0 || oy >= oh || ox < 0 || ox >= ow) return 0;
    return mold_resize_value(src, h, w, C, oh, ow, oy, ox, c, mm);
}

// canvas [OH, OW, C] float32: the padded, resized image, every value minus its channel's mean pixel
__global__ __launch_bounds__(256) void mold_resize_kernel(const unsigned char* __restrict__ src, int h, int w, int C, int oh, int ow, int top,
                                                          int left, int OH, int OW, const int* __restrict__ mm, const MoldMean mean,
                                                          float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)OH * OW * C;
    if (i >= total) return;
    const int byte = mold_canvas_value(src, h, w, C, oh, ow, top, left, OW, mm, i);
    out[i] = (float)((double)(float)byte - mean.m[(int)(i % C)]);       // mold_image: images.astype(float32) - MEAN_PIXEL (float64), then float32
}

// canvas [OH, OW, C] uint8: utils.resize_image's own result (training augments it before the molding)
__global__ __launch_bounds__(256) void resize_u8_kernel(const unsigned char* __restrict__ src, int h, int w, int C, int oh, int ow, int top,
                                                        int left, int OH, int OW, const int* __restrict__ mm, unsigned char* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)OH * OW * C;
    if (i >= total) return;
    out[i] = (unsigned char)mold_canvas_value(src, h, w, C, oh, ow, top, left, OW, mm, i);
}

static int mold_args_status(const void* src, const void* out, int h, int w, int C, int oh, int ow, int top, int left, int OH, int OW) {
    if (!src || !out || h <= 0 || w <= 0 || C <= 0 || C > 4 || oh <= 0 || ow <= 0 || OH <= 0 || OW <= 0 || top < 0 || left < 0 ||
        top + oh > OH || left + ow > OW)
        return MRCNN_ERR_ARG;
    return MRCNN_OK;
}

extern "C" int mrcnn_mold_image_u8(const void* src, int h, int w, int C, int oh, int ow, int top, int left, int OH, int OW,
                                   const double* mean_pixel, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (mold_args_status(src, out, h, w, C, oh, ow, top, left, OH, OW)) return MRCNN_ERR_ARG;
    if (!workspace || workspace_bytes < 2 * sizeof(int)) return MRCNN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int* mm = (int*)workspace;
    MoldMean mean = {};
    for (int c = 0; c < C; ++c) mean.m[c] = mean_pixel ? mean_pixel[c] : 0.0;
    if (oh != h || ow != w)
        hipLaunchKernelGGL(mold_minmax_kernel, dim3(1), dim3(1024), 0, s, (const unsigned char*)src, (long long)h * w * C, mm);
    const long long total = (long long)OH * OW * C;
    hipLaunchKernelGGL(mold_resize_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, s, (const unsigned char*)src, h, w, C, oh, ow,
                       top, left, OH, OW, mm, mean, out);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_resize_image_u8(const void* src, int h, int w, int C, int oh, int ow, int top, int left, int OH, int OW, void* out,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    if (mold_args_status(src, out, h, w, C, oh, ow, top, left, OH, OW)) return MRCNN_ERR_ARG;
    if (!workspace || workspace_bytes < 2 * sizeof(int)) return MRCNN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int* mm = (int*)workspace;
    if (oh != h || ow != w)
        hipLaunchKernelGGL(mold_minmax_kernel, dim3(1), dim3(1024), 0, s, (const unsigned char*)src, (long long)h * w * C, mm);
    const long long total = (long long)OH * OW * C;
    hipLaunchKernelGGL(resize_u8_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, s, (const unsigned char*)src, h, w, C, oh, ow,
                       top, left, OH, OW, mm, (unsigned char*)out);
    return mrcnn_launch_status();
}

// ---------------------------------------------------------------------------------------------------
// The float32 twin (mrcnn_mold_image_f32): read_fits(to_uint8=False) and gray images are float32, and resize_image keeps their
// dtype -- the same float64 bilinear, clipped to the source's float minimum / maximum as np.clip does, rounded to float32
// (image.astype(dtype)), zero padding, minus MEAN_PIXEL in float64, rounded to float32 (_run_graph's cast).
//
// Minimum / maximum: tiles reach 2048 x 2048 x 3 floats (48 MiB) here, so one workgroup is not enough.  Stage 1: MOLD_F32_MM_WGS
// workgroups at most, each reduces a grid-strided share (16-byte loads where the source is aligned) to one {min, max, NaN seen}
// record in the workspace; stage 2: one workgroup reduces the records.  No atomics; min and max are taken in the total order of the
// bit patterns (-0.0 < +0.0), so the result does not depend on which workgroup saw which element.  A NaN anywhere makes the
// host's img.min() / img.max() NaN and np.clip then returns NaN everywhere: the final record holds NaN bounds then.
// Workspace: the final record {min, max} (16 bytes), then one 16-byte record per stage-1 workgroup.
#define MOLD_F32_MM_WGS 1024
#define MOLD_F32_MM_NT 256
#define MOLD_F32_MM_PER_THREAD 16        // floats a stage-1 thread reduces at least, before another workgroup is added

struct MoldMinMaxRec { int kmin, kmax, nan, pad; };

// monotone, self-inverse map between a non-NaN float's bits and a signed integer: a < b as floats, with -0.0 < +0.0,
// <=> key(a) < key(b)
__device__ __forceinline__ int mold_f32_key(int bits) { return bits >= 0 ? bits : bits ^ 0x7fffffff; }

struct MoldMinMaxAcc {
    int kmin, kmax, nan;
    __device__ __forceinline__ void init() { kmin = 0x7fffffff; kmax = (int)0x80000000u; nan = 0; }
    __device__ __forceinline__ void add(float v) {
        if (v != v) { nan = 1; return; }
        const int k = mold_f32_key(__float_as_int(v));
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
    }
    __device__ __forceinline__ void merge(int mn, int mx, int n) {
        kmin = mn < kmin ? mn : kmin;
        kmax = mx > kmax ? mx : kmax;
        nan |= n;
    }
};

// the workgroup's threads' accumulators -> thread 0's (MOLD_F32_MM_NT threads)
__device__ __forceinline__ void mold_f32_wg_reduce(MoldMinMaxAcc& a) {
    __shared__ int s_mn[MOLD_F32_MM_NT], s_mx[MOLD_F32_MM_NT], s_nan[MOLD_F32_MM_NT];
    const int tid = threadIdx.x;
    s_mn[tid] = a.kmin; s_mx[tid] = a.kmax; s_nan[tid] = a.nan;
    __syncthreads();
    for (int s = MOLD_F32_MM_NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            s_mn[tid] = s_mn[tid] < s_mn[tid + s] ? s_mn[tid] : s_mn[tid + s];
            s_mx[tid] = s_mx[tid] > s_mx[tid + s] ? s_mx[tid] : s_mx[tid + s];
            s_nan[tid] |= s_nan[tid + s];
        }
        __syncthreads();
    }
    a.kmin = s_mn[0]; a.kmax = s_mx[0]; a.nan = s_nan[0];
}

// stage 1: workgroup b reduces elements b * NT + tid, + gridDim.x * NT, ... (float4 units when vec) to rec[b]
__global__ __launch_bounds__(MOLD_F32_MM_NT) void mold_f32_minmax_partial_kernel(const float* __restrict__ src, long long n, int vec,
                                                                                 MoldMinMaxRec* __restrict__ rec) {
    MoldMinMaxAcc a;
    a.init();
    const long long stride = (long long)gridDim.x * MOLD_F32_MM_NT;
    const long long t = (long long)blockIdx.x * MOLD_F32_MM_NT + threadIdx.x;
    if (vec) {                                                   // src is 16-byte aligned
        const long long n4 = n >> 2;
        const f32x4* __restrict__ s4 = (const f32x4*)src;
        for (long long i = t; i < n4; i += stride) {
            const f32x4 v = s4[i];
            a.add(v[0]); a.add(v[1]); a.add(v[2]); a.add(v[3]);
        }
        for (long long i = (n4 << 2) + t; i < n; i += stride) a.add(src[i]);
    } else {
        for (long long i = t; i < n; i += stride) a.add(src[i]);
    }
    mold_f32_wg_reduce(a);
    if (threadIdx.x == 0) {
        MoldMinMaxRec r;
        r.kmin = a.kmin; r.kmax = a.kmax; r.nan = a.nan; r.pad = 0;
        rec[blockIdx.x] = r;
    }
}

// stage 2: one workgroup, the nrec records -> mm[0] = min, mm[1] = max (both NaN when a NaN was seen)
__global__ __launch_bounds__(MOLD_F32_MM_NT) void mold_f32_minmax_final_kernel(const MoldMinMaxRec* __restrict__ rec, int nrec,
                                                                               float* __restrict__ mm) {
    MoldMinMaxAcc a;
    a.init();
    for (int i = threadIdx.x; i < nrec; i += MOLD_F32_MM_NT) {
        const MoldMinMaxRec r = rec[i];
        a.merge(r.kmin, r.kmax, r.nan);
    }
    mold_f32_wg_reduce(a);
    if (threadIdx.x == 0) {
        const float qnan = __int_as_float(0x7fc00000);
        mm[0] = a.nan ? qnan : __int_as_float(mold_f32_key(a.kmin));
        mm[1] = a.nan ? qnan : __int_as_float(mold_f32_key(a.kmax));
    }
}

// One value of utils.resize_image before the padding, for a float32 image: utils.resize's float64 bilinear in its order, then
// np.clip(out, img.min(), img.max()) as NumPy evaluates it for scalar bounds -- NaN everywhere when a bound is NaN, else
// x < lo ? lo : (x > hi ? hi : x), which keeps a NaN x and the sign of a zero that ties with a bound -- then astype(float32)
__device__ __forceinline__ float mold_f32_resize_value(const float* __restrict__ src, int h, int w, int C, int oh, int ow, int oy, int ox,
                                                       int c, double mn, double mx) {
    if (oh == h && ow == w) return src[((long long)oy * w + ox) * C + c];
    const double ry = ((double)oy + 0.5) * ((double)h / (double)oh) - 0.5;
    const double rx = ((double)ox + 0.5) * ((double)w / (double)ow) - 0.5;
    const double fy0 = floor(ry), fx0 = floor(rx);
    const int y0 = (int)fy0, x0 = (int)fx0;
    const double fy = ry - fy0, fx = rx - fx0;
    const bool yt = y0 >= 0 && y0 < h, yb = y0 + 1 >= 0 && y0 + 1 < h;
    const bool xl = x0 >= 0 && x0 < w, xr = x0 + 1 >= 0 && x0 + 1 < w;
    const double tl = (yt && xl) ? (double)src[((long long)y0 * w + x0) * C + c] : 0.0;
    const double tr = (yt && xr) ? (double)src[((long long)y0 * w + x0 + 1) * C + c] : 0.0;
    const double bl = (yb && xl) ? (double)src[((long long)(y0 + 1) * w + x0) * C + c] : 0.0;
    const double br = (yb && xr) ? (double)src[((long long)(y0 + 1) * w + x0 + 1) * C + c] : 0.0;
    double o = (tl * (1.0 - fx) + tr * fx) * (1.0 - fy) + (bl * (1.0 - fx) + br * fx) * fy;
    if (mn != mn) return __int_as_float(0x7fc00000);              // (the final record holds NaN in both bounds or in neither)
    o = o < mn ? mn : (o > mx ? mx : o);
    return (float)o;
}

// element i of the molded canvas [OH, OW, C]
__device__ __forceinline__ float mold_f32_canvas_value(const float* __restrict__ src, int h, int w, int C, int oh, int ow, int top, int left,
                                                       int OW, double mn, double mx, const MoldMean& mean, long long i) {
    const int c = (int)(i % C);
    const long long pix = i / C;
    const int X = (int)(pix % OW), Y = (int)(pix / OW);
    const int oy = Y - top, ox = X - left;
    float v = 0.f;                                                // np.pad(..., constant_values=0)
    if (oy >= 0 && oy < oh && ox >= 0 && ox < ow) v = mold_f32_resize_value(src, h, w, C, oh, ow, oy, ox, c, mn, mx);
    return (float)((double)v - mean.m[c]);                        // mold_image (float32 minus float64 MEAN_PIXEL), then float32
}

// a thread owns four consecutive canvas elements: one 16-byte store when vec (total % 4 == 0, out 16-byte aligned)
__global__ __launch_bounds__(256) void mold_f32_resize_kernel(const float* __restrict__ src, int h, int w, int C, int oh, int ow, int top,
                                                              int left, int OH, int OW, const float* __restrict__ mm, int scaled,
                                                              const MoldMean mean, int vec, float* __restrict__ out) {
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    const long long total = (long long)OH * OW * C;
    if (i0 >= total) return;
    double mn = 0.0, mx = 0.0;
    if (scaled) { mn = (double)mm[0]; mx = (double)mm[1]; }       // (unscaled: the min / max pass did not run, mm is not read)
    if (vec) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = mold_f32_canvas_value(src, h, w, C, oh, ow, top, left, OW, mn, mx, mean, i0 + e);
        *(f32x4*)(out + i0) = v;
    } else {
        for (int e = 0; e < 4; ++e)
            if (i0 + e < total) out[i0 + e] = mold_f32_canvas_value(src, h, w, C, oh, ow, top, left, OW, mn, mx, mean, i0 + e);
    }
}

// workgroups of the stage-1 reduction over n floats
static int mold_f32_minmax_wgs(long long n) {
    const long long per_wg = (long long)MOLD_F32_MM_NT * MOLD_F32_MM_PER_THREAD;
    long long g = (n + per_wg - 1) / per_wg;
    return (int)(g < 1 ? 1 : (g > MOLD_F32_MM_WGS ? MOLD_F32_MM_WGS : g));
}

extern "C" size_t mrcnn_mold_image_f32_workspace_bytes(void) { return sizeof(MoldMinMaxRec) * (1 + MOLD_F32_MM_WGS); }

extern "C" int mrcnn_mold_image_f32(const void* src, int h, int w, int C, int oh, int ow, int top, int left, int OH, int OW,
                                    const double* mean_pixel, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (mold_args_status(src, out, h, w, C, oh, ow, top, left, OH, OW)) return MRCNN_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(src) & 3) || (reinterpret_cast<uintptr_t>(out) & 3)) return MRCNN_ERR_ARG;
    if (!workspace || workspace_bytes < mrcnn_mold_image_f32_workspace_bytes() || (reinterpret_cast<uintptr_t>(workspace) & 15))
        return MRCNN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float* mm = (float*)workspace;
    MoldMinMaxRec* rec = (MoldMinMaxRec*)workspace + 1;
    MoldMean mean = {};
    for (int c = 0; c < C; ++c) mean.m[c] = mean_pixel ? mean_pixel[c] : 0.0;
    const int scaled = (oh != h || ow != w) ? 1 : 0;
    if (scaled) {
        const long long n = (long long)h * w * C;
        const int wgs = mold_f32_minmax_wgs(n);
        const int vec_in = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
        hipLaunchKernelGGL(mold_f32_minmax_partial_kernel, dim3(wgs), dim3(MOLD_F32_MM_NT), 0, s, (const float*)src, n, vec_in, rec);
        hipLaunchKernelGGL(mold_f32_minmax_final_kernel, dim3(1), dim3(MOLD_F32_MM_NT), 0, s, rec, wgs, mm);
    }
    const long long total = (long long)OH * OW * C;
    const int vec_out = (total % 4 == 0) && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    hipLaunchKernelGGL(mold_f32_resize_kernel, dim3((unsigned)cdiv64(cdiv64(total, 4), 256)), dim3(256), 0, s, (const float*)src, h, w, C, oh,
                       ow, top, left, OH, OW, mm, scaled, mean, vec_out, out);
    return mrcnn_launch_status();
}
