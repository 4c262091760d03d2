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
