// Training augmentation on the device: the per-pixel warps of the reference's default pipeline
// (scripts/run.py:1091-1100: imgaug SomeOf((0, 2), [Fliplr, Flipud, Affine(rotate=(-90, 90)), Affine(translate_percent=
// (-0.3, 0.3))], random_order=True), mode='constant', cval=0), applied by load_image_gt to the image and to the instance
// masks (mrcnn/model.py:1323-1359).  The contract is the float64 host statement caesar-mrcnn_amd/augment.py:warp_host
// [imgaug bit-parity unpinned: imgaug is not installed]:
//   * one stage = one inverse map of an output pixel (x, y) to a source point (sx, sy) = (m0 x + m1 y + m2, m3 x + m4 y + m5),
//     the six doubles computed on the host (cos / sin never evaluated here) and passed by value;
//   * bilinear in float64, in this order: x0 = floor(sx), fx = sx - x0 (same for y), then
//     (tl (1 - fx) + tr fx) (1 - fy) + (bl (1 - fx) + br fx) fy; a tap outside the image reads 0;
//   * uint8 image: rint (half to even); masks: a bit is set when the value is > 0.5.
// Every stage writes its output before the next one reads it (the caller ping-pongs two buffers): two interpolating stages
// round twice, as the reference does.  The build's -ffp-contract=off keeps the products and sums unfused, so the results are
// byte-identical to NumPy's.
#include "common.h"

struct AugMat { double m[6]; };

// Where output pixel `pix` samples from: the tap origin (x0, y0), the fractions (fx, fy) and which of the four taps lie in
// the image.  False when no tap does (the pixel is 0 whatever it samples).
struct AugTaps {
    long long x0, y0;
    double fx, fy;
    bool l, r, t, b;
};

__device__ __forceinline__ bool aug_taps(const AugMat& M, int x, int y, int H, int W, AugTaps& T) {
    const double X = (double)x, Y = (double)y;
    const double sx = M.m[0] * X + M.m[1] * Y + M.m[2];
    const double sy = M.m[3] * X + M.m[4] * Y + M.m[5];
    // outside [-1, W] x [-1, H] (or not finite) no tap can land in the image; the range check also keeps the integer
    // conversion below defined
    if (!(sx > -1.0 && sx < (double)W && sy > -1.0 && sy < (double)H)) return false;
    const double fx0 = floor(sx), fy0 = floor(sy);
    T.x0 = (long long)fx0;
    T.y0 = (long long)fy0;
    T.fx = sx - fx0;
    T.fy = sy - fy0;
    T.l = T.x0 >= 0;
    T.r = T.x0 + 1 < W;
    T.t = T.y0 >= 0;
    T.b = T.y0 + 1 < H;
    return true;
}

__device__ __forceinline__ double aug_bilinear(double tl, double tr, double bl, double br, double fx, double fy) {
    return (tl * (1.0 - fx) + tr * fx) * (1.0 - fy) + (bl * (1.0 - fx) + br * fx) * fy;
}

// uint8 [H, W, C] image, C <= 4: a thread owns one output pixel, computes its weights once and writes all C channels.
__global__ __launch_bounds__(256) void augment_warp_u8_kernel(const unsigned char* __restrict__ src, int H, int W, int C,
                                                              const AugMat M, unsigned char* __restrict__ dst) {
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (long long)H * W) return;
    const int x = (int)(pix % W), y = (int)(pix / W);
    unsigned char* o = dst + pix * C;
    AugTaps T;
    if (!aug_taps(M, x, y, H, W, T)) {
        for (int c = 0; c < C; ++c) o[c] = 0;
        return;
    }
    const long long i00 = (T.y0 * W + T.x0) * C, i10 = i00 + (long long)W * C;     // element offsets of the top-left / bottom-left taps
    for (int c = 0; c < C; ++c) {
        const double tl = (T.t && T.l) ? (double)src[i00 + c] : 0.0;
        const double tr = (T.t && T.r) ? (double)src[i00 + C + c] : 0.0;
        const double bl = (T.b && T.l) ? (double)src[i10 + c] : 0.0;
        const double br = (T.b && T.r) ? (double)src[i10 + C + c] : 0.0;
        // 0 <= value <= 255 (convex weights of bytes): rint never leaves the byte range
        o[c] = (unsigned char)(int)rint(aug_bilinear(tl, tr, bl, br, T.fx, T.fy));
    }
}

// Bit-packed masks [H, W, nbytes] (numpy.packbits(mask, axis=-1, bitorder="little"): instance j = bit j & 7 of byte j >> 3),
// never unpacked.  Per output pixel the bilinear value of a 0/1 plane depends only on its four tap bits, so the thread
// evaluates the float64 expression once for each of the 16 tap patterns (a truth table) and then produces 32 instances at a
// time as the OR of the set minterms over the four tap words.  A tap outside the image is the all-zero word.  The all-zero
// pattern evaluates to 0, so padding bits stay 0.  WORDS: nbytes % 4 == 0 and both buffers 4-byte aligned (32-bit loads
// and stores); otherwise each word is assembled from its bytes and only the nbytes bytes are stored.
template <bool WORDS>
__device__ __forceinline__ unsigned aug_load_word(const unsigned char* p, int k, int nbytes) {
    if (WORDS) return ((const unsigned*)p)[k];
    unsigned w = 0;
    for (int i = 0; i < 4; ++i) {
        const int byte = 4 * k + i;
        if (byte < nbytes) w |= (unsigned)p[byte] << (8 * i);
    }
    return w;
}

template <bool WORDS>
__device__ __forceinline__ void aug_store_word(unsigned char* p, int k, int nbytes, unsigned w) {
    if (WORDS) {
        ((unsigned*)p)[k] = w;
        return;
    }
    for (int i = 0; i < 4; ++i) {
        const int byte = 4 * k + i;
        if (byte < nbytes) p[byte] = (unsigned char)(w >> (8 * i));
    }
}

template <bool WORDS>
__global__ __launch_bounds__(256) void augment_warp_mask_bits_kernel(const unsigned char* __restrict__ src, int H, int W, int nbytes,
                                                                     const AugMat M, unsigned char* __restrict__ dst) {
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (long long)H * W) return;
    const int x = (int)(pix % W), y = (int)(pix / W);
    const int nwords = (nbytes + 3) >> 2;
    unsigned char* o = dst + pix * nbytes;
    AugTaps T;
    unsigned table = 0;                 // bit p: value > 0.5 for tap pattern p = tl | tr << 1 | bl << 2 | br << 3
    if (aug_taps(M, x, y, H, W, T)) {
        for (int p = 1; p < 16; ++p) {
            const double v = aug_bilinear((double)(p & 1), (double)((p >> 1) & 1), (double)((p >> 2) & 1), (double)((p >> 3) & 1), T.fx, T.fy);
            table |= (v > 0.5 ? 1u : 0u) << p;
        }
    }
    if (!table) {
        for (int k = 0; k < nwords; ++k) aug_store_word<WORDS>(o, k, nbytes, 0u);
        return;
    }
    const long long i00 = (T.y0 * W + T.x0) * nbytes, i10 = i00 + (long long)W * nbytes;
    const unsigned char* q_tl = (T.t && T.l) ? src + i00 : nullptr;
    const unsigned char* q_tr = (T.t && T.r) ? src + i00 + nbytes : nullptr;
    const unsigned char* q_bl = (T.b && T.l) ? src + i10 : nullptr;
    const unsigned char* q_br = (T.b && T.r) ? src + i10 + nbytes : nullptr;
    for (int k = 0; k < nwords; ++k) {
        const unsigned a = q_tl ? aug_load_word<WORDS>(q_tl, k, nbytes) : 0u;
        const unsigned b = q_tr ? aug_load_word<WORDS>(q_tr, k, nbytes) : 0u;
        const unsigned c = q_bl ? aug_load_word<WORDS>(q_bl, k, nbytes) : 0u;
        const unsigned d = q_br ? aug_load_word<WORDS>(q_br, k, nbytes) : 0u;
        unsigned w = 0;
        for (int p = 1; p < 16; ++p) {
            if (!((table >> p) & 1u)) continue;
            w |= ((p & 1) ? a : ~a) & ((p & 2) ? b : ~b) & ((p & 4) ? c : ~c) & ((p & 8) ? d : ~d);
        }
        aug_store_word<WORDS>(o, k, nbytes, w);
    }
}

extern "C" int mrcnn_augment_warp_u8(const void* src, int H, int W, int C, const double* m, void* dst, void* stream) {
    if (!src || !dst || !m || H <= 0 || W <= 0 || C <= 0 || C > 4 || src == dst) return MRCNN_ERR_ARG;
    AugMat M;
    for (int i = 0; i < 6; ++i) M.m[i] = m[i];
    const long long npix = (long long)H * W;
    hipLaunchKernelGGL(augment_warp_u8_kernel, dim3((unsigned)cdiv64(npix, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)src, H, W, C, M, (unsigned char*)dst);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_augment_warp_mask_bits(const void* src, int H, int W, int nbytes_per_pixel, const double* m, void* dst,
                                            void* stream) {
    if (!src || !dst || !m || H <= 0 || W <= 0 || nbytes_per_pixel <= 0 || src == dst) return MRCNN_ERR_ARG;
    AugMat M;
    for (int i = 0; i < 6; ++i) M.m[i] = m[i];
    const long long npix = (long long)H * W;
    const dim3 grid((unsigned)cdiv64(npix, 256)), block(256);
    const bool words = nbytes_per_pixel % 4 == 0 && ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0;
    if (words)
        hipLaunchKernelGGL(augment_warp_mask_bits_kernel<true>, grid, block, 0, (hipStream_t)stream, (const unsigned char*)src, H, W,
                           nbytes_per_pixel, M, (unsigned char*)dst);
    else
        hipLaunchKernelGGL(augment_warp_mask_bits_kernel<false>, grid, block, 0, (hipStream_t)stream, (const unsigned char*)src, H, W,
                           nbytes_per_pixel, M, (unsigned char*)dst);
    return mrcnn_launch_status();
}
