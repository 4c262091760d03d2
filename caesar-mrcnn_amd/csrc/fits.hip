// FITS tile -> network input image on the device: the numeric part of utils.read_fits (mrcnn/utils.py:1033-1163).  As the run.py
// path calls it (stretch = normalize = convertToRGB = to_uint8 = True, no bias / contrast stretch):
//   out = data.astype(float32); out[isnan(out)] = nanmin(out)                                   (:1088-1091)
//   per channel c (zscale contrast zc):  ZScaleInterval(contrast=zc)(out)  -> [0, 1]            (:1101-1111, stretch_img :1166-1172)
//                                        / max                                                  (normalize_img :1182-1188)
//   uint8 RGB = round(255 * channel)                                                            (gray2rgb :1190-1208)
// and every other flag combination through the same three launches (the descriptor mrcnn_fits_chain; the second part of this file).
// astropy's ZScaleInterval [3P, SURVEY App. C-6] is the restatement of caesar-mrcnn_amd/fits.py:zscale_limits (<= 1000 strided
// samples of the finite values, sorted; <= 5 rounds of a straight-line fit with 2.5 sigma rejection grown by 1 % of the samples;
// limits = median -/+ slope / contrast, clamped to the sample range).  Three launches: per-chunk statistics (+ byte swap of the
// big-endian FITS floats), ONE workgroup for sampling / sort / fit, one pass that writes the image.  The per-pixel arithmetic is
// the host's, type for type (float32 subtraction, float64 division and clip, float32 normalisation, round-half-even), so the
// image is identical to fits.read_fits's; the fit uses the closed form of the weighted least-squares line where the host
// goes through numpy.polyfit's SVD (agreement ~1e-15 relative in the limits: far below half a grey level).
//
// mrcnn_fits_tiles_to_image runs the same three stages over T tiles of ONE resident plane (the mosaic of the tiled source finder)
// with the tile as a grid dimension: the statistics pass reads every tile row as a strided segment of the plane (consecutive
// lanes = consecutive pixels of a row: a wavefront's loads stay in one row segment, two at a row end) and leaves the tile's
// native-endian values row-major and contiguous in the workspace, so the sampling and the pixel pass address a tile exactly as
// the single-tile path does -- the bodies below are shared, not copied.  mrcnn_fits_to_rgb / mrcnn_fits_tiles_to_rgb are these
// entries with the run.py descriptor.
//
// mrcnn_mosaic_overview (at the end of this file) stretches a WHOLE plane of any size up to 2^31 - 1 pixels and shrinks it by
// block maxima: the same statistics per 1024-pixel chunk, a two-level scan of the chunks' finite counts instead of the one LDS
// table, the sampling from the plane where it lies (no native-endian copy), then fits_zscale_fit and fits_byte.
#include "common.h"
#include <math.h>

#define FITS_CHUNK 1024          // pixels per statistics chunk
#define FITS_MAX_CHUNKS 4096     // one workgroup scans the chunk table in LDS: tiles up to 2048 x 2048
#define FITS_NSAMPLES 1000

struct FitsChunk { float mn, mx; int n_nan, n_inf; };
struct FitsChannel { float vmin32; int divide; double range; float cmax; int pad; };
struct FitsParams { float fill; int all_nan; FitsChannel ch[3]; };

__device__ __forceinline__ float fits_load(const unsigned* raw, long long i, int big_endian) {
    unsigned u = raw[i];
    if (big_endian) u = __builtin_bswap32(u);
    return __uint_as_float(u);
}

// where pixel i (row-major within the tile) of a tile sits in `raw`
struct FitsLinear {                                     // the tile IS the buffer
    __device__ __forceinline__ long long operator()(long long i) const { return i; }
};
struct FitsRect {                                       // w columns from (x0, y0) of a plane of row stride NX
    long long origin, NX;
    int w;
    __device__ __forceinline__ long long operator()(long long i) const {
        const long long y = i / w;
        return origin + y * NX + (i - y * w);
    }
};

// statistics of chunk `chunk` of a tile of n pixels; vals gets the native-endian copy (row-major within the tile)
template <class Addr>
__device__ __forceinline__ void fits_stats_body(const unsigned* __restrict__ raw, const Addr addr, float* __restrict__ vals, long long n,
                                                int big_endian, int chunk, FitsChunk* __restrict__ chunks) {
    __shared__ float s_mn[256], s_mx[256];
    __shared__ int s_nan[256], s_inf[256];
    const int tid = threadIdx.x;
    const long long base = (long long)chunk * FITS_CHUNK;
    float mn = INFINITY, mx = -INFINITY;
    int nn = 0, ni = 0;
    for (int k = tid; k < FITS_CHUNK; k += 256) {
        const long long i = base + k;
        if (i >= n) break;
        const float v = fits_load(raw, addr(i), big_endian);
        vals[i] = v;
        if (v != v) { ++nn; continue; }
        if (isinf(v)) ++ni;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    s_mn[tid] = mn; s_mx[tid] = mx; s_nan[tid] = nn; s_inf[tid] = ni;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            s_mn[tid] = fminf(s_mn[tid], s_mn[tid + s]);
            s_mx[tid] = fmaxf(s_mx[tid], s_mx[tid + s]);
            s_nan[tid] += s_nan[tid + s];
            s_inf[tid] += s_inf[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) chunks[chunk] = {s_mn[0], s_mx[0], s_nan[0], s_inf[0]};
}

__global__ __launch_bounds__(256) void fits_stats_kernel(const unsigned* __restrict__ raw, float* __restrict__ vals, long long n,
                                                         int big_endian, FitsChunk* __restrict__ chunks) {
    fits_stats_body(raw, FitsLinear(), vals, n, big_endian, (int)blockIdx.x, chunks);
}

__device__ __forceinline__ double fits_block_sum(double v, double* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// one channel's value of a pixel after stretch + normalisation input (stretch_img then .astype(float32))
__device__ __forceinline__ float fits_stretch(float v, const FitsChannel& c) {
    double o = (double)(v - c.vmin32);                  // np.subtract(float32 array, python float) stays float32, then .astype(float64)
    if (c.divide) o = o / c.range;
    o = o < 0.0 ? 0.0 : o;                              // np.clip(out, 0, 1)
    o = o > 1.0 ? 1.0 : o;
    return (float)o;
}

// Sort, iterative fit and limits of the npix samples in s_samp[0 .. npix) (+inf in s_samp[npix .. 1024)): the part of
// ZScaleInterval.get_limits after the sampling, for ONE workgroup of 1024 threads; every thread passes the same npix, fill and
// dmax (the plane's maximum).  s_samp and s_red are the caller's LDS arrays of 1024 entries; the caller has synchronised after
// writing s_samp.  Shared by the tile chain and the mosaic overview.
__device__ __forceinline__ void fits_zscale_fit(float* s_samp, double* s_red, int npix, float fill, float dmax, double c0, double c1,
                                                double c2, FitsParams* __restrict__ params) {
    __shared__ unsigned char s_bad[1024], s_bad2[1024];
    const int tid = threadIdx.x;
    // ---- bitonic sort, ascending; the +inf padding ends up behind the npix samples ----------------------------------------
    for (int k = 2; k <= 1024; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int p = tid ^ j;
            if (p > tid) {
                const float a = s_samp[tid], b = s_samp[p];
                const bool up = (tid & k) == 0;
                if ((a > b) == up) { s_samp[tid] = b; s_samp[p] = a; }
            }
            __syncthreads();
        }
    // ---- ZScaleInterval.get_limits -------------------------------------------------------------------------------------------
    double slope = 0.0;
    int ngood = npix;
    if (npix > 0) {
        const int minpix = max(5, (int)(npix * 0.5));
        const int ngrow = max(1, (int)(npix * 0.01));
        const int back = ngrow / 2, fwd = (ngrow - 1) / 2;             // np.convolve(bad, ones(ngrow), 'same'): out[i] = OR bad[i - back .. i + fwd]
        int last = npix + 1;
        const bool in = tid < npix;
        const double x = (double)tid, y = in ? (double)s_samp[tid] : 0.0;
        s_bad[tid] = 0;
        __syncthreads();
        for (int it = 0; it < 5; ++it) {
            if (ngood >= last || ngood < minpix) break;
            const double w = (in && !s_bad[tid]) ? 1.0 : 0.0;
            // weighted least-squares line through the good samples (np.polyfit(x, samples, 1, w = good)), centred form
            const double sw = fits_block_sum(w, s_red, tid);
            const double xm = fits_block_sum(w * x, s_red, tid) / sw, ym = fits_block_sum(w * y, s_red, tid) / sw;
            const double sxx = fits_block_sum(w * (x - xm) * (x - xm), s_red, tid);
            const double sxy = fits_block_sum(w * (x - xm) * (y - ym), s_red, tid);
            slope = sxx > 0.0 ? sxy / sxx : 0.0;
            const double icpt = ym - slope * xm;
            const double flat = y - (slope * x + icpt);
            const double fm = fits_block_sum(w * flat, s_red, tid) / sw;
            const double var = fits_block_sum(w * (flat - fm) * (flat - fm), s_red, tid) / sw;
            const double thr = 2.5 * sqrt(var);
            if (in && (flat < -thr || flat > thr)) s_bad[tid] = 1;
            __syncthreads();
            unsigned char b = 0;
            if (in) {
                const int a0 = max(0, tid - back), a1 = min(npix - 1, tid + fwd);
                for (int k = a0; k <= a1; ++k) b |= s_bad[k];
            }
            s_bad2[tid] = b;
            __syncthreads();
            s_bad[tid] = s_bad2[tid];
            last = ngood;
            ngood = (int)fits_block_sum((in && !s_bad2[tid]) ? 1.0 : 0.0, s_red, tid);
        }
        if (tid == 0) {
            const float smin = s_samp[0], smax = s_samp[npix - 1];
            float median;                                               // np.median of a float32 array: float32
            if (npix & 1) median = s_samp[npix / 2];
            else median = (s_samp[npix / 2 - 1] + s_samp[npix / 2]) / 2.0f;
            const int center = (npix - 1) / 2;
            const double contrast[3] = {c0, c1, c2};
            for (int c = 0; c < 3; ++c) {
                // vmin / vmax are numpy float32 scalars (the sample ends) or float64 (the fitted limits): the type of their
                // difference -- float32 subtraction or float64 -- follows
                double vmin = (double)smin, vmax = (double)smax;
                bool vmin32 = true, vmax32 = true;
                if (ngood >= minpix) {
                    double sl = slope;
                    if (contrast[c] > 0.0) sl = sl / contrast[c];
                    const double lo = (double)median - (double)(center - 1) * sl, hi = (double)median + (double)(npix - center) * sl;
                    if (lo > vmin) { vmin = lo; vmin32 = false; }         // max(vmin, lo): the first argument wins a tie
                    if (hi < vmax) { vmax = hi; vmax32 = false; }
                }
                FitsChannel ch;
                ch.vmin32 = (float)vmin;
                ch.range = (vmin32 && vmax32) ? (double)(smax - smin) : vmax - vmin;
                ch.divide = ch.range != 0.0;
                ch.pad = 0;
                ch.cmax = 0.f;
                ch.cmax = fits_stretch(dmax, ch);                       // every step of the map is monotone: max(channel) = channel(max)
                params->ch[c] = ch;
            }
            params->fill = fill;
            params->all_nan = 0;
        }
    } else if (tid == 0) {                                                // no finite pixel at all (only +-inf): numpy's sort of an empty
        params->all_nan = 1;                                               // sample raises on the host; the device writes zeros
        params->fill = fill;
    }
}

// sampling, sort, iterative fit and limits of one tile: ONE workgroup of 1024 threads
__device__ __forceinline__ void fits_zscale_body(const float* __restrict__ vals, long long n, int nchunks,
                                                 const FitsChunk* __restrict__ chunks, double c0, double c1, double c2,
                                                 FitsParams* __restrict__ params) {
    __shared__ int s_prefix[FITS_MAX_CHUNKS + 1];
    __shared__ float s_samp[1024];
    __shared__ double s_red[1024];
    const int tid = threadIdx.x;
    // ---- global min / max / counts ------------------------------------------------------------------------------------
    float mn = INFINITY, mx = -INFINITY;
    int nn = 0;
    for (int k = tid; k < nchunks; k += 1024) {
        const FitsChunk c = chunks[k];
        mn = fminf(mn, c.mn); mx = fmaxf(mx, c.mx); nn += c.n_nan;
    }
    s_samp[tid] = mn;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) { if (tid < s) s_samp[tid] = fminf(s_samp[tid], s_samp[tid + s]); __syncthreads(); }
    const float fill = s_samp[0];                       // np.nanmin(out): +inf only when every pixel is NaN
    __syncthreads();
    s_samp[tid] = mx;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) { if (tid < s) s_samp[tid] = fmaxf(s_samp[tid], s_samp[tid + s]); __syncthreads(); }
    const float dmax = s_samp[0];
    __syncthreads();
    const long long total_nan = (long long)fits_block_sum((double)nn, s_red, tid);
    if (total_nan == n) {                               // nothing to scale: the host gets NaN everywhere (uint8 of NaN: 0)
        if (tid == 0) { params->all_nan = 1; params->fill = fill; }
        return;
    }
    const bool fill_finite = !isinf(fill);
    // ---- finite pixels per chunk, exclusive prefix ------------------------------------------------------------------------
    for (int k = tid; k < nchunks; k += 1024) {
        const long long left = n - (long long)k * FITS_CHUNK;
        const int size = left < FITS_CHUNK ? (int)left : FITS_CHUNK;
        s_prefix[k + 1] = size - chunks[k].n_inf - (fill_finite ? 0 : chunks[k].n_nan);
    }
    if (tid == 0) s_prefix[0] = 0;
    __syncthreads();
    if (tid == 0) for (int k = 0; k < nchunks; ++k) s_prefix[k + 1] += s_prefix[k];     // <= 4096 adds: microseconds
    __syncthreads();
    const long long nfinite = s_prefix[nchunks];
    int npix = 0, stride = 1;
    if (nfinite > 0) {
        stride = (int)fmax(1.0, (double)nfinite / (double)FITS_NSAMPLES);
        const long long avail = (nfinite + stride - 1) / stride;
        npix = avail < FITS_NSAMPLES ? (int)avail : FITS_NSAMPLES;
    }
    // ---- values[isfinite][::stride][:nsamples] ---------------------------------------------------------------------------
    float sv = INFINITY;
    if (tid < npix) {
        const long long rank = (long long)tid * stride;
        int lo = 0, hi = nchunks;                       // last chunk with prefix <= rank
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_prefix[mid] <= rank) lo = mid; else hi = mid; }
        int need = (int)(rank - s_prefix[lo]);
        const long long base = (long long)lo * FITS_CHUNK;
        const long long left = n - base;
        const int size = left < FITS_CHUNK ? (int)left : FITS_CHUNK;
        if (s_prefix[lo + 1] - s_prefix[lo] == size) {
            float v = vals[base + need];
            sv = v != v ? fill : v;
        } else {
            for (int k = 0; k < size; ++k) {
                float v = vals[base + k];
                if (v != v) v = fill;
                if (isinf(v)) continue;
                if (need-- == 0) { sv = v; break; }
            }
        }
    }
    s_samp[tid] = sv;
    __syncthreads();
    fits_zscale_fit(s_samp, s_red, npix, fill, dmax, c0, c1, c2, params);
}

// one channel's byte of a (NaN-filled) pixel value on the run.py path (the mosaic overview's pixel pass)
__device__ __forceinline__ unsigned char fits_byte(float v, const FitsChannel& c) {
    const float s = fits_stretch(v, c);
    const float q = rintf((s / c.cmax) * 255.f);                         // normalize_img (float32), gray2rgb: (c * 255).round()
    return (q >= 0.f && q <= 255.f) ? (unsigned char)q : (unsigned char)0;             // 0 / 0 (constant tile): NaN -> 0
}

// ---- T tiles of one plane: the tile is grid dimension y (stats, pixels) or x (zscale) ------------------------------------------
// mrcnn_fits_tile (include/mrcnn_hip.h): rectangle + where the tile's pixels / chunks start in the pools
__device__ __forceinline__ long long fits_tile_chunks(long long n) { return (n + FITS_CHUNK - 1) / FITS_CHUNK; }

__global__ __launch_bounds__(256) void fits_tiles_stats_kernel(const unsigned* __restrict__ plane, long long NX, int big_endian,
                                                               const mrcnn_fits_tile* __restrict__ tiles, float* __restrict__ vals,
                                                               FitsChunk* __restrict__ chunks) {
    const mrcnn_fits_tile t = tiles[blockIdx.y];
    const long long n = (long long)t.w * t.h;
    if ((long long)blockIdx.x >= fits_tile_chunks(n)) return;            // the grid is sized for the largest tile of the batch
    const FitsRect addr = {(long long)t.y0 * NX + t.x0, NX, t.w};
    fits_stats_body(plane, addr, vals + t.pixel_offset, n, big_endian, (int)blockIdx.x, chunks + t.chunk_offset);
}

extern "C" size_t mrcnn_fits_workspace(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    const long long n = (long long)H * W;
    const long long chunks = (n + FITS_CHUNK - 1) / FITS_CHUNK;
    return (size_t)n * sizeof(float) + (size_t)chunks * sizeof(FitsChunk) + 256;
}

// Host-side check of a tile table: every rectangle inside the plane and within the chunk limit, the pools laid out back to back
// in table order.  Fills the totals the launches and the workspace need.
struct FitsTilesLayout { long long pixels, chunks, max_pixels, max_chunks; };

static int fits_tiles_layout(const mrcnn_fits_tile* tiles, int T, int NY, int NX, FitsTilesLayout* out) {
    if (!tiles || T <= 0 || NY <= 0 || NX <= 0) return MRCNN_ERR_ARG;
    FitsTilesLayout l = {0, 0, 0, 0};
    for (int t = 0; t < T; ++t) {
        const mrcnn_fits_tile& r = tiles[t];
        if (r.w <= 0 || r.h <= 0 || r.x0 < 0 || r.y0 < 0 || (long long)r.x0 + r.w > NX || (long long)r.y0 + r.h > NY) return MRCNN_ERR_ARG;
        if (r.pixel_offset != l.pixels || r.chunk_offset != l.chunks) return MRCNN_ERR_ARG;
        const long long n = (long long)r.w * r.h;
        const long long c = (n + FITS_CHUNK - 1) / FITS_CHUNK;
        if (c > FITS_MAX_CHUNKS) return MRCNN_ERR_UNSUPPORTED;
        l.pixels += n;
        l.chunks += c;
        if (n > l.max_pixels) l.max_pixels = n;
        if (c > l.max_chunks) l.max_chunks = c;
    }
    if (T > 65535) return MRCNN_ERR_UNSUPPORTED;                          // grid dimension y
    *out = l;
    return MRCNN_OK;
}

extern "C" int mrcnn_fits_tiles_check(const mrcnn_fits_tile* tiles, int T, int NY, int NX) {
    FitsTilesLayout l;
    return fits_tiles_layout(tiles, T, NY, NX, &l);
}

extern "C" size_t mrcnn_fits_tiles_workspace(const mrcnn_fits_tile* tiles, int T, int NY, int NX) {
    FitsTilesLayout l;
    if (fits_tiles_layout(tiles, T, NY, NX, &l) != MRCNN_OK) return 0;
    return (size_t)l.pixels * sizeof(float) + (size_t)l.chunks * sizeof(FitsChunk) + (size_t)T * sizeof(FitsParams) + 256;
}

// a workspace of either size above: the native-endian values, the chunk table, the tiles' parameters (64-byte aligned)
struct FitsWorkspace { float* vals; FitsChunk* ch; FitsParams* params; };

static FitsWorkspace fits_carve(void* workspace, long long pixels, long long chunks) {
    FitsWorkspace w;
    w.vals = (float*)workspace;
    w.ch = (FitsChunk*)(w.vals + pixels);
    w.params = (FitsParams*)(((uintptr_t)(w.ch + chunks) + 63) & ~(uintptr_t)63);
    return w;
}

// ---- the chain and its entries: mrcnn_fits_to_image / mrcnn_fits_tiles_to_image (include/mrcnn_hip.h) -------------------------
// The host statement, per channel c of zscale contrast zc (caesar-mrcnn_amd/fits.py:read_fits):
//   c = out (float32, NaN-filled)
//   zscale:        c = float32(stretch_img(c, zc))                                   fits_zscale_* and fits_stretch above
//   biascontrast:  c = float32(clip((float64(c) - bias) * contrast + 0.5, 0, 1))     three separately rounded float64 operations
//   normalize, or an RGB output:  c = c / max(c)                                     float32
//   uint8 RGB: round(255 c)      float32 RGB: c * 255      gray: channel 0 as it is
// Launches: the statistics pass as above; with zscale its one workgroup, without it fits_minmax_kernel (a reduction of the chunk
// table: minimum = the NaN fill, maximum, NaN count -- no sampling, no sort, no fit); one pixel pass.  The channel maximum is
// not reduced over the pixels: every step of the map is monotone and correctly rounded, so it is the chain applied to the tile's
// maximum (contrast >= 0) or minimum (contrast < 0); a NaN at either end (inf * 0) makes numpy's max -- and the channel -- NaN.
// The thread that writes a tile's FitsParams (thread 0 of the zscale workgroup or of the reduction) finishes the three maxima.
// The pixel pass: a lane owns FOUR consecutive pixels, the group aligned in the POOL (pixel_offset + i a multiple of 4), so a
// tile that starts anywhere in the pools still loads one aligned float4 and stores 12 bytes (uint8 RGB: one dwordx3), 48 bytes
// (float32 RGB: three dwordx4) or 16 bytes (gray: one dwordx4) at their natural alignment; the partial groups at a tile's two
// ends, and every group when a base pointer is not 16-byte aligned, store pixel by pixel.  Channels of equal zscale contrast
// (all three without zscale) are computed once, as the host does.
struct FitsChainDev {
    int zscale, biascontrast, divide, out_kind;
    int src[3];                                          // channel c repeats channel src[c] <= c
    int vec;                                             // the pools' base pointers are 16-byte aligned
    double bias, contrast;
};

__device__ __forceinline__ float fits_biascontrast(float c, double bias, double contrast) {
#pragma clang fp contract(off)
    double o = (double)c - bias;                         // (the library is built with -ffp-contract=off as well)
    o = o * contrast;
    o = o + 0.5;
    o = (o != o) ? o : (o > 0.0 ? o : 0.0);              // np.clip(o, 0, 1): a NaN stays
    o = (o != o) ? o : (o < 1.0 ? o : 1.0);
    return (float)o;
}

// a channel's value of a (NaN-filled) pixel before the normalisation
__device__ __forceinline__ float fits_chain_value(float v, const FitsChannel& ch, const FitsChainDev& d) {
    float c = v;
    if (d.zscale) c = fits_stretch(v, ch);
    if (d.biascontrast) c = fits_biascontrast(c, d.bias, d.contrast);
    return c;
}

// The maxima of the whole chain, by the ONE thread that wrote *params: ch[c].cmax comes in as the channel's value at the tile's
// maximum before the bias / contrast stretch and goes out as the maximum of the finished channel (see the head of this part).
__device__ __forceinline__ void fits_chain_finish(FitsParams* __restrict__ params, const FitsChainDev& d) {
    if (params->all_nan || !d.biascontrast) return;
    for (int c = 0; c < 3; ++c) {
        const FitsChannel ch = params->ch[c];
        const float lo = fits_biascontrast(d.zscale ? fits_stretch(params->fill, ch) : params->fill, d.bias, d.contrast);
        float hi = fits_biascontrast(ch.cmax, d.bias, d.contrast);
        if (lo != lo || hi != hi) hi = NAN;
        else if (d.contrast < 0.0) hi = lo;
        params->ch[c].cmax = hi;
    }
}

// the reduction of one tile's chunk table that replaces the zscale workgroup: ONE workgroup of 256 threads
__device__ __forceinline__ void fits_minmax_body(long long n, int nchunks, const FitsChunk* __restrict__ chunks, const FitsChainDev& d,
                                                 FitsParams* __restrict__ params) {
    __shared__ float s_mn[256], s_mx[256];
    __shared__ int s_nan[256];
    const int tid = threadIdx.x;
    float mn = INFINITY, mx = -INFINITY;
    int nn = 0;                                          // <= 4096 * 1024 pixels
    for (int k = tid; k < nchunks; k += 256) {
        const FitsChunk c = chunks[k];
        mn = fminf(mn, c.mn); mx = fmaxf(mx, c.mx); nn += c.n_nan;
    }
    s_mn[tid] = mn; s_mx[tid] = mx; s_nan[tid] = nn;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            s_mn[tid] = fminf(s_mn[tid], s_mn[tid + s]);
            s_mx[tid] = fmaxf(s_mx[tid], s_mx[tid + s]);
            s_nan[tid] += s_nan[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        params->fill = s_mn[0];                          // np.nanmin(out)
        params->all_nan = (long long)s_nan[0] == n;
        FitsChannel ch;
        ch.vmin32 = 0.f; ch.divide = 0; ch.range = 0.0; ch.pad = 0;
        ch.cmax = s_mx[0];                               // no stretch: the channel is the tile
        for (int c = 0; c < 3; ++c) params->ch[c] = ch;
        fits_chain_finish(params, d);
    }
}

__global__ __launch_bounds__(256) void fits_minmax_kernel(long long n, int nchunks, const FitsChunk* __restrict__ chunks, const FitsChainDev d,
                                                          FitsParams* __restrict__ params) {
    fits_minmax_body(n, nchunks, chunks, d, params);
}

__global__ __launch_bounds__(256) void fits_tiles_minmax_kernel(const mrcnn_fits_tile* __restrict__ tiles, const FitsChunk* __restrict__ chunks,
                                                                const FitsChainDev d, FitsParams* __restrict__ params) {
    const mrcnn_fits_tile t = tiles[blockIdx.x];
    const long long n = (long long)t.w * t.h;
    fits_minmax_body(n, (int)fits_tile_chunks(n), chunks + t.chunk_offset, d, params + blockIdx.x);
}

// the zscale workgroup, then the maxima of the whole chain (thread 0 wrote the parameters it now reads)
__global__ __launch_bounds__(1024) void fits_zscale_kernel(const float* __restrict__ vals, long long n, int nchunks,
                                                           const FitsChunk* __restrict__ chunks, double c0, double c1, double c2,
                                                           const FitsChainDev d, FitsParams* __restrict__ params) {
    fits_zscale_body(vals, n, nchunks, chunks, c0, c1, c2, params);
    if (threadIdx.x == 0) fits_chain_finish(params, d);
}

__global__ __launch_bounds__(1024) void fits_tiles_zscale_kernel(const mrcnn_fits_tile* __restrict__ tiles, const float* __restrict__ vals,
                                                                 const FitsChunk* __restrict__ chunks, double c0, double c1, double c2,
                                                                 const FitsChainDev d, FitsParams* __restrict__ params) {
    const mrcnn_fits_tile t = tiles[blockIdx.x];
    const long long n = (long long)t.w * t.h;
    fits_zscale_body(vals + t.pixel_offset, n, (int)fits_tile_chunks(n), chunks + t.chunk_offset, c0, c1, c2, params + blockIdx.x);
    if (threadIdx.x == 0) fits_chain_finish(params + blockIdx.x, d);
}

typedef float fits_f32x4 __attribute__((ext_vector_type(4)));          // a native vector: stored as one dwordx4

// one pixel's channels after the whole chain (uint8 output: the rounded grey levels, still float); gray: o[0] alone
template <int OUT>
__device__ __forceinline__ void fits_image_pixel(float x, const FitsParams& p, const FitsChainDev& d, float* o) {
    if (x != x) x = p.fill;
#pragma unroll
    for (int c = 0; c < (OUT == 2 ? 1 : 3); ++c) {
        float r;
        if (p.all_nan) {
            r = NAN;                                     // (uint8: byte 0, as mrcnn_fits_to_rgb)
        } else if (d.src[c] == c) {
            r = fits_chain_value(x, p.ch[c], d);
            if (d.divide) r = r / p.ch[c].cmax;          // normalize_img (float32)
            if (OUT == 0) r = rintf(r * 255.f);          // gray2rgb: (c * 255).round()
            if (OUT == 1) r = r * 255.f;
        } else {
            r = d.src[c] == 0 ? o[0] : o[1];
        }
        o[c] = r;
    }
}

__device__ __forceinline__ unsigned fits_image_byte(float q) {
    return (q >= 0.f && q <= 255.f) ? (unsigned)q : 0u;                     // 0 / 0 (constant tile): NaN -> 0
}

// Pixels of one tile, four per thread.  vals / out: the POOLS; off: where the tile starts in them (in pixels).
// OUT: mrcnn_fits_chain.out_kind.
template <int OUT>
__device__ __forceinline__ void fits_image_body(const float* __restrict__ vals, long long off, long long n, const FitsParams& p,
                                                const FitsChainDev& d, void* __restrict__ out, long long group) {
    const long long g0 = (off & ~3ll) + group * 4;        // first pool pixel of this thread's group
    const long long lo = g0 > off ? g0 : off, hi = g0 + 4 < off + n ? g0 + 4 : off + n;
    if (lo >= hi) return;
    if (d.vec && hi - lo == 4) {
        const float4 q = *(const float4*)(vals + g0);
        float o[4][3];
        fits_image_pixel<OUT>(q.x, p, d, o[0]); fits_image_pixel<OUT>(q.y, p, d, o[1]);
        fits_image_pixel<OUT>(q.z, p, d, o[2]); fits_image_pixel<OUT>(q.w, p, d, o[3]);
        if (OUT == 0) {
            unsigned b[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) b[k] = fits_image_byte(o[k / 3][k % 3]);
            uint3 w;
            w.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            w.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            w.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
            *(uint3*)((unsigned char*)out + 3 * g0) = w;
        } else if (OUT == 1) {
            fits_f32x4* d4 = (fits_f32x4*)((float*)out + 3 * g0);         // 48 bytes: three 16-byte stores
            d4[0] = fits_f32x4{o[0][0], o[0][1], o[0][2], o[1][0]};
            d4[1] = fits_f32x4{o[1][1], o[1][2], o[2][0], o[2][1]};
            d4[2] = fits_f32x4{o[2][2], o[3][0], o[3][1], o[3][2]};
        } else {
            *(fits_f32x4*)((float*)out + g0) = fits_f32x4{o[0][0], o[1][0], o[2][0], o[3][0]};
        }
        return;
    }
    // the partial groups at a tile's two ends (every group of pools that are not 16-byte aligned): pixel by pixel
#pragma nounroll
    for (long long i = lo; i < hi; ++i) {
        float o[3];
        fits_image_pixel<OUT>(vals[i], p, d, o);
        if (OUT == 0) {
            unsigned char* dst = (unsigned char*)out + 3 * i;
            dst[0] = (unsigned char)fits_image_byte(o[0]); dst[1] = (unsigned char)fits_image_byte(o[1]);
            dst[2] = (unsigned char)fits_image_byte(o[2]);
        } else if (OUT == 1) {
            float* dst = (float*)out + 3 * i;
            dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
        } else {
            ((float*)out)[i] = o[0];
        }
    }
}

template <int OUT>
__global__ __launch_bounds__(256) void fits_image_kernel(const float* __restrict__ vals, long long n, const FitsParams* __restrict__ params,
                                                         const FitsChainDev d, void* __restrict__ out) {
    const FitsParams p = *params;                        // once, into registers: the stores below could alias *params
    fits_image_body<OUT>(vals, 0, n, p, d, out, (long long)blockIdx.x * 256 + threadIdx.x);
}

template <int OUT>
__global__ __launch_bounds__(256) void fits_tiles_image_kernel(const mrcnn_fits_tile* __restrict__ tiles, const float* __restrict__ vals,
                                                               const FitsParams* __restrict__ params, const FitsChainDev d,
                                                               void* __restrict__ out) {
    const mrcnn_fits_tile t = tiles[blockIdx.y];
    const FitsParams p = params[blockIdx.y];
    fits_image_body<OUT>(vals, t.pixel_offset, (long long)t.w * t.h, p, d, out, (long long)blockIdx.x * 256 + threadIdx.x);
}

// the descriptor as the kernels take it; the refusals of include/mrcnn_hip.h
static int fits_chain_dev(const mrcnn_fits_chain* c, FitsChainDev* d) {
    if (!c || c->out_kind < 0 || c->out_kind > 2) return MRCNN_ERR_ARG;
    if (c->out_kind == 0 && !c->zscale && !c->biascontrast) return MRCNN_ERR_UNSUPPORTED;      // nothing clips to [0, 1]: uint8 of any float
    d->zscale = c->zscale != 0;
    d->biascontrast = c->biascontrast != 0;
    d->divide = c->normalize != 0 || c->out_kind != 2;
    d->out_kind = c->out_kind;
    for (int k = 0; k < 3; ++k) {
        d->src[k] = k;
        for (int j = k - 1; j >= 0; --j)
            if (!d->zscale || c->zscale_contrasts[j] == c->zscale_contrasts[k]) d->src[k] = j;
    }
    d->vec = 0;
    d->bias = c->bias;
    d->contrast = c->contrast;
    return MRCNN_OK;
}

static size_t fits_image_pixel_bytes(int out_kind) { return out_kind == 0 ? 3 : out_kind == 1 ? 12 : 4; }

extern "C" int mrcnn_fits_image_check(const mrcnn_fits_chain* chain, int H, int W) {
    FitsChainDev d;
    const int rc = fits_chain_dev(chain, &d);
    if (rc != MRCNN_OK) return rc;
    if (H <= 0 || W <= 0) return MRCNN_ERR_ARG;
    if (((long long)H * W + FITS_CHUNK - 1) / FITS_CHUNK > FITS_MAX_CHUNKS) return MRCNN_ERR_UNSUPPORTED;
    return MRCNN_OK;
}

template <int OUT>
static void fits_image_launch(hipStream_t s, const float* vals, long long n, const FitsParams* params, const FitsChainDev& d, void* out) {
    hipLaunchKernelGGL(fits_image_kernel<OUT>, dim3((unsigned)cdiv64(cdiv64(n, 4), 256)), dim3(256), 0, s, vals, n, params, d, out);
}

template <int OUT>
static void fits_tiles_image_launch(hipStream_t s, const mrcnn_fits_tile* tiles, int T, long long max_pixels, const float* vals,
                                    const FitsParams* params, const FitsChainDev& d, void* out) {
    // a tile that starts 3 pixels into a group of four has ceil((n + 3) / 4) groups
    hipLaunchKernelGGL(fits_tiles_image_kernel<OUT>, dim3((unsigned)cdiv64(cdiv64(max_pixels + 3, 4), 256), (unsigned)T), dim3(256), 0, s,
                       tiles, vals, params, d, out);
}

extern "C" int mrcnn_fits_to_image(const void* raw, int big_endian, int H, int W, const mrcnn_fits_chain* chain, void* out, size_t out_bytes,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    FitsChainDev d;
    const int rc = mrcnn_fits_image_check(chain, H, W);
    if (rc != MRCNN_OK) return rc;
    fits_chain_dev(chain, &d);
    if (!raw || !out) return MRCNN_ERR_ARG;
    const long long n = (long long)H * W;
    const long long chunks = (n + FITS_CHUNK - 1) / FITS_CHUNK;
    if (out_bytes < (size_t)n * fits_image_pixel_bytes(d.out_kind)) return MRCNN_ERR_ARG;
    if (!workspace || workspace_bytes < mrcnn_fits_workspace(H, W)) return MRCNN_ERR_WORKSPACE;
    const FitsWorkspace w = fits_carve(workspace, n, chunks);
    d.vec = (((uintptr_t)workspace | (uintptr_t)out) & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fits_stats_kernel, dim3((unsigned)chunks), dim3(256), 0, s, (const unsigned*)raw, w.vals, n, big_endian, w.ch);
    if (d.zscale)
        hipLaunchKernelGGL(fits_zscale_kernel, dim3(1), dim3(1024), 0, s, (const float*)w.vals, n, (int)chunks, (const FitsChunk*)w.ch,
                           chain->zscale_contrasts[0], chain->zscale_contrasts[1], chain->zscale_contrasts[2], d, w.params);
    else
        hipLaunchKernelGGL(fits_minmax_kernel, dim3(1), dim3(256), 0, s, n, (int)chunks, (const FitsChunk*)w.ch, d, w.params);
    if (d.out_kind == 0) fits_image_launch<0>(s, w.vals, n, w.params, d, out);
    else if (d.out_kind == 1) fits_image_launch<1>(s, w.vals, n, w.params, d, out);
    else fits_image_launch<2>(s, w.vals, n, w.params, d, out);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_fits_tiles_to_image(const void* plane, int big_endian, int NY, int NX, const mrcnn_fits_tile* tiles_host,
                                         const mrcnn_fits_tile* tiles_dev, int T, const mrcnn_fits_chain* chain, void* out,
                                         size_t out_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    FitsChainDev d;
    int rc = fits_chain_dev(chain, &d);
    if (rc != MRCNN_OK) return rc;
    if (!plane || !out || !tiles_dev) return MRCNN_ERR_ARG;
    FitsTilesLayout l;
    rc = fits_tiles_layout(tiles_host, T, NY, NX, &l);
    if (rc != MRCNN_OK) return rc;
    if (out_bytes < (size_t)l.pixels * fits_image_pixel_bytes(d.out_kind)) return MRCNN_ERR_ARG;
    if (!workspace || workspace_bytes < mrcnn_fits_tiles_workspace(tiles_host, T, NY, NX)) return MRCNN_ERR_WORKSPACE;
    const FitsWorkspace w = fits_carve(workspace, l.pixels, l.chunks);
    d.vec = (((uintptr_t)workspace | (uintptr_t)out) & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fits_tiles_stats_kernel, dim3((unsigned)l.max_chunks, (unsigned)T), dim3(256), 0, s, (const unsigned*)plane,
                       (long long)NX, big_endian, tiles_dev, w.vals, w.ch);
    if (d.zscale)
        hipLaunchKernelGGL(fits_tiles_zscale_kernel, dim3((unsigned)T), dim3(1024), 0, s, tiles_dev, (const float*)w.vals,
                           (const FitsChunk*)w.ch, chain->zscale_contrasts[0], chain->zscale_contrasts[1], chain->zscale_contrasts[2], d,
                           w.params);
    else
        hipLaunchKernelGGL(fits_tiles_minmax_kernel, dim3((unsigned)T), dim3(256), 0, s, tiles_dev, (const FitsChunk*)w.ch, d, w.params);
    if (d.out_kind == 0) fits_tiles_image_launch<0>(s, tiles_dev, T, l.max_pixels, w.vals, w.params, d, out);
    else if (d.out_kind == 1) fits_tiles_image_launch<1>(s, tiles_dev, T, l.max_pixels, w.vals, w.params, d, out);
    else fits_tiles_image_launch<2>(s, tiles_dev, T, l.max_pixels, w.vals, w.params, d, out);
    return mrcnn_launch_status();
}

// The run.py flags (zscale, / max, uint8 RGB) under their own names: the descriptor of that chain, then the entries above.
static mrcnn_fits_chain fits_rgb_chain(const double* zc) {
    return {1, 0, 1, 0, {zc[0], zc[1], zc[2]}, 0.5, 1.0};
}

extern "C" int mrcnn_fits_to_rgb(const void* raw, int big_endian, int H, int W, const double* zscale_contrasts, void* rgb, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!zscale_contrasts) return MRCNN_ERR_ARG;
    const mrcnn_fits_chain chain = fits_rgb_chain(zscale_contrasts);
    const size_t rgb_bytes = H > 0 && W > 0 ? (size_t)H * W * 3 : 0;
    return mrcnn_fits_to_image(raw, big_endian, H, W, &chain, rgb, rgb_bytes, workspace, workspace_bytes, stream);
}

extern "C" int mrcnn_fits_tiles_to_rgb(const void* plane, int big_endian, int NY, int NX, const mrcnn_fits_tile* tiles_host,
                                       const mrcnn_fits_tile* tiles_dev, int T, const double* zscale_contrasts, void* rgb, size_t rgb_bytes,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    if (!zscale_contrasts) return MRCNN_ERR_ARG;
    const mrcnn_fits_chain chain = fits_rgb_chain(zscale_contrasts);
    return mrcnn_fits_tiles_to_image(plane, big_endian, NY, NX, tiles_host, tiles_dev, T, &chain, rgb, rgb_bytes, workspace, workspace_bytes,
                                     stream);
}

// ---- the overview of a whole mosaic (include/mrcnn_hip.h: mrcnn_mosaic_overview) -----------------------------------------------
// G = one channel of the chain above on the WHOLE plane [ny, nx] with one contrast; O[Y, X] = max of G over the k x k block
// (partial at the right and lower edge); out = O in three channels.  Four launches, the plane read twice where it lies:
//   mosaic_stats_kernel    one wavefront per 1024-pixel chunk (16-byte loads, shuffles, no LDS): FitsChunk per chunk;
//   mosaic_scan_kernel     one workgroup per super-chunk of 1024 chunks: exclusive prefixes of the NaN and the infinity counts
//                          within the super-chunk (which of the two count as "not finite" depends on the plane's minimum, known
//                          only one level up) and the super-chunk's own FitsChunk;
//   mosaic_zscale_kernel   ONE workgroup: minimum / maximum / counts over <= 2048 super-chunks, their prefix in LDS, per sample a
//                          binary search of the super-chunk (LDS) and of the chunk inside it (10 loads), the sample read from the
//                          plane -- a chunk with pixels that are not finite is walked by a whole wavefront, 16 ballots -- then
//                          fits_zscale_fit;
//   mosaic_pixels_kernel   one workgroup per output row Y and run of output pixels: a thread owns one plane column of the block
//                          row (consecutive lanes = consecutive pixels of a plane row, whatever k), keeps the maximum of the
//                          NaN-filled VALUE down its k rows, LDS folds k columns, and one fits_byte per output pixel: the byte map
//                          is non-decreasing in the value, so the byte of the maximum is the maximum of the bytes.
// Integer sums and min / max only: bitwise the same from run to run.
#define MOSAIC_SUPER 1024                // chunks per super-chunk
#define MOSAIC_MAX_SUPERS 2048           // 2^31 - 1 pixels: 2097152 chunks
#define MOSAIC_MAX_PIXELS 0x7FFFFFFFll

__device__ __forceinline__ void mosaic_take(unsigned u, int big_endian, float& mn, float& mx, int& nn, int& ni) {
    if (big_endian) u = __builtin_bswap32(u);
    const float v = __uint_as_float(u);
    if (v != v) { ++nn; return; }
    if (isinf(v)) ++ni;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
}

__global__ __launch_bounds__(256) void mosaic_stats_kernel(const unsigned* __restrict__ raw, long long n, long long nchunks, int big_endian,
                                                           int vec, FitsChunk* __restrict__ chunks) {
    const int lane = threadIdx.x & 63;
    const long long nwaves = (long long)gridDim.x * 4;
    for (long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); c < nchunks; c += nwaves) {       // wave-uniform
        const long long base = c * FITS_CHUNK;
        float mn = INFINITY, mx = -INFINITY;
        int nn = 0, ni = 0;
        if (vec && base + FITS_CHUNK <= n) {
            const uint4* p = (const uint4*)(raw + base);
            uint4 q[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = p[j * 64 + lane];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                mosaic_take(q[j].x, big_endian, mn, mx, nn, ni); mosaic_take(q[j].y, big_endian, mn, mx, nn, ni);
                mosaic_take(q[j].z, big_endian, mn, mx, nn, ni); mosaic_take(q[j].w, big_endian, mn, mx, nn, ni);
            }
        } else {
            for (int k = lane; k < FITS_CHUNK && base + k < n; k += 64) mosaic_take(raw[base + k], big_endian, mn, mx, nn, ni);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            nn += __shfl_xor(nn, o, 64); ni += __shfl_xor(ni, o, 64);
        }
        if (lane == 0) chunks[c] = {mn, mx, nn, ni};
    }
}

__global__ __launch_bounds__(1024) void mosaic_scan_kernel(const FitsChunk* __restrict__ chunks, long long nchunks, int2* __restrict__ pre,
                                                           FitsChunk* __restrict__ supers) {
    __shared__ int s_nan[16], s_inf[16];
    __shared__ float s_mn[16], s_mx[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long c = (long long)blockIdx.x * MOSAIC_SUPER + tid;
    FitsChunk ch = {INFINITY, -INFINITY, 0, 0};
    if (c < nchunks) ch = chunks[c];
    int in = ch.n_nan, ii = ch.n_inf;                    // inclusive scan within the wavefront
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(in, o, 64), b = __shfl_up(ii, o, 64);
        if (lane >= o) { in += a; ii += b; }
    }
    float mn = ch.mn, mx = ch.mx;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
    if (lane == 63) { s_nan[wv] = in; s_inf[wv] = ii; }
    if (lane == 0) { s_mn[wv] = mn; s_mx[wv] = mx; }
    __syncthreads();
    int bn = 0, bi = 0;
    for (int w = 0; w < wv; ++w) { bn += s_nan[w]; bi += s_inf[w]; }
    if (c < nchunks) pre[c] = make_int2(bn + in - ch.n_nan, bi + ii - ch.n_inf);
    if (tid == 0) {
        FitsChunk t = {INFINITY, -INFINITY, 0, 0};
        for (int w = 0; w < 16; ++w) { t.mn = fminf(t.mn, s_mn[w]); t.mx = fmaxf(t.mx, s_mx[w]); t.n_nan += s_nan[w]; t.n_inf += s_inf[w]; }
        supers[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(1024) void mosaic_zscale_kernel(const unsigned* __restrict__ raw, long long n, long long nchunks, int nsupers,
                                                             int big_endian, const FitsChunk* __restrict__ chunks,
                                                             const int2* __restrict__ pre, const FitsChunk* __restrict__ supers,
                                                             double contrast, FitsParams* __restrict__ params) {
    __shared__ long long s_sprefix[MOSAIC_MAX_SUPERS + 1];
    __shared__ float s_samp[1024];
    __shared__ double s_red[1024];
    __shared__ int s_walk_chunk[1024], s_walk_need[1024];
    const int tid = threadIdx.x;
    // ---- global min / max / counts ------------------------------------------------------------------------------------
    float mn = INFINITY, mx = -INFINITY;
    long long nn = 0;
    for (int k = tid; k < nsupers; k += 1024) {
        const FitsChunk c = supers[k];
        mn = fminf(mn, c.mn); mx = fmaxf(mx, c.mx); nn += c.n_nan;
    }
    s_samp[tid] = mn;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) { if (tid < s) s_samp[tid] = fminf(s_samp[tid], s_samp[tid + s]); __syncthreads(); }
    const float fill = s_samp[0];
    __syncthreads();
    s_samp[tid] = mx;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) { if (tid < s) s_samp[tid] = fmaxf(s_samp[tid], s_samp[tid + s]); __syncthreads(); }
    const float dmax = s_samp[0];
    __syncthreads();
    const long long total_nan = (long long)fits_block_sum((double)nn, s_red, tid);     // < 2^31: exact
    if (total_nan == n) {
        if (tid == 0) { params->all_nan = 1; params->fill = fill; }
        return;
    }
    const bool fill_finite = !isinf(fill);
    // ---- finite pixels per super-chunk, exclusive prefix --------------------------------------------------------------------
    const long long super_pixels = (long long)MOSAIC_SUPER * FITS_CHUNK;
    for (int k = tid; k < nsupers; k += 1024) {
        const long long left = n - (long long)k * super_pixels;
        const long long size = left < super_pixels ? left : super_pixels;
        s_sprefix[k + 1] = size - supers[k].n_inf - (fill_finite ? 0 : supers[k].n_nan);
    }
    if (tid == 0) s_sprefix[0] = 0;
    __syncthreads();
    if (tid == 0) for (int k = 0; k < nsupers; ++k) s_sprefix[k + 1] += s_sprefix[k];   // <= 2048 adds
    __syncthreads();
    const long long nfinite = s_sprefix[nsupers];
    int npix = 0, stride = 1;
    if (nfinite > 0) {
        stride = (int)fmax(1.0, (double)nfinite / (double)FITS_NSAMPLES);
        const long long avail = (nfinite + stride - 1) / stride;
        npix = avail < FITS_NSAMPLES ? (int)avail : FITS_NSAMPLES;
    }
    // ---- values[isfinite][::stride][:nsamples]: the chunk of every sample's rank; the sample itself where the chunk is all finite
    float sv = INFINITY;
    int wc = -1, wn = 0;
    if (tid < npix) {
        const long long rank = (long long)tid * stride;
        int lo = 0, hi = nsupers;                       // last super-chunk with prefix <= rank
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_sprefix[mid] <= rank) lo = mid; else hi = mid; }
        const long long r2 = rank - s_sprefix[lo];
        const long long c0 = (long long)lo * MOSAIC_SUPER;
        const int nc = nchunks - c0 < MOSAIC_SUPER ? (int)(nchunks - c0) : MOSAIC_SUPER;
        // finite pixels before chunk j of the super-chunk: every chunk before another one is full
        int a = 0, b = nc;                              // last chunk with that count <= r2
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            const int2 p = pre[c0 + mid];
            if ((long long)mid * FITS_CHUNK - p.y - (fill_finite ? 0 : p.x) <= r2) a = mid; else b = mid;
        }
        const int2 p = pre[c0 + a];
        const int need = (int)(r2 - ((long long)a * FITS_CHUNK - p.y - (fill_finite ? 0 : p.x)));
        const long long c = c0 + a, base = c * FITS_CHUNK;
        const int size = n - base < FITS_CHUNK ? (int)(n - base) : FITS_CHUNK;
        const FitsChunk ch = chunks[c];
        if (size - ch.n_inf - (fill_finite ? 0 : ch.n_nan) == size) {
            if (need >= 0 && need < size) {
                const float v = fits_load(raw, base + need, big_endian);
                sv = v != v ? fill : v;
            }
        } else {
            wc = (int)c;
            wn = need;
        }
    }
    s_samp[tid] = sv;
    s_walk_chunk[tid] = wc;
    s_walk_need[tid] = wn;
    __syncthreads();
    // ---- a chunk with pixels that are not finite: one wavefront walks it, 64 pixels per ballot ------------------------------
    const int lane = tid & 63;
    for (int s = tid >> 6; s < npix; s += 16) {           // wave-uniform
        const int c = s_walk_chunk[s];
        if (c < 0) continue;
        int need = s_walk_need[s];
        const long long base = (long long)c * FITS_CHUNK;
        float v[16];
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const long long i = base + it * 64 + lane;
            float x = INFINITY;                           // past the plane: skipped like an infinity
            if (i < n) x = fits_load(raw, i, big_endian);
            v[it] = x != x ? fill : x;
        }
        bool found = false;
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const bool ok = !isinf(v[it]);
            const unsigned long long m = __ballot(ok);
            const int cnt = __popcll(m);
            if (!found) {
                if (need < cnt) {
                    if (ok && __popcll(m & ((1ull << lane) - 1ull)) == need) s_samp[s] = v[it];
                    found = true;
                } else {
                    need -= cnt;
                }
            }
        }
    }
    __syncthreads();
    fits_zscale_fit(s_samp, s_red, npix, fill, dmax, contrast, contrast, contrast, params);
}

__global__ __launch_bounds__(256) void mosaic_pixels_kernel(const unsigned* __restrict__ raw, int ny, int nx, int big_endian, int k, int w,
                                                            int nout, int nbx, const FitsParams* __restrict__ params,
                                                            unsigned char* __restrict__ out) {
    __shared__ float s_col[256];
    __shared__ unsigned char s_byte[256];
    const int tid = threadIdx.x;
    const int Y = blockIdx.x / nbx, X0 = (blockIdx.x % nbx) * nout;
    const int nq = min(nout, w - X0);                                     // output pixels of this workgroup
    unsigned char* o = out + ((long long)Y * w + X0) * 3;
    if (params->all_nan) {                                                 // (the same for every thread)
        for (int t = tid; t < 3 * nq; t += 256) o[t] = 0;
        return;
    }
    const float fill = params->fill;
    const long long y0 = (long long)Y * k, y1 = y0 + k < ny ? y0 + k : ny;
    const long long xs = (long long)X0 * k;
    const long long span = (long long)nout * k < nx - xs ? (long long)nout * k : nx - xs;
    float m = -INFINITY;
    for (long long cx = tid; cx < span; cx += 256) {                       // one trip unless k > 256 (then nout == 1)
        long long i = y0 * nx + xs + cx;
#pragma unroll 4
        for (long long y = y0; y < y1; ++y, i += nx) {
            float v = fits_load(raw, i, big_endian);
            if (v != v) v = fill;
            m = fmaxf(m, v);
        }
    }
    s_col[tid] = m;
    __syncthreads();
    if (tid < nq) {
        const int lo = nout == 1 ? 0 : tid * k, hi = nout == 1 ? 256 : lo + k;
        float r = -INFINITY;
        for (int j = lo; j < hi; ++j) r = fmaxf(r, s_col[j]);
        s_byte[tid] = fits_byte(r, params->ch[0]);
    }
    __syncthreads();
    for (int t = tid; t < 3 * nq; t += 256) o[t] = s_byte[t / 3];
}

struct MosaicLayout { long long n, chunks, supers; int h, w, nout, nbx; };

static int mosaic_layout(int ny, int nx, int shrink, double contrast, MosaicLayout* out) {
    if (ny <= 0 || nx <= 0 || shrink <= 0 || !(contrast == contrast) || isinf(contrast)) return MRCNN_ERR_ARG;
    MosaicLayout l;
    l.n = (long long)ny * nx;
    if (l.n > MOSAIC_MAX_PIXELS) return MRCNN_ERR_UNSUPPORTED;
    l.chunks = (l.n + FITS_CHUNK - 1) / FITS_CHUNK;
    l.supers = (l.chunks + MOSAIC_SUPER - 1) / MOSAIC_SUPER;
    l.h = (int)(((long long)ny + shrink - 1) / shrink);
    l.w = (int)(((long long)nx + shrink - 1) / shrink);
    l.nout = shrink <= 256 ? 256 / shrink : 1;
    l.nbx = (l.w + l.nout - 1) / l.nout;
    *out = l;
    return MRCNN_OK;
}

extern "C" int mrcnn_mosaic_overview_check(int ny, int nx, int shrink, double contrast) {
    MosaicLayout l;
    return mosaic_layout(ny, nx, shrink, contrast, &l);
}

extern "C" size_t mrcnn_mosaic_overview_workspace(int ny, int nx) {
    MosaicLayout l;
    if (mosaic_layout(ny, nx, 1, 0.25, &l) != MRCNN_OK) return 0;
    return (size_t)l.chunks * (sizeof(FitsChunk) + sizeof(int2)) + (size_t)l.supers * sizeof(FitsChunk) + sizeof(FitsParams) + 256;
}

extern "C" int mrcnn_mosaic_overview(const void* plane, int big_endian, int ny, int nx, int shrink, double contrast, void* out,
                                     size_t out_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    MosaicLayout l;
    const int rc = mosaic_layout(ny, nx, shrink, contrast, &l);
    if (rc != MRCNN_OK) return rc;
    if (!plane || !out || ((uintptr_t)plane & 3) || out_bytes < (size_t)l.h * l.w * 3) return MRCNN_ERR_ARG;
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < mrcnn_mosaic_overview_workspace(ny, nx)) return MRCNN_ERR_WORKSPACE;
    FitsChunk* ch = (FitsChunk*)workspace;
    FitsChunk* sup = ch + l.chunks;
    int2* pre = (int2*)(sup + l.supers);
    FitsParams* params = (FitsParams*)(((uintptr_t)(pre + l.chunks) + 63) & ~(uintptr_t)63);
    hipStream_t s = (hipStream_t)stream;
    const unsigned* raw = (const unsigned*)plane;
    const long long stat_blocks = (l.chunks + 3) / 4;
    hipLaunchKernelGGL(mosaic_stats_kernel, dim3((unsigned)(stat_blocks < 4096 ? stat_blocks : 4096)), dim3(256), 0, s, raw, l.n, l.chunks,
                       big_endian, ((uintptr_t)plane & 15) == 0 ? 1 : 0, ch);
    hipLaunchKernelGGL(mosaic_scan_kernel, dim3((unsigned)l.supers), dim3(1024), 0, s, (const FitsChunk*)ch, l.chunks, pre, sup);
    hipLaunchKernelGGL(mosaic_zscale_kernel, dim3(1), dim3(1024), 0, s, raw, l.n, l.chunks, (int)l.supers, big_endian, (const FitsChunk*)ch,
                       (const int2*)pre, (const FitsChunk*)sup, contrast, params);
    hipLaunchKernelGGL(mosaic_pixels_kernel, dim3((unsigned)((long long)l.h * l.nbx)), dim3(256), 0, s, raw, ny, nx, big_endian, shrink, l.w,
                       l.nout, l.nbx, (const FitsParams*)params, (unsigned char*)out);
    return mrcnn_launch_status();
}
