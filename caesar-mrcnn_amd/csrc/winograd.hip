// Winograd F(2x2, 3x3) / F(4x4, 3x3) for the stride-1 "same" 3x3 convolutions of the mask head (float32):
// Y = A^T [(G g G^T) . (B^T d B)] A per 4 x 4 input tile / 2 x 2 output tile, summed over input channels -- 16 multiplications per 4
// outputs and channel pair instead of 36, i.e. 16 batched GEMMs [tiles x Cin] . [Cin x Cout] in the transform domain (2.25 x fewer
// MFMA flops than the direct form); with 6 x 6 / 4 x 4 tiles 36 GEMMs over a quarter of the tiles (4 x fewer).  Three passes per layer:
//   winograd_input_kernel    x [N, H, W, C]            -> V [16][T][C],   T = N (H/2)(W/2) tiles   (reads x once through L2, writes 4 x its size)
//   16 GEMMs                 V[xi] [T, C] . U[xi] [C, Cout] -> Mt [16][T][Cout]                     (conv_fwd_blds_kernel, batched over xi)
//   winograd_output_kernel   Mt -> out [N, H, W, Cout] with the convolution's epilogue (bias, frozen-BN affine, activation, z)
// (between two such layers of the training forward, winograd_chain_kernel: the output transform of the first and the input transform of
// the second in one pass, the activated tensor between them kept in LDS)
// plus winograd_weight_kernel U = G g G^T once per weight update.  For the 2 x 2 tile the transforms are exact additions / halvings
// in float32 (B^T, A^T have entries 0, +-1; G has 0, 1, +-1/2), so the result differs from the direct kernel by summation order
// only, and H and W must be even (mask head: 14 x 14); the 4 x 4 tile takes any extent (its last tiles hang over the edge).
#include "common.h"
#include <type_traits>
#include <string.h>

// ---- the 1-D transforms, m = OT outputs per tile and dimension (IT = OT + 2 inputs) -------------------------------------------
// OT = 2: B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1], G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1], A^T = [1 1 1 0; 0 1 -1 -1].
// OT = 4 (F(4x4, 3x3), interpolation points 0, +-1, +-2, inf): 36 multiplications per 16 outputs (4 x fewer than direct, 1.78 x
// fewer than OT = 2 -- 1.36 x on 14 x 14 maps, which it covers with 4 x 4 tiles of which the last row / column is half used);
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   G   = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
// its constants up to 8 cost about a decimal digit: ~7e-6 of the output range against ~5e-7 for OT = 2 (float32, K = 256).
template <int CV> struct WinoVec;
template <> struct WinoVec<4> { typedef f32x4 type; };
template <> struct WinoVec<2> { typedef float type __attribute__((ext_vector_type(2))); };

template <int OT, typename V> __device__ __forceinline__ void wino_bt(const V (&d)[OT + 2], V (&t)[OT + 2]) {
    if constexpr (OT == 2) {
        t[0] = d[0] - d[2];
        t[1] = d[1] + d[2];
        t[2] = d[2] - d[1];
        t[3] = d[1] - d[3];
    } else {
        const V a = d[4] - 4.f * d[2], b = d[3] - 4.f * d[1], c = d[4] - d[2], e = 2.f * (d[3] - d[1]);
        t[0] = 4.f * d[0] - 5.f * d[2] + d[4];
        t[1] = a + b;
        t[2] = a - b;
        t[3] = c + e;
        t[4] = c - e;
        t[5] = 4.f * d[1] - 5.f * d[3] + d[5];
    }
}
template <int OT, typename V> __device__ __forceinline__ void wino_at(const V (&m)[OT + 2], V (&y)[OT]) {
    if constexpr (OT == 2) {
        y[0] = m[0] + m[1] + m[2];
        y[1] = m[1] - m[2] - m[3];
    } else {
        const V p = m[1] + m[2], q = m[1] - m[2], r = m[3] + m[4], s = m[3] - m[4];
        y[0] = m[0] + p + r;
        y[1] = q + 2.f * s;
        y[2] = p + 4.f * r;
        y[3] = q + 8.f * s + m[5];
    }
}
// the adjoint of wino_at: A y
template <int OT, typename V> __device__ __forceinline__ void wino_a(const V (&y)[OT], V (&m)[OT + 2]) {
    if constexpr (OT == 2) {
        m[0] = y[0];
        m[1] = y[0] + y[1];
        m[2] = y[0] - y[1];
        m[3] = -y[1];
    } else {
        const V e = y[0] + y[2], o = y[1] + y[3], e4 = y[0] + 4.f * y[2], o4 = 2.f * y[1] + 8.f * y[3];
        m[0] = y[0];
        m[1] = e + o;
        m[2] = e - o;
        m[3] = e4 + o4;
        m[4] = e4 - o4;
        m[5] = y[3];
    }
}
template <int OT> __device__ __forceinline__ void wino_g(const float (&g)[3], float (&u)[OT + 2]) {
    if constexpr (OT == 2) {
        u[0] = g[0];
        u[1] = 0.5f * (g[0] + g[1] + g[2]);
        u[2] = 0.5f * (g[0] - g[1] + g[2]);
        u[3] = g[2];
    } else {
        const float e = g[0] + g[2];
        u[0] = 0.25f * g[0];
        u[1] = (-1.f / 6.f) * (e + g[1]);
        u[2] = (-1.f / 6.f) * (e - g[1]);
        const float f = (1.f / 24.f) * g[0] + (1.f / 6.f) * g[2], h = (1.f / 12.f) * g[1];
        u[3] = f + h;
        u[4] = f - h;
        u[5] = g[2];
    }
}
// the adjoint of wino_g: G^T u
template <int OT> __device__ __forceinline__ void wino_gt(const float (&u)[OT + 2], float (&w)[3]) {
    if constexpr (OT == 2) {
        w[0] = u[0] + 0.5f * (u[1] + u[2]);
        w[1] = 0.5f * (u[1] - u[2]);
        w[2] = 0.5f * (u[1] + u[2]) + u[3];
    } else {
        const float p = u[1] + u[2], q = u[3] + u[4];
        w[0] = 0.25f * u[0] - (1.f / 6.f) * p + (1.f / 24.f) * q;
        w[1] = (1.f / 6.f) * (u[2] - u[1]) + (1.f / 12.f) * (u[3] - u[4]);
        w[2] = (1.f / 6.f) * (q - p) + u[5];
    }
}

// A GROUP of tiles: th_n x tw_n tiles per map of OTH x OTW outputs each, the first one at output (oh0, ow0).  A uniform tiling is
// one group at (0, 0); a 14 x 14 map without overhang is four: 3 x 3 tiles of 4 x 4, 3 x 1 of 4 x 2 (columns 12..13), 1 x 3 of
// 2 x 4 (rows 12..13) and one 2 x 2 -- 484 multiplications per map and channel pair instead of 576.
// tile t of [0, N * th_n * tw_n) -> (n, th, tw), row-major
struct WinoGrp { int th_n, tw_n, oh0, ow0; };
struct WinoTile { int n, th, tw; };
__device__ __forceinline__ WinoTile wino_tile(long long t, int th_n, int tw_n) {
    WinoTile r;
    r.tw = (int)(t % tw_n);
    const long long q = t / tw_n;
    r.th = (int)(q % th_n);
    r.n = (int)(q / th_n);
    return r;
}

// B^T d B: one thread = one tile x CV channels.  V [ITH * ITW][Tp][C]
template <int OTH, int OTW, int CV>
__global__ __launch_bounds__(256) void winograd_input_kernel(const float* __restrict__ x, float* __restrict__ V, int N, int H, int W,
                                                             int C, long long T, long long Tp, const WinoGrp g) {
    typedef typename WinoVec<CV>::type vec;
    constexpr int ITH = OTH + 2, ITW = OTW + 2;
    const int cn = C / CV;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * cn) return;
    const long long t = i / cn;
    const int c = (int)(i - t * cn) * CV;
    const WinoTile q = wino_tile(t, g.th_n, g.tw_n);
    const int ih0 = g.oh0 + OTH * q.th - 1, iw0 = g.ow0 + OTW * q.tw - 1;
    vec tt[ITH][ITW];
#pragma unroll
    for (int s = 0; s < ITW; ++s) {              // columns of the tile: B^T applied down the rows
        vec col[ITH], o[ITH];
#pragma unroll
        for (int r = 0; r < ITH; ++r) {
            const int ih = ih0 + r, iw = iw0 + s;
            vec val = {};
            if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) val = *(const vec*)(x + (((long long)q.n * H + ih) * W + iw) * C + c);
            col[r] = val;
        }
        wino_bt<OTH>(col, o);
#pragma unroll
        for (int r = 0; r < ITH; ++r) tt[r][s] = o[r];
    }
#pragma unroll
    for (int r = 0; r < ITH; ++r) {              // then along each row
        vec v[ITW];
        wino_bt<OTW>(tt[r], v);
#pragma unroll
        for (int s = 0; s < ITW; ++s) *(vec*)(V + ((long long)(r * ITW + s) * Tp + t) * C + c) = v[s];
    }
}

// U[xi][ci][co] = (G_h g G_w^T)[xi] from the HWIO kernel g[3][3][ci][co]; one thread per (ci, co)
template <int OTH, int OTW>
__global__ __launch_bounds__(256) void winograd_weight_kernel(const float* __restrict__ g, float* __restrict__ U, int Cin, int Cout) {
    constexpr int ITH = OTH + 2, ITW = OTW + 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = (long long)Cin * Cout;
    if (i >= n) return;
    float t[ITH][3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        float col[3], o[ITH];
#pragma unroll
        for (int a = 0; a < 3; ++a) col[a] = g[(long long)(a * 3 + b) * n + i];
        wino_g<OTH>(col, o);
#pragma unroll
        for (int a = 0; a < ITH; ++a) t[a][b] = o[a];
    }
#pragma unroll
    for (int a = 0; a < ITH; ++a) {
        float u[ITW];
        wino_g<OTW>(t[a], u);
#pragma unroll
        for (int b = 0; b < ITW; ++b) U[(long long)(a * ITW + b) * n + i] = u[b];
    }
}

// A^T m A (OTH x OTW outputs of one tile) + epilogue: z = y + bias (stored when asked), out = act(scale z + shift)
// wino_output_tile: tile t x CV channels from c on
template <int OTH, int OTW, int CV>
__device__ __forceinline__ void wino_output_tile(const float* __restrict__ Mt, float* __restrict__ out, float* __restrict__ z,
                                                 const typename WinoVec<CV>::type bi, const typename WinoVec<CV>::type sc,
                                                 const typename WinoVec<CV>::type sh, int H, int W, int C, long long Tp, int act,
                                                 const WinoGrp& g, long long t, int c) {
    typedef typename WinoVec<CV>::type vec;
    constexpr int ITH = OTH + 2, ITW = OTW + 2;
    const WinoTile q = wino_tile(t, g.th_n, g.tw_n);
    vec s[OTH][ITW];
#pragma unroll
    for (int k = 0; k < ITW; ++k) {              // A^T down the rows of every column k
        vec col[ITH], o[OTH];
#pragma unroll
        for (int r = 0; r < ITH; ++r) col[r] = *(const vec*)(Mt + ((long long)(r * ITW + k) * Tp + t) * C + c);
        wino_at<OTH>(col, o);
#pragma unroll
        for (int a = 0; a < OTH; ++a) s[a][k] = o[a];
    }
#pragma unroll
    for (int a = 0; a < OTH; ++a) {
        vec y[OTW];
        wino_at<OTW>(s[a], y);
        const int oh = g.oh0 + OTH * q.th + a;
        if (oh >= H) continue;
#pragma unroll
        for (int b = 0; b < OTW; ++b) {
            const int ow = g.ow0 + OTW * q.tw + b;
            if (ow >= W) continue;
            const long long addr = (((long long)q.n * H + oh) * W + ow) * C + c;
            vec zv, o;
#pragma unroll
            for (int e = 0; e < CV; ++e) {
                zv[e] = y[b][e] + bi[e];
                float v = sc[e] * zv[e] + sh[e];
                if (act == MRCNN_ACT_RELU) v = fmaxf(v, 0.f);
                o[e] = v;
            }
            if (z) *(vec*)(z + addr) = zv;
            *(vec*)(out + addr) = o;
        }
    }
}

template <int OTH, int OTW, int CV>
__global__ __launch_bounds__(256) void winograd_output_kernel(const float* __restrict__ Mt, float* __restrict__ out, float* __restrict__ z,
                                                              const float* __restrict__ bias, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, int N, int H, int W, int C, long long T,
                                                              long long Tp, int act, const WinoGrp g) {
    typedef typename WinoVec<CV>::type vec;
    const int cn = C / CV;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * cn) return;
    const long long t = i / cn;
    const int c = (int)(i - t * cn) * CV;
    vec bi = {}, sc, sh = {};
#pragma unroll
    for (int e = 0; e < CV; ++e) sc[e] = 1.f;
    if (bias) bi = *(const vec*)(bias + c);
    if (scale) { sc = *(const vec*)(scale + c); sh = *(const vec*)(shift + c); }
    wino_output_tile<OTH, OTW, CV>(Mt, out, z, bi, sc, sh, H, W, C, Tp, act, g, t, c);
}

// wino_buffer_load: CV floats at base + lane offset + uniform offset (bytes) -- ONE address register per lane for all the
// (OTH + 2)(OTW + 2) matrices of a tile (as 64-bit addresses they take 72 registers of a 6 x 6 tile's budget)
template <int CV>
__device__ __forceinline__ typename WinoVec<CV>::type wino_buffer_load(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
    typename WinoVec<CV>::type r;
    if constexpr (CV == 2) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)voff, (int)soff, 0);
        r[0] = __uint_as_float(v[0]); r[1] = __uint_as_float(v[1]);
    } else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, (int)soff, 0);
        r[0] = __uint_as_float(v[0]); r[1] = __uint_as_float(v[1]); r[2] = __uint_as_float(v[2]); r[3] = __uint_as_float(v[3]);
    }
    return r;
}
// its store twin (two floats)
__device__ __forceinline__ void wino_buffer_store2(const WinoVec<2>::type v, __amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    u32x2 d;
    d[0] = __float_as_uint(v[0]); d[1] = __float_as_uint(v[1]);
    __builtin_amdgcn_raw_buffer_store_b64(d, rsrc, (int)voff, (int)soff, 0);
}

// ---- the forward chain: output transform + epilogue of layer l and input transform of layer l + 1 in one pass ------------------
// Mixed tiling only (H, W = 2 mod 4: a x b tiles of 4 x 4, a of 4 x 2, b of 2 x 4, one 2 x 2).  A workgroup owns ONE map and CS of its
// channels: lane = channel pair (L = CS / 2 lanes), 256 / L tiles in flight.  Phase 1 walks the map's tiles of all four groups --
// wino_output_tile's arithmetic, operation for operation, with all of a tile's transform-domain values requested before the first
// addition --, stores z when asked and leaves the activated H x W x CS map in LDS; phase 2 cuts the next layer's input tiles from
// it (zero halo) and writes B^T d B as winograd_input_kernel does.  The activated output never reaches memory.  Mt and V hold
// the four groups end to end, each [nb][Tp][C] (the same offsets: the next layer's Cin is this layer's Cout).
struct WinoChainGeo {
    int a, b;                      // H / 4, W / 4
    unsigned tp[4];                // rows per transform-domain matrix of each group
    long long off[4];              // first float of each group in Mt / V
};

template <int OTH, int OTW>
__device__ __forceinline__ void wino_chain_out_tile(__amdgpu_buffer_rsrc_t rsrc, unsigned mstride, unsigned t, int oh0, int ow0, int c,
                                                    int cl, const WinoVec<2>::type bi, const WinoVec<2>::type sc,
                                                    const WinoVec<2>::type sh, int act, float* __restrict__ z, float* map, int W,
                                                    int C, int CS) {
    typedef WinoVec<2>::type vec;
    constexpr int ITH = OTH + 2, ITW = OTW + 2;
    vec m[ITH][ITW];
    const unsigned moff = (t * (unsigned)C + (unsigned)c) * 4u;
#pragma unroll
    for (int r = 0; r < ITH; ++r)
#pragma unroll
        for (int k = 0; k < ITW; ++k) m[r][k] = wino_buffer_load<2>(rsrc, moff, (unsigned)(r * ITW + k) * mstride);
    vec s[OTH][ITW];
#pragma unroll
    for (int k = 0; k < ITW; ++k) {              // A^T down the rows of every column k
        vec col[ITH], o[OTH];
#pragma unroll
        for (int r = 0; r < ITH; ++r) col[r] = m[r][k];
        wino_at<OTH>(col, o);
#pragma unroll
        for (int a = 0; a < OTH; ++a) s[a][k] = o[a];
    }
#pragma unroll
    for (int a = 0; a < OTH; ++a) {
        vec y[OTW];
        wino_at<OTW>(s[a], y);
#pragma unroll
        for (int b = 0; b < OTW; ++b) {           // the mixed tiling has no overhang: every output lies inside the map
            const int pix = (oh0 + a) * W + ow0 + b;
            vec zv, o;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                zv[e] = y[b][e] + bi[e];
                float v = sc[e] * zv[e] + sh[e];
                if (act == MRCNN_ACT_RELU) v = fmaxf(v, 0.f);
                o[e] = v;
            }
            if (z) *(vec*)(z + (unsigned)(pix * C + c)) = zv;      // z: this map's
            *(vec*)(map + pix * CS + cl) = o;
        }
    }
}

template <int OTH, int OTW>
__device__ __forceinline__ void wino_chain_in_tile(const float* map, float* __restrict__ Vg, long long Tp, unsigned t, int oh0, int ow0, int c,
                                                   int cl, int H, int W, int C, int CS) {
    typedef WinoVec<2>::type vec;
    constexpr int ITH = OTH + 2, ITW = OTW + 2;
    const int ih0 = oh0 - 1, iw0 = ow0 - 1;
    vec tt[ITH][ITW];
#pragma unroll
    for (int s = 0; s < ITW; ++s) {              // columns of the tile: B^T applied down the rows
        vec col[ITH], o[ITH];
#pragma unroll
        for (int r = 0; r < ITH; ++r) {
            const int ih = ih0 + r, iw = iw0 + s;
            vec val = {};
            if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) val = *(const vec*)(map + (ih * W + iw) * CS + cl);
            col[r] = val;
        }
        wino_bt<OTH>(col, o);
#pragma unroll
        for (int r = 0; r < ITH; ++r) tt[r][s] = o[r];
    }
#pragma unroll
    for (int r = 0; r < ITH; ++r) {              // then along each row
        vec v[ITW];
        wino_bt<OTW>(tt[r], v);
#pragma unroll
        for (int s = 0; s < ITW; ++s) *(vec*)(Vg + ((long long)(r * ITW + s) * Tp + t) * C + c) = v[s];
    }
}

__global__ __launch_bounds__(256, 3) void winograd_chain_kernel(const float* __restrict__ Mt, float* __restrict__ z, const float* __restrict__ bias,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             float* __restrict__ V, int H, int W, int C, int act, int lg,
                                                             const WinoChainGeo geo) {
    typedef WinoVec<2>::type vec;
    extern __shared__ __attribute__((aligned(16))) float wino_chain_map[];     // [H][W][CS]
    const int L = 1 << lg, CS = 2 << lg, slots = 256 >> lg;
    const int slices = C / CS;
    const int n = (int)(blockIdx.x / (unsigned)slices), slice = (int)(blockIdx.x - (unsigned)n * slices);
    const int slot = threadIdx.x >> lg, cl = (threadIdx.x & (L - 1)) * 2;
    const int c = slice * CS + cl;
    const int a = geo.a, b = geo.b, n0 = a * b, per_map = n0 + a + b + 1;
    vec bi = {}, sc, sh = {};
    sc[0] = sc[1] = 1.f;
    if (bias) bi = *(const vec*)(bias + c);
    if (scale) { sc = *(const vec*)(scale + c); sh = *(const vec*)(shift + c); }
    // one descriptor per group, made where the base is plainly uniform (the host checks that every group fits 4 GiB)
    const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc((void*)(Mt + geo.off[0]), 0, 0xFFFFFFF0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc((void*)(Mt + geo.off[1]), 0, 0xFFFFFFF0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc((void*)(Mt + geo.off[2]), 0, 0xFFFFFFF0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t r3 = __builtin_amdgcn_make_buffer_rsrc((void*)(Mt + geo.off[3]), 0, 0xFFFFFFF0u, 0x00020000);
    const unsigned cb = (unsigned)C * 4u;
    float* zn = z ? z + (long long)n * H * W * C : nullptr;     // a map of <= 2048 pixels: 32-bit offsets inside it
    for (int it = slot; it < per_map; it += slots) {
        if (it < n0) {
            const int th = it / b, tw = it - th * b;
            wino_chain_out_tile<4, 4>(r0, geo.tp[0] * cb, (unsigned)n * n0 + it, 4 * th, 4 * tw, c, cl, bi, sc, sh, act, zn, wino_chain_map, W, C, CS);
        } else if (it < n0 + a) {
            const int th = it - n0;
            wino_chain_out_tile<4, 2>(r1, geo.tp[1] * cb, (unsigned)n * a + th, 4 * th, W - 2, c, cl, bi, sc, sh, act, zn, wino_chain_map, W, C, CS);
        } else if (it < n0 + a + b) {
            const int tw = it - n0 - a;
            wino_chain_out_tile<2, 4>(r2, geo.tp[2] * cb, (unsigned)n * b + tw, H - 2, 4 * tw, c, cl, bi, sc, sh, act, zn, wino_chain_map, W, C, CS);
        } else {
            wino_chain_out_tile<2, 2>(r3, geo.tp[3] * cb, (unsigned)n, H - 2, W - 2, c, cl, bi, sc, sh, act, zn, wino_chain_map, W, C, CS);
        }
    }
    __syncthreads();
    for (int it = slot; it < per_map; it += slots) {
        if (it < n0) {
            const int th = it / b, tw = it - th * b;
            wino_chain_in_tile<4, 4>(wino_chain_map, V + geo.off[0], geo.tp[0], (unsigned)n * n0 + it, 4 * th, 4 * tw, c, cl, H, W, C, CS);
        } else if (it < n0 + a) {
            const int th = it - n0;
            wino_chain_in_tile<4, 2>(wino_chain_map, V + geo.off[1], geo.tp[1], (unsigned)n * a + th, 4 * th, W - 2, c, cl, H, W, C, CS);
        } else if (it < n0 + a + b) {
            const int tw = it - n0 - a;
            wino_chain_in_tile<2, 4>(wino_chain_map, V + geo.off[2], geo.tp[2], (unsigned)n * b + tw, H - 2, 4 * tw, c, cl, H, W, C, CS);
        } else {
            wino_chain_in_tile<2, 2>(wino_chain_map, V + geo.off[3], geo.tp[3], (unsigned)n, H - 2, W - 2, c, cl, H, W, C, CS);
        }
    }
}

// The output transform of a DATA gradient together with the epilogue backward of the layer below (what mrcnn_conv2d_dgrad_ep does
// for the direct kernel): y = A^T m A is d(loss)/d(activated output of the layer below);
//   g = y * act'(out_below);  dz = g * scale_below -> stored;  channel sums of g, g (z_below - mean) rstd and dz.
// A persistent grid (a few workgroups per CU) walks the tiles: lane = CV-channel group (C / CV of them, a power of two <= 256),
// R = 256 / (C / CV) tiles in flight per workgroup, tiles blockIdx.x * R + rsub, + gridDim.x * R, ...  Everything a tile reads --
// its (OTH + 2)(OTW + 2) transform-domain values AND the z (or activated output) of the layer below under its outputs -- is
// requested before the first addition, so a tile costs one memory round trip, like the forward output transform.  Channel sums
// stay in registers over the walk, meet in LDS in fixed order and leave as ONE row of partials [3][C] per workgroup (plain
// stores); winograd_bwd_sums_kernel adds the rows of all groups of a layer up, in fixed order, once per layer.
// MASK: 0 no activation below, 1 ReLU mask recomputed from z (fwd_shift), 2 ReLU mask from the activated output
template <int OTH, int OTW, int CV, int MASK>
__global__ __launch_bounds__(256) void winograd_output_bwd_kernel(const float* __restrict__ Mt, float* __restrict__ dz_out,
                                                                  const float* __restrict__ below_out, const float* __restrict__ below_z,
                                                                  const float* __restrict__ scale, const float* __restrict__ mean,
                                                                  const float* __restrict__ rstd, const float* __restrict__ fwd_shift,
                                                                  float* __restrict__ partials, int want_dg, int H, int W, int C, unsigned T,
                                                                  long long Tp, int lg, const WinoGrp g, const FastDiv d_th,
                                                                  const FastDiv d_tw) {
    typedef typename WinoVec<CV>::type vec;
    constexpr int ITH = OTH + 2, ITW = OTW + 2;
    __shared__ float sacc[3 * 4 * 256];                         // [3][R][C]
    const int L = 1 << lg, R = 256 >> lg;                       // L = C / CV lanes, R tiles in flight
    const int rsub = threadIdx.x >> lg, lane = threadIdx.x & (L - 1);
    const int c = lane * CV;
    vec sc, mu = {}, rs = {}, fsh = {};
#pragma unroll
    for (int e = 0; e < CV; ++e) sc[e] = 1.f;
    if (scale) sc = *(const vec*)(scale + c);
    if (want_dg) { mu = *(const vec*)(mean + c); rs = *(const vec*)(rstd + c); }
    // MASK 1: out > 0 <=> scale * z + shift > 0, the very expression (operation for operation, no contraction) the forward
    // epilogue fed to max(., 0) -- so the activated output of the layer below is not read at all, same bits
    if (MASK == 1) fsh = *(const vec*)(fwd_shift + c);
    const bool need_z = MASK == 1 || want_dg;
    vec a_db = {}, a_dg = {}, a_bias = {};
    const unsigned step = gridDim.x * (unsigned)R;
    const __amdgpu_buffer_rsrc_t rsrc_m = __builtin_amdgcn_make_buffer_rsrc((void*)Mt, 0, 0xFFFFFFF0u, 0x00020000);
    const unsigned mstride = (unsigned)Tp * (unsigned)C * 4u;   // bytes per transform-domain matrix (the host checks that all fit 4 GiB)
    for (unsigned t = blockIdx.x * (unsigned)R + rsub; t < T; t += step) {
        const unsigned q = fast_div(t, d_tw), n = fast_div(q, d_th);
        const int tw = (int)(t - q * (unsigned)g.tw_n), th = (int)(q - n * (unsigned)g.th_n);
        const int oh0 = g.oh0 + OTH * th, ow0 = g.ow0 + OTW * tw;
        // all the tile's loads first: outputs past the map's edge (uniform 4 x 4 tiling) read the last row / column, unused
        // (addresses = a uniform base + a 32-bit byte offset per lane: one register per stream instead of two per load)
        vec m[ITH][ITW], zz[OTH][OTW], oo[OTH][OTW];
        const unsigned moff = (t * (unsigned)C + c) * 4u;
#pragma unroll
        for (int r = 0; r < ITH; ++r)
#pragma unroll
            for (int k = 0; k < ITW; ++k)
                m[r][k] = wino_buffer_load<CV>(rsrc_m, moff, (unsigned)(r * ITW + k) * mstride);
        // byte offsets of the tile's outputs, clamped to the map
        const unsigned base = (((n * (unsigned)H + oh0) * W + ow0) * C + c) * 4u;
        unsigned roff[OTH], coff[OTW];
#pragma unroll
        for (int a = 0; a < OTH; ++a) roff[a] = base + (unsigned)(min(a, H - 1 - oh0) * W * C) * 4u;
#pragma unroll
        for (int b = 0; b < OTW; ++b) coff[b] = (unsigned)(min(b, W - 1 - ow0) * C) * 4u;
        if (need_z) {
#pragma unroll
            for (int a = 0; a < OTH; ++a)
#pragma unroll
                for (int b = 0; b < OTW; ++b) zz[a][b] = *(const vec*)((const char*)below_z + (roff[a] + coff[b]));
        } else {
#pragma unroll
            for (int a = 0; a < OTH; ++a)
#pragma unroll
                for (int b = 0; b < OTW; ++b) zz[a][b] = vec{};
        }
        if (MASK == 2) {
#pragma unroll
            for (int a = 0; a < OTH; ++a)
#pragma unroll
                for (int b = 0; b < OTW; ++b) oo[a][b] = *(const vec*)((const char*)below_out + (roff[a] + coff[b]));
        }
        vec s[OTH][ITW];
#pragma unroll
        for (int k = 0; k < ITW; ++k) {              // A^T down the rows of every column k
            vec col[ITH], o[OTH];
#pragma unroll
            for (int r = 0; r < ITH; ++r) col[r] = m[r][k];
            wino_at<OTH>(col, o);
#pragma unroll
            for (int a = 0; a < OTH; ++a) s[a][k] = o[a];
        }
#pragma unroll
        for (int a = 0; a < OTH; ++a) {
            vec y[OTW];
            wino_at<OTW>(s[a], y);
#pragma unroll
            for (int b = 0; b < OTW; ++b) {
                const bool inside = oh0 + a < H && ow0 + b < W;     // past the edge: nothing stored, zeros into the sums
                vec gg = y[b], dz;
                if (MASK == 1) {
#pragma unroll
                    for (int e = 0; e < CV; ++e) {
                        const float v = sc[e] * zz[a][b][e] + fsh[e];
                        gg[e] = v > 0.f ? gg[e] : 0.f;
                    }
                } else if (MASK == 2) {
#pragma unroll
                    for (int e = 0; e < CV; ++e) gg[e] = oo[a][b][e] > 0.f ? gg[e] : 0.f;
                }
#pragma unroll
                for (int e = 0; e < CV; ++e) {
                    gg[e] = inside ? gg[e] : 0.f;
                    dz[e] = gg[e] * sc[e];
                }
                if (inside) *(vec*)((char*)dz_out + (roff[a] + coff[b])) = dz;
                if (want_dg) {
#pragma unroll
                    for (int e = 0; e < CV; ++e) a_dg[e] += gg[e] * (zz[a][b][e] - mu[e]) * rs[e];
                }
#pragma unroll
                for (int e = 0; e < CV; ++e) { a_db[e] += gg[e]; a_bias[e] += dz[e]; }
            }
        }
    }
    if (!partials) return;
#pragma unroll
    for (int e = 0; e < CV; ++e) {
        sacc[(0 * R + rsub) * C + c + e] = a_db[e];
        sacc[(1 * R + rsub) * C + c + e] = a_dg[e];
        sacc[(2 * R + rsub) * C + c + e] = a_bias[e];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < 3 * C; j += 256) {
        const int k = j / C, cc = j - k * C;
        float v = sacc[k * R * C + cc];
        for (int r = 1; r < R; ++r) v += sacc[(k * R + r) * C + cc];
        partials[(long long)blockIdx.x * 3 * C + j] = v;
    }
}

// sums over the rows of partials [rows][3][C] (the workgroups of every group of a layer), added to dbeta / dgamma / dbias: a
// workgroup = 16 columns x 64 row slices, slice s takes rows s, s + 64, ...; the slices meet in LDS and are added in order, so
// the result does not depend on timing.  One atomic per column (the buffers may be accumulated into from elsewhere).
#define WINO_SUMS_COLS 16
#define WINO_SUMS_SLICES 64
__global__ __launch_bounds__(WINO_SUMS_COLS * WINO_SUMS_SLICES) void winograd_bwd_sums_kernel(const float* __restrict__ partials, int rows,
                                                                                              int C, float* dgamma, float* dbeta,
                                                                                              float* dbias) {
    __shared__ float sm[WINO_SUMS_SLICES][WINO_SUMS_COLS];
    const int col = threadIdx.x % WINO_SUMS_COLS, slice = threadIdx.x / WINO_SUMS_COLS;
    const int j = blockIdx.x * WINO_SUMS_COLS + col;
    const int k = j / C;
    float* dst = k == 0 ? dbeta : k == 1 ? dgamma : k == 2 ? dbias : nullptr;      // k == 3: past the last column
    float v = 0.f;
    if (dst) {
#pragma unroll 8
        for (int r = slice; r < rows; r += WINO_SUMS_SLICES) v += partials[(long long)r * 3 * C + j];
    }
    sm[slice][col] = v;
    __syncthreads();
    if (slice == 0 && dst) {
        for (int s = 1; s < WINO_SUMS_SLICES; ++s) v += sm[s][col];
        atomicAdd(&dst[j - k * C], v);
    }
}

// ---- the backward chain: the data gradient's output transform + epilogue backward of the layer below, and BOTH transforms of the
// resulting dz -- the input transform for the next data gradient and the weight gradient's A dz A^T -- in one pass ----------------
// winograd_chain_kernel's plan (mixed tiling, a workgroup = one map x CS channels, lane = channel pair).  Phase 1 is
// winograd_output_bwd_kernel<.., MASK = 1>'s arithmetic, operation for operation, on the map's tiles of all four groups; dz stays in
// LDS [H][W][CS] (and is stored when dz_out is given).  Phase 2 cuts both kinds of tiles from it: V = B^T dz B (zero halo) as
// winograd_input_kernel writes it and dM = A dz A^T as winograd_dy_kernel does, four groups end to end at WinoChainGeo's offsets.
// The channel sums stay in registers over both phases, meet in the map's LDS (free by then) in slot order and leave as the
// workgroup's CS columns of row n of partials [N][3][C]: plain stores, every element written by exactly one workgroup, so
// winograd_bwd_sums_kernel adds the N rows up as it does the per-workgroup rows of the separate launches.
template <int OTH, int OTW, bool DZ>
__device__ __forceinline__ void wino_bwd_chain_out_tile(__amdgpu_buffer_rsrc_t rsrc, unsigned mstride, unsigned t, int oh0, int ow0, int c,
                                                        int cl, __amdgpu_buffer_rsrc_t rz, __amdgpu_buffer_rsrc_t rdz,
                                                        const WinoVec<2>::type sc, const WinoVec<2>::type fsh, const WinoVec<2>::type mu,
                                                        const WinoVec<2>::type rs, int want_dg, float* map, WinoVec<2>::type& a_db,
                                                        WinoVec<2>::type& a_dg, WinoVec<2>::type& a_bias, int W, int C, int CS) {
    typedef WinoVec<2>::type vec;
    constexpr int ITH = OTH + 2, ITW = OTW + 2;
    vec m[ITH][ITW], zz[OTH][OTW];
    const unsigned moff = (t * (unsigned)C + (unsigned)c) * 4u;
    const unsigned zoff = (unsigned)((oh0 * W + ow0) * C + c) * 4u;     // z: this map's; the outputs' offsets from the tile's first are uniform
#pragma unroll
    for (int r = 0; r < ITH; ++r)
#pragma unroll
        for (int k = 0; k < ITW; ++k) m[r][k] = wino_buffer_load<2>(rsrc, moff, (unsigned)(r * ITW + k) * mstride);
#pragma unroll
    for (int a = 0; a < OTH; ++a)
#pragma unroll
        for (int b = 0; b < OTW; ++b) zz[a][b] = wino_buffer_load<2>(rz, zoff, (unsigned)((a * W + b) * C) * 4u);
    vec s[OTH][ITW];
#pragma unroll
    for (int k = 0; k < ITW; ++k) {              // A^T down the rows of every column k
        vec col[ITH], o[OTH];
#pragma unroll
        for (int r = 0; r < ITH; ++r) col[r] = m[r][k];
        wino_at<OTH>(col, o);
#pragma unroll
        for (int a = 0; a < OTH; ++a) s[a][k] = o[a];
    }
#pragma unroll
    for (int a = 0; a < OTH; ++a) {
        vec y[OTW];
        wino_at<OTW>(s[a], y);
#pragma unroll
        for (int b = 0; b < OTW; ++b) {           // the mixed tiling has no overhang: every output lies inside the map
            const int pix = (oh0 + a) * W + ow0 + b;
            vec gg = y[b], dz;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float v = sc[e] * zz[a][b][e] + fsh[e];
                gg[e] = v > 0.f ? gg[e] : 0.f;
                dz[e] = gg[e] * sc[e];
            }
            if (DZ) wino_buffer_store2(dz, rdz, zoff, (unsigned)((a * W + b) * C) * 4u);
            *(vec*)(map + pix * CS + cl) = dz;
            if (want_dg) {
#pragma unroll
                for (int e = 0; e < 2; ++e) a_dg[e] += gg[e] * (zz[a][b][e] - mu[e]) * rs[e];
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) { a_db[e] += gg[e]; a_bias[e] += dz[e]; }
        }
    }
}

// Both transforms of the tile at (oh0, ow0), cut from the map with ONE read of its (OTH + 2) x (OTW + 2) window -- rows and columns
// past the map's edge (the halo) read a row of CS zeros kept behind the map, so no read is conditional --: from the window's inner OTH x OTW values
// dM = A d A^T in winograd_dy_kernel's sequence, from the whole window V = B^T d B in wino_chain_in_tile's.  Stores go through
// one buffer resource per group: one address register per lane for all of a tile's matrices, as the loads of phase 1.
template <int OTH, int OTW>
__device__ __forceinline__ void wino_bwd_chain_cut_tile(const float* map, __amdgpu_buffer_rsrc_t rv, __amdgpu_buffer_rsrc_t rdm, bool want_dm,
                                                        unsigned mstride, unsigned t, int oh0, int ow0, int c, int cl, int H, int W, int C,
                                                        int CS) {
    typedef WinoVec<2>::type vec;
    constexpr int ITH = OTH + 2, ITW = OTW + 2;
    const unsigned off = (t * (unsigned)C + (unsigned)c) * 4u;
    const int zero = H * W * CS + cl;            // the row of zeros behind the map
    int roff[ITH], coff[ITW];
    bool rok[ITH], cok[ITW];
#pragma unroll
    for (int r = 0; r < ITH; ++r) {
        const int ih = oh0 - 1 + r;
        rok[r] = (unsigned)ih < (unsigned)H;
        roff[r] = ih * W * CS;
    }
#pragma unroll
    for (int s = 0; s < ITW; ++s) {
        const int iw = ow0 - 1 + s;
        cok[s] = (unsigned)iw < (unsigned)W;
        coff[s] = iw * CS + cl;
    }
    vec d[ITH][ITW];
#pragma unroll
    for (int r = 0; r < ITH; ++r)
#pragma unroll
        for (int s = 0; s < ITW; ++s) d[r][s] = *(const vec*)(map + ((rok[r] && cok[s]) ? roff[r] + coff[s] : zero));
    if (want_dm) {
        vec u[ITH][OTW];
#pragma unroll
        for (int b = 0; b < OTW; ++b) {          // A down the rows of every output column b
            vec col[OTH], o[ITH];
#pragma unroll
            for (int a = 0; a < OTH; ++a) col[a] = d[a + 1][b + 1];
            wino_a<OTH>(col, o);
#pragma unroll
            for (int r = 0; r < ITH; ++r) u[r][b] = o[r];
        }
#pragma unroll
        for (int r = 0; r < ITH; ++r) {          // (A d) A^T
            vec m[ITW];
            wino_a<OTW>(u[r], m);
#pragma unroll
            for (int k = 0; k < ITW; ++k) wino_buffer_store2(m[k], rdm, off, (unsigned)(r * ITW + k) * mstride);
        }
    }
    vec tt[ITH][ITW];
#pragma unroll
    for (int s = 0; s < ITW; ++s) {              // columns of the tile: B^T applied down the rows
        vec col[ITH], o[ITH];
#pragma unroll
        for (int r = 0; r < ITH; ++r) col[r] = d[r][s];
        wino_bt<OTH>(col, o);
#pragma unroll
        for (int r = 0; r < ITH; ++r) tt[r][s] = o[r];
    }
#pragma unroll
    for (int r = 0; r < ITH; ++r) {              // then along each row
        vec v[ITW];
        wino_bt<OTW>(tt[r], v);
#pragma unroll
        for (int s = 0; s < ITW; ++s) wino_buffer_store2(v[s], rv, off, (unsigned)(r * ITW + s) * mstride);
    }
}

#define WINO_RSRC(p) __builtin_amdgcn_make_buffer_rsrc((void*)(p), 0, 0xFFFFFFF0u, 0x00020000)
template <bool DZ>
__global__ __launch_bounds__(256, 3) void winograd_bwd_chain_kernel(const float* __restrict__ Mt, const float* __restrict__ below_z,
                                                                 const float* __restrict__ scale, const float* __restrict__ fwd_shift,
                                                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 float* __restrict__ partials, float* __restrict__ V,
                                                                 float* __restrict__ dM, float* __restrict__ dz_out, int H, int W, int C,
                                                                 int lg, const WinoChainGeo geo) {
    typedef WinoVec<2>::type vec;
    extern __shared__ __attribute__((aligned(16))) float wino_bwd_chain_map[];     // [H * W + 1][CS], the last row zeros; afterwards the sums [3][slots][CS]
    float* map = wino_bwd_chain_map;
    const int L = 1 << lg, CS = 2 << lg, slots = 256 >> lg;
    const int slices = C / CS;
    const int n = (int)(blockIdx.x / (unsigned)slices), slice = (int)(blockIdx.x - (unsigned)n * slices);
    const int slot = threadIdx.x >> lg, cl = (threadIdx.x & (L - 1)) * 2;
    const int c = slice * CS + cl;
    const int a = geo.a, b = geo.b, n0 = a * b, per_map = n0 + a + b + 1;
    const int want_dg = partials && mean;
    const bool want_dm = dM != nullptr;
    const unsigned cb = (unsigned)C * 4u;
    vec a_db = {}, a_dg = {}, a_bias = {};
    if (slot == 0) *(vec*)(map + H * W * CS + cl) = vec{};
    {
        const vec sc = *(const vec*)(scale + c), fsh = *(const vec*)(fwd_shift + c);
        vec mu = {}, rs = {};
        if (want_dg) { mu = *(const vec*)(mean + c); rs = *(const vec*)(rstd + c); }
        // one descriptor per group, made where the base is plainly uniform (the host checks that every group fits 4 GiB); z and dz:
        // this map's (<= 2048 pixels: 32-bit offsets inside it)
        const long long mapoff = (long long)n * H * W * C;
        const __amdgpu_buffer_rsrc_t rz = WINO_RSRC(below_z + mapoff), rdz = WINO_RSRC(dz_out + mapoff);
        for (int it = slot; it < per_map; it += slots) {
            if (it < n0) {
                const int th = it / b, tw = it - th * b;
                wino_bwd_chain_out_tile<4, 4, DZ>(WINO_RSRC(Mt + geo.off[0]), geo.tp[0] * cb, (unsigned)n * n0 + it, 4 * th, 4 * tw, c, cl, rz, rdz, sc,
                                                  fsh, mu, rs, want_dg, map, a_db, a_dg, a_bias, W, C, CS);
            } else if (it < n0 + a) {
                const int th = it - n0;
                wino_bwd_chain_out_tile<4, 2, DZ>(WINO_RSRC(Mt + geo.off[1]), geo.tp[1] * cb, (unsigned)n * a + th, 4 * th, W - 2, c, cl, rz, rdz, sc,
                                                  fsh, mu, rs, want_dg, map, a_db, a_dg, a_bias, W, C, CS);
            } else if (it < n0 + a + b) {
                const int tw = it - n0 - a;
                wino_bwd_chain_out_tile<2, 4, DZ>(WINO_RSRC(Mt + geo.off[2]), geo.tp[2] * cb, (unsigned)n * b + tw, H - 2, 4 * tw, c, cl, rz, rdz, sc,
                                                  fsh, mu, rs, want_dg, map, a_db, a_dg, a_bias, W, C, CS);
            } else {
                wino_bwd_chain_out_tile<2, 2, DZ>(WINO_RSRC(Mt + geo.off[3]), geo.tp[3] * cb, (unsigned)n, H - 2, W - 2, c, cl, rz, rdz, sc, fsh, mu,
                                                  rs, want_dg, map, a_db, a_dg, a_bias, W, C, CS);
            }
        }
    }
    __syncthreads();
    for (int it = slot; it < per_map; it += slots) {
        if (it < n0) {
            const int th = it / b, tw = it - th * b;
            wino_bwd_chain_cut_tile<4, 4>(map, WINO_RSRC(V + geo.off[0]), WINO_RSRC(dM + geo.off[0]), want_dm, geo.tp[0] * cb, (unsigned)n * n0 + it,
                                          4 * th, 4 * tw, c, cl, H, W, C, CS);
        } else if (it < n0 + a) {
            const int th = it - n0;
            wino_bwd_chain_cut_tile<4, 2>(map, WINO_RSRC(V + geo.off[1]), WINO_RSRC(dM + geo.off[1]), want_dm, geo.tp[1] * cb, (unsigned)n * a + th,
                                          4 * th, W - 2, c, cl, H, W, C, CS);
        } else if (it < n0 + a + b) {
            const int tw = it - n0 - a;
            wino_bwd_chain_cut_tile<2, 4>(map, WINO_RSRC(V + geo.off[2]), WINO_RSRC(dM + geo.off[2]), want_dm, geo.tp[2] * cb, (unsigned)n * b + tw,
                                          H - 2, 4 * tw, c, cl, H, W, C, CS);
        } else {
            wino_bwd_chain_cut_tile<2, 2>(map, WINO_RSRC(V + geo.off[3]), WINO_RSRC(dM + geo.off[3]), want_dm, geo.tp[3] * cb, (unsigned)n, H - 2,
                                          W - 2, c, cl, H, W, C, CS);
        }
    }
    if (!partials) return;
    __syncthreads();                                            // the map has been read: its LDS takes the sums, 3 * 256 * 2 floats
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        map[(0 * slots + slot) * CS + cl + e] = a_db[e];
        map[(1 * slots + slot) * CS + cl + e] = a_dg[e];
        map[(2 * slots + slot) * CS + cl + e] = a_bias[e];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < 3 * CS; j += 256) {
        const int k = j / CS, cc = j - k * CS;
        float v = map[k * slots * CS + cc];
        for (int r = 1; r < slots; ++r) v += map[(k * slots + r) * CS + cc];
        partials[((long long)n * 3 + k) * C + slice * CS + cc] = v;
    }
}
#undef WINO_RSRC

// Weight gradient through the same domain: dU[xi] = V[xi]^T . dM[xi] (ITH * ITW GEMMs contracting over the tiles: 1 x 1 weight
// gradients for the float32 weight-gradient kernel), with V = B^T d B the forward's input transform (kept from the forward
// pass) and dM = A dy A^T the ADJOINT of the output transform (outputs past the map's edge count as zero); then dW = G^T dU G.
template <int OTH, int OTW, int CV>
__global__ __launch_bounds__(256) void winograd_dy_kernel(const float* __restrict__ dy, float* __restrict__ dM, int N, int H, int W, int C,
                                                          long long T, long long Tp, const WinoGrp g) {
    typedef typename WinoVec<CV>::type vec;
    constexpr int ITH = OTH + 2, ITW = OTW + 2;
    const int cn = C / CV;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * cn) return;
    const long long t = i / cn;
    const int c = (int)(i - t * cn) * CV;
    const WinoTile q = wino_tile(t, g.th_n, g.tw_n);
    vec u[ITH][OTW];
#pragma unroll
    for (int b = 0; b < OTW; ++b) {              // A down the rows of every output column b
        vec col[OTH], o[ITH];
#pragma unroll
        for (int a = 0; a < OTH; ++a) {
            const int oh = g.oh0 + OTH * q.th + a, ow = g.ow0 + OTW * q.tw + b;
            vec val = {};
            if (oh < H && ow < W) val = *(const vec*)(dy + (((long long)q.n * H + oh) * W + ow) * C + c);
            col[a] = val;
        }
        wino_a<OTH>(col, o);
#pragma unroll
        for (int r = 0; r < ITH; ++r) u[r][b] = o[r];
    }
#pragma unroll
    for (int r = 0; r < ITH; ++r) {              // (A d) A^T
        vec m[ITW];
        wino_a<OTW>(u[r], m);
#pragma unroll
        for (int k = 0; k < ITW; ++k) *(vec*)(dM + ((long long)(r * ITW + k) * Tp + t) * C + c) = m[k];
    }
}

// dW [3][3][ci][co] (= or +=) G_h^T dU G_w, dU [ITH * ITW][ci][co]; one thread per (ci, co)
template <int OTH, int OTW>
__global__ __launch_bounds__(256) void winograd_dw_kernel(const float* __restrict__ dU, float* dW, int Cin, int Cout, int accumulate) {
    constexpr int ITH = OTH + 2, ITW = OTW + 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = (long long)Cin * Cout;
    if (i >= n) return;
    float t[3][ITW];
#pragma unroll
    for (int b = 0; b < ITW; ++b) {
        float col[ITH], o[3];
#pragma unroll
        for (int a = 0; a < ITH; ++a) col[a] = dU[(long long)(a * ITW + b) * n + i];
        wino_gt<OTH>(col, o);
#pragma unroll
        for (int a = 0; a < 3; ++a) t[a][b] = o[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float w[3];
        wino_gt<OTW>(t[a], w);
        float* o = dW + (long long)(a * 3) * n + i;
#pragma unroll
        for (int b = 0; b < 3; ++b) o[b * n] = accumulate ? o[b * n] + w[b] : w[b];
    }
}

// ---- the 16 transform-domain GEMMs, persistent form ----------------------------------------------------------------------------
// V [nb][rows][K] . U [nb][K][N] -> Mt [nb][rows][N] with the tile, LDS image and MFMA loop of conv_fwd_blds_kernel (128 x 128
// tile, K-step 16, both operands by buffer-addressed LDS-DMA, A chunks XOR-swizzled on the source side), but workgroups that
// walk tiles blockIdx.x, + gridDim.x, ...: K is only 256 here (16 K-steps per tile), so the one-tile-per-workgroup kernel spends
// ~26 % of a launch in phases where every resident workgroup of a CU is storing its tile or waiting for its first stage at the
// same time (tools/gemm_k_probe.py: 0.15 ms fixed + 1.5 us per unit of K over 4.9 rounds).  Here the first stage of the NEXT
// tile is on its way before the stores of the current tile are issued, and the workgroups of a CU drift apart.
typedef __attribute__((address_space(3))) void* wino_lds_ptr;
#define WINO_OOB 0xFFFFFFF0u

// DECONV: the product is a 2 x 2 stride-2 transposed convolution (mrcnn_deconv2x2_gemm): row m = input pixel (img, h, w), column
// n = (tap a b, channel co) -> out[img][2 h + a][2 w + b][co] = act(acc + bias[co]) -- the pixel-shuffle store of the direct kernel
struct GemmDeconvEp {
    const float* bias;
    int Cd, H, W, act;
    FastDiv d_hw, d_w;
};

// MASK (with DECONV, TN = 4, Cd = 256: tile column block n0 / 256 is the tap, and a tile holds all 256 channels of its 128 output
// pixels): the mask head's output layer in the same epilogue (mrcnn_deconv2x2_mask_gemm) --
// m[img][2 h + a][2 w + b][k] = sigmoid(b_mask[k] + sum_co out[..][co] . w_mask[co][k]), k < C <= 16.  Mt may be null then (inference:
// `out` itself is not stored).  The sum runs in a fixed order: in the lane over its four column groups, across the 32 lanes that
// share a row by halving exchanges, then N-wave 0 + N-wave 1 through LDS.
struct GemmMaskEp : GemmDeconvEp {
    const float* w_mask;     // [Cd][C]
    const float* b_mask;     // [C] or null
    float* m;                // [N][2 H][2 W][C]
    int C;
};

// the value of lane (l ^ X) within each half wave, X < 32: ds_swizzle in its bit-mask mode (and 0x1f, or 0, xor X) -- an LDS-pipe
// instruction that touches no memory and, unlike ds_bpermute, takes no address register
template <int X>
__device__ __forceinline__ float wino_swz_xor(float v) {
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x1f | (X << 10)));
}
// one halving exchange over lane bit HS: s[0 .. 2 HS) on every lane -> s[0 .. HS), each the sum of the two partner lanes' values of
// row i (lanes with the bit clear) or row i + HS (bit set)
template <int HS>
__device__ __forceinline__ void wino_halve(float* s, int li) {
    const bool hi = li & HS;
#pragma unroll
    for (int i = 0; i < HS; ++i) {
        const float lo_v = s[i], hi_v = s[i + HS];         // values, not lvalues: a conditional over array elements becomes a
        const float keep = hi ? hi_v : lo_v;               // dynamic index into registers
        const float send = hi ? lo_v : hi_v;
        s[i] = keep + wino_swz_xor<HS>(send);
    }
}

template <int TN, bool DECONV, bool MASK = false>   // TN 2: 128 x 128 tile (5 workgroups per CU); 4: 128 x 256 tile -- N = 256 whole: every V row block is fetched once
__global__ __launch_bounds__(256, MASK ? 3 : 2) void winograd_gemm_kernel(const float* __restrict__ V, const float* __restrict__ U, float* __restrict__ Mt,
                                                               int rows, int K, int N, int total_tiles, unsigned v_records,
                                                               const std::conditional_t<MASK, GemmMaskEp, GemmDeconvEp> ep) {
    static_assert(!MASK || (DECONV && TN == 4), "the mask epilogue wants one tap's 256 channels in a tile");
    constexpr int BM = 128, BN = 64 * TN, BK = 16, TM = 2;
    constexpr int AF = BM * BK, BF = BK * BN;
    __shared__ __attribute__((aligned(16))) float lds[2 * (AF + BF)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int ntiles = N / BN;
    const int nk = K / BK;
    const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc((void*)V, 0, v_records, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc((void*)U, 0, 0x7FFFFFF0u, 0x00020000);

    // per tile: lane offsets of the two A pieces (16 rows x 64 bytes each) and the B pieces (2 k-rows x 512 bytes each)
    constexpr int NBP = BF / 256 / 4;                     // 1 KiB B pieces per wave and stage (2 or 4)
    unsigned a_voff[2], b_voff[4];                        // fixed bound: a template-dependent one captured by the lambdas below makes
                                                          // hipcc drop the kernel's host stub (build.py checks for that)
    int m0 = 0, n0 = 0;
    auto setup = [&](int tile) {
        const int mtile = tile / ntiles;
        const int ntile = tile - mtile * ntiles;
        m0 = mtile * BM; n0 = ntile * BN;
        const unsigned wbase = (unsigned)(((long long)(m0 / rows) * K * N + n0) * 4);      // the tile's weight matrix (U [nb][K][N], < 2 GiB)
        if constexpr (MASK) {
            // The mask epilogue needs every register beside the 128 accumulators, so this instantiation keeps three offsets, not
            // six, and none of their lane-only parts across the K loop (the empty asm has them recomputed per tile).  The second A
            // piece is 64 rows below the first with the same swizzle; with BN = 256 B piece jj is k row wave + 4 jj whole, and
            // stage() puts those 4 jj rows into the scalar offset (the weights are never addressed out of range).
            int ln = lane;
            asm volatile("" : "+v"(ln));
            const int r = wave * 16 + (ln >> 2);
            const int cl = (ln & 3) ^ ((r >> 2) & 3);
            a_voff[0] = (unsigned)(((long long)(m0 + r) * K + cl * 4) * 4);
            a_voff[1] = a_voff[0] + (unsigned)(64 * K * 4);
            b_voff[0] = wbase + (unsigned)((wave * N + ln * 4) * 4);
            return;
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int r = (wave + jj * 4) * 16 + (lane >> 2);
            const int cl = (lane & 3) ^ ((r >> 2) & 3);
            a_voff[jj] = (unsigned)(((long long)(m0 + r) * K + cl * 4) * 4);
        }
        // B [16 k][BN]: a 1 KiB piece is 256 consecutive floats of the tile: piece pc -> k row (pc * 256) / BN, columns (pc * 256) % BN ..
#pragma unroll
        for (int jj = 0; jj < NBP; ++jj) {
            const int f = (wave + jj * 4) * 256 + lane * 4;       // float index inside the [16][BN] tile
            b_voff[jj] = wbase + (unsigned)(((f / BN) * N + (f % BN)) * 4);
        }
    };
    int k0 = 0;
    auto stage = [&](float* ab) {
        float* bb = ab + AF;
        const unsigned soff_a = (unsigned)(k0 * 4), soff_b = (unsigned)(k0 * N * 4);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, (wino_lds_ptr)(ab + (wave + jj * 4) * 256), 16, a_voff[jj], soff_a, 0, 0);
#pragma unroll
        for (int jj = 0; jj < NBP; ++jj) {
            if constexpr (MASK)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_b, (wino_lds_ptr)(bb + (wave + jj * 4) * 256), 16, b_voff[0],
                                                         soff_b + (unsigned)(jj * 16 * N), 0, 0);
            else
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_b, (wino_lds_ptr)(bb + (wave + jj * 4) * 256), 16, b_voff[jj], soff_b, 0, 0);
        }
        k0 += BK;
    };
    f32x16 acc[TM][TN];
    const int li = lane & 31, lh = lane >> 5;
    const int row0 = wm * 64 + li;
    const float* a_rd0 = lds + row0 * BK + (((2 * lh + 0) ^ ((row0 >> 2) & 3)) << 2);
    const float* a_rd1 = lds + row0 * BK + (((2 * lh + 1) ^ ((row0 >> 2) & 3)) << 2);
    const float* b_rd = lds + AF + lh * 8 * BN + wn * (32 * TN) + li;
    auto compute = [&](auto curc) {
        constexpr int BO = decltype(curc)::value * (AF + BF);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            f32x4 av[TM];
#pragma unroll
            for (int a = 0; a < TM; ++a) av[a] = *(const f32x4*)((q ? a_rd1 : a_rd0) + BO + a * 32 * BK);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float bv[TN];
#pragma unroll
                for (int b = 0; b < TN; ++b) bv[b] = b_rd[BO + (q * 4 + e) * BN + b * 32];
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int b = 0; b < TN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a][e], bv[b], acc[a][b], 0, 0, 0);
            }
        }
    };
    typedef std::integral_constant<int, 0> I0;
    typedef std::integral_constant<int, 1> I1;

    if constexpr (MASK) {                                  // once per workgroup; the first tile's top-of-loop barrier publishes it
        extern __shared__ __attribute__((aligned(16))) float wino_mask_w[];   // w_mask as [k][256 co]: 256 C floats of dynamic LDS
        for (int i = tid; i < 256 * ep.C; i += 256) {
            const int co = i / ep.C;
            wino_mask_w[(i - co * ep.C) * 256 + co] = ep.w_mask[i];
        }
    }

    int tile = blockIdx.x;
    setup(tile);
    stage(lds);
    for (;;) {
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
        __syncthreads();
        for (int ks = 0; ks < nk; ks += 2) {
            if (ks + 1 < nk) stage(lds + (AF + BF));
            compute(I0{});
            __syncthreads();
            if (ks + 1 < nk) {
                if (ks + 2 < nk) stage(lds);
                compute(I1{});
                __syncthreads();
            }
        }
        const int mw0 = m0 + wm * 64 + 4 * lh, nw0 = n0 + wn * (32 * TN) + li;   // the tile the accumulators belong to
        const int next = tile + (int)gridDim.x;
        const bool more = next < total_tiles;
        if (more) { k0 = 0; setup(next); stage(lds); }                         // its first stage travels under this tile's stores
        const int Mtot = (int)(v_records / (unsigned)(K * 4));
        if constexpr (!DECONV) {
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = mw0 + a * 32 + (r & 3) + 8 * (r >> 2);
                        if (m < Mtot) Mt[(long long)m * N + nw0 + b * 32] = acc[a][b][r];
                    }
        } else if constexpr (MASK) {
            extern __shared__ __attribute__((aligned(16))) float wino_mask_w[];
            // Cd = 256 = BN: every column of the tile belongs to tap nw0 / 256; this lane's channels are co0 + 32 b
            // Lane and wave coordinates are taken back out of the tile's own mw0 / nw0 (m0 % 128 == 0, n0 % 256 == 0), so that what
            // the epilogue derives from them is computed per tile and does not sit in registers across the K loop.
            // (The empty asm keeps the compiler from seeing through that: n0 is a multiple of 256 by construction.)
            int nw0_e = nw0, mw0_e = mw0;
            asm volatile("" : "+v"(nw0_e), "+v"(mw0_e));
            const int tap = nw0 >> 8, co0 = nw0_e & 255;
            const int li_e = nw0_e & 31, lane_e = ((mw0_e >> 2) & 1) * 32 + li_e;
            const int hw = ep.H * ep.W;
#pragma unroll
            for (int b = 0; b < TN; ++b) {
                const float bi = ep.bias ? ep.bias[co0 + b * 32] : 0.f;
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = acc[a][b][r] + bi;
                        if (ep.act == MRCNN_ACT_RELU) v = fmaxf(v, 0.f);
                        acc[a][b][r] = v;
                    }
            }
            if (Mt) {                                                          // the pixel-shuffle store of the DECONV epilogue
                const int coff = ((tap >> 1) * 2 * ep.W + (tap & 1)) * 256 + co0;
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = mw0 + a * 32 + (r & 3) + 8 * (r >> 2);
                        if (m >= Mtot) continue;
                        const int img = (int)fast_div((unsigned)m, ep.d_hw), rem = m - img * hw;
                        const int h = (int)fast_div((unsigned)rem, ep.d_w), w = rem - h * ep.W;
                        const long long base = (((long long)img * 2 * ep.H + 2 * h) * 2 * ep.W + 2 * w) * 256;
#pragma unroll
                        for (int b = 0; b < TN; ++b) Mt[base + coff + b * 32] = acc[a][b][r];
                        __builtin_amdgcn_sched_barrier(0);                     // one row's addresses at a time: the 128 accumulators stay live
                    }
            }
            // Partial logits.  The exchange area is stage buffer 1: the K loop's last barrier is behind its last reader and no DMA
            // into it is outstanding (the next tile's first stage, already issued above, fills buffer 0).
            float* xch = lds + (AF + BF);                                      // [wn][wm][k < 16][lane]
#pragma unroll 1
            for (int k = 0; k < ep.C; ++k) {
                float wk[TN];
#pragma unroll
                for (int b = 0; b < TN; ++b) wk[b] = wino_mask_w[k * 256 + co0 + b * 32];
                float mine = 0.f;                                              // the sum of this lane's row: block li >> 4, row li & 15
#pragma unroll
                for (int g = 0; g < 2 * TM; ++g) {                             // eight rows at a time: rows 8 (g & 1) .. of block g >> 1
                    float s[8];                                                // this lane's four channels of each
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        s[i] = acc[g >> 1][0][(g & 1) * 8 + i] * wk[0];
#pragma unroll
                        for (int b = 1; b < TN; ++b) s[i] = fmaf(acc[g >> 1][b][(g & 1) * 8 + i], wk[b], s[i]);
                    }
                    // 8 rows x 32 lanes: three halving exchanges leave row li & 7 summed over 8 lanes, two plain ones finish it
                    wino_halve<4>(s, li_e); wino_halve<2>(s, li_e); wino_halve<1>(s, li_e);
                    float t = s[0] + wino_swz_xor<8>(s[0]);
                    t = t + wino_swz_xor<16>(t);
                    mine = ((li_e >> 3) == g) ? t : mine;
                    __builtin_amdgcn_sched_barrier(0);                         // one group after the other: 8 sums live beside the accumulators
                }
                xch[((wn * 2 + wm) * 16 + k) * 64 + lane_e] = mine;
            }
            __syncthreads();                                                   // both N-waves' partial sums are in LDS
            if (wn == 0) {
                const int r = li_e & 15;
                const int m = mw0 + (li_e >> 4) * 32 + (r & 3) + 8 * (r >> 2);
                if (m < Mtot) {
                    const int img = (int)fast_div((unsigned)m, ep.d_hw), rem = m - img * hw;
                    const int h = (int)fast_div((unsigned)rem, ep.d_w), w = rem - h * ep.W;
                    float* mo = ep.m + (((long long)img * 2 * ep.H + 2 * h + (tap >> 1)) * 2 * ep.W + 2 * w + (tap & 1)) * ep.C;
                    for (int k = 0; k < ep.C; ++k) {
                        const float y = (xch[(wm * 16 + k) * 64 + lane] + xch[((2 + wm) * 16 + k) * 64 + lane]) + (ep.b_mask ? ep.b_mask[k] : 0.f);
                        mo[k] = 1.f / (1.f + expf(-y));
                    }
                }
            }
            // This barrier orders the reads of xch above before the next tile's first stage(lds + AF + BF), which overwrites it.
            // (The loop's top barrier would do the same today; this one keeps the epilogue safe on its own.)
            __syncthreads();
        } else {
            float bi[TN];
            int coff[TN];                                                      // (a * 2 W + b) * Cd + co of this lane's column in group b
#pragma unroll
            for (int b = 0; b < TN; ++b) {
                const int n = nw0 + b * 32;
                const int tap = (n >= ep.Cd) + (n >= 2 * ep.Cd) + (n >= 3 * ep.Cd);
                const int co = n - tap * ep.Cd;
                bi[b] = ep.bias ? ep.bias[co] : 0.f;
                coff[b] = ((tap >> 1) * 2 * ep.W + (tap & 1)) * ep.Cd + co;
            }
            const int hw = ep.H * ep.W;
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = mw0 + a * 32 + (r & 3) + 8 * (r >> 2);
                    if (m >= Mtot) continue;
                    const int img = (int)fast_div((unsigned)m, ep.d_hw), rem = m - img * hw;
                    const int h = (int)fast_div((unsigned)rem, ep.d_w), w = rem - h * ep.W;
                    const long long base = (((long long)img * 2 * ep.H + 2 * h) * 2 * ep.W + 2 * w) * ep.Cd;
#pragma unroll
                    for (int b = 0; b < TN; ++b) {
                        float v = acc[a][b][r] + bi[b];
                        if (ep.act == MRCNN_ACT_RELU) v = fmaxf(v, 0.f);
                        Mt[base + coff[b]] = v;
                    }
                }
        }
        if (!more) break;
        tile = next;
    }
}

// ---- host side: tile groups ------------------------------------------------------------------------------------------------------
static inline long long wino_rows(long long T) { return (T + 127) / 128 * 128; }      // rows per transform-domain matrix: whole 128-row tiles
static inline int wino_tdim(int extent, int tile) { return (extent + tile - 1) / tile; }

static int wino_grp_ok(const mrcnn_wino_group* g, int N, int H, int W, int C) {
    if (!g || (g->oth != 2 && g->oth != 4) || (g->otw != 2 && g->otw != 4)) return 0;
    if (g->th_n <= 0 || g->tw_n <= 0 || g->oh0 < 0 || g->ow0 < 0 || g->oh0 >= H || g->ow0 >= W) return 0;
    return N > 0 && H > 0 && W > 0 && C > 0 && !(C & 3);
}
static inline long long wino_grp_tiles(const mrcnn_wino_group* g, int N) { return (long long)N * g->th_n * g->tw_n; }
static inline int wino_grp_nb(const mrcnn_wino_group* g) { return (g->oth + 2) * (g->otw + 2); }
static inline int wino_grp_cv(const mrcnn_wino_group* g) { return g->oth == 2 && g->otw == 2 ? 4 : 2; }   // channels per thread

// launch the instantiation of a transform kernel for a group: <2, 2, 4> (one thread = a tile x 4 channels), the others x 2 channels
// (36 + 36 values of 4 channels would not fit the register file without spilling)
#define WINO_LAUNCH_G(kernel, g, grid4, grid2, ...)                                                                          \
    do {                                                                                                                     \
        if ((g)->oth == 2 && (g)->otw == 2) hipLaunchKernelGGL((kernel<2, 2, 4>), grid4, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); \
        else if ((g)->oth == 4 && (g)->otw == 4) hipLaunchKernelGGL((kernel<4, 4, 2>), grid2, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); \
        else if ((g)->oth == 4) hipLaunchKernelGGL((kernel<4, 2, 2>), grid2, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); \
        else hipLaunchKernelGGL((kernel<2, 4, 2>), grid2, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);                  \
    } while (0)
#define WINO_LAUNCH_W(kernel, oth, otw, grid, ...)                                                                           \
    do {                                                                                                                     \
        if ((oth) == 2 && (otw) == 2) hipLaunchKernelGGL((kernel<2, 2>), grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); \
        else if ((oth) == 4 && (otw) == 4) hipLaunchKernelGGL((kernel<4, 4>), grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); \
        else if ((oth) == 4) hipLaunchKernelGGL((kernel<4, 2>), grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);     \
        else hipLaunchKernelGGL((kernel<2, 4>), grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);                     \
    } while (0)

extern "C" size_t mrcnn_winograd_group_floats(const mrcnn_wino_group* g, int N, int C) {
    if (!g || N <= 0 || C <= 0 || (g->oth != 2 && g->oth != 4) || (g->otw != 2 && g->otw != 4) || g->th_n <= 0 || g->tw_n <= 0) return 0;
    return (size_t)wino_grp_nb(g) * (size_t)wino_rows(wino_grp_tiles(g, N)) * (size_t)C;
}

extern "C" int mrcnn_winograd_input_g(const float* x, float* V, int N, int H, int W, int C, const mrcnn_wino_group* g, void* stream) {
    if (!x || !V || !wino_grp_ok(g, N, H, W, C)) return MRCNN_ERR_ARG;
    const long long T = wino_grp_tiles(g, N);
    const WinoGrp k = {g->th_n, g->tw_n, g->oh0, g->ow0};
    const dim3 g4((unsigned)cdiv64(T * C / 4, 256)), g2((unsigned)cdiv64(T * C / 2, 256));
    WINO_LAUNCH_G(winograd_input_kernel, g, g4, g2, x, V, N, H, W, C, T, wino_rows(T), k);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_winograd_weights_g(const float* w, float* U, int Cin, int Cout, int oth, int otw, void* stream) {
    if (!w || !U || Cin <= 0 || Cout <= 0 || (oth != 2 && oth != 4) || (otw != 2 && otw != 4)) return MRCNN_ERR_ARG;
    const dim3 grid((unsigned)cdiv64((long long)Cin * Cout, 256));
    WINO_LAUNCH_W(winograd_weight_kernel, oth, otw, grid, w, U, Cin, Cout);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_winograd_output_g(const float* Mt, float* out, float* z, const float* bias, const float* scale, const float* shift,
                                       int N, int H, int W, int C, int act, const mrcnn_wino_group* g, void* stream) {
    if (!Mt || !out || !wino_grp_ok(g, N, H, W, C) || (scale && !shift)) return MRCNN_ERR_ARG;
    if (act != MRCNN_ACT_NONE && act != MRCNN_ACT_RELU) return MRCNN_ERR_UNSUPPORTED;
    const long long T = wino_grp_tiles(g, N);
    const WinoGrp k = {g->th_n, g->tw_n, g->oh0, g->ow0};
    const dim3 g4((unsigned)cdiv64(T * C / 4, 256)), g2((unsigned)cdiv64(T * C / 2, 256));
    WINO_LAUNCH_G(winograd_output_kernel, g, g4, g2, Mt, out, z, bias, scale, shift, N, H, W, C, T, wino_rows(T), act, k);
    return mrcnn_launch_status();
}

// ---- forward chain: output transform + epilogue of a layer and the input transform of the next, mixed tiling -------------------------
// channels per workgroup: the widest slice whose H x W map leaves three workgroups per CU their LDS (14 x 14 x 64 floats = 49 KiB)
static int wino_chain_slice(int H, int W) {
    for (int cs = 64; cs >= 8; cs >>= 1)
        if ((long long)H * W * cs * 4 <= 53 * 1024) return cs;
    return (long long)H * W * 8 * 4 <= 64 * 1024 ? 8 : 0;
}

// the shapes both chain kernels take, and their launch geometry: channel slice cs, lg = log2(lanes per tile), workgroups
static int wino_chain_plan(int N, int H, int W, int C, int tile, WinoChainGeo* geo, int* cs_out, int* lg_out, long long* wgs_out) {
    if (tile != MRCNN_WINO_TILE_MIXED || H % 4 != 2 || W % 4 != 2 || H <= 4 || W <= 4 || C % 128) return MRCNN_ERR_UNSUPPORTED;
    const int cs = wino_chain_slice(H, W);
    if (!cs) return MRCNN_ERR_UNSUPPORTED;
    geo->a = H / 4; geo->b = W / 4;
    const long long tiles[4] = {(long long)N * geo->a * geo->b, (long long)N * geo->a, (long long)N * geo->b, N};
    const int nb[4] = {36, 24, 24, 16};
    long long off = 0;
    for (int i = 0; i < 4; ++i) {
        const long long tp = wino_rows(tiles[i]);
        // tile ids and the byte offsets into a group's matrices are 32-bit
        if (tiles[i] >= (1LL << 31) || nb[i] * tp * C * 4 >= (1LL << 32)) return MRCNN_ERR_UNSUPPORTED;
        geo->tp[i] = (unsigned)tp;
        geo->off[i] = off;
        off += nb[i] * tp * C;
    }
    const long long wgs = (long long)N * (C / cs);
    if (wgs >= (1LL << 31)) return MRCNN_ERR_UNSUPPORTED;
    int lg = 0;
    while ((2 << lg) < cs) ++lg;                                // lanes per tile = cs / 2
    *cs_out = cs; *lg_out = lg; *wgs_out = wgs;
    return MRCNN_OK;
}

extern "C" int mrcnn_winograd_chain(const float* Mt, float* z_out, const float* bias, const float* scale, const float* shift, float* V_next,
                                    int N, int H, int W, int C, int act, int tile, void* stream) {
    if (!Mt || !V_next || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (scale && !shift)) return MRCNN_ERR_ARG;
    if (act != MRCNN_ACT_NONE && act != MRCNN_ACT_RELU) return MRCNN_ERR_UNSUPPORTED;
    WinoChainGeo geo;
    int cs, lg;
    long long wgs;
    const int rc = wino_chain_plan(N, H, W, C, tile, &geo, &cs, &lg, &wgs);
    if (rc != MRCNN_OK) return rc;
    hipLaunchKernelGGL(winograd_chain_kernel, dim3((unsigned)wgs), dim3(256), (size_t)H * W * cs * 4, (hipStream_t)stream, Mt, z_out, bias, scale,
                       shift, V_next, H, W, C, act, lg, geo);
    return mrcnn_launch_status();
}

// ---- data gradient: output transform + epilogue backward of the layer below --------------------------------------------------------
// workgroups of a group's launch = rows of partials it writes: every R tiles once, at most 4 workgroups per CU (what fits at
// <= 128 registers), each walking its tiles
static int wino_bwd_lanes_lg(const mrcnn_wino_group* g, int C) {            // log2(C / CV), or -1
    const int cn = C / wino_grp_cv(g);
    if (cn <= 0 || cn > 256 || (cn & (cn - 1)) || cn * wino_grp_cv(g) != C) return -1;
    int lg = 0;
    while ((1 << lg) < cn) ++lg;
    return lg;
}
extern "C" int mrcnn_winograd_output_bwd_rows(const mrcnn_wino_group* g, int N, int C) {
    if (!g || N <= 0 || (g->oth != 2 && g->oth != 4) || (g->otw != 2 && g->otw != 4) || g->th_n <= 0 || g->tw_n <= 0) return 0;
    const int lg = wino_bwd_lanes_lg(g, C);
    if (lg < 0) return 0;
    const long long T = wino_grp_tiles(g, N), R = 256 >> lg, cap = 4LL * mrcnn_num_cus();
    const long long wgs = cdiv64(T, R);
    return (int)(wgs < cap ? wgs : cap);
}

template <int MASK>
static int wino_output_bwd_launch(const float* Mt, float* dz_below, const float* below_out, const float* below_z, const float* scale,
                                  const float* mean, const float* rstd, const float* fwd_shift, float* partials, int N, int H, int W,
                                  int C, const mrcnn_wino_group* g, void* stream) {
    const int lg = wino_bwd_lanes_lg(g, C);
    const long long T = wino_grp_tiles(g, N);
    if (lg < 0) return MRCNN_ERR_UNSUPPORTED;
    // tile ids (and their fast division) and the byte offsets into a transform-domain matrix and into the maps are 32-bit
    if ((long long)wino_grp_nb(g) * wino_rows(T) * C * 4 >= (1LL << 32) || (long long)N * H * W * C * 4 >= (1LL << 32)) return MRCNN_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)mrcnn_winograd_output_bwd_rows(g, N, C));
    const WinoGrp k = {g->th_n, g->tw_n, g->oh0, g->ow0};
    const int want_dg = partials && mean && rstd && below_z;
#define WINO_BWD_INST(oth, otw, cv)                                                                                            \
    hipLaunchKernelGGL((winograd_output_bwd_kernel<oth, otw, cv, MASK>), grid, dim3(256), 0, (hipStream_t)stream, Mt, dz_below, below_out, \
                       below_z, scale, mean, rstd, fwd_shift, partials, want_dg, H, W, C, (unsigned)T, wino_rows(T), lg, k,    \
                       make_fastdiv((unsigned)g->th_n), make_fastdiv((unsigned)g->tw_n))
    if (g->oth == 2 && g->otw == 2) WINO_BWD_INST(2, 2, 4);
    else if (g->oth == 4 && g->otw == 4) WINO_BWD_INST(4, 4, 2);
    else if (g->oth == 4) WINO_BWD_INST(4, 2, 2);
    else WINO_BWD_INST(2, 4, 2);
#undef WINO_BWD_INST
    return mrcnn_launch_status();
}

extern "C" int mrcnn_winograd_output_bwd_g(const float* Mt, float* dz_below, const float* below_out, const float* below_z, const float* scale,
                                           const float* mean, const float* rstd, float* partials, int N, int H, int W, int C, int act,
                                           const mrcnn_wino_group* g, void* stream) {
    if (!Mt || !dz_below || !wino_grp_ok(g, N, H, W, C) || (!mean != !rstd) || (mean && !below_z)) return MRCNN_ERR_ARG;
    if (act == MRCNN_ACT_NONE)
        return wino_output_bwd_launch<0>(Mt, dz_below, nullptr, below_z, scale, mean, rstd, nullptr, partials, N, H, W, C, g, stream);
    if (act != MRCNN_ACT_RELU || !below_out) return MRCNN_ERR_ARG;
    return wino_output_bwd_launch<2>(Mt, dz_below, below_out, below_z, scale, mean, rstd, nullptr, partials, N, H, W, C, g, stream);
}

/* the same for a ReLU layer below whose forward epilogue was out = max(scale * z + shift, 0): the mask comes from z (bit for bit
 * the forward's decision), `out` is never read */
extern "C" int mrcnn_winograd_output_bwd_zmask_g(const float* Mt, float* dz_below, const float* below_z, const float* scale,
                                                 const float* shift, const float* mean, const float* rstd, float* partials, int N, int H,
                                                 int W, int C, const mrcnn_wino_group* g, void* stream) {
    if (!Mt || !dz_below || !wino_grp_ok(g, N, H, W, C) || !below_z || !scale || !shift || (!mean != !rstd)) return MRCNN_ERR_ARG;
    return wino_output_bwd_launch<1>(Mt, dz_below, nullptr, below_z, scale, mean, rstd, shift, partials, N, H, W, C, g, stream);
}

extern "C" int mrcnn_winograd_output_bwd_sums(const float* partials, int rows, int C, float* dgamma, float* dbeta, float* dbias,
                                              void* stream) {
    if (!partials || rows <= 0 || C <= 0) return MRCNN_ERR_ARG;
    if (!dgamma && !dbeta && !dbias) return MRCNN_OK;
    const dim3 grid((unsigned)cdiv64(3LL * C, WINO_SUMS_COLS));
    hipLaunchKernelGGL(winograd_bwd_sums_kernel, grid, dim3(WINO_SUMS_COLS * WINO_SUMS_SLICES), 0, (hipStream_t)stream, partials, rows, C,
                       dgamma, dbeta, dbias);
    return mrcnn_launch_status();
}

// ---- backward chain: the four output transforms + epilogue backward, and the input and dy transforms of that dz, one launch -------
extern "C" int mrcnn_winograd_bwd_chain(const float* Mt, const float* below_z, const float* scale, const float* shift, const float* mean,
                                        const float* rstd, float* partials, float* V_next, float* dM, float* dz_out, int N, int H, int W,
                                        int C, int tile, void* stream) {
    if (!Mt || !V_next || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (!mean != !rstd)) return MRCNN_ERR_ARG;
    if (!below_z || !scale || !shift) return MRCNN_ERR_UNSUPPORTED;     // no activation below / mask from the activated output: the separate launches
    WinoChainGeo geo;
    int cs, lg;
    long long wgs;
    const int rc = wino_chain_plan(N, H, W, C, tile, &geo, &cs, &lg, &wgs);
    if (rc != MRCNN_OK) return rc;
    if ((long long)N * 3 * C >= (1LL << 31)) return MRCNN_ERR_UNSUPPORTED;
    size_t lds = ((size_t)H * W + 1) * cs * 4;                                     // the map and a row of zeros for the halo (<= 53.25 KiB: three per CU)
    if (lds > 64 * 1024) return MRCNN_ERR_UNSUPPORTED;
    if (lds < 3 * 256 * 2 * sizeof(float)) lds = 3 * 256 * 2 * sizeof(float);     // the channel sums meet in the map's place
    if (dz_out)
        hipLaunchKernelGGL(winograd_bwd_chain_kernel<true>, dim3((unsigned)wgs), dim3(256), lds, (hipStream_t)stream, Mt, below_z, scale, shift, mean,
                           rstd, partials, V_next, dM, dz_out, H, W, C, lg, geo);
    else
        hipLaunchKernelGGL(winograd_bwd_chain_kernel<false>, dim3((unsigned)wgs), dim3(256), lds, (hipStream_t)stream, Mt, below_z, scale, shift, mean,
                           rstd, partials, V_next, dM, dz_out, H, W, C, lg, geo);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_winograd_dy_g(const float* dy, float* dM, int N, int H, int W, int C, const mrcnn_wino_group* g, void* stream) {
    if (!dy || !dM || !wino_grp_ok(g, N, H, W, C)) return MRCNN_ERR_ARG;
    const long long T = wino_grp_tiles(g, N);
    const WinoGrp k = {g->th_n, g->tw_n, g->oh0, g->ow0};
    const dim3 g4((unsigned)cdiv64(T * C / 4, 256)), g2((unsigned)cdiv64(T * C / 2, 256));
    WINO_LAUNCH_G(winograd_dy_kernel, g, g4, g2, dy, dM, N, H, W, C, T, wino_rows(T), k);
    return mrcnn_launch_status();
}

extern "C" int mrcnn_winograd_dw_g(const float* dU, float* dw_hwio, int Cin, int Cout, int accumulate, int oth, int otw, void* stream) {
    if (!dU || !dw_hwio || Cin <= 0 || Cout <= 0 || (oth != 2 && oth != 4) || (otw != 2 && otw != 4)) return MRCNN_ERR_ARG;
    const dim3 grid((unsigned)cdiv64((long long)Cin * Cout, 256));
    WINO_LAUNCH_W(winograd_dw_kernel, oth, otw, grid, dU, dw_hwio, Cin, Cout, accumulate);
    return mrcnn_launch_status();
}

// ---- the uniform tiling (tile = 2 or 4 outputs per tile and dimension) as one group at (0, 0) -------------------------------------
/* floats of V (input transform) or Mt (transform-domain product) for a layer: (tile + 2)^2 x rows x C; tile 2 wants even extents,
 * tile 4 lets the last tiles hang over the edge */
extern "C" size_t mrcnn_winograd_buffer_floats(int N, int H, int W, int C, int tile) {
    if ((tile != 2 && tile != 4) || (tile == 2 && ((H & 1) || (W & 1)))) return 0;
    if (!(N > 0 && H > 0 && W > 0 && C > 0 && !(C & 3))) return 0;
    const mrcnn_wino_group g = {tile, tile, wino_tdim(H, tile), wino_tdim(W, tile), 0, 0};
    return mrcnn_winograd_group_floats(&g, N, C);
}

extern "C" int mrcnn_winograd_weights(const float* w, float* U, int Cin, int Cout, int tile, void* stream) {
    return mrcnn_winograd_weights_g(w, U, Cin, Cout, tile, tile, stream);
}

/* the persistent form of mrcnn_gemm_batched_f32 (same arguments and result; K % 16 == 0, N % 128 == 0, rows % 128 == 0) */
extern "C" int mrcnn_winograd_gemm(const float* V, const float* U, float* Mt, int nb, int rows, int K, int N, void* stream) {
    if (!V || !U || !Mt || nb <= 0 || rows <= 0 || rows % 128 || K <= 0 || K % 16 || N <= 0 || N % 128) return MRCNN_ERR_ARG;
    const long long M = (long long)nb * rows;
    if (M * K * 4 >= 0x7FFFFFF0LL || (long long)nb * K * N * 4 >= 0x7FFFFFF0LL || M * N >= (1LL << 40)) return MRCNN_ERR_UNSUPPORTED;
    // The wide tile (N = 256 whole: every V row block is fetched once; 166 VGPRs, 48 KiB LDS, 3 workgroups per CU) is 4-5 % faster
    // alone (F(4x4) layer: 1.25 -> 1.19 ms, 0.79 -> 0.83 of the matrix peak).  Inside the step it used to lose (F(2x2): 44.0 ->
    // 44.9 ms, less room for the other stream's kernels on a CU); with the F(4x4) layers it is level or slightly ahead on the
    // dense step (40.85 / 40.60 -> 40.61 / 40.51 ms) and level on the positive-quota step, so it is taken for products of at least
    // MRCNN_WINOGRAD_GEMM_WIDE_MIN (4096) wide tiles -- the dense layers and their halves; 0 = always, -1 = never.
    const char* wenv = getenv("MRCNN_WINOGRAD_GEMM_WIDE_MIN");                  // read per call (tests compare the two tiles)
    const long long wide_min = wenv ? atoll(wenv) : 4096;
    const bool wide = wide_min >= 0 && N % 256 == 0 && (M / 128) * (N / 256) >= wide_min;
    GemmDeconvEp none = {};
    if (wide) {                                                 // 128 x 256 tiles: 48 KiB LDS, 3 workgroups per CU
        const long long tiles = (M / 128) * (N / 256);
        const long long slots = 3LL * mrcnn_num_cus();
        const unsigned grid = (unsigned)(tiles < slots ? tiles : slots);
        hipLaunchKernelGGL((winograd_gemm_kernel<4, false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, V, U, Mt, rows, K, N, (int)tiles,
                           (unsigned)(M * K * 4), none);
        return mrcnn_launch_status();
    }
    const long long tiles = (M / 128) * (N / 128);
    const long long slots = 5LL * mrcnn_num_cus();
    const unsigned grid = (unsigned)(tiles < slots ? tiles : slots);
    hipLaunchKernelGGL((winograd_gemm_kernel<2, false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, V, U, Mt, rows, K, N, (int)tiles,
                       (unsigned)(M * K * 4), none);
    return mrcnn_launch_status();
}

/* Conv2DTranspose(2 x 2, stride 2) as ONE product [N H W x Cin] . [Cin x 4 Cd] on the persistent GEMM above with the pixel-shuffle
 * store in its epilogue (bias, ReLU): K is one filter tap deep (256 in the mask head), the case the persistent form exists for.
 * w_gemm [Cin][(a, b, co)]; out [N][2 H][2 W][Cd].  Cin % 16 == 0, Cd % 32 == 0, 4 Cd % 128 == 0. */
extern "C" int mrcnn_deconv2x2_gemm(const float* x, const float* w_gemm, const float* bias, float* out, int N, int H, int W, int Cin, int Cd,
                                    int act, void* stream) {
    if (!x || !w_gemm || !out || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cd <= 0) return MRCNN_ERR_ARG;
    if (act != MRCNN_ACT_NONE && act != MRCNN_ACT_RELU) return MRCNN_ERR_UNSUPPORTED;
    const long long M = (long long)N * H * W;
    const int Nn = 4 * Cd;
    if (Cin % 16 || Cd % 32 || Nn % 128 || M * Cin * 4 >= 0x7FFFFFF0LL || (long long)Cin * Nn * 4 >= 0x7FFFFFF0LL || M >= (1LL << 31) - 128)
        return MRCNN_ERR_UNSUPPORTED;
    GemmDeconvEp ep = {};
    ep.bias = bias; ep.Cd = Cd; ep.H = H; ep.W = W; ep.act = act;
    ep.d_hw = make_fastdiv((unsigned)(H * W)); ep.d_w = make_fastdiv((unsigned)W);
    const long long tiles = ((M + 127) / 128) * (Nn / 128);
    const long long slots = 5LL * mrcnn_num_cus();
    const unsigned grid = (unsigned)(tiles < slots ? tiles : slots);
    const int rows = (int)((M + 127) / 128 * 128);              // one matrix: every tile uses weight matrix 0
    hipLaunchKernelGGL((winograd_gemm_kernel<2, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, x, w_gemm, out, rows, Cin, Nn, (int)tiles,
                       (unsigned)(M * Cin * 4), ep);
    return mrcnn_launch_status();
}

/* The mask head's output stage in one launch: the transposed convolution above on the wide tile, with the mrcnn_mask 1 x 1
 * convolution (Cd -> C), its bias and the sigmoid in the same epilogue -- `up` is not read back.  up [N][2 H][2 W][Cd] may be NULL
 * (inference: not stored); w_mask [Cd][C], b_mask [C] or NULL, mask_out [N][2 H][2 W][C].  Cd == 256, 1 <= C <= 16. */
extern "C" int mrcnn_deconv2x2_mask_gemm(const float* x, const float* w_gemm, const float* bias, float* up, const float* w_mask,
                                         const float* b_mask, float* mask_out, int N, int H, int W, int Cin, int Cd, int C, int act,
                                         void* stream) {
    if (!x || !w_gemm || !w_mask || !mask_out || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cd <= 0) return MRCNN_ERR_ARG;
    if (act != MRCNN_ACT_NONE && act != MRCNN_ACT_RELU) return MRCNN_ERR_UNSUPPORTED;
    if (Cd != 256 || C < 1 || C > 16) return MRCNN_ERR_UNSUPPORTED;
    const long long M = (long long)N * H * W;
    const int Nn = 4 * Cd;
    if (Cin % 16 || M * Cin * 4 >= 0x7FFFFFF0LL || (long long)Cin * Nn * 4 >= 0x7FFFFFF0LL || M >= (1LL << 31) - 128)
        return MRCNN_ERR_UNSUPPORTED;
    GemmMaskEp ep = {};
    ep.bias = bias; ep.Cd = Cd; ep.H = H; ep.W = W; ep.act = act;
    ep.d_hw = make_fastdiv((unsigned)(H * W)); ep.d_w = make_fastdiv((unsigned)W);
    ep.w_mask = w_mask; ep.b_mask = b_mask; ep.m = mask_out; ep.C = C;
    const long long tiles = ((M + 127) / 128) * (Nn / 256);
    const long long slots = 3LL * mrcnn_num_cus();              // 128 x 256 tiles, as the wide Winograd launch
    const unsigned grid = (unsigned)(tiles < slots ? tiles : slots);
    const int rows = (int)((M + 127) / 128 * 128);
    hipLaunchKernelGGL((winograd_gemm_kernel<4, true, true>), dim3(grid), dim3(256), (size_t)256 * C * sizeof(float), (hipStream_t)stream, x,
                       w_gemm, up, rows, Cin, Nn, (int)tiles, (unsigned)(M * Cin * 4), ep);
    return mrcnn_launch_status();
}
