// Weight gradient of the implicit-GEMM convolution on the fp32 matrix cores:
//   dW[(kh,kw,ci), co] = sum over pixels m of  X[n, oh*s+kh-pt, ow*s+kw-pl, ci] * dY[m, co]
// (the reference obtains it from TF autodiff of KL.Conv2D; mrcnn/model.py:2487 fit_generator).
// GEMM view: rows i = (tap, ci) in [0, K), columns co, contraction over the M = N*OH*OW pixels.
// A workgroup owns a BI x BN tile of dW for one pixel range ("split"); BI divides Cin on the fast path
// so the tile sits inside one filter tap and its X rows are contiguous channel runs.  Both operands are
// staged pixel-major in LDS ([32 pixels][channels]) which is already the layout the 32x32x2 MFMA wants
// (lane = channel, k = pixel): every LDS read is a conflict-free ds_read_b32.  Splits write partial
// slabs that a second kernel sums in a fixed order, so dW is bitwise reproducible.
#include "common.h"
#include <type_traits>

struct WgradArgs {
    const float* x; const float* dy; float* out;   // out: dw (splits==1) or slabs
    int N, H, W, Cin, Cout, KH, KW, stride, pad_t, pad_l, OH, OW;
    int M, Ktot, fast, splits, chunk, acc;
    FastDiv d_ohw, d_ow;
    const PixelEntry* table;      // large layers: per-pixel offsets / tap masks (conv_wgrad_blds_kernel<.., true>)
};

template <int BI, int BN, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64, 2) void conv_wgrad_kernel(const WgradArgs p) {
    constexpr int NT = WM * WN * 64;
    constexpr int TM = BI / WM / 32, TN = BN / WN / 32;
    constexpr int XST = BI + 4, YST = BN + 4;
    constexpr int XV = 8 * BI / NT, YV = 8 * BN / NT;     // float4 loads per thread per step
    __shared__ __attribute__((aligned(16))) float lds[32 * XST + 32 * YST];
    float* Xs = lds;
    float* Ys = lds + 32 * XST;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int ntiles = (p.Cout + BN - 1) / BN;
    const int itiles = (p.Ktot + BI - 1) / BI;
    int bid = blockIdx.x;
    const int ntile = bid % ntiles; bid /= ntiles;
    const int itile = bid % itiles;
    const int split = bid / itiles;
    const int i0 = itile * BI, n0 = ntile * BN;
    const int m_begin = split * p.chunk;
    const int m_end = (m_begin + p.chunk < p.M) ? m_begin + p.chunk : p.M;
    const int tap = i0 / p.Cin, ci0 = i0 - tap * p.Cin;
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
    const int ohw = p.OH * p.OW;

    f32x4 rx[XV], ry[YV];
    auto load_tiles = [&](int mb) {
#pragma unroll
        for (int v = 0; v < XV; ++v) {
            const int idx = tid + v * NT;
            const int row = idx / (BI / 4), c4 = idx % (BI / 4);
            const int m = mb + row;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (m < m_end) {
                const int n = (int)fast_div((unsigned)m, p.d_ohw), rem = m - n * ohw;
                const int oh = (int)fast_div((unsigned)rem, p.d_ow), ow = rem - oh * p.OW;
                if (p.fast) {
                    const int ih = oh * p.stride - p.pad_t + kh, iw = ow * p.stride - p.pad_l + kw;
                    if ((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W)
                        val = *(const f32x4*)(p.x + (((long long)n * p.H + ih) * p.W + iw) * p.Cin + ci0 + c4 * 4);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = i0 + c4 * 4 + e;
                        if (i < p.Ktot) {
                            const int t2 = i / p.Cin, ci = i - t2 * p.Cin;
                            const int k2 = t2 / p.KW, l2 = t2 - k2 * p.KW;
                            const int ih = oh * p.stride - p.pad_t + k2, iw = ow * p.stride - p.pad_l + l2;
                            if ((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W)
                                val[e] = p.x[(((long long)n * p.H + ih) * p.W + iw) * p.Cin + ci];
                        }
                    }
                }
            }
            rx[v] = val;
        }
#pragma unroll
        for (int v = 0; v < YV; ++v) {
            const int idx = tid + v * NT;
            const int row = idx / (BN / 4), c4 = idx % (BN / 4);
            const int m = mb + row, n = n0 + c4 * 4;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (m < m_end) {
                const float* ptr = p.dy + (long long)m * p.Cout + n;
                if ((p.Cout & 3) == 0) {
                    if (n < p.Cout) val = *(const f32x4*)ptr;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (n + e < p.Cout) val[e] = ptr[e];
                }
            }
            ry[v] = val;
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int v = 0; v < XV; ++v) {
            const int idx = tid + v * NT;
            *(f32x4*)&Xs[(idx / (BI / 4)) * XST + (idx % (BI / 4)) * 4] = rx[v];
        }
#pragma unroll
        for (int v = 0; v < YV; ++v) {
            const int idx = tid + v * NT;
            *(f32x4*)&Ys[(idx / (BN / 4)) * YST + (idx % (BN / 4)) * 4] = ry[v];
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int li = lane & 31, lh = lane >> 5;
    if (m_begin < m_end) {
        load_tiles(m_begin);
        store_tiles();
        __syncthreads();
        for (int mb = m_begin; mb < m_end; mb += 32) {
            const bool more = mb + 32 < m_end;
            if (more) load_tiles(mb + 32);
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int prow = lh * 16 + t;
                float av[TM], bv[TN];
#pragma unroll
                for (int a = 0; a < TM; ++a) av[a] = Xs[prow * XST + wm * TM * 32 + a * 32 + li];
#pragma unroll
                for (int b = 0; b < TN; ++b) bv[b] = Ys[prow * YST + wn * TN * 32 + b * 32 + li];
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int b = 0; b < TN; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
            }
            __syncthreads();
            if (more) {
                store_tiles();
                __syncthreads();
            }
        }
    }

    float* dst = p.out + (p.splits > 1 ? (long long)split * p.Ktot * p.Cout : 0LL);
    const bool accumulate = p.splits == 1 && p.acc;
    auto store_tile = [&](const f32x16& c, int ibase, int n) {
        if (n >= p.Cout) return;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = ibase + (r & 3) + 8 * (r >> 2);
            if (i < p.Ktot) {
                float* q = dst + (long long)i * p.Cout + n;
                *q = accumulate ? *q + c[r] : c[r];
            }
        }
    };
    const int ib = i0 + wm * TM * 32 + 4 * lh, nb = n0 + wn * TN * 32 + li;
    if constexpr (TM >= 1 && TN >= 1) store_tile(acc[0][0], ib, nb);
    if constexpr (TM >= 1 && TN >= 2) store_tile(acc[0][1], ib, nb + 32);
    if constexpr (TM >= 2 && TN >= 1) store_tile(acc[1][0], ib + 32, nb);
    if constexpr (TM >= 2 && TN >= 2) store_tile(acc[1][1], ib + 32, nb + 32);
}

// ---------------------------------------------------------------------------------------------------
// LDS-DMA variant for full tiles (Cin % BI == 0, Cout % BN == 0): both operand tiles are [BP pixels][128
// channels] with 512-byte rows, exactly the lane-linear image a `global_load_lds_dwordx4` writes (1 KiB =
// 2 rows per wave-instruction) and exactly what the MFMA operand reads want (lane = channel: conflict-free
// ds_read_b32, no padding, no swizzle).  No staging VGPRs, no ds_write, one barrier per step: the DMA of
// step t+1 lands in the other LDS buffer while the MFMAs of step t run.  Out-of-image taps and rows past
// the pixel range read from a 64-byte zero page instead of being masked.
__device__ __attribute__((aligned(64))) float g_zero_page[16];

#ifndef WGRAD_BP
#define WGRAD_BP 16
#endif

__device__ __forceinline__ void glds16(const float* gsrc, float* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

template <int BI, int BN, int BP>
__global__ __launch_bounds__(256, 2) void conv_wgrad_glds_kernel(const WgradArgs p) {
    constexpr int TM = BI / 2 / 32, TN = BN / 2 / 32;
    constexpr int XF = BP * BI, YF = BP * BN;
    constexpr int NXI = XF / 256, NYI = YF / 256;            // 1 KiB DMA pieces per tile
    constexpr int XLPR = BI / 4, YLPR = BN / 4;              // lanes per row
    constexpr int XRPI = 64 / XLPR, YRPI = 64 / YLPR;        // rows per piece
    __shared__ __attribute__((aligned(16))) float lds[2 * (XF + YF)];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ntiles = p.Cout / BN, itiles = p.Ktot / BI;
    int bid = blockIdx.x;
    const int ntile = bid % ntiles; bid /= ntiles;
    const int itile = bid % itiles;
    const int split = bid / itiles;
    const int i0 = itile * BI, n0 = ntile * BN;
    const int m_begin = split * p.chunk;
    const int m_end = (m_begin + p.chunk < p.M) ? m_begin + p.chunk : p.M;
    const int tap = i0 / p.Cin, ci0 = i0 - tap * p.Cin;
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
    const int ohw = p.OH * p.OW;

    auto stage = [&](int buf, int mb) {
        float* xb = lds + buf * (XF + YF);
        float* yb = xb + XF;
#pragma unroll
        for (int jj = 0; jj < (NXI + 3) / 4; ++jj) {
            const int j = wave + jj * 4;
            if (j < NXI) {
                const int m = mb + j * XRPI + lane / XLPR, c4 = lane % XLPR;
                const float* src = g_zero_page;
                if (m < m_end) {
                    const int n = (int)fast_div((unsigned)m, p.d_ohw), rem = m - n * ohw;
                    const int oh = (int)fast_div((unsigned)rem, p.d_ow), ow = rem - oh * p.OW;
                    const int ih = oh * p.stride - p.pad_t + kh, iw = ow * p.stride - p.pad_l + kw;
                    if ((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W)
                        src = p.x + (((long long)n * p.H + ih) * p.W + iw) * p.Cin + ci0 + c4 * 4;
                }
                glds16(src, xb + j * 256);
            }
        }
#pragma unroll
        for (int jj = 0; jj < (NYI + 3) / 4; ++jj) {
            const int j = wave + jj * 4;
            if (j < NYI) {
                const int m = mb + j * YRPI + lane / YLPR, c4 = lane % YLPR;
                const float* src = (m < m_end) ? p.dy + (long long)m * p.Cout + n0 + c4 * 4 : g_zero_page;
                glds16(src, yb + j * 256);
            }
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int li = lane & 31, lh = lane >> 5;
    if (m_begin < m_end) {
        stage(0, m_begin);
        __syncthreads();
        int cur = 0;
        for (int mb = m_begin; mb < m_end; mb += BP) {
            if (mb + BP < m_end) stage(cur ^ 1, mb + BP);
            const float* xb = lds + cur * (XF + YF);
            const float* yb = xb + XF;
#pragma unroll
            for (int t = 0; t < BP / 2; ++t) {
                const int prow = lh * (BP / 2) + t;
                float av[TM], bv[TN];
#pragma unroll
                for (int a = 0; a < TM; ++a) av[a] = xb[prow * BI + wm * TM * 32 + a * 32 + li];
#pragma unroll
                for (int b = 0; b < TN; ++b) bv[b] = yb[prow * BN + wn * TN * 32 + b * 32 + li];
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int b = 0; b < TN; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
            }
            __syncthreads();
            cur ^= 1;
        }
    }

    float* dst = p.out + (p.splits > 1 ? (long long)split * p.Ktot * p.Cout : 0LL);
    const bool accumulate = p.splits == 1 && p.acc;
    auto store_tile = [&](const f32x16& c, int ibase, int n) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = ibase + (r & 3) + 8 * (r >> 2);
            float* q = dst + (long long)i * p.Cout + n;
            *q = accumulate ? *q + c[r] : c[r];
        }
    };
    const int ib = i0 + wm * TM * 32 + 4 * lh, nb = n0 + wn * TN * 32 + li;
    if constexpr (TM >= 1 && TN >= 1) store_tile(acc[0][0], ib, nb);
    if constexpr (TM >= 1 && TN >= 2) store_tile(acc[0][1], ib, nb + 32);
    if constexpr (TM >= 2 && TN >= 1) store_tile(acc[1][0], ib + 32, nb);
    if constexpr (TM >= 2 && TN >= 2) store_tile(acc[1][1], ib + 32, nb + 32);
}

// Same tile with buffer addressing (default; the flat variant above stays for tensors >= 2 GiB).  The flat
// variant spends ~3 vector instructions per MFMA on per-lane pixel decomposition (two divisions), bounds
// tests and 64-bit pointers, and vector instructions do not overlap the matrix pipe of their SIMD.  Here a
// 1 KiB piece = two pixel rows, so the pixel -> (n, oh, ow) decomposition is wave-uniform and runs on the
// SCALAR unit; a lane only selects one of the two row offsets and adds its channel offset (3 vector
// instructions per X piece, none per dY piece); padded taps and rows past the tensor take an out-of-range
// offset and the buffer range check writes zeros; the dY descriptor is rebuilt per piece (scalar) with the
// rows left in this split as its size, so the pixel tail needs no per-lane test either.  The loop is
// unrolled over the two LDS buffers: every LDS read is base register + immediate.
typedef __attribute__((address_space(3))) void* wgrad_lds_ptr;
#define WGRAD_OOB_OFFSET 0x80000000u

template <int BP, bool TABLE>
__device__ __forceinline__ void conv_wgrad_blds_body(const WgradArgs& p, const unsigned x_shift, const unsigned x_records,
                                                     const int block) {
    constexpr int BI = 128, BN = 128, TM = 2, TN = 2;
    constexpr int XF = BP * BI, YF = BP * BN;
    constexpr int NP = XF / 256;                              // 1 KiB pieces per tile (two pixel rows each)
    __shared__ __attribute__((aligned(16))) float lds[2 * (XF + YF)];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int ntiles = p.Cout / BN, itiles = p.Ktot / BI;
    int bid = block;
    const int ntile = bid % ntiles; bid /= ntiles;
    const int itile = bid % itiles;
    const int split = bid / itiles;
    const int i0 = itile * BI, n0 = ntile * BN;
    const int m_begin = split * p.chunk;
    const int m_end = (m_begin + p.chunk < p.M) ? m_begin + p.chunk : p.M;
    const int tap = i0 / p.Cin, ci0 = i0 - tap * p.Cin;
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
    const int ohw = p.OH * p.OW;

    const __amdgpu_buffer_rsrc_t rsrc_x =
        __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.x - x_shift), 0, x_records, 0x00020000);
    const unsigned lane_chan = (unsigned)(lane & 31) * 16u;
    const bool upper = lane >= 32;
    const unsigned y_voff = (unsigned)(((lane >> 5) * p.Cout + (lane & 31) * 4) * 4);

    // TABLE (layers with many pixels): the row offsets and tap masks come from a table built once per call and are
    // prefetched one step ahead -- nothing but a bit test is left per piece; otherwise the decomposition runs on the
    // scalar unit (no extra launch for the many small layers).
    const unsigned soff_tab = (unsigned)(((kh * p.W + kw) * p.Cin + ci0) * 4);
    const unsigned tapbit = 1u << (tap & 31);
    const bool tap_hi = tap >= 32;
    const PixelEntry* tab = TABLE ? p.table + (lane >> 5) : nullptr;
    PixelEntry ent[NP / 4];
    auto fetch = [&](int mb) {
        if constexpr (TABLE) {
#pragma unroll
            for (int jj = 0; jj < NP / 4; ++jj) ent[jj] = tab[mb + 2 * (wave + jj * 4)];
        }
    };
    auto stage = [&](float* xb, int mb) {
        float* yb = xb + XF;
#pragma unroll
        for (int jj = 0; jj < NP / 4; ++jj) {
            const int j = wave + jj * 4;
            if constexpr (TABLE) {
                const unsigned word = tap_hi ? ent[jj].mask_hi : ent[jj].mask_lo;
                const unsigned vo = ((word & tapbit) ? ent[jj].off : WGRAD_OOB_OFFSET) + lane_chan;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (wgrad_lds_ptr)(xb + j * 256), 16, vo, soff_tab, 0, 0);
                continue;
            }
            unsigned off[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {                       // wave-uniform: scalar unit
                const int m = mb + j * 2 + h;
                const int n = (int)fast_div((unsigned)m, p.d_ohw), rem = m - n * ohw;
                const int oh = (int)fast_div((unsigned)rem, p.d_ow), ow = rem - oh * p.OW;
                const int ih = oh * p.stride - p.pad_t + kh, iw = ow * p.stride - p.pad_l + kw;
                const bool ok = (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
                off[h] = ok ? (unsigned)((((n * p.H + ih) * p.W + iw) * p.Cin + ci0) * 4) + x_shift : WGRAD_OOB_OFFSET;
            }
            const unsigned vo = (upper ? off[1] : off[0]) + lane_chan;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (wgrad_lds_ptr)(xb + j * 256), 16, vo, 0, 0, 0);
        }
#pragma unroll
        for (int jj = 0; jj < NP / 4; ++jj) {
            const int j = wave + jj * 4;
            const int row0 = mb + j * 2;
            const int left = m_end - row0;                      // rows of this split from row0 on
            const unsigned rec = left > 0 ? (unsigned)(((left - 1) * p.Cout + BN) * 4) : 0u;
            const __amdgpu_buffer_rsrc_t rsrc_y =
                __builtin_amdgcn_make_buffer_rsrc((void*)(p.dy + (long long)row0 * p.Cout + n0), 0, rec, 0x00020000);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_y, (wgrad_lds_ptr)(yb + j * 256), 16, y_voff, 0, 0, 0);
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int li = lane & 31, lh = lane >> 5;
    const float* x_rd = lds + lh * (BP / 2) * BI + wm * TM * 32 + li;
    const float* y_rd = lds + XF + lh * (BP / 2) * BN + wn * TN * 32 + li;
    auto compute = [&](auto curc) {
        constexpr int BO = decltype(curc)::value * (XF + YF);
#pragma unroll
        for (int t = 0; t < BP / 2; ++t) {
            float av[TM], bv[TN];
#pragma unroll
            for (int a = 0; a < TM; ++a) av[a] = x_rd[BO + t * BI + a * 32];
#pragma unroll
            for (int b = 0; b < TN; ++b) bv[b] = y_rd[BO + t * BN + b * 32];
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
    };

    if (m_begin < m_end) {
        // Table entries are fetched one half-step ahead of the stage() that consumes them, UNCONDITIONALLY (index
        // clamped into the table, which carries BP rows past M): a fetch under `if (more rows)` makes the entries a
        // conditional loop-carried value, the compiler copies the freshly loaded registers at the join, and the wait
        // those copies need (vmcnt(0): younger than the LDS-DMA just issued) stalled every step until the next
        // tile's DMA had landed -- no overlap of DMA and MFMA left (the table variant ran at 79 % MFMA-busy).
        auto fetch_at = [&](int mb) { fetch(mb < p.M ? mb : p.M); };
        fetch(m_begin);
        stage(lds, m_begin);
        fetch_at(m_begin + BP);
        __syncthreads();
        for (int mb = m_begin; mb < m_end; mb += 2 * BP) {
            const bool has1 = mb + BP < m_end;
            if (has1) stage(lds + (XF + YF), mb + BP);
            fetch_at(mb + 2 * BP);
            compute(std::integral_constant<int, 0>{});
            __syncthreads();
            if (has1 && mb + 2 * BP < m_end) stage(lds, mb + 2 * BP);
            fetch_at(mb + 3 * BP);
            if (has1) {
                compute(std::integral_constant<int, 1>{});
                __syncthreads();
            }
        }
    }

    float* dst = p.out + (p.splits > 1 ? (long long)split * p.Ktot * p.Cout : 0LL);
    const bool accumulate = p.splits == 1 && p.acc;
    auto store_tile = [&](const f32x16& c, int ibase, int n) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = ibase + (r & 3) + 8 * (r >> 2);
            float* q = dst + (long long)i * p.Cout + n;
            *q = accumulate ? *q + c[r] : c[r];
        }
    };
    const int ib = i0 + wm * TM * 32 + 4 * lh, nb = n0 + wn * TN * 32 + li;
    store_tile(acc[0][0], ib, nb);
    store_tile(acc[0][1], ib, nb + 32);
    store_tile(acc[1][0], ib + 32, nb);
    store_tile(acc[1][1], ib + 32, nb + 32);
}

template <int BP, bool TABLE>
__global__ __launch_bounds__(256, 2) void conv_wgrad_blds_kernel(const WgradArgs p, const unsigned x_shift, const unsigned x_records) {
    conv_wgrad_blds_body<BP, TABLE>(p, x_shift, x_records, (int)blockIdx.x);
}

// Up to WGRAD_MULTI_MAX weight gradients in one launch (mrcnn_conv2d_wgrad_multi): the three convolutions of a
// bottleneck block.  Workgroups first[g] .. first[g+1]-1 belong to problem g; the slab reductions share a launch too.
#define WGRAD_MULTI_MAX 16      // 4 covers a bottleneck block; 16 = the transform-domain weight gradients of a Winograd F(2x2) layer (F(4x4): 3 x 12; 18 per launch measured no faster)
struct WgradMultiArgs {
    WgradArgs a[WGRAD_MULTI_MAX];
    unsigned x_shift[WGRAD_MULTI_MAX], x_records[WGRAD_MULTI_MAX];
    int first[WGRAD_MULTI_MAX + 1];
    float* dw[WGRAD_MULTI_MAX];
    int rfirst[WGRAD_MULTI_MAX + 1];      // reduction launch: blocks of 256 float4
    int n;
};

static_assert(sizeof(WgradMultiArgs) <= 4096, "kernel argument block");

template <int BP>
__global__ __launch_bounds__(256, 2) void conv_wgrad_blds_multi_kernel(const WgradMultiArgs mp) {
    int g = 0;
    while (g + 1 < mp.n && (int)blockIdx.x >= mp.first[g + 1]) ++g;
    conv_wgrad_blds_body<BP, false>(mp.a[g], mp.x_shift[g], mp.x_records[g], (int)blockIdx.x - mp.first[g]);
}

__global__ void wgrad_reduce_multi_kernel(const WgradMultiArgs mp) {
    int g = 0;
    while (g + 1 < mp.n && (int)blockIdx.x >= mp.rfirst[g + 1]) ++g;
    const WgradArgs& p = mp.a[g];
    if (p.splits <= 1) return;
    const long long n4 = (long long)p.Ktot * p.Cout / 4;
    const long long i = (long long)(blockIdx.x - mp.rfirst[g]) * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (p.acc) s = *(const f32x4*)(mp.dw[g] + 4 * i);
    *(f32x4*)(mp.dw[g] + 4 * i) = mrcnn_slab_sum<f32x4>(s, p.out, 4 * n4, 4 * i, p.splits);

}

__global__ void wgrad_reduce_kernel(const float* __restrict__ slabs, float* dw, long long n, int splits, int acc) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    dw[i] = mrcnn_slab_sum<float>(acc ? dw[i] : 0.f, slabs, n, i, splits);
}

// n % 4 == 0, 16-byte aligned buffers: four elements per thread
__global__ void wgrad_reduce_vec_kernel(const float* __restrict__ slabs, float* dw, long long n4, int splits, int acc) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (acc) s = *(const f32x4*)(dw + 4 * i);
    *(f32x4*)(dw + 4 * i) = mrcnn_slab_sum<f32x4>(s, slabs, 4 * n4, 4 * i, splits);
}

// ---------------------------------------------------------------------------------------------------
// Host side: validate, plan, launch.  One plan (mrcnn_wgrad_plan / mrcnn_wgrad_multi_plan, include/mrcnn_hip.h) states what
// a launch does; the workspace queries, the host-only *_plan entry points and the launches all read it.
// tests/golden/wgrad_plan_table.json pins it row by row.
#define WGRAD_TARGET_WGS 1024        // workgroups a launch aims at: four per CU (what a launch gets beside another stream's kernels;
                                     // 1280 = all five slots per CU -- the 36 transform-domain GEMMs of a Winograd layer go 48 tiles
                                     // x 21 -> x 26 splits -- measured 0.3 ms slower on the dense step)
#define WGRAD_MIN_PIXELS 128         // a pixel split contracts at least this many pixels
#define WGRAD_MAX_SPLITS 64
#define WGRAD_TABLE_MIN_PIXELS 65536 // layers with at least this many output pixels address X through the pixel table (one extra tiny launch)
#define WGRAD_TABLE_MAX_TAPS 64      // the table's tap mask has 64 bits
#define WGRAD_BUFFER_RANGE 0x7FFFFFF0LL

static inline long long wgrad_pixels(const mrcnn_conv_desc* d) { return (long long)d->N * d->OH * d->OW; }
static inline bool wgrad_dims_positive(const mrcnn_conv_desc* d) {
    return d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0 && d->KH > 0 && d->KW > 0 && d->stride > 0 && d->OH > 0 && d->OW > 0;
}
static inline bool wgrad_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// X as the LDS-DMA kernels' buffer descriptor sees it: the base moved back by the padding (x_shift bytes), x_records bytes long
static inline long long wgrad_x_bytes(const mrcnn_conv_desc* d) { return (long long)d->N * d->H * d->W * d->Cin * 4; }
static inline long long wgrad_x_shift(const mrcnn_conv_desc* d) { return ((long long)d->pad_t * d->W + d->pad_l) * d->Cin * 4; }
// both operands within a 32-bit buffer descriptor; + 16 pixel rows: offsets of rows past the tensor must not wrap before the
// range check sees them
static inline bool wgrad_in_buffer_range(const mrcnn_conv_desc* d) {
    return wgrad_x_bytes(d) + wgrad_x_shift(d) + 16LL * d->H * d->W * d->Cin * 4 < WGRAD_BUFFER_RANGE &&
           wgrad_pixels(d) * d->Cout * 4 < WGRAD_BUFFER_RANGE;
}
// whole 128 x 128 tiles of dW inside one filter tap: the LDS-DMA kernels (buffer addressed, or flat where a tensor is out of range)
static inline bool wgrad_dma_shape(const mrcnn_conv_desc* d) { return d->Cin % 128 == 0 && d->Cout % 128 == 0; }
static inline bool wgrad_wants_table(const mrcnn_conv_desc* d) {
    return wgrad_dma_shape(d) && d->KH * d->KW <= WGRAD_TABLE_MAX_TAPS && wgrad_pixels(d) >= WGRAD_TABLE_MIN_PIXELS;
}
static inline size_t wgrad_table_bytes(const mrcnn_conv_desc* d) {
    return wgrad_wants_table(d) ? (size_t)(wgrad_pixels(d) + WGRAD_BP) * sizeof(PixelEntry) + 256 : 0;
}
static inline size_t wgrad_slab_bytes(const mrcnn_conv_desc* d, int splits) {
    return splits > 1 ? (size_t)splits * d->KH * d->KW * d->Cin * d->Cout * sizeof(float) : 0;
}
static inline long long wgrad_tiles(const mrcnn_conv_desc* d, int bi, int bn) {
    return (((long long)d->KH * d->KW * d->Cin + bi - 1) / bi) * ((d->Cout + bn - 1) / bn);
}

// `want` splits of M pixels -> splits of `chunk` pixels each: at least WGRAD_MIN_PIXELS per split, at most WGRAD_MAX_SPLITS,
// chunks whole 32-pixel steps (which can lower the count again)
static void wgrad_pixel_split(long long want, long long M, int32_t* splits, int32_t* chunk) {
    const long long cap = (M + WGRAD_MIN_PIXELS - 1) / WGRAD_MIN_PIXELS;
    long long s = want > cap ? cap : want;
    if (s < 1) s = 1;
    if (s > WGRAD_MAX_SPLITS) s = WGRAD_MAX_SPLITS;
    const long long c = ((M + s - 1) / s + 31) / 32 * 32;
    *chunk = (int32_t)c;
    *splits = c != 0 ? (int32_t)((M + c - 1) / c) : 1;
}

// what depends on the descriptor alone (all the workspace query needs): tile, kernel family, pixel split, workspace
static void wgrad_plan_shape(const mrcnn_conv_desc* d, mrcnn_wgrad_plan* p) {
    *p = mrcnn_wgrad_plan{};
    p->bi = d->Cin % 128 == 0 ? 128 : 64;
    p->fast = d->Cin % 64 == 0;                     // the tile sits inside one filter tap
    p->bn = d->Cout >= 128 ? 128 : (d->Cout >= 64 ? 64 : 32);
    if (!wgrad_dma_shape(d)) p->kernel = MRCNN_WGRAD_TILE;
    else p->kernel = wgrad_in_buffer_range(d) && !mrcnn_force_flat_glds() ? MRCNN_WGRAD_BLDS : MRCNN_WGRAD_GLDS;
    const long long tiles = wgrad_tiles(d, p->bi, p->bn);
    wgrad_pixel_split(WGRAD_TARGET_WGS / (tiles > 0 ? tiles : 1), wgrad_pixels(d), &p->splits, &p->chunk);
    p->grid = (int32_t)(tiles * p->splits);
    p->lds_bytes = p->kernel == MRCNN_WGRAD_BLDS ? g_mrcnn_wgrad_lds_pad : 0;
    p->table_bytes = (int64_t)wgrad_table_bytes(d);
    p->slab_bytes = (int64_t)wgrad_slab_bytes(d, p->splits);
    p->workspace_bytes = p->slab_bytes + p->table_bytes;
}

extern "C" size_t mrcnn_conv2d_wgrad_workspace(const mrcnn_conv_desc* d) {
    if (!d || d->N <= 0 || d->Cin <= 0 || d->Cout <= 0) return 0;
    mrcnn_wgrad_plan p;
    wgrad_plan_shape(d, &p);
    return (size_t)p.workspace_bytes;
}

extern "C" int mrcnn_conv2d_wgrad_plan(const mrcnn_conv_desc* d, const float* x, const float* dy, const float* dw,
                                       const void* workspace, size_t workspace_bytes, mrcnn_wgrad_plan* plan) {
    if (!d || !x || !dy || !dw || !plan) return MRCNN_ERR_ARG;
    if (!wgrad_dims_positive(d) || wgrad_pixels(d) >= (1LL << 31)) return MRCNN_ERR_ARG;
    if (!wgrad_aligned16(x) || !wgrad_aligned16(dy)) return MRCNN_ERR_ARG;
    mrcnn_wgrad_plan p;
    wgrad_plan_shape(d, &p);
    if (p.splits > 1 && (!workspace || workspace_bytes < (size_t)p.slab_bytes)) return MRCNN_ERR_WORKSPACE;
    // the pixel table where the workspace holds it behind the slabs; a shorter one runs the kernel without it
    if (p.kernel == MRCNN_WGRAD_BLDS && p.table_bytes && workspace && workspace_bytes >= (size_t)p.workspace_bytes) {
        p.kernel = MRCNN_WGRAD_BLDS_TABLE;
        p.table_grid = (int32_t)cdiv64(wgrad_pixels(d) + WGRAD_BP, 256);
    }
    if (p.splits > 1) {
        const long long n = (long long)d->KH * d->KW * d->Cin * d->Cout;
        p.reduce = n % 4 == 0 && wgrad_aligned16(workspace) && wgrad_aligned16(dw) ? MRCNN_WGRAD_RED_VEC : MRCNN_WGRAD_RED_SCALAR;
        p.reduce_grid = (int32_t)(p.reduce == MRCNN_WGRAD_RED_VEC ? cdiv64(n / 4, 256) : cdiv64(n, 256));
    }
    *plan = p;
    return MRCNN_OK;
}

static WgradArgs wgrad_args(const mrcnn_conv_desc* d, const float* x, const float* dy, float* out, int fast, int splits, int chunk,
                            int acc) {
    WgradArgs a;
    a.x = x; a.dy = dy; a.out = out;
    a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout; a.KH = d->KH; a.KW = d->KW;
    a.stride = d->stride; a.pad_t = d->pad_t; a.pad_l = d->pad_l; a.OH = d->OH; a.OW = d->OW;
    a.M = (int)wgrad_pixels(d); a.Ktot = d->KH * d->KW * d->Cin; a.fast = fast; a.splits = splits; a.chunk = chunk;
    a.acc = acc;
    a.d_ohw = make_fastdiv((unsigned)(d->OH * d->OW)); a.d_ow = make_fastdiv((unsigned)d->OW);
    a.table = nullptr;
    return a;
}

template <int BI, int BN, int WM, int WN>
static void launch_wgrad_tile(const WgradArgs& a, unsigned grid, hipStream_t s) {
    hipLaunchKernelGGL((conv_wgrad_kernel<BI, BN, WM, WN>), dim3(grid), dim3(WM * WN * 64), 0, s, a);
}

extern "C" int mrcnn_conv2d_wgrad(const mrcnn_conv_desc* d, const float* x, const float* dy, float* dw,
                                  float* workspace, size_t workspace_bytes, int beta_acc, void* stream) {
    mrcnn_wgrad_plan p;
    const int rc = mrcnn_conv2d_wgrad_plan(d, x, dy, dw, workspace, workspace_bytes, &p);
    if (rc != MRCNN_OK) return rc;
    WgradArgs a = wgrad_args(d, x, dy, p.splits > 1 ? workspace : dw, p.fast, p.splits, p.chunk, beta_acc);
    const unsigned x_shift = (unsigned)wgrad_x_shift(d), x_records = (unsigned)(wgrad_x_bytes(d) + wgrad_x_shift(d));
    const unsigned grid = (unsigned)p.grid;
    hipStream_t s = (hipStream_t)stream;
    switch (p.kernel) {
    case MRCNN_WGRAD_BLDS_TABLE: {
        const uintptr_t q = reinterpret_cast<uintptr_t>(workspace) + (size_t)p.slab_bytes;
        a.table = (const PixelEntry*)((q + 255) & ~(uintptr_t)255);
        hipLaunchKernelGGL(pixel_table_kernel, dim3((unsigned)p.table_grid), dim3(256), 0, s, (PixelEntry*)a.table, d->N, d->H, d->W,
                           d->Cin, d->KH, d->KW, d->stride, d->pad_t, d->pad_l, d->OH, d->OW, a.M, a.M + WGRAD_BP, x_shift, 4);
        hipLaunchKernelGGL((conv_wgrad_blds_kernel<WGRAD_BP, true>), dim3(grid), dim3(256), (size_t)p.lds_bytes, s, a, x_shift, x_records);
        break;
    }
    case MRCNN_WGRAD_BLDS:
        hipLaunchKernelGGL((conv_wgrad_blds_kernel<WGRAD_BP, false>), dim3(grid), dim3(256), (size_t)p.lds_bytes, s, a, x_shift, x_records);
        break;
    case MRCNN_WGRAD_GLDS:
        hipLaunchKernelGGL((conv_wgrad_glds_kernel<128, 128, WGRAD_BP>), dim3(grid), dim3(256), 0, s, a);
        break;
    default:
        if (p.bi == 128 && p.bn == 128) launch_wgrad_tile<128, 128, 2, 2>(a, grid, s);
        else if (p.bi == 128 && p.bn == 64) launch_wgrad_tile<128, 64, 2, 2>(a, grid, s);
        else if (p.bi == 128) launch_wgrad_tile<128, 32, 4, 1>(a, grid, s);
        else if (p.bn == 128) launch_wgrad_tile<64, 128, 2, 2>(a, grid, s);
        else if (p.bn == 64) launch_wgrad_tile<64, 64, 2, 2>(a, grid, s);
        else launch_wgrad_tile<64, 32, 2, 1>(a, grid, s);
    }
    const long long n = (long long)a.Ktot * a.Cout;
    if (p.reduce == MRCNN_WGRAD_RED_VEC)
        hipLaunchKernelGGL(wgrad_reduce_vec_kernel, dim3((unsigned)p.reduce_grid), dim3(256), 0, s, (const float*)workspace, dw, n / 4,
                           p.splits, beta_acc);
    else if (p.reduce == MRCNN_WGRAD_RED_SCALAR)
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)p.reduce_grid), dim3(256), 0, s, workspace, dw, n, p.splits, beta_acc);
    return mrcnn_launch_status();
}

// ---------------------------------------------------------------------------------------------------
// mrcnn_conv2d_wgrad_multi: the weight gradients of up to WGRAD_MULTI_MAX layers in one launch (+ one for their slab
// reductions).  On the small feature maps of the backbone a weight gradient is 16-36 output tiles with a few hundred pixels to
// contract: ~30 us of mostly latency per launch plus its reduction, three per bottleneck block, and together they
// had become the longest chain of the backward pass (knock-out run: 2 ms of the step).  LDS-DMA kernel only, no pixel table.
static_assert(WGRAD_MULTI_MAX == MRCNN_WGRAD_MULTI_MAX, "mrcnn_wgrad_multi_plan holds one entry per problem");

// a problem the shared launch takes: the buffer-addressed LDS-DMA kernel without a pixel table (pure GEMM rows -- a 1 x 1
// layer on a 1 x 1 map -- have no pixel decomposition to pay for and need none at any size)
static bool wgrad_multi_fits(const mrcnn_conv_desc* d) {
    const bool gemm = d->KH == 1 && d->KW == 1 && d->H == 1 && d->W == 1 && d->stride == 1;
    return wgrad_dims_positive(d) && wgrad_dma_shape(d) && d->KH * d->KW <= WGRAD_TABLE_MAX_TAPS && (!wgrad_wants_table(d) || gemm) &&
           wgrad_in_buffer_range(d);
}

// the descriptors' part of the plan (all the workspace query needs, and what it answers whatever MRCNN_CONV_FLAT_GLDS says)
static bool wgrad_multi_plan_shape(const mrcnn_wgrad_problem* pr, int n, mrcnn_wgrad_multi_plan* p) {
    if (!pr || n < 1 || n > WGRAD_MULTI_MAX) return false;
    long long tiles = 0;
    for (int g = 0; g < n; ++g) {
        if (!wgrad_multi_fits(&pr[g].d)) return false;
        tiles += wgrad_tiles(&pr[g].d, 128, 128);
    }
    *p = mrcnn_wgrad_multi_plan{};
    p->n = n;
    const long long want = WGRAD_TARGET_WGS / (tiles > 0 ? tiles : 1);
    long long blocks = 0, rblocks = 0;
    for (int g = 0; g < n; ++g) {
        const mrcnn_conv_desc* d = &pr[g].d;
        wgrad_pixel_split(want, wgrad_pixels(d), &p->splits[g], &p->chunk[g]);
        p->slab_offset[g] = p->slab_bytes;
        p->slab_bytes += (int64_t)((wgrad_slab_bytes(d, p->splits[g]) + 255) & ~(size_t)255);
        p->first[g] = (int32_t)blocks;
        blocks += wgrad_tiles(d, 128, 128) * p->splits[g];
        p->rfirst[g] = (int32_t)rblocks;
        if (p->splits[g] > 1) rblocks += cdiv64((long long)d->KH * d->KW * d->Cin * d->Cout / 4, 256);      // blocks of 256 float4
    }
    for (int g = n; g <= WGRAD_MULTI_MAX; ++g) { p->first[g] = (int32_t)blocks; p->rfirst[g] = (int32_t)rblocks; }
    p->grid = (int32_t)blocks;
    p->reduce_grid = (int32_t)rblocks;
    p->workspace_bytes = p->slab_bytes + 256;
    return true;
}

extern "C" size_t mrcnn_conv2d_wgrad_multi_workspace(const mrcnn_wgrad_problem* problems, int n) {
    mrcnn_wgrad_multi_plan p;
    return wgrad_multi_plan_shape(problems, n, &p) ? (size_t)p.workspace_bytes : 0;
}

extern "C" int mrcnn_conv2d_wgrad_multi_plan(const mrcnn_wgrad_problem* problems, int n, const void* workspace, size_t workspace_bytes,
                                             mrcnn_wgrad_multi_plan* plan) {
    mrcnn_wgrad_multi_plan p;
    if (!plan) return MRCNN_ERR_ARG;
    if (!wgrad_multi_plan_shape(problems, n, &p) || mrcnn_force_flat_glds()) return MRCNN_ERR_UNSUPPORTED;
    if (p.slab_bytes && (!workspace || workspace_bytes < (size_t)p.slab_bytes || !wgrad_aligned16(workspace))) return MRCNN_ERR_WORKSPACE;
    for (int g = 0; g < n; ++g) {
        const mrcnn_wgrad_problem& q = problems[g];
        if (!q.x || !q.dy || !q.dw) return MRCNN_ERR_ARG;
        if (!wgrad_aligned16(q.x) || !wgrad_aligned16(q.dy) || !wgrad_aligned16(q.dw)) return MRCNN_ERR_UNSUPPORTED;
    }
    *plan = p;
    return MRCNN_OK;
}

extern "C" int mrcnn_conv2d_wgrad_multi(const mrcnn_wgrad_problem* problems, int n, float* workspace, size_t workspace_bytes,
                                        void* stream) {
    mrcnn_wgrad_multi_plan p;
    const int rc = mrcnn_conv2d_wgrad_multi_plan(problems, n, workspace, workspace_bytes, &p);
    if (rc != MRCNN_OK) return rc;
    WgradMultiArgs mp;
    mp.n = n;
    for (int g = 0; g < n; ++g) {
        const mrcnn_wgrad_problem& q = problems[g];
        float* out = p.splits[g] > 1 ? (float*)((char*)workspace + p.slab_offset[g]) : q.dw;
        mp.a[g] = wgrad_args(&q.d, q.x, q.dy, out, 1, p.splits[g], p.chunk[g], q.accumulate);
        mp.x_shift[g] = (unsigned)wgrad_x_shift(&q.d);
        mp.x_records[g] = (unsigned)(wgrad_x_bytes(&q.d) + wgrad_x_shift(&q.d));
        mp.dw[g] = q.dw;
    }
    for (int g = 0; g <= WGRAD_MULTI_MAX; ++g) { mp.first[g] = p.first[g]; mp.rfirst[g] = p.rfirst[g]; }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((conv_wgrad_blds_multi_kernel<WGRAD_BP>), dim3((unsigned)p.grid), dim3(256), 0, s, mp);
    if (p.reduce_grid > 0) hipLaunchKernelGGL(wgrad_reduce_multi_kernel, dim3((unsigned)p.reduce_grid), dim3(256), 0, s, mp);
    return mrcnn_launch_status();
}

// w_t[((KH-1-kh)*KW + (KW-1-kw))*Cout + co][ci] = w[((kh*KW + kw)*Cin + ci)][co]
__global__ void flip_transpose_kernel(const float* __restrict__ w, float* wt, int KH, int KW, int Cin, int Cout) {
    __shared__ float tile[32][33];
    const int tap = blockIdx.z;
    const int kh = tap / KW, kw = tap % KW;
    const int tap_t = (KH - 1 - kh) * KW + (KW - 1 - kw);
    const int ci0 = blockIdx.y * 32, co0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;    // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        int ci = ci0 + r, co = co0 + tx;
        tile[r][tx] = (ci < Cin && co < Cout) ? w[((long long)tap * Cin + ci) * Cout + co] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        int co = co0 + r, ci = ci0 + tx;
        if (co < Cout && ci < Cin) wt[((long long)tap_t * Cout + co) * Cin + ci] = tile[tx][r];
    }
}

extern "C" int mrcnn_weight_flip_transpose(const float* w, float* w_t, int KH, int KW, int Cin, int Cout, void* stream) {
    if (!w || !w_t || KH <= 0 || KW <= 0 || Cin <= 0 || Cout <= 0) return MRCNN_ERR_ARG;
    dim3 grid((Cout + 31) / 32, (Cin + 31) / 32, KH * KW);
    hipLaunchKernelGGL(flip_transpose_kernel, grid, dim3(256), 0, (hipStream_t)stream, w, w_t, KH, KW, Cin, Cout);
    return mrcnn_launch_status();
}

// All layers of a flat parameter buffer in one launch: table[l] = {offset (floats, same in w and w_t), KH, KW,
// Cin, Cout, first_tile}; a tile is 32 ci x 32 co of one tap.  The weights change once per optimiser step, so
// the data-gradient operands of every layer are refreshed by one HBM-bound pass instead of one launch per layer.
struct FlipEntry { long long off; int KH, KW, Cin, Cout, first_tile, pad; };

__global__ void flip_transpose_batched_kernel(const float* __restrict__ w, float* wt, const FlipEntry* __restrict__ table, int n) {
    __shared__ float tile[32][33];
    int lo = 0, hi = n - 1;                         // last entry with first_tile <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_tile <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const FlipEntry e = table[lo];
    int t = blockIdx.x - e.first_tile;
    const int cot = (e.Cout + 31) / 32, cit = (e.Cin + 31) / 32;
    const int co0 = (t % cot) * 32; t /= cot;
    const int ci0 = (t % cit) * 32;
    const int tap = t / cit;
    const int kh = tap / e.KW, kw = tap % e.KW;
    const int tap_t = (e.KH - 1 - kh) * e.KW + (e.KW - 1 - kw);
    const float* src = w + e.off;
    float* dst = wt + e.off;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int ci = ci0 + r, co = co0 + tx;
        tile[r][tx] = (ci < e.Cin && co < e.Cout) ? src[((long long)tap * e.Cin + ci) * e.Cout + co] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int co = co0 + r, ci = ci0 + tx;
        if (co < e.Cout && ci < e.Cin) dst[((long long)tap_t * e.Cout + co) * e.Cin + ci] = tile[tx][r];
    }
}

extern "C" int mrcnn_weight_flip_transpose_batched(const float* params, float* params_t, const void* table, int n_layers,
                                                   int total_tiles, void* stream) {
    if (!params || !params_t || !table || n_layers <= 0 || total_tiles <= 0) return MRCNN_ERR_ARG;
    hipLaunchKernelGGL(flip_transpose_batched_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, params,
                       params_t, (const FlipEntry*)table, n_layers);
    return mrcnn_launch_status();
}
