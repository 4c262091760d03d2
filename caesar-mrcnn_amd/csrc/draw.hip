// The detection overlay of Analyzer.draw_results (mrcnn/analyze.py:2039-2135) as the integer raster of DESIGN.md 4.12, composed
// in ONE pass over the canvas: every canvas pixel is written once, as finished RGB.  draw.render_host is the NumPy statement of
// the same text; the two give the same bytes.  Layers, later over earlier:
//   1. the frame (nearest neighbour, scale s, a white margin of 2 frame pixels), shaded per mask in item order by table look-up
//      (shade [K][3][256]: visualize.apply_mask's expression for every 8-bit value, built on the host);
//   2. the items in table order: a ground-truth box is a dashed outline of thickness t1 = max(1, s / 4), a detection is its box
//      outline (solid, t2 = max(1, s / 2)) and then its mask contour (t1, opaque); box outlines are blended with alpha 0.7 in
//      integers, out = (179 colour + 76 below + 127) / 255;
//   3. the captions in table order, a 5 x 7 glyph (35 bits, bit 5 row + column) per character, a cell of s canvas pixels, an
//      advance of 6 cells, opaque.
// A workgroup owns a tile of DR_TW x DR_TH canvas pixels.  It first culls the items and the texts against the tile (box
// rectangles, MaskPlanes.box for the masks, the text blocks): one ballot per 64 items, kept in LDS as bit lists, so the order of
// the tables is the order of the set bits and no pixel tests an item that cannot reach its tile.  A thread then owns DR_PX
// contiguous pixels of one row and walks the lists three times (shading, items, captions).  The planes [n][H][wpr] are read in
// place.  No atomics, no floating point: the canvas is bitwise the same from run to run.
// Every index that comes from a table is checked on the host before the launch (dr_check) AND guarded where it is used.
#include "common.h"

#define DR_M 2                           // margin, frame pixels
#define DR_TW 128                        // tile: canvas pixels per row ...
#define DR_TH 8                          // ... and rows
#define DR_PX 4                          // contiguous pixels of a thread: 12 bytes, one 96-bit store when the rows are 4-byte aligned
#define DR_T (DR_TW / DR_PX * DR_TH)     // 256 threads
#define DR_MAX_ITEMS 4096
#define DR_MAX_TEXTS 4096
#define DR_MAX_TEXT_CHARS 256
#define DR_MAX_COLOURS 256
#define DR_MAX_SCALE 64
#define DR_MAX_DIM 16384
#define DR_MAX_COORD (1 << 20)
#define DR_GLYPH_BITS 35
#define DR_MAX_CANVAS 65536              // canvas rows and columns: the grid stays below 65536 workgroups a side

struct DrParams {
    int H, W, s, Hc, Wc, t1, t2, n_planes, wpr, n_items, n_texts, n_glyphs, n_colours, shaded, vec;
};
struct DrRgb { unsigned a, b, c; };      // 12 bytes, 4-byte aligned

// frame coordinate of canvas coordinate v (a neighbour may lie off the canvas: off the frame as well)
__device__ __forceinline__ int dr_frame(int v, int s) { return v < 0 ? -1 : v / s - DR_M; }

__device__ __forceinline__ unsigned dr_bit(const unsigned* __restrict__ planes, const DrParams& p, int plane, int fy, int fx) {
    if ((unsigned)fy >= (unsigned)p.H || (unsigned)fx >= (unsigned)p.W) return 0u;
    return (planes[((long long)plane * p.H + fy) * p.wpr + (fx >> 5)] >> (fx & 31)) & 1u;
}

__device__ __forceinline__ bool dr_overlap(int y1, int y2, int x1, int x2, int ty1, int ty2, int tx1, int tx2) {
    return y1 < y2 && x1 < x2 && y1 < ty2 && y2 > ty1 && x1 < tx2 && x2 > tx1;
}

__global__ __launch_bounds__(DR_T) void dr_render_kernel(DrParams p, const unsigned char* __restrict__ image,
                                                         const unsigned* __restrict__ planes, const int* __restrict__ plane_box,
                                                         const mrcnn_draw_item* __restrict__ items, const mrcnn_draw_text* __restrict__ texts,
                                                         const unsigned long long* __restrict__ glyphs,
                                                         const unsigned char* __restrict__ palette, const unsigned char* __restrict__ shade,
                                                         unsigned char* __restrict__ canvas) {
    __shared__ unsigned long long s_items[DR_MAX_ITEMS / 64], s_texts[DR_MAX_TEXTS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = p.s;
    const int tx1 = blockIdx.x * DR_TW, ty1 = blockIdx.y * DR_TH;
    const int tx2 = min(tx1 + DR_TW, p.Wc), ty2 = min(ty1 + DR_TH, p.Hc);

    // ---- cull: the items and texts that can reach this tile, as bit lists in table order
    for (int base = wave * 64; base < p.n_items; base += DR_T) {             // uniform within a wave
        const int i = base + lane;
        bool hit = false;
        if (i < p.n_items) {
            const mrcnn_draw_item it = items[i];
            hit = dr_overlap(s * (it.y1 + DR_M), s * (it.y2 + DR_M), s * (it.x1 + DR_M), s * (it.x2 + DR_M), ty1, ty2, tx1, tx2);
            if (!hit && it.kind == MRCNN_DRAW_DETECTION && it.plane >= 0 && it.plane < p.n_planes) {
                const int* b = plane_box + 4 * it.plane;                       // (y1, x1, y2, x2) of the set pixels
                const int by1 = min(max(b[0], 0), p.H), bx1 = min(max(b[1], 0), p.W), by2 = min(max(b[2], 0), p.H), bx2 = min(max(b[3], 0), p.W);
                hit = dr_overlap(s * (by1 + DR_M), s * (by2 + DR_M), s * (bx1 + DR_M), s * (bx2 + DR_M), ty1, ty2, tx1, tx2);
            }
        }
        const unsigned long long bits = __ballot(hit);
        if (lane == 0) s_items[base >> 6] = bits;
    }
    for (int base = wave * 64; base < p.n_texts; base += DR_T) {
        const int i = base + lane;
        bool hit = false;
        if (i < p.n_texts) {
            const mrcnn_draw_text t = texts[i];
            const int bottom = s * (t.ya + DR_M), left = s * (t.xa + DR_M);
            const int count = min(max(t.count, 0), DR_MAX_TEXT_CHARS);
            hit = dr_overlap(bottom - 7 * s, bottom, left, left + 6 * s * count, ty1, ty2, tx1, tx2);
        }
        const unsigned long long bits = __ballot(hit);
        if (lane == 0) s_texts[base >> 6] = bits;
    }
    __syncthreads();

    const int Y = ty1 + tid / (DR_TW / DR_PX), X0 = tx1 + (tid % (DR_TW / DR_PX)) * DR_PX;
    if (Y >= p.Hc || X0 >= p.Wc) return;                                      // (no barrier below)
    const int fy = dr_frame(Y, s), fyu = dr_frame(Y - p.t1, s), fyd = dr_frame(Y + p.t1, s);
    int fx[DR_PX], fxl[DR_PX], fxr[DR_PX];
    unsigned r[DR_PX], g[DR_PX], b[DR_PX];
#pragma unroll
    for (int j = 0; j < DR_PX; ++j) {
        const int X = X0 + j;
        fx[j] = dr_frame(X, s); fxl[j] = dr_frame(X - p.t1, s); fxr[j] = dr_frame(X + p.t1, s);
        r[j] = g[j] = b[j] = 255u;
        if ((unsigned)fy < (unsigned)p.H && (unsigned)fx[j] < (unsigned)p.W) {
            const unsigned char* px = image + 3ll * ((long long)fy * p.W + fx[j]);
            r[j] = px[0]; g[j] = px[1]; b[j] = px[2];
        }
    }
    const int item_words = (p.n_items + 63) >> 6, text_words = (p.n_texts + 63) >> 6;

    // ---- 1. shading, mask by mask
    if (p.shaded && (unsigned)fy < (unsigned)p.H) {
        for (int w = 0; w < item_words; ++w) {
            unsigned long long bits = s_items[w];
            while (bits) {
                const int i = (w << 6) + __ffsll((long long)bits) - 1;
                bits &= bits - 1ull;
                const mrcnn_draw_item it = items[i];
                if (it.kind != MRCNN_DRAW_DETECTION || it.plane < 0 || it.plane >= p.n_planes || (unsigned)it.colour >= (unsigned)p.n_colours) continue;
                const unsigned char* tab = shade + 768ll * it.colour;
#pragma unroll
                for (int j = 0; j < DR_PX; ++j)
                    if (dr_bit(planes, p, it.plane, fy, fx[j])) {
                        r[j] = tab[r[j]]; g[j] = tab[256 + g[j]]; b[j] = tab[512 + b[j]];
                    }
            }
        }
    }

    // ---- 2. ground-truth boxes and detections, in table order
    for (int w = 0; w < item_words; ++w) {
        unsigned long long bits = s_items[w];
        while (bits) {
            const int i = (w << 6) + __ffsll((long long)bits) - 1;
            bits &= bits - 1ull;
            const mrcnn_draw_item it = items[i];
            if ((unsigned)it.colour >= (unsigned)p.n_colours) continue;
            const unsigned char* col = palette + 4 * it.colour;
            const unsigned cr = col[0], cg = col[1], cb = col[2];
            const bool gt = it.kind == MRCNN_DRAW_GT_BOX;
            const int t = gt ? p.t1 : p.t2;
            const int y1 = s * (it.y1 + DR_M), y2 = s * (it.y2 + DR_M), x1 = s * (it.x1 + DR_M), x2 = s * (it.x2 + DR_M);
            if (it.y2 > it.y1 && it.x2 > it.x1 && Y >= y1 && Y < y2) {
                const bool row_inner = Y >= y1 + t && Y < y2 - t;
#pragma unroll
                for (int j = 0; j < DR_PX; ++j) {
                    const int X = X0 + j;
                    bool on = X >= x1 && X < x2 && !(row_inner && X >= x1 + t && X < x2 - t);
                    if (gt) on = on && (((X + Y) / (4 * p.t1)) & 1) == 0;
                    if (on) {
                        r[j] = (179u * cr + 76u * r[j] + 127u) / 255u;
                        g[j] = (179u * cg + 76u * g[j] + 127u) / 255u;
                        b[j] = (179u * cb + 76u * b[j] + 127u) / 255u;
                    }
                }
            }
            if (!gt && it.plane >= 0 && it.plane < p.n_planes && (unsigned)fy < (unsigned)p.H) {
#pragma unroll
                for (int j = 0; j < DR_PX; ++j) {
                    if (!dr_bit(planes, p, it.plane, fy, fx[j])) continue;
                    const unsigned around = dr_bit(planes, p, it.plane, fyu, fx[j]) & dr_bit(planes, p, it.plane, fyd, fx[j]) &
                                            dr_bit(planes, p, it.plane, fy, fxl[j]) & dr_bit(planes, p, it.plane, fy, fxr[j]);
                    if (!around) { r[j] = cr; g[j] = cg; b[j] = cb; }
                }
            }
        }
    }

    // ---- 3. captions
    for (int w = 0; w < text_words; ++w) {
        unsigned long long bits = s_texts[w];
        while (bits) {
            const int i = (w << 6) + __ffsll((long long)bits) - 1;
            bits &= bits - 1ull;
            const mrcnn_draw_text t = texts[i];
            if ((unsigned)t.colour >= (unsigned)p.n_colours) continue;
            const int bottom = s * (t.ya + DR_M), top = bottom - 7 * s, left = s * (t.xa + DR_M);
            const int count = min(max(t.count, 0), DR_MAX_TEXT_CHARS);
            if (Y < top || Y >= bottom) continue;
            const int row = (Y - top) / s;                                     // 0 .. 6
            const unsigned char* col = palette + 4 * t.colour;
#pragma unroll
            for (int j = 0; j < DR_PX; ++j) {
                const int cx = X0 + j - left;
                if (cx < 0) continue;
                const int k = cx / (6 * s);
                if (k >= count) continue;
                const int cell = (cx - k * 6 * s) / s;                         // 0 .. 5; 5 is the gap between two characters
                const long long gi = (long long)t.first + k;
                if (cell >= 5 || gi < 0 || gi >= p.n_glyphs) continue;
                if ((glyphs[gi] >> (5 * row + cell)) & 1ull) { r[j] = col[0]; g[j] = col[1]; b[j] = col[2]; }
            }
        }
    }

    unsigned char* out = canvas + 3ll * ((long long)Y * p.Wc + X0);
    if (p.vec) {                                                              // Wc % 4 == 0: every group is whole and 4-byte aligned
        DrRgb v;
        v.a = r[0] | (g[0] << 8) | (b[0] << 16) | (r[1] << 24);
        v.b = g[1] | (b[1] << 8) | (r[2] << 16) | (g[2] << 24);
        v.c = b[2] | (r[3] << 8) | (g[3] << 16) | (b[3] << 24);
        *reinterpret_cast<DrRgb*>(out) = v;
    } else {
#pragma unroll
        for (int j = 0; j < DR_PX; ++j)
            if (X0 + j < p.Wc) {
                out[3 * j] = (unsigned char)r[j]; out[3 * j + 1] = (unsigned char)g[j]; out[3 * j + 2] = (unsigned char)b[j];
            }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
static int dr_check(const mrcnn_draw_desc* d, const mrcnn_draw_item* items, const mrcnn_draw_text* texts, const uint64_t* glyphs) {
    if (!d) return MRCNN_ERR_ARG;
    if (d->H <= 0 || d->W <= 0 || d->scale <= 0 || d->n_planes < 0 || d->n_items < 0 || d->n_texts < 0 || d->n_glyphs < 0 || d->n_colours <= 0)
        return MRCNN_ERR_ARG;
    if ((d->n_items > 0 && !items) || (d->n_texts > 0 && !texts) || (d->n_glyphs > 0 && !glyphs)) return MRCNN_ERR_ARG;
    bool past = d->H > DR_MAX_DIM || d->W > DR_MAX_DIM || d->scale > DR_MAX_SCALE || d->n_items > DR_MAX_ITEMS || d->n_texts > DR_MAX_TEXTS ||
                d->n_colours > DR_MAX_COLOURS || d->n_glyphs > DR_MAX_TEXTS * DR_MAX_TEXT_CHARS;
    auto far = [](int v) { return v > DR_MAX_COORD || v < -DR_MAX_COORD; };
    for (int i = 0; i < d->n_items; ++i) {
        const mrcnn_draw_item& it = items[i];
        if (it.kind != MRCNN_DRAW_GT_BOX && it.kind != MRCNN_DRAW_DETECTION) return MRCNN_ERR_ARG;
        if (it.colour < 0 || it.colour >= d->n_colours || it.plane < -1 || it.plane >= d->n_planes) return MRCNN_ERR_ARG;
        if (it.kind == MRCNN_DRAW_GT_BOX && it.plane != -1) return MRCNN_ERR_ARG;
        if (far(it.y1) || far(it.x1) || far(it.y2) || far(it.x2)) past = true;
    }
    for (int i = 0; i < d->n_texts; ++i) {
        const mrcnn_draw_text& t = texts[i];
        if (t.colour < 0 || t.colour >= d->n_colours || t.first < 0 || t.count < 0 || (long long)t.first + t.count > d->n_glyphs) return MRCNN_ERR_ARG;
        if (t.count > DR_MAX_TEXT_CHARS || far(t.ya) || far(t.xa)) past = true;
    }
    for (int i = 0; i < d->n_glyphs; ++i)
        if (glyphs[i] >> DR_GLYPH_BITS) return MRCNN_ERR_ARG;
    if (!past) {
        const long long Hc = (long long)d->scale * (d->H + 2 * DR_M), Wc = (long long)d->scale * (d->W + 2 * DR_M);
        past = Hc > DR_MAX_CANVAS || Wc > DR_MAX_CANVAS || 3 * Hc * Wc > 0x7FFFFFFFll;
    }
    return past ? MRCNN_ERR_UNSUPPORTED : MRCNN_OK;
}

extern "C" int mrcnn_draw_check(const mrcnn_draw_desc* d, const mrcnn_draw_item* items_host, const mrcnn_draw_text* texts_host,
                                const uint64_t* glyphs_host) {
    return dr_check(d, items_host, texts_host, glyphs_host);
}

extern "C" int mrcnn_draw_overlay(const mrcnn_draw_desc* d, const mrcnn_draw_item* items_host, const mrcnn_draw_text* texts_host,
                                  const uint64_t* glyphs_host, const void* image, const void* planes, const int32_t* plane_box,
                                  const mrcnn_draw_item* items, const mrcnn_draw_text* texts, const uint64_t* glyphs, const void* palette,
                                  const void* shade, void* canvas, void* stream) {
    const int rc = dr_check(d, items_host, texts_host, glyphs_host);
    if (rc != MRCNN_OK) return rc;
    if (!image || !palette || !canvas) return MRCNN_ERR_ARG;
    if ((d->n_planes > 0 && (!planes || !plane_box)) || (d->n_items > 0 && !items) || (d->n_texts > 0 && !texts) ||
        (d->n_glyphs > 0 && !glyphs) || (d->shaded && !shade))
        return MRCNN_ERR_ARG;
    DrParams p;
    p.H = d->H; p.W = d->W; p.s = d->scale;
    p.Hc = d->scale * (d->H + 2 * DR_M); p.Wc = d->scale * (d->W + 2 * DR_M);
    p.t1 = d->scale / 4 > 1 ? d->scale / 4 : 1;
    p.t2 = d->scale / 2 > 1 ? d->scale / 2 : 1;
    p.n_planes = d->n_planes; p.wpr = (d->W + 31) / 32;
    p.n_items = d->n_items; p.n_texts = d->n_texts; p.n_glyphs = d->n_glyphs; p.n_colours = d->n_colours;
    p.shaded = d->shaded ? 1 : 0;
    p.vec = (p.Wc % DR_PX == 0 && ((uintptr_t)canvas & 3u) == 0) ? 1 : 0;
    const dim3 grid((unsigned)cdiv64(p.Wc, DR_TW), (unsigned)cdiv64(p.Hc, DR_TH));
    hipLaunchKernelGGL(dr_render_kernel, grid, dim3(DR_T), 0, (hipStream_t)stream, p, (const unsigned char*)image, (const unsigned*)planes,
                       (const int*)plane_box, items, texts, (const unsigned long long*)glyphs, (const unsigned char*)palette,
                       (const unsigned char*)shade, (unsigned char*)canvas);
    return mrcnn_launch_status();
}
