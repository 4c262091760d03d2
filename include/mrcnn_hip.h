/*
 * mrcnn_hip.h -- C-ABI of the MI355X (gfx950) Mask R-CNN hot path.
 *
 * The reference (SKA-INAF/caesar-mrcnn) has no FFI: its hot path is the Keras/TF1 graph wired by
 * MaskRCNN.build (mrcnn/model.py:1935-2166).  Each entry point below replaces one group of TF/Keras ops
 * of that graph; the reference call site it stands in for is cited next to it.  All pointers are DEVICE
 * pointers (allocated by the caller, e.g. PyTorch-ROCm), all tensors are float32 NHWC unless stated,
 * `stream` is a hipStream_t passed as void*, and every function returns 0 on success or a negative
 * status (mirroring the reference's 0 / -1 convention, scripts/run.py:1747-1757).  No function
 * allocates, frees or synchronises; all are re-entrant per stream.
 */
#ifndef MRCNN_HIP_H
#define MRCNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRCNN_OK 0
#define MRCNN_ERR_ARG (-1)
#define MRCNN_ERR_LAUNCH (-2)
#define MRCNN_ERR_WORKSPACE (-3)
#define MRCNN_ERR_UNSUPPORTED (-4)   /* valid request this entry point has no kernel for: use the unfused calls */

#define MRCNN_ACT_NONE 0
#define MRCNN_ACT_RELU 1
#define MRCNN_ACT_SIGMOID 2

#define MRCNN_RES_NONE 0
#define MRCNN_RES_SAME 1     /* res has the shape/strides of out                            */
#define MRCNN_RES_UP2 2      /* res is [N, OH/2, OW/2, Cout]; nearest 2x upsample then add   */

#define MRCNN_OUT_NHWC 0     /* out[n*out_n_stride + oh*out_h_stride + ow*out_w_stride + co] */
#define MRCNN_OUT_DECONV2 1  /* GEMM column = (a*2+b)*cmod + co -> pixel (2oh+a, 2ow+b), channel co */

/* Convolution as implicit GEMM: M = N*OH*OW pixels, N = Cout, K = KH*KW*Cin.
 * Replaces KL.Conv2D / TimeDistributed(Conv2D) / Dense / Conv2DTranspose(2x2,s2) with the following
 * BatchNorm(training=False) + Add + Activation folded into the epilogue
 * (mrcnn/model.py:99-210, 916-957, 986-1091, 2005-2022).
 * Weights are HWIO ([KH,KW,Cin,Cout] row-major == the GEMM B matrix [K, Cout]), i.e. the Keras layout.
 * Epilogue:  z = acc + bias[c];  (z_out gets z);  y = scale ? scale[c]*z + shift[c] : z;
 *            y += res (res_mode);  y = act(y);  out gets y.        c = column % cmod.          */
typedef struct mrcnn_conv_desc {
    int32_t N, H, W, Cin;
    int32_t Cout;            /* GEMM N (for DECONV2: 4*cmod) */
    int32_t KH, KW, stride, pad_t, pad_l;
    int32_t OH, OW;
    int32_t act, res_mode, out_mode;
    int32_t cmod;            /* channel modulus for bias/scale/shift (== Cout except DECONV2) */
    int64_t out_n_stride, out_h_stride, out_w_stride;   /* element strides of out / z_out / res(SAME) */
} mrcnn_conv_desc;

int mrcnn_conv2d_fwd(const mrcnn_conv_desc* d, const float* x, const float* w, const float* bias,
                     const float* scale, const float* shift, const float* res, float* out,
                     float* z_out, void* stream);

/* Same, with scratch for split-K: layers with few output tiles (small feature maps) cut the K loop
 * into slices run by separate workgroups; partial slabs are summed in a fixed order by a second
 * kernel that also applies the epilogue.  mrcnn_conv2d_fwd_workspace() gives the bytes needed
 * (0 = no split); a NULL/short workspace silently runs unsplit.                                     */
size_t mrcnn_conv2d_fwd_workspace(const mrcnn_conv_desc* d);
int mrcnn_conv2d_fwd_ws(const mrcnn_conv_desc* d, const float* x, const float* w, const float* bias,
                        const float* scale, const float* shift, const float* res, float* out,
                        float* z_out, void* workspace, size_t workspace_bytes, void* stream);

/* dW[K, Cout] = sum over pixels of im2col(x)^T . dy   (gradient of KL.Conv2D kernels, taken by TF
 * autodiff in the reference: keras fit_generator, mrcnn/model.py:2487).  dy is dense [N,OH,OW,Cout].
 * Partial sums over `splits` pixel ranges go to `workspace` (splits*K*Cout floats) and are reduced in
 * a fixed order (bitwise reproducible); beta_acc != 0 accumulates into dw instead of overwriting.   */
int mrcnn_conv2d_wgrad(const mrcnn_conv_desc* d, const float* x, const float* dy, float* dw,
                       float* workspace, size_t workspace_bytes, int beta_acc, void* stream);
size_t mrcnn_conv2d_wgrad_workspace(const mrcnn_conv_desc* d);
/* Host-only query, as mrcnn_conv2d_fwd_plan: what mrcnn_conv2d_wgrad would launch for these arguments and the status it would
 * return.  Launches nothing and never dereferences a tensor pointer: only nullness and 16-byte alignment are looked at, so it
 * runs without a GPU.  Reads what the launch reads: the tuning key "wgrad_lds_pad" (per call) and MRCNN_CONV_FLAT_GLDS (once per
 * process).  *plan is written only with MRCNN_OK.                                                                           */
#define MRCNN_WGRAD_TILE 0         /* conv_wgrad_kernel<bi, bn> (six tile shapes) */
#define MRCNN_WGRAD_BLDS 1         /* conv_wgrad_blds_kernel<16, false>: LDS-DMA 128 x 128 tiles, buffer addressing */
#define MRCNN_WGRAD_BLDS_TABLE 2   /* pixel_table_kernel, then conv_wgrad_blds_kernel<16, true>: X addressed through the pixel table */
#define MRCNN_WGRAD_GLDS 3         /* conv_wgrad_glds_kernel: the same tiles with flat addressing */
#define MRCNN_WGRAD_RED_NONE 0     /* one pixel split: the kernel stores (or accumulates into) dw */
#define MRCNN_WGRAD_RED_SCALAR 1   /* wgrad_reduce_kernel */
#define MRCNN_WGRAD_RED_VEC 2      /* wgrad_reduce_vec_kernel: KH*KW*Cin*Cout % 4 == 0, workspace and dw 16-byte aligned */
typedef struct mrcnn_wgrad_plan {
    int32_t kernel;                /* MRCNN_WGRAD_* */
    int32_t bi, bn, fast;          /* dW tile (rows of KH*KW*Cin x columns of Cout); fast: Cin % 64 == 0, a tile lies inside one tap */
    int32_t splits, chunk;         /* pixel splits (= slabs when > 1) and pixels per split */
    int32_t grid, table_grid;      /* workgroups of the gradient kernel; of pixel_table_kernel (0 = not launched) */
    int32_t reduce, reduce_grid;   /* MRCNN_WGRAD_RED_* and its workgroups */
    int32_t lds_bytes;             /* dynamic LDS of the gradient kernel ("wgrad_lds_pad"; the BLDS kernels only) */
    int32_t reserved;
    int64_t slab_bytes;            /* workspace the launch needs: the slabs, from the workspace's start */
    int64_t table_bytes;           /* room the query adds for the pixel table (256-byte aligned behind the slabs); a workspace that
                                      holds the slabs but not the table runs MRCNN_WGRAD_BLDS instead of _BLDS_TABLE */
    int64_t workspace_bytes;       /* what mrcnn_conv2d_wgrad_workspace answers: slab_bytes + table_bytes */
} mrcnn_wgrad_plan;
int mrcnn_conv2d_wgrad_plan(const mrcnn_conv_desc* d, const float* x, const float* dy, const float* dw, const void* workspace,
                            size_t workspace_bytes, mrcnn_wgrad_plan* plan);

/* w_t[(KH-1-kh, KW-1-kw, co), ci] = w[(kh,kw,ci), co]: the weights of the data-gradient convolution. */
int mrcnn_weight_flip_transpose(const float* w, float* w_t, int KH, int KW, int Cin, int Cout,
                                void* stream);
/* The same for every layer of a flat parameter buffer in one launch.  table (device): n_layers records of
 * { int64 offset (floats; same in params and params_t), int32 KH, KW, Cin, Cout, first_tile, pad } sorted by
 * first_tile, a tile being 32 x 32 (ci, co) of one tap; total_tiles = sum over layers of
 * KH*KW*ceil(Cin/32)*ceil(Cout/32).                                                                     */
int mrcnn_weight_flip_transpose_batched(const float* params, float* params_t, const void* table, int n_layers,
                                        int total_tiles, void* stream);

/* n <= 5 independent convolutions in ONE launch (plus one for their split-K reductions).  Replaces the Python loops
 * of the reference that apply one layer to several small feature maps in turn: the shared RPN model over the pyramid
 * levels (mrcnn/model.py:2040-2055, rpn_graph :916-957) and the FPN smoothing convolutions (:2018-2026).  Every problem
 * is an ordinary mrcnn_conv2d_fwd (own descriptor, pointers and output strides); all must fall into the same output
 * tile class (Cout <= 32, <= 64 or larger), else MRCNN_ERR_UNSUPPORTED and nothing is launched.  Results are those of
 * n mrcnn_conv2d_fwd_ws calls (same kernels; the K-slice count may differ, i.e. fp32 summation order only).      */
typedef struct mrcnn_conv_problem {
    mrcnn_conv_desc d;
    const float* x; const float* w; const float* bias; const float* scale; const float* shift; const float* res;
    float* out; float* z_out;
} mrcnn_conv_problem;
size_t mrcnn_conv2d_fwd_multi_workspace(const mrcnn_conv_problem* problems, int n);
int mrcnn_conv2d_fwd_multi(const mrcnn_conv_problem* problems, int n, void* workspace, size_t workspace_bytes,
                           void* stream);

/* The weight gradients of up to MRCNN_WGRAD_MULTI_MAX layers in one launch (+ one for their slab reductions): TF autodiff of
 * the three Conv2D layers of a bottleneck block (mrcnn/model.py:99-172) on the small feature maps, where each is a few dozen
 * output tiles with a few hundred pixels to contract, and the transform-domain GEMMs of a Winograd layer.  Every problem is an
 * ordinary mrcnn_conv2d_wgrad (accumulate != 0 adds to dw); all must fit the LDS-DMA kernel without a pixel table (Cin, Cout
 * multiples of 128, at most 64 taps, both tensors within a 32-bit buffer descriptor, fewer than 65 536 output pixels unless the
 * problem is a pure GEMM -- 1 x 1, stride 1, on a 1 x 1 map -- and 16-byte aligned buffers), else MRCNN_ERR_UNSUPPORTED
 * (workspace query: 0) and nothing is launched.  With MRCNN_CONV_FLAT_GLDS set the launch (and its plan) refuse every call
 * with MRCNN_ERR_UNSUPPORTED while the workspace query still answers the bytes: the query looks at the descriptors alone.     */
#define MRCNN_WGRAD_MULTI_MAX 16
typedef struct mrcnn_wgrad_problem {
    mrcnn_conv_desc d;
    const float* x; const float* dy; float* dw;
    int32_t accumulate;
} mrcnn_wgrad_problem;
size_t mrcnn_conv2d_wgrad_multi_workspace(const mrcnn_wgrad_problem* problems, int n);
int mrcnn_conv2d_wgrad_multi(const mrcnn_wgrad_problem* problems, int n, float* workspace, size_t workspace_bytes,
                             void* stream);
/* Host-only query, as mrcnn_conv2d_wgrad_plan: what mrcnn_conv2d_wgrad_multi would launch (conv_wgrad_blds_multi_kernel, then
 * wgrad_reduce_multi_kernel where a problem has slabs; no dynamic LDS) and the status it would return.  Workgroups first[g] ..
 * first[g + 1] - 1 of the gradient launch and rfirst[g] .. rfirst[g + 1] - 1 of the reduction (blocks of 256 float4) belong to
 * problem g; entries from n on repeat the totals.  *plan is written only with MRCNN_OK.                                        */
typedef struct mrcnn_wgrad_multi_plan {
    int32_t n;
    int32_t grid, reduce_grid;                        /* workgroups of the two launches (reduce_grid 0: no reduction launch) */
    int32_t reserved;
    int32_t splits[MRCNN_WGRAD_MULTI_MAX], chunk[MRCNN_WGRAD_MULTI_MAX];
    int32_t first[MRCNN_WGRAD_MULTI_MAX + 1], rfirst[MRCNN_WGRAD_MULTI_MAX + 1];
    int64_t slab_offset[MRCNN_WGRAD_MULTI_MAX];       /* where problem g's slabs start in the workspace (256-byte steps) */
    int64_t slab_bytes;                               /* workspace the launch needs */
    int64_t workspace_bytes;                          /* what mrcnn_conv2d_wgrad_multi_workspace answers: slab_bytes + 256 */
} mrcnn_wgrad_multi_plan;
int mrcnn_conv2d_wgrad_multi_plan(const mrcnn_wgrad_problem* problems, int n, const void* workspace, size_t workspace_bytes,
                                  mrcnn_wgrad_multi_plan* plan);

/* Data-gradient convolution fused with the epilogue backward of the layer below (TF autodiff through Conv2D, then
 * through the lower layer's Activation / BatchNorm / bias): y = conv(dz, w_t) (+ res) is d(loss)/d(out_below); stored is
 *   dz_below = y * act'(out_below) * scale_below,   and   dbeta += sum y*act',  dgamma += sum y*act'*(z-mean)*rstd,
 *   dbias += sum dz_below   (atomics, like mrcnn_epilogue_bwd).
 * Same result as mrcnn_conv2d_fwd followed by mrcnn_epilogue_bwd, without writing / re-reading y.  Supported: the
 * large layers (LDS-DMA kernel: >= 640 tiles of 128x128, Cin % 32 == 0, Cout % 128 == 0) and the split-K layers (small
 * feature maps; Cout a power of two, workspace as for mrcnn_conv2d_fwd_ws: the slab reduction then carries the
 * backward epilogue), dense output; otherwise MRCNN_ERR_UNSUPPORTED and nothing is launched.  res_mode SAME adds
 * `res` to y first.                                                                                            */
typedef struct mrcnn_bwd_epilogue {
    const float* out; const float* z; const float* scale; const float* mean; const float* rstd;
    float* dgamma; float* dbeta; float* dbias;
    int32_t act;                 /* MRCNN_ACT_NONE or MRCNN_ACT_RELU of the layer below */
    float* dy;                   /* optional second output y*act' (what a residual branch of the layer below receives: the
                                    block-output gradient of a bottleneck block); split-K layers only, else
                                    MRCNN_ERR_UNSUPPORTED */
} mrcnn_bwd_epilogue;
int mrcnn_conv2d_dgrad_ep(const mrcnn_conv_desc* d, const float* dz, const float* w_t, const float* res,
                          float* dz_below, const mrcnn_bwd_epilogue* ep, void* workspace, size_t workspace_bytes,
                          void* stream);

/* Host-only query: what mrcnn_conv2d_fwd_ws (ep == NULL) or mrcnn_conv2d_dgrad_ep (ep != NULL; x = dz, w = w_t) would
 * launch for these arguments, and the status it would return.  Launches nothing and never dereferences a tensor pointer:
 * only nullness and 16-byte alignment are looked at, so it runs without a GPU (the tail split then assumes the MI355X's
 * 256 CUs).  Reads the same switches as the launch (tuning keys "sk16" / "sk64", MRCNN_CONV_TAIL_SPLIT,
 * MRCNN_CONV_FLAT_GLDS).  *plan is written only with MRCNN_OK.                                                      */
#define MRCNN_CONV_TILE 0          /* conv_fwd_kernel<bm, bn> (six tile shapes), K cut into ksplit slices of ksteps */
#define MRCNN_CONV_BLDS 1          /* conv_fwd_blds_kernel: LDS-DMA 128 x 128 tiles, buffer addressing */
#define MRCNN_CONV_GLDS 2          /* conv_fwd_glds_kernel: the same with flat addressing */
#define MRCNN_CONV_BLDS_SPLITK 3   /* conv_fwd_blds_splitk_kernel: LDS-DMA tiles, K slices of ksteps steps of 16 */
#define MRCNN_CONV_BLDS_TAIL 4     /* conv_fwd_blds_kernel on mt_full row tiles + conv_fwd_blds_splitk_kernel on the others */
#define MRCNN_CONV_SK 5            /* conv_fwd_sk_kernel: 32 x 32 tiles, the four waves split K */
#define MRCNN_CONV_SK16 6          /* conv_fwd_sk16_kernel: 16 x 16 tiles */
#define MRCNN_CONV_SK64 7          /* conv_fwd_sk64_kernel: 64 x 64 tiles, two K slices of ksteps as accumulators */
#define MRCNN_CONV_RED_NONE 0      /* the kernel stores the result */
#define MRCNN_CONV_RED_SCALAR 1    /* conv_splitk_epilogue_kernel */
#define MRCNN_CONV_RED_VEC 2       /* conv_splitk_epilogue_vec_kernel */
#define MRCNN_CONV_RED_BWD 3       /* conv_splitk_epilogue_bwd_kernel: the slab sum carries the backward epilogue */
typedef struct mrcnn_conv_plan {
    int32_t kernel;                          /* MRCNN_CONV_* */
    int32_t bm, bn;                          /* output tile of that kernel */
    int32_t ksplit, ksteps;                  /* K slices and K-steps per slice the kernel runs with */
    int32_t grid;                            /* workgroups of the (first) launch */
    int32_t reduce;                          /* MRCNN_CONV_RED_*: the launch that follows */
    int32_t mt_full, tail_ksplit, tail_ksteps;   /* MRCNN_CONV_BLDS_TAIL: row tiles left unsplit, slices of the others */
    int32_t slab_bytes;                      /* workspace the launch uses (a split plan stays below 2^30 bytes) */
} mrcnn_conv_plan;
int mrcnn_conv2d_fwd_plan(const mrcnn_conv_desc* d, const float* x, const float* w, const float* bias,
                          const float* scale, const float* shift, const float* res, float* out,
                          float* z_out, void* workspace, size_t workspace_bytes,
                          const mrcnn_bwd_epilogue* ep, mrcnn_conv_plan* plan);

/* Frozen BatchNorm (KL.BatchNormalization with training=False, mrcnn/model.py:57-72; eps = Keras
 * default 1e-3):  scale = gamma*rsqrt(var+eps), shift = beta - mean*scale, for n channels.          */
int mrcnn_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var,
                  float eps, float* scale, float* shift, float* rstd, int64_t n, void* stream);

/* Backward of the conv epilogue over a dense [M, C] tensor:
 *   dy = dout * act'(out)  (relu: out > 0; sigmoid: out*(1-out));  dy_out (optional) gets dy;  dz_out gets dy*scale (or dy);
 *   dbeta[c] += sum dy;  dgamma[c] += sum dy*(z-mean)*rstd;  dbias[c] += sum dz.
 * (reference: TF autodiff through BatchNorm/Add/Activation).  dbeta/dgamma/dbias accumulate (atomics);
 * any of scale/z/mean/rstd/dgamma/dbeta may be NULL for layers without BatchNorm.                     */
int mrcnn_epilogue_bwd(const float* dout, const float* out, const float* z, const float* scale,
                       const float* mean, const float* rstd, float* dy_out, float* dz_out,
                       float* dgamma, float* dbeta, float* dbias, int64_t M, int C, int act,
                       void* stream);

/* KL.MaxPooling2D((3,3), strides=(2,2), padding="same") (mrcnn/model.py:187); TF SAME padding:
 * pad_before = total/2 (0 at even input sizes), window clipped at the borders.  argmax index kept
 * for the backward pass (first maximum in window scan order, as TF's MaxPoolGrad... see DESIGN.md). */
int mrcnn_maxpool3x3s2_fwd(const float* x, float* out, int32_t* argmax, int N, int H, int W, int C,
                           int OH, int OW, int pad_t, int pad_l, void* stream);
int mrcnn_maxpool3x3s2_bwd(const float* dout, const int32_t* argmax, float* dx, int N, int H, int W,
                           int C, int OH, int OW, void* stream);

/* out[n, oh, ow, c] = x[n, 2oh, 2ow, c]  (KL.MaxPooling2D(pool_size=(1,1), strides=2) "fpn_p6",
 * mrcnn/model.py:2022) and its adjoint (accumulating scatter).                                       */
int mrcnn_subsample2_fwd(const float* x, float* out, int N, int H, int W, int C, void* stream);
int mrcnn_subsample2_bwd_acc(const float* dout, float* dx, int N, int H, int W, int C, void* stream);

/* dsrc[n, h, w, c] (+)= sum of the 2x2 block of dout: adjoint of KL.UpSampling2D(2,2)
 * (mrcnn/model.py:2007-2013).                                                                       */
int mrcnn_upsample2_bwd(const float* dout, float* dsrc, int N, int H, int W, int C, int accumulate,
                        void* stream);

/* dst[n,h,w,(a*2+b)*C+c] = src[n,2h+a,2w+b,c] (gradient regrouping for Conv2DTranspose 2x2/s2). */
int mrcnn_pixel_unshuffle2(const float* src, float* dst, int N, int H, int W, int C, void* stream);
/* Fused backward of the mask-head output stage (mrcnn/model.py:1087-1090): given dL/dmask [M,H,W,C] (after
 * the sigmoid), mask [M,H,W,C], up = relu(deconv) [M,H,W,Cd] and the 1x1 kernel w_mask [Cd,C]:
 * dzg [M,H/2,W/2,4*Cd] = ReLU-masked gradient of the deconv GEMM output (columns (a*2+b)*Cd+co);
 * dw_mask [Cd,C], db_mask [C], db_deconv [Cd] accumulate (float atomics).  C <= 16, Cd % 64 == 0.     */
int mrcnn_mask_out_bwd(const float* d_mask_out, const float* mask_out, const float* up, const float* w_mask,
                       float* dzg, float* dw_mask, float* db_mask, float* db_deconv, int64_t M, int H, int W,
                       int Cd, int C, void* stream);
/* DMA helpers (hipMemcpy2DAsync / hipMemsetAsync on `stream`), device to device. */
int mrcnn_copy2d(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t row_bytes,
                 size_t rows, void* stream);
int mrcnn_fill_zero(void* dst, size_t bytes, void* stream);
/* GT instance masks of a batch (mrcnn/model.py:1721-1904: [B, H, W, MAX_GT_INSTANCES] bool from data_generator) cross PCIe
 * bit-packed: byte b of a pixel = instances 8b .. 8b+7, least significant bit first.  out [npix, G] uint8 (0 / 1); instances
 * >= n_used are written as zeros.                                                                                           */
int mrcnn_unpack_mask_bits(const void* packed, void* out, int64_t npix, int nbytes_per_pixel, int n_used, int G, void* stream);

/* Training augmentation (the reference's default pipeline, scripts/run.py:1091-1100: imgaug SomeOf((0, 2), [Fliplr, Flipud,
 * Affine(rotate=(-90, 90)), Affine(translate_percent=(-0.3, 0.3))], mode='constant', cval=0), applied by load_image_gt to the
 * image and the instance masks, mrcnn/model.py:1323-1359): ONE stage of a plan.  m = 6 doubles on the HOST, the inverse map
 * (sx, sy) = (m0 x + m1 y + m2, m3 x + m4 y + m5) of output pixel (x, y); float64 bilinear sampling, taps outside the image
 * read 0 -- identical to the host statement caesar-mrcnn_amd/augment.py:warp_host [imgaug bit-parity unpinned].  src and dst
 * are distinct device buffers of the same shape.
 *   _u8:        [H, W, C] uint8 image, C <= 4; rint (half to even).
 *   _mask_bits: [H, W, nbytes_per_pixel] instance masks bit-packed as for mrcnn_unpack_mask_bits (instance j = bit j & 7 of
 *               byte j >> 3), warped without unpacking; a bit is set when the value is > 0.5.  Any nbytes_per_pixel (32-bit
 *               words when it is a multiple of 4).                                                                         */
int mrcnn_augment_warp_u8(const void* src, int H, int W, int C, const double* m, void* dst, void* stream);
int mrcnn_augment_warp_mask_bits(const void* src, int H, int W, int nbytes_per_pixel, const double* m, void* dst, void* stream);

/* Ground truth of a training sample from its bit-packed instance masks, without unpacking them.  packed [H, W, nb] uint8 =
 * numpy.packbits(mask != 0, axis=-1, bitorder="little") padded with zero bytes to nb % 4 == 0 (4-byte aligned: it is read as
 * 32-bit words; the layout mrcnn_augment_warp_mask_bits reads and writes).  Integer arithmetic only: exact, the same from run
 * to run.  All pointers are device pointers; nothing is allocated on the device.
 *   mrcnn_mask_bits_stats   replaces np.sum(mask, axis=(0, 1)) of load_image_gt (mrcnn/model.py:1361-1363) and the per-instance
 *                           loop of utils.extract_bboxes (mrcnn/utils.py:49-77): for every instance k < n, count[k] = its
 *                           pixels and box[k] = (y1, x1, y2 + 1, x2 + 1) int32, (0, 0, 0, 0) when it has none.  Bits >= n of the
 *                           last word(s) are ignored, whatever they hold.  ws: mrcnn_mask_bits_stats_workspace(nb) bytes
 *                           (20 per bit of a pixel's words), 4-byte aligned, initialised by the call; smaller:
 *                           MRCNN_ERR_WORKSPACE.  Three launches: table reset, ballots + integer atomics, boxes.
 *   mrcnn_mask_bits_gather  replaces mask[:, :, keep], the MAX_GT_INSTANCES subsample gt_masks[:, :, ids] and the copy into the
 *                           zeroed batch planes (mrcnn/model.py:1364, 1831-1835, 1866-1870): out[y, x, j] = bit sel[j] of
 *                           pixel (y, x) for j < k and 0 for k <= j < G; out [H, W, G] uint8 is one image's slice of the
 *                           [B, H, W, G] batch.  sel: k int32 on the device, 0 <= sel[j] < 8 nb (an entry outside gives 0).
 *                           k == 0 writes zeros.  One launch; 32-bit stores when G % 4 == 0 and out is 4-byte aligned, else
 *                           bytes.
 *   mrcnn_mask_bits_zoom    replaces utils.resize_mask (mrcnn/utils.py:564-583) for an image resize_image scales:
 *                           scipy.ndimage.zoom(mask, [s, s, 1], order=0) [3P] and np.pad, in one launch.  The zoom copies one
 *                           input pixel or the constant 0 per output pixel, the row chosen by the output row and the column by
 *                           the output column: iy [oh], ix [ow] int32 on the device are those choices, taken from scipy itself
 *                           (gtprep.zoom_index_tables); an entry outside [0, h) / [0, w) (-1 by convention) is the constant.
 *                           out [OH, OW, nb] (4-byte aligned): pixel (top + y, left + x) = packed pixel (iy[y], ix[x]) for
 *                           y < oh, x < ow, zero words everywhere else.  One thread per canvas pixel and 32-bit word.  The
 *                           caps hold for h x w and for OH x OW; MRCNN_ERR_ARG also for oh, ow <= 0, top, left < 0,
 *                           top + oh > OH, left + ow > OW.
 * Malformed (MRCNN_ERR_ARG): H, W, nb or G <= 0, nb % 4 != 0, n <= 0, n > 8 nb, k < 0, k > G, a missing or misaligned pointer.
 * Caps (past any: MRCNN_ERR_UNSUPPORTED, use the host statement): H, W <= MRCNN_GTPREP_MAX_SIDE; n, 8 nb and G <=
 * MRCNN_GTPREP_MAX_INSTANCES (the stats table is one workspace slot per bit).  A refused call launches and writes nothing.
 * The _check entries give the status for those sizes and launch nothing.                                                      */
#define MRCNN_GTPREP_MAX_SIDE 8192
#define MRCNN_GTPREP_MAX_INSTANCES 4096
int mrcnn_mask_bits_stats_check(int H, int W, int nb, int n);
size_t mrcnn_mask_bits_stats_workspace(int nb);
int mrcnn_mask_bits_stats(const void* packed, int H, int W, int nb, int n, int* count, int* box, void* ws, size_t ws_bytes,
                          void* stream);
int mrcnn_mask_bits_gather_check(int H, int W, int nb, int k, int G);
int mrcnn_mask_bits_gather(const void* packed, int H, int W, int nb, const int* sel, int k, int G, void* out, void* stream);
int mrcnn_mask_bits_zoom_check(int h, int w, int nb, int oh, int ow, int top, int left, int OH, int OW);
int mrcnn_mask_bits_zoom(const void* packed, int h, int w, int nb, const int* iy, int oh, const int* ix, int ow, int top, int left,
                         int OH, int OW, void* out, void* stream);

/* Stitching of sources across tile borders (SFinder.merge_edge_sources, mrcnn/sfinder.py:711-935).  Sources are row-major bit
 * masks of their bounding boxes in mosaic coordinates: ONE pool of 32-bit words and a descriptor per source; pixel (x, y) of a
 * source is bit (x - x0) & 31 of word word_offset + (y - y0) * words_per_row + ((x - x0) >> 5), least significant bit first
 * (numpy.packbits(..., bitorder="little"), as for mrcnn_unpack_mask_bits); bits past w in a row's last word are ignored.
 * Rows, words and addresses outside a source or outside the pool read as zero; pool_words is the pool's length (at most
 * 2^31 - 1 words, else MRCNN_ERR_UNSUPPORTED).  All pointers are device pointers; nothing is allocated on the device.
 *   mrcnn_tile_adjacency  replaces the pixel-pair loops :787-810: out[p] = 1 iff some pixel of source pairs[p][0] and some pixel of
 *                         source pairs[p][1] have |dx| <= 1 and |dy| <= 1 (:797-799), else 0.  One wavefront per pair; only the
 *                         intersection of j's box with i's box grown by one pixel is read.  An index outside [0, n) gives 0.
 *   mrcnn_tile_union      replaces the membership-test union :848-862 and the pixel min / max box :873-884.  Components in CSR
 *                         form: the members of component c are member_ids[comp_offsets[c] .. comp_offsets[c + 1]) (M ids in all),
 *                         in the order the reference visits them.  Per component: out_desc[c] = the box of the set bits
 *                         (w = h = 0 when there are none) with word_offset = out_offsets[c], the union bitmap in that box at
 *                         out_pool + out_offsets[c], out_count[c] = its pixel count.  Per member position q: at fresh_pool +
 *                         fresh_offsets[q], in the member's OWN box and row pitch, member AND NOT (the members before it) -- the
 *                         set bits of the fresh bitmaps, member after member in raster order, are the reference's first-seen
 *                         pixel list.  The caller sizes both pools from the boxes: out_offsets[c] leaves room for the members'
 *                         common box (rows x ceil(width / 32) words), fresh_offsets[q] for h * words_per_row of the member;
 *                         writes past out_pool_words / fresh_pool_words are dropped.                                            */
typedef struct mrcnn_tile_source {
    int32_t x0, y0, w, h;            /* bounding box in mosaic pixels: columns x0 .. x0 + w - 1, rows y0 .. y0 + h - 1 */
    int32_t word_offset;             /* first word of row 0 in the pool */
    int32_t words_per_row;           /* >= ceil(w / 32) */
} mrcnn_tile_source;
int mrcnn_tile_adjacency(const void* pool, int64_t pool_words, const mrcnn_tile_source* desc, int n, const int32_t* pairs, int P,
                         int32_t* out, void* stream);
int mrcnn_tile_union(const void* pool, int64_t pool_words, const mrcnn_tile_source* desc, int n, const int32_t* comp_offsets,
                     const int32_t* member_ids, int C, int M, const int64_t* out_offsets, const int64_t* fresh_offsets,
                     mrcnn_tile_source* out_desc, int32_t* out_count, void* out_pool, int64_t out_pool_words, void* fresh_pool,
                     int64_t fresh_pool_words, void* stream);

/* Source parameters of a tiled run (SFinder.compute_source_params, mrcnn/sfinder.py:994-1211): the masked reductions of all n
 * sources of a mosaic in one launch, one workgroup per source.  Nothing is allocated, nothing synchronises.
 *   img          the image plane [H, W] float32 on the device (big_endian != 0: the file's byte order, swapped on read);
 *   pool, desc   the sources as for mrcnn_tile_adjacency (pixel masks in mosaic = image coordinates);
 *   cutouts      [n, 4] int32 (cx0, cy0, cx1, cy1): the padded rectangle the reference cuts per source, columns cx0 .. cx1 - 1 and
 *                rows cy0 .. cy1 - 1; clipped to the image as a NumPy slice is; mask pixels outside it are ignored;
 *   val_offsets  [n + 1] int64: source s gathers its pixel values into values[val_offsets[s] .. val_offsets[s + 1]) (room for its
 *                pixel count; h * words_per_row * 32 always suffices); values_len = length of `values` in floats.  Pixels past a
 *                slice are counted but not gathered (n_gathered < n_mask: the clipped statistics then cover the gathered ones);
 *   sigma, maxiters  of the clipping loop: non-finite values dropped; per iteration c = median, s = std (ddof 0) of the kept
 *                values, keep c - sigma s <= x <= c + sigma s; stops when an iteration removes nothing or after maxiters.
 * Per source one record.  NaN pixels are first replaced by `fill`, the minimum of the cut-out's non-NaN pixels (NaN if there
 * are none), as utils.read_fits does (mrcnn/utils.py:1090-1091).  x, y below are relative to (cx0, cy0).  Sums only: the
 * caller forms every ratio.  Results are bitwise reproducible (fixed-order reductions, no float atomics).                     */
typedef struct mrcnn_source_record {
    double s64;                      /* sum of the non-NaN masked values (np.nansum, in float64) */
    double w00, w10, w01;            /* sum I, sum x I, sum y I over the masked pixels, IEEE propagation of NaN / inf */
    double clip_mean, clip_median, clip_std;   /* of the values kept by the clipping (NaN when none is) */
    int64_t m00, m10, m01;           /* sum 1, sum x, sum y over the masked pixels */
    float fill;
    float smin, smax;                /* np.nanmin / np.nanmax of the masked values (NaN when npix == 0) */
    int32_t n_mask;                  /* masked pixels inside the cut-out */
    int32_t npix;                    /* those that are not NaN after the fill */
    int32_t clip_kept, clip_iters;   /* values kept at the end, iterations run */
    int32_t n_gathered;              /* min(n_mask, slice length) */
} mrcnn_source_record;
int mrcnn_source_params(const void* img, int big_endian, int H, int W, const void* pool, int64_t pool_words,
                        const mrcnn_tile_source* desc, int n, const int32_t* cutouts, const int64_t* val_offsets, void* values,
                        int64_t values_len, double sigma, int maxiters, mrcnn_source_record* out, void* stream);

/* Contours and pixel lists of bit masks: the pixel work of Analyzer.make_json_results (mrcnn/analyze.py:1902-1927) and of the
 * merged sources of SFinder.merge_edge_sources (mrcnn/sfinder.py:887-909) for all n sources of one call.  Sources are given as
 * for mrcnn_tile_adjacency (pool, pool_words, one mrcnn_tile_source each; x0 / y0 are not read: results are in the source's own
 * frame, pixel centres at integers); desc_host is the host copy of the device table desc.  The bit planes of the mask graph
 * below are the table word_offset = i * H * wpr, and mrcnn_tile_union's out_pool / out_desc is one as it stands.  Per source:
 *   contours   skimage.measure.find_contours(level = 0.5) [3P] of the zero-padded 0 / 1 mask, restated as analyze.find_contours
 *              (marching squares in raster order, 'low' connectivity; parity with skimage itself stays unpinned), padding
 *              subtracted, as (x, y): the same contours, in the same order, from the same starting vertex, first point repeated
 *              at the end (analyze.outline_statement states the rule without the sequential stitching); every coordinate is a
 *              multiple of 0.5 in [-0.5, w - 0.5], exact in float32;
 *   pixels     np.argwhere: (y, x) of the set bits in raster order.
 * Sizes are unknown before a first pass, so the work is two calls:
 *   mrcnn_outline_count  totals[n][2] = (contour segments, set pixels) per source, pixel_offsets[n + 1] = exclusive scan of the
 *                        pixel counts, and the per-row offsets kept in count_ws for the second call;
 *   mrcnn_outline_emit   with totals_host = those totals read back (S segments, K pixels in all): points [P][2] float32,
 *                        contour_offsets [C + 1] (contour k of the call: points contour_offsets[k] .. contour_offsets[k + 1]),
 *                        source_contours [n + 1] (source i: contours source_contours[i] .. source_contours[i + 1]), pixels
 *                        [K][2] int32.  P = S + C and C <= S / 4 are not known to the host before the call: points_cap >=
 *                        S + S / 4 points, contours_cap >= S / 4 (contour_offsets holds contours_cap + 1 ints), pixels_cap >= K,
 *                        else MRCNN_ERR_ARG; C = source_contours[n].  The pool must not change between the two calls.
 *   mrcnn_outline_workspace  bytes of count_ws (totals_host == NULL) or of emit_ws (totals_host given); 0 for a refused table.
 *   mrcnn_outline_check  the status the calls would return for that table (and those totals, when not NULL); launches nothing.
 * n <= 0, pool_words < 0, a negative total, or a source with w, h > 0 and word_offset < 0, words_per_row < ceil(w / 32) or rows
 * past pool_words: MRCNN_ERR_ARG.  Caps (past any: MRCNN_ERR_UNSUPPORTED, use the host path): w, h <= 8192; n <= 65535;
 * pool_words <= 2^31 - 1; at most 2^22 segments per source; S + S / 4 <= 2^31 - 1 points and K <= 2^31 - 1 pixels per call.  A
 * source with w <= 0 or h <= 0 is no error: it has no contours and no pixels.  A refused call launches and writes nothing.
 * Nothing is allocated on the device, nothing synchronises, no atomics: the results are bitwise the same from run to run.  */
int mrcnn_outline_check(const mrcnn_tile_source* desc_host, int n, int64_t pool_words, const int32_t* totals_host);
size_t mrcnn_outline_workspace(const mrcnn_tile_source* desc_host, int n, int64_t pool_words, const int32_t* totals_host);
int mrcnn_outline_count(const void* pool, int64_t pool_words, const mrcnn_tile_source* desc_host, const mrcnn_tile_source* desc, int n,
                        void* count_ws, size_t count_ws_bytes, int32_t* totals, int32_t* pixel_offsets, void* stream);
int mrcnn_outline_emit(const void* pool, int64_t pool_words, const mrcnn_tile_source* desc_host, const mrcnn_tile_source* desc, int n,
                       const int32_t* totals_host, const void* count_ws, size_t count_ws_bytes, void* emit_ws, size_t emit_ws_bytes,
                       const int32_t* pixel_offsets, float* points, int64_t points_cap, int32_t* contour_offsets, int64_t contours_cap,
                       int32_t* source_contours, int32_t* pixels, int64_t pixels_cap, void* stream);

/* The detection overlay of Analyzer.draw_results (mrcnn/analyze.py:2039-2135) as the integer raster of DESIGN.md 4.12, composed in
 * one pass over the canvas (draw.render_host is the NumPy statement; the two give the same bytes).  image [H][W][3] uint8; the
 * masks are the bit planes of the mask graph below (planes [n_planes][H][wpr], plane_box [n_planes][4] as _pack / _union give
 * them: the box culls, so a smaller one hides pixels); canvas [scale (H + 4)][scale (W + 4)][3] uint8, every byte written.
 *   items    in layer order.  MRCNN_DRAW_GT_BOX: the dashed outline of (y1, x1, y2, x2), thickness max(1, scale / 4).
 *            MRCNN_DRAW_DETECTION: the solid outline of the box, thickness max(1, scale / 2), then the contour of plane `plane`
 *            (-1: none) in the opaque colour.  Outlines are blended, (179 colour + 76 below + 127) / 255.  An empty or inverted
 *            box paints nothing.  With `shaded`, the planes of all detections shade the frame first, in item order.
 *   texts    in order, over the items: `count` glyphs from glyphs[first], the block's bottom-left corner at frame point (xa, ya).
 *   glyphs   one per character: 35 bits, bit 5 row + column of a 5 x 7 cell, row 0 on top.
 *   palette  [n_colours][4] uint8 (r, g, b, unused); shade [n_colours][3][256] uint8 (read only when `shaded`): the value a
 *            channel value takes under a mask of that colour.
 * items / texts / glyphs are given twice, as the host tables the call validates and as their device copies.  Malformed
 * (MRCNN_ERR_ARG): H, W, scale or n_colours <= 0, a negative count, a kind other than the two, a colour outside [0, n_colours),
 * a plane outside [-1, n_planes), a ground-truth box with a plane, a text that leaves glyphs, a glyph with a bit past 35, a
 * missing pointer.  Caps (past any: MRCNN_ERR_UNSUPPORTED, use the host statement): H, W <= 16384; scale <= 64; canvas sides
 * <= 65536 and canvas bytes <= 2^31 - 1; 4096 items; 4096 texts of at most 256 glyphs; 256 colours; coordinates within +-2^20.
 * A refused call launches and writes nothing.  mrcnn_draw_check: the status for those tables; launches nothing.
 * Nothing is allocated on the device, nothing synchronises, no atomics: the canvas is bitwise the same from run to run.  */
#define MRCNN_DRAW_GT_BOX 0
#define MRCNN_DRAW_DETECTION 1
typedef struct {
    int32_t kind;
    int32_t y1, x1, y2, x2;          /* frame pixels, y2 / x2 exclusive */
    int32_t colour;                  /* palette index */
    int32_t plane;                   /* bit plane of a detection, or -1 */
    int32_t pad;
} mrcnn_draw_item;
typedef struct {
    int32_t ya, xa;                  /* anchor, frame pixels */
    int32_t colour;                  /* palette index */
    int32_t first, count;            /* glyphs[first .. first + count) */
    int32_t pad[3];
} mrcnn_draw_text;
typedef struct {
    int32_t H, W, scale, n_planes, n_items, n_texts, n_glyphs, n_colours, shaded, pad;
} mrcnn_draw_desc;
int mrcnn_draw_check(const mrcnn_draw_desc* d, const mrcnn_draw_item* items_host, const mrcnn_draw_text* texts_host,
                     const uint64_t* glyphs_host);
int mrcnn_draw_overlay(const mrcnn_draw_desc* d, const mrcnn_draw_item* items_host, const mrcnn_draw_text* texts_host,
                       const uint64_t* glyphs_host, const void* image, const void* planes, const int32_t* plane_box,
                       const mrcnn_draw_item* items, const mrcnn_draw_text* texts, const uint64_t* glyphs, const void* palette,
                       const void* shade, void* canvas, void* stream);

/* The mask graph of Analyzer.extract_det_masks (mrcnn/analyze.py:1162-1496): which detection masks of a frame overlap or touch,
 * and the unions of those that are merged.  The masks of ONE frame are bit planes, planes[n][H][wpr] 32-bit words, wpr =
 * ceil(W / 32): pixel x of a row is bit x & 31 of word x >> 5, least significant bit first (numpy.packbits(...,
 * bitorder="little"), as for mrcnn_unpack_mask_bits); the bits past W in a row's last word are always zero.  A box is
 * (y1, x1, y2, x2) as utils.extract_bboxes gives it: y2 / x2 exclusive, all four 0 for an empty plane.  Integer arithmetic
 * throughout; all pointers are device pointers; nothing is allocated on the device.  n, H or W <= 0: MRCNN_ERR_ARG.
 *   mrcnn_mask_planes_pack  masks [H, W, n] uint8 (nonzero = set: what mrcnn_unmold_masks writes) -> planes, count[n] (set pixels
 *                           per plane) and box[n, 4].
 *   mrcnn_mask_pair_stats   for pairs[P, 2] (plane indices a, b): inter[p] = popcount(a & b) -- the caller forms the union of
 *                           mask_iou as count_a + count_b - inter -- and touch[p] = 1 iff some pixel of a equals or is a
 *                           4-neighbour (up, down, left, right; NOT diagonal) of some pixel of b, which is
 *                           Analyzer.are_mask_connected(a, b) (analyze.masks_touch4 is the NumPy statement).  box = the planes'
 *                           boxes from _pack / _union: only b's box intersected with a's box grown by one pixel is read.  One
 *                           wavefront per pair.  An index outside [0, n) gives 0, 0.
 *   mrcnn_mask_union        components in CSR form as for mrcnn_tile_union (members of component c: member_ids[comp_offsets[c] ..
 *                           comp_offsets[c + 1]), M ids in all): out_planes[C][H][wpr] = OR of the members (merge_masks chains),
 *                           with out_count[C] and out_box[C, 4].  An empty component gives a zero plane; members may repeat; ids
 *                           outside [0, n) are skipped.  out_planes must not be planes.                                        */
int mrcnn_mask_planes_pack(const void* masks, int H, int W, int n, void* planes, int32_t* count, int32_t* box, void* stream);
int mrcnn_mask_pair_stats(const void* planes, const int32_t* box, int n, int H, int W, const int32_t* pairs, int P, int32_t* inter,
                          int32_t* touch, void* stream);
int mrcnn_mask_union(const void* planes, int n, int H, int W, const int32_t* comp_offsets, const int32_t* member_ids, int C, int M,
                     void* out_planes, int32_t* out_count, int32_t* out_box, void* stream);

/* The sources of a mosaic as the planes of its overview frame (the host statement is
 * sfinder.source_planes_host): pool, pool_words, desc[n] as for mrcnn_tile_adjacency (x0 / y0 in mosaic pixels); planes
 * [n][h][ceil(w / 32)] in the layout above: bit (Y, X) of plane i is set iff source i has a pixel (y, x) with y / shrink == Y and
 * x / shrink == X; pixels outside [0, shrink h) x [0, shrink w) are dropped, the bits past w are zero, a descriptor that is not
 * valid (w or h <= 0, ...) gives a zero plane, words past the pool read as zero.  count[n] and box[n, 4] as
 * mrcnn_mask_planes_pack fills them.  One thread gathers one output word (no atomics), then the statistics launch of _pack.
 * n, shrink, h or w <= 0 or a missing pointer: MRCNN_ERR_ARG; n h ceil(w / 32), shrink h or shrink w beyond 2^31 - 1:
 * MRCNN_ERR_UNSUPPORTED; nothing is launched then.  mrcnn_sources_to_planes_check: the status for those sizes.               */
int mrcnn_sources_to_planes_check(int n, int shrink, int h, int w);
int mrcnn_sources_to_planes(const void* pool, int64_t pool_words, const mrcnn_tile_source* desc, int n, int shrink, int h, int w,
                            void* planes, int32_t* count, int32_t* box, void* stream);

/* The pixel work of the tester (Analyzer.compute_performances / compute_det_mask_pars, mrcnn/analyze.py:1502-1861), on the bit
 * planes and boxes of the mask graph above (boxes as _pack / _union give them; a box larger than the plane's own is allowed, a
 * smaller one hides pixels).  Nothing is allocated, nothing synchronises, no atomics.  na, nb, n, H or W <= 0: MRCNN_ERR_ARG.
 *   mrcnn_mask_cross_stats  inter[i * nb + j] = popcount(a_i & b_j) for all na x nb pairs of two plane sets of ONE frame (the sets
 *                           may be the same buffer), in one launch, one wavefront per cell.  Only the intersection of the two
 *                           boxes is read; an empty intersection gives 0.  Every cell is written.  The Jaccard index of the
 *                           reference's jaccard_score(average='binary') [3P] is inter / (count_a + count_b - inter), 0 when the
 *                           union is 0, on the host.
 *   mrcnn_mask_plane_sums   sum[p] = float64 sum of the non-NaN values of img at plane p's set pixels (np.nansum: an infinity
 *                           propagates; 0 for an empty plane).  img [H, W] float32 (big_endian != 0: the file's byte order,
 *                           swapped on read, as for mrcnn_source_params).  One workgroup per plane; the partial sums are combined
 *                           in a fixed order, so the result is bitwise the same from run to run.                                 */
int mrcnn_mask_cross_stats(const void* planes_a, const int32_t* box_a, int na, const void* planes_b, const int32_t* box_b, int nb,
                           int H, int W, int32_t* inter, void* stream);
int mrcnn_mask_plane_sums(const void* img, int big_endian, const void* planes, const int32_t* box, int n, int H, int W, double* sum,
                          void* stream);

/* Connected components of the bit planes of the mask graph above (csrc/components.hip): the labelling behind
 * Analyzer.split_masks, extract_gt_masks(split_gtmasks) and the island count of compute_det_mask_pars, and the per-row extents
 * the hull of analyze.min_area_rect starts from.  Planes, boxes and conventions are those of the mask graph: integer arithmetic
 * throughout, nothing is allocated on the device, no call synchronises.  A plane is labelled INSIDE its box cut to the frame (the
 * box of _pack / _union covers the plane; a smaller one hides pixels, an empty one gives no component).  box_host is the host
 * copy of the device table box: it sizes the workspace and is what the caps are checked on; the kernels place their tables from
 * the device copy by the same rule and touch nothing when that would leave the workspace.
 *   numbering   components are numbered 1..k in raster order of their first pixel, which is what analyze.label_components
 *               (scipy.ndimage.label, or its breadth-first fallback) gives.  connectivity 4: up, down, left, right; 8: the
 *               diagonals too (analyze.count_islands).  The labelling is a union-find over row runs whose root is the smallest
 *               run id, ranked by a prefix sum: the atomics it uses (integer min, on LDS up to 12288 runs in a box, else on the
 *               workspace) cannot change the result, so two calls on the same input give the same bytes.
 *   mrcnn_mask_components_check      the status the calls below return for this frame, connectivity, host box table and workspace
 *                                    size; launches nothing.  n, H or W <= 0, a connectivity other than 4 or 8, no table:
 *                                    MRCNN_ERR_ARG.  Caps (past any: MRCNN_ERR_UNSUPPORTED, use the host statement): H, W <= 8192;
 *                                    n <= 4096; rows * ceil(columns / 2) of one box <= 2^22 (its run capacity); workspace <= 2^31
 *                                    - 1 words.  A workspace below mrcnn_mask_components_workspace: MRCNN_ERR_WORKSPACE.
 *   mrcnn_mask_components_workspace  bytes of workspace for that table; 0 for a refused one.  Per box, in 32-bit words:
 *                                    rows + 1 + 2 * capacity, and one capacity more when the capacity is above 12288.
 *   mrcnn_mask_components_count      ncomp[n] = components per plane; the run table and its labels stay in the workspace.
 *   mrcnn_mask_components_emit       the components as planes out_planes[P][H][wpr] with out_count[P] and out_box[P, 4], laid out
 *                                    as mrcnn_mask_union's outputs (every word written).  piece_offsets[n + 1], given as the host
 *                                    prefix and its device copy, places them: plane p owns pieces piece_offsets[p] ..
 *                                    piece_offsets[p + 1], P = piece_offsets[n], the j-th of them being component j + 1.  mode
 *                                    MRCNN_COMPONENTS_ALL: the caller gives every plane ncomp[p] pieces; MRCNN_COMPONENTS_FIRST: at
 *                                    most one, component 1.  A piece past ncomp[p] is a zero plane; a plane with no set pixel has
 *                                    no component and no piece.  workspace, box tables and ncomp: those of the count call,
 *                                    unchanged.  A prefix that is not 0-based and monotone (or grows by more than 1 in FIRST
 *                                    mode), another mode: MRCNN_ERR_ARG; P > 2^24: MRCNN_ERR_UNSUPPORTED.  P == 0 launches nothing.
 *   mrcnn_mask_row_extents           extents[R][2] = (x of the leftmost, x of the rightmost set pixel), (-1, -1) for a row without
 *                                    one, for every row of every plane's box: plane p's rows at row_offsets[p] (device, [n + 1],
 *                                    the prefix of the box heights), R = the sum of the heights of box_host, else MRCNN_ERR_ARG.
 *                                    Bit scans of the words; no labelling, no workspace.
 * A refused call launches and writes nothing.                                                                                   */
#define MRCNN_COMPONENTS_ALL 0
#define MRCNN_COMPONENTS_FIRST 1
int mrcnn_mask_components_check(int n, int H, int W, int connectivity, const int32_t* box_host, size_t ws_bytes);
size_t mrcnn_mask_components_workspace(int n, int H, int W, const int32_t* box_host);
int mrcnn_mask_components_count(const void* planes, const int32_t* box_host, const int32_t* box, int n, int H, int W, int connectivity,
                                void* ws, size_t ws_bytes, int32_t* ncomp, void* stream);
int mrcnn_mask_components_emit(const int32_t* box_host, const int32_t* box, int n, int H, int W, const void* ws, size_t ws_bytes,
                               const int32_t* ncomp, const int32_t* piece_offsets_host, const int32_t* piece_offsets, int mode,
                               void* out_planes, int32_t* out_count, int32_t* out_box, void* stream);
int mrcnn_mask_row_extents(const void* planes, const int32_t* box_host, const int32_t* box, int n, int H, int W,
                           const int32_t* row_offsets, int R, int32_t* extents, void* stream);

/* The matching step of the Pascal-VOC box metrics of the reference's vendored tool (Object-Detection-Metrics,
 * lib/Evaluator.py:99-122: best ground truth per detection and the "seen" flag; :382-426: the IoU), for the detections and ground
 * truths of a whole test set, flat, in one launch.  Rows of one image are contiguous: image i owns detections det_off[i] ..
 * det_off[i + 1] and ground truths gt_off[i] .. gt_off[i + 1] (CSR, I + 1 entries each, 0 = off[0] <= ... <= off[I] = D resp. G --
 * the caller's contract; rows outside the tables are never touched).  Boxes [., 4] float64 in corner form (c0, c1, c2, c3), classes
 * int32, scores float64, thr [T] float64, all > 0.  float64 in the tool's order of operations:
 *   IoU       0 when a0 > b2, b0 > a2, a3 < b1 or a1 > b3; else inter = (min(a2, b2) - max(a0, b0) + 1) (min(a3, b3) - max(a1, b1) + 1),
 *             area = (c2 - c0 + 1) (c3 - c1 + 1), iou = inter / (areaA + areaB - inter);
 *   best_gt   [D] the global ground-truth row of the detection's image and class with the greatest IoU, the first one in row order
 *             on a tie; -1 (and best_iou 0) when every IoU is 0 (the tool starts from sys.float_info.min);  best_iou [D] that IoU;
 *   tp        [T, D] uint8: 1 iff best_iou[d] >= thr[t] and no detection d' of the image with the same best_gt and
 *             best_iou[d'] >= thr[t] precedes d -- a higher score, or the same score and an earlier row (the tool's stable sort by
 *             descending confidence and its "seen" flag).
 * One workgroup (one wavefront) per image; the image's ground truths are staged in LDS up to 256 of them and read from global
 * memory above that.  No atomics, nothing allocated, bitwise the same from run to run.  D, I or T <= 0, G < 0: MRCNN_ERR_ARG.   */
int mrcnn_voc_match(const double* det_box, const int32_t* det_cls, const double* det_score, const int32_t* det_off, int D,
                    const double* gt_box, const int32_t* gt_cls, const int32_t* gt_off, int G, int I, const double* thr, int T,
                    int32_t* best_gt, double* best_iou, uint8_t* tp, void* stream);

/* The matching step of the sweep mAP of the reference's second vendored tool (tarlen5-calculate-mean-ap/calculate.py:
 * calc_iou_individual :40-77, get_single_image_results :80-139), for the N problems of a test set, flat, in one launch.  A problem is
 * the detections of one image -- all of them or those of one class, ALREADY in ascending-score order -- against its ground truths:
 * problem p owns detection rows det_off[p] .. det_off[p + 1] and ground-truth rows gt_off[p] .. gt_off[p + 1] (CSR, N + 1 entries
 * each, 0 = off[0] <= ... <= off[N] = D resp. G -- the caller's contract; rows outside the tables are never touched).  Boxes
 * [., 4] float64 corner boxes (c0, c1, c2, c3) with c0 <= c2 and c1 <= c3 (the tool raises on others; the caller checks), thr [T]
 * float64, all > 0.  float64 in the tool's order of operations:
 *   IoU     0 when t2 < p0, p2 < t0, t3 < p1 or p3 < t1 (p the detection, t the ground truth); else
 *           inter = (min(t2, p2) - max(t0, p0) + 1) (min(t3, p3) - max(t1, p1) + 1), area = (c2 - c0 + 1) (c3 - c1 + 1),
 *           iou = inter / (area_t + area_p - inter);
 *   tp      int32, problem p at tp[T * (det_off[p] + p)], T rows of P + 1 entries (P = the problem's detections; T * (D + N) entries in
 *           all): tp[t][k] = the matches of the tool's walk when detections k .. P - 1 are kept (a score threshold keeps a suffix
 *           of the ascending order), tp[t][P] = 0.  The walk: the pairs (d >= k, g) with iou > thr[t], strictly, in descending IoU
 *           -- among bit-equal IoUs the pair enumerated later (detection-major, ground-truth-minor) first, which is
 *           np.argsort(ious, kind="stable")[::-1] where the tool leaves the order of equal keys to NumPy's unstable sort; a pair is
 *           a match when neither its detection nor its ground truth is matched yet;
 *   status  [N] int32: MRCNN_AP_SWEEP_OK; MRCNN_AP_SWEEP_OVER_CANDIDATES when more than MRCNN_AP_SWEEP_MAX_CAND pairs of the problem
 *           lie above the smallest threshold (found on the device: the list is kept in LDS); MRCNN_AP_SWEEP_OVER_ROWS for a problem
 *           of more than MRCNN_AP_SWEEP_MAX_DET detections or MRCNN_AP_SWEEP_MAX_GT ground truths.  The tp rows of a problem whose
 *           status is not OK are zeros: the caller computes that problem, and only that, with the host statement.
 * One workgroup of 256 lanes per problem, 62 KiB of LDS (two per CU): the pairs above the smallest threshold are collected, sorted
 * by the unique key (IoU descending, pair descending) and walked once per (t, k) by a lane with its own bit sets.  No atomics on
 * global memory, nothing allocated, bitwise the same from run to run.  N or T <= 0, D or G < 0: MRCNN_ERR_ARG;
 * T > MRCNN_AP_SWEEP_MAX_THR: MRCNN_ERR_UNSUPPORTED, nothing launched.  mrcnn_ap_sweep_caps writes the four caps (detections,
 * ground truths, thresholds, candidates) to caps[0 .. 3] (HOST pointer).                                                         */
#define MRCNN_AP_SWEEP_MAX_DET 128      /* >= DETECTION_MAX_INSTANCES = 100 of the reference configuration */
#define MRCNN_AP_SWEEP_MAX_GT 320       /* >= MAX_GT_INSTANCES = 300 */
#define MRCNN_AP_SWEEP_MAX_THR 16
#define MRCNN_AP_SWEEP_MAX_CAND 4096
#define MRCNN_AP_SWEEP_OK 0
#define MRCNN_AP_SWEEP_OVER_CANDIDATES 1
#define MRCNN_AP_SWEEP_OVER_ROWS 2
int mrcnn_ap_sweep_caps(int32_t* caps);
int mrcnn_ap_sweep(const double* det_box, const int32_t* det_off, int D, const double* gt_box, const int32_t* gt_off, int G, int N,
                   const double* thr, int T, int32_t* tp, int32_t* status, void* stream);

/* detect() post-processing (MaskRCNN.unmold_detections, mrcnn/model.py:2607-2619; utils.unmold_mask, mrcnn/utils.py:629-645;
 * utils.resize -> skimage.transform.resize(order=1, mode='constant', cval=0, clip=True), mrcnn/utils.py:957-978): for each of
 * the n detections of ONE image, resize the class channel of its MH x MW mask to its integer pixel box (float64, half-pixel
 * centres, zero outside the mask, clipped to the mask's [min, max]), threshold `>= 0.5` and paste it into the image plane.
 *   mrcnn_mask [n_rows, MH, MW, C] float32 (the graph's output for this image);
 *   dets [n, 6] int32 = (y1, x1, y2, x2, class_id, row): box in pixels of the ORIGINAL image (y2 / x2 exclusive, as
 *        utils.denorm_boxes returns them; the box arithmetic and the zero-area filter stay with the caller), the class
 *        channel and the row of mrcnn_mask the detection came from;
 *   out  packed == 0: [H, W, n] uint8 0 / 1 (np.stack(full_masks, axis=-1) of the reference, viewable as bool);
 *        packed != 0: [H, W, ceil(n / 8)] uint8, bit (d & 7) of byte d >> 3 = detection d (little bit order).
 * Pixels of a box outside the image are dropped.  workspace: mrcnn_unmold_masks_workspace(n, MH, MW) bytes.          */
size_t mrcnn_unmold_masks_workspace(int n, int MH, int MW);
int mrcnn_unmold_masks(const float* mrcnn_mask, int n_rows, int MH, int MW, int C, const int32_t* dets, int n, int H, int W,
                       int packed, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* FITS tile -> network input image (utils.read_fits, mrcnn/utils.py:1033-1163, on the run.py path: stretch, normalize,
 * convertToRGB, to_uint8; per-channel astropy ZScaleInterval(contrast) [3P] -> / max -> round(255 x), :1101-1111, :1166-1208):
 *   raw   [H, W] float32 as stored in the file (big_endian != 0: FITS byte order, swapped on the device) -- the caller has
 *         parsed the header and cut the tile; NaN pixels are replaced by the minimum of the others (:1090-1091);
 *   zscale_contrasts  3 doubles (HOST pointer, read at call time);
 *   rgb   [H, W, 3] uint8, byte-identical to the host statement caesar-mrcnn_amd/fits.py:read_fits.
 * Tiles up to 4096 x 1024 pixels (else MRCNN_ERR_UNSUPPORTED: use the host path).  workspace: mrcnn_fits_workspace(H, W).
 * The call IS mrcnn_fits_to_image (below) with the descriptor {zscale 1, biascontrast 0, normalize 1, out_kind 0, these
 * contrasts, bias 0.5, contrast 1} and out_bytes = 3 * H * W: the same launches, the same statuses in the same order, after
 * MRCNN_ERR_ARG for a null zscale_contrasts.                                                                                */
size_t mrcnn_fits_workspace(int H, int W);
int mrcnn_fits_to_rgb(const void* raw, int big_endian, int H, int W, const double* zscale_contrasts, void* rgb, void* workspace,
                      size_t workspace_bytes, void* stream);

/* The same chain for T tiles of ONE plane that stays on the device (the mosaic of the tiled source finder), each of the three
 * stages one launch over all tiles:
 *   plane       [NY, NX] float32, native or (big_endian != 0) in FITS byte order; addressed with 64-bit indices, row stride NX;
 *   tiles_host  T rectangles (columns x0 .. x0 + w - 1, rows y0 .. y0 + h - 1; sizes may differ, rectangles may overlap) with the
 *               layout of the pools: pixel_offset[t] = sum of w * h of the tiles before t, chunk_offset[t] = sum of their
 *               ceil(w * h / 1024); HOST pointer, checked before anything is launched: T <= 0, w or h <= 0, a rectangle that
 *               leaves the plane or offsets other than these: MRCNN_ERR_ARG; a tile of more than 2048 x 2048 pixels (or
 *               T > 65535): MRCNN_ERR_UNSUPPORTED -- nothing launched, nothing written;
 *   tiles_dev   the same table on the device;
 *   rgb         pool of rgb_bytes >= 3 * sum(w * h) bytes (else MRCNN_ERR_ARG): tile t is the [h, w, 3] uint8 image at byte
 *               3 * pixel_offset[t], each byte-identical to mrcnn_fits_to_rgb of that cut (pixels enumerated row-major within the
 *               tile).
 * The call IS mrcnn_fits_tiles_to_image (below) with the descriptor of mrcnn_fits_to_rgb.
 * workspace: mrcnn_fits_tiles_workspace(tiles_host, T, NY, NX) bytes (0 for a table the call would refuse);
 * mrcnn_fits_tiles_check: the status the call would return for that table (the host-side check alone; launches nothing).     */
typedef struct mrcnn_fits_tile {
    int32_t x0, y0, w, h;
    int64_t pixel_offset;
    int64_t chunk_offset;
} mrcnn_fits_tile;
int mrcnn_fits_tiles_check(const mrcnn_fits_tile* tiles_host, int T, int NY, int NX);
size_t mrcnn_fits_tiles_workspace(const mrcnn_fits_tile* tiles_host, int T, int NY, int NX);
int mrcnn_fits_tiles_to_rgb(const void* plane, int big_endian, int NY, int NX, const mrcnn_fits_tile* tiles_host,
                            const mrcnn_fits_tile* tiles_dev, int T, const double* zscale_contrasts, void* rgb, size_t rgb_bytes,
                            void* workspace, size_t workspace_bytes, void* stream);

/* The chain itself, for every flag combination of utils.read_fits (stretch, stretch_biascontrast, normalize, convertToRGB,
 * to_uint8; the host statement is caesar-mrcnn_amd/fits.py:read_fits, held bit for bit).  Per channel c of zscale contrast zc:
 *   zscale        c = float32(ZScaleInterval(zc)(c))
 *   biascontrast  c = float32(clip((float64(c) - bias) * contrast + 0.5, 0, 1))    three separately rounded operations
 *   normalize, or out_kind 0 / 1:  c = c / max(c)                           float32
 *   out_kind 0: uint8 [H, W, 3] = round(255 c)   1: float32 [H, W, 3] = c * 255   2: float32 [H, W] = channel 0 as it is
 * Without zscale the sampling / sort / fit workgroup is not launched: a reduction of the statistics table gives the minimum
 * (the NaN fill) and the maximum.
 * MRCNN_ERR_UNSUPPORTED: out_kind 0 with neither stretch (nothing clips the channel to [0, 1]; the host casts out-of-range
 * floats to uint8, which is platform-defined) and a tile above 2048 x 2048 pixels; MRCNN_ERR_ARG: out_kind outside 0 .. 2.
 * A tile without a finite pixel under zscale, or of NaNs alone: zeros for out_kind 0, NaN for the float outputs (the host
 * raises under zscale).  out: out_bytes >= 3 / 12 / 4 bytes per pixel; for the tiled entry a pool with tile t at
 * pixel_offset[t] times that.  workspace: mrcnn_fits_workspace / mrcnn_fits_tiles_workspace; the tile table and its check are
 * those described above.  mrcnn_fits_image_check: the status mrcnn_fits_to_image would return for that descriptor and size
 * (host-side alone; launches nothing).  16-byte aligned out and workspace take the vector stores; any other alignment (of the
 * element type) stores pixel by pixel, to the same values.
 * A call that is faulty in more than one way reports the first of, for mrcnn_fits_to_image: the descriptor (null or out_kind:
 * MRCNN_ERR_ARG; the refused combination: MRCNN_ERR_UNSUPPORTED), H or W <= 0 (MRCNN_ERR_ARG), the tile's size
 * (MRCNN_ERR_UNSUPPORTED), a null raw or out, out_bytes (MRCNN_ERR_ARG), the workspace (MRCNN_ERR_WORKSPACE) -- so a null
 * pointer WITH an oversize tile is MRCNN_ERR_UNSUPPORTED; for mrcnn_fits_tiles_to_image: the descriptor, a null plane, out or
 * tiles_dev (MRCNN_ERR_ARG), the tile table (MRCNN_ERR_ARG or MRCNN_ERR_UNSUPPORTED, as above), out_bytes, the workspace -- so
 * there a null pointer with an oversize tile is MRCNN_ERR_ARG.  Nothing is launched or written on any of them.                */
typedef struct mrcnn_fits_chain {
    int32_t zscale;        /* stretch_img per channel */
    int32_t biascontrast;  /* stretch_img_biasconstrast after it */
    int32_t normalize;     /* normalize_img */
    int32_t out_kind;
    double zscale_contrasts[3];
    double bias, contrast;
} mrcnn_fits_chain;
int mrcnn_fits_image_check(const mrcnn_fits_chain* chain, int H, int W);
int mrcnn_fits_to_image(const void* raw, int big_endian, int H, int W, const mrcnn_fits_chain* chain, void* out, size_t out_bytes,
                        void* workspace, size_t workspace_bytes, void* stream);
int mrcnn_fits_tiles_to_image(const void* plane, int big_endian, int NY, int NX, const mrcnn_fits_tile* tiles_host,
                              const mrcnn_fits_tile* tiles_dev, int T, const mrcnn_fits_chain* chain, void* out, size_t out_bytes,
                              void* workspace, size_t workspace_bytes, void* stream);

/* The overview frame of a whole mosaic (the host statement is fits.mosaic_overview_host): the chain of
 * mrcnn_fits_to_rgb on the WHOLE plane with one zscale contrast, then shrunk by block maxima:
 *   plane   [ny, nx] float32 where it lies, native or (big_endian != 0) in FITS byte order; 4-byte aligned (16-byte aligned
 *           planes are read with 16-byte loads).  It is read twice, once for the statistics and once for the pixels; no copy of
 *           it is made;
 *   G       [ny, nx] = one channel of mrcnn_fits_to_rgb(plane) with zscale_contrasts = (contrast, contrast, contrast);
 *   out     [h, w, 3] uint8, h = ceil(ny / shrink), w = ceil(nx / shrink): out[Y, X, :] = max of G over rows shrink Y ..
 *           min(shrink (Y + 1), ny) - 1 and columns shrink X .. min(shrink (X + 1), nx) - 1; out_bytes >= 3 h w.  A plane
 *           without a finite pixel gives zeros.
 * ny, nx or shrink <= 0, a contrast that is not finite, a missing or misaligned pointer, out_bytes too small: MRCNN_ERR_ARG;
 * ny * nx > 2^31 - 1: MRCNN_ERR_UNSUPPORTED; a workspace below mrcnn_mosaic_overview_workspace(ny, nx) (24 bytes per 1024
 * pixels; 0 for a plane the call would refuse) or not 16-byte aligned: MRCNN_ERR_WORKSPACE.  A refused call launches and writes
 * nothing.  mrcnn_mosaic_overview_check: the status for those sizes; launches nothing.  Four launches on `stream`, nothing
 * allocated, nothing synchronised, no floating-point atomics: bitwise the same from run to run.                              */
int mrcnn_mosaic_overview_check(int ny, int nx, int shrink, double contrast);
size_t mrcnn_mosaic_overview_workspace(int ny, int nx);
int mrcnn_mosaic_overview(const void* plane, int big_endian, int ny, int nx, int shrink, double contrast, void* out, size_t out_bytes,
                          void* workspace, size_t workspace_bytes, void* stream);

/* detect() pre-processing (MaskRCNN.mold_inputs, mrcnn/model.py:2519-2556, for uint8 images): utils.resize_image's pixel work
 * (mrcnn/utils.py:456-561: bilinear up-scaling h x w -> oh x ow through skimage.transform.resize(order=1, mode='constant',
 * clip=True, preserve_range=True) [3P], zero padding into the OH x OW canvas at (top, left), cast to uint8) and mold_image
 * (mrcnn/model.py:2964-2969: float32 minus MEAN_PIXEL).  src [h, w, C] uint8 (C <= 4), out [OH, OW, C] float32 -- identical to
 * the host path (caesar-mrcnn_amd/utils.py:resize_image + mold_image); the caller computes scale, (oh, ow) = (round(h * scale),
 * round(w * scale)) and the padding as the reference does.  mean_pixel: C doubles on the HOST.  workspace: >= 8 bytes.   */
int mrcnn_mold_image_u8(const void* src, int h, int w, int C, int oh, int ow, int top, int left, int OH, int OW,
                        const double* mean_pixel, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* The first half alone, for the training loader (load_image_gt augments between resize_image and mold_image,
 * mrcnn/model.py:1300-1359): out [OH, OW, C] uint8 = utils.resize_image(src) -- the same float64 bilinear, clip to the source's
 * min / max and truncation per value, zero padding.  Same arguments, refusals and workspace.                              */
int mrcnn_resize_image_u8(const void* src, int h, int w, int C, int oh, int ow, int top, int left, int OH, int OW, void* out,
                          void* workspace, size_t workspace_bytes, void* stream);
/* The float32 twin of mrcnn_mold_image_u8, for read_fits' float32 RGB and gray images: src [h, w, C] float32 (C <= 4), same
 * scalar arguments.  resize_image keeps the image's dtype: utils.resize's float64 bilinear in its order, np.clip to the source's
 * minimum / maximum as NumPy evaluates it, rounded to float32, zero padding, minus mean_pixel in float64, rounded to float32 --
 * MaskRCNN.mold_inputs followed by the float32 cast of the graph's input, bit for bit wherever the value is not NaN, NaN in the
 * same places.  A NaN in a source that is scaled makes the bounds NaN and the scaled image NaN throughout (np.clip); unscaled,
 * nothing is clipped and a NaN stays where it was.  The min / max pass runs only when (oh, ow) != (h, w): up to 1024 workgroups
 * write one record each, a one-workgroup second stage reduces them (no atomics, bitwise reproducible; -0.0 orders below +0.0).
 * workspace: mrcnn_mold_image_f32_workspace_bytes() bytes, 16-byte aligned (MRCNN_ERR_WORKSPACE otherwise); src / out not
 * 4-byte aligned: MRCNN_ERR_ARG.  At most three launches on `stream`, nothing allocated or synchronised.                    */
size_t mrcnn_mold_image_f32_workspace_bytes(void);
int mrcnn_mold_image_f32(const void* src, int h, int w, int C, int oh, int ow, int top, int left, int OH, int OW,
                         const double* mean_pixel, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* Elementwise helpers on flat buffers. */
int mrcnn_add_inplace(float* dst, const float* src, int64_t n, void* stream);
int mrcnn_softmax_rows(const float* logits, float* probs, int64_t rows, int C, void* stream);

/* PyramidROIAlign (mrcnn/model.py:428-534): level = clamp(4 + round(log2(sqrt(h*w)/(224/sqrt(area)))),
 * 2, 5); tf.image.crop_and_resize(bilinear, extrapolation 0), one sample per bin, output in the
 * original ROI order.  boxes [B, R, 4] normalised (y1,x1,y2,x2); fm[l] = P(2+l) as [B, Hl, Wl, C].
 * out [B, R, P, P, C].  C must be a multiple of 64*4 = 256 lanes-of-float4 ... any multiple of 4.   */
typedef struct mrcnn_roialign_desc {
    int32_t B, R, P, C;
    int32_t H[4], W[4];
    float image_area;        /* IMAGE_SHAPE[0]*IMAGE_SHAPE[1] as float32 */
} mrcnn_roialign_desc;
int mrcnn_roialign_fwd(const mrcnn_roialign_desc* d, const float* boxes, const float* fm2,
                       const float* fm3, const float* fm4, const float* fm5, float* out,
                       int32_t* level_out, void* stream);
/* Adjoint: scatter-add (float atomics) of dout into the four pre-zeroed/accumulating maps. */
int mrcnn_roialign_bwd(const mrcnn_roialign_desc* d, const float* boxes, const float* dout,
                       float* dfm2, float* dfm3, float* dfm4, float* dfm5, void* stream);

/* Same adjoint in gather form for the case where every ROI carries gradient (the class head in training: TF autodiff
 * of tf.image.crop_and_resize at mrcnn/model.py:505).  Bilinear sampling is separable, so each destination pixel reads
 * off its contributions directly: one wave per pyramid pixel walks the ROIs of its image and level, finds the sample
 * rows / columns whose floor or ceil is that pixel, and accumulates  wy*wx*dout[roi,py,px,:]  in registers -- one row of
 * atomics per pixel instead of four per bin, no sorting, fixed summation order.  C must be 256 and P <= 32 (else
 * MRCNN_ERR_UNSUPPORTED, nothing launched); same values as mrcnn_roialign_bwd up to fp32 summation order.          */
int mrcnn_roialign_bwd_gather(const mrcnn_roialign_desc* d, const float* boxes, const float* dout, float* dfm2,
                              float* dfm3, float* dfm4, float* dfm5, void* stream);
/* The same with 16-bit pyramid levels and a 16-bit pooled output (BASELINE configs[4]; dtype MRCNN_DTYPE_F16 / _BF16):
 * interpolation in float32, one rounding.  The adjoint reads the 16-bit gradient (times `multiplier`, e.g. 1 / loss scale)
 * and adds float32 atomics into the float32 pyramid gradients.                                                        */
int mrcnn_roialign_fwd_h16(const mrcnn_roialign_desc* d, int dtype, const float* boxes, const void* fm2, const void* fm3,
                           const void* fm4, const void* fm5, void* out, void* stream);
int mrcnn_roialign_bwd_h16(const mrcnn_roialign_desc* d, int dtype, const float* boxes, const void* dout, float multiplier,
                           float* dfm2, float* dfm3, float* dfm4, float* dfm5, void* stream);

/* ProposalLayer (mrcnn/model.py:329-406): per image, scores = rpn_probs[:, 1]; top-k(min(pre_nms, A),
 * sorted, ties -> lower index); decode with deltas*std; clip to [0,1]; greedy NMS (IoU > thr
 * suppresses, TF non_max_suppression semantics); gather; zero-pad to proposal_count.
 * Outputs: rois [B, proposal_count, 4]; optional debug outputs top_idx [B, K] (int32 anchor ids in
 * sorted order), keep_idx [B, proposal_count] (positions into the sorted list, -1 padded),
 * num_keep [B].  workspace from mrcnn_proposal_workspace().                                        */
typedef struct mrcnn_proposal_desc {
    int32_t B, A, pre_nms_limit, proposal_count;
    float nms_threshold;
    float std_dev[4];
} mrcnn_proposal_desc;
size_t mrcnn_proposal_workspace(const mrcnn_proposal_desc* d);
int mrcnn_proposal_fwd(const mrcnn_proposal_desc* d, const float* rpn_probs, const float* rpn_bbox,
                       const float* anchors, float* rois, int32_t* top_idx, int32_t* keep_idx,
                       int32_t* num_keep, void* workspace, size_t workspace_bytes, void* stream);

/* Health words of the multi-workgroup top-k selection (A >= 32 768), for a host that has synchronised anyway: returns
 * the byte offset from `workspace` of image 0's three uint32 {keys collected, keys announced, stores refused by the
 * bounds guard}; *stride_bytes = distance between images.  A healthy call leaves collected == announced == K and
 * refused == 0; anything else makes the sort kernel discard the pre-selection and select by itself (same result).
 * A call without a pre-selection (A < 32 768, or A <= pre_nms_limit) writes {0, 0, 0}.  */
size_t mrcnn_proposal_status_offset(const mrcnn_proposal_desc* d, const void* workspace, size_t* stride_bytes);

/* DetectionTargetLayer (mrcnn/model.py:570-763) for one batch.  rand_keys [B, R] uniform floats
 * replace tf.random.shuffle: candidates are taken in increasing key order (ties -> lower index).
 * gt_masks is the reference layout [B, MH, MW, G] (uint8 0/1).  Outputs are zero padded to T.       */
typedef struct mrcnn_dettarget_desc {
    int32_t B, R, G, T, MH, MW, mask_h, mask_w;
    int32_t positive_count;      /* int(TRAIN_ROIS_PER_IMAGE * ROI_POSITIVE_RATIO), model.py:635 */
    float negative_ratio_r;      /* float32(1.0 / ROI_POSITIVE_RATIO), model.py:641-642 */
    float bbox_std_dev[4];
    int32_t use_mini_mask;
} mrcnn_dettarget_desc;
int mrcnn_detection_targets(const mrcnn_dettarget_desc* d, const float* proposals,
                            const int32_t* gt_class_ids, const float* gt_boxes,
                            const uint8_t* gt_masks, const float* rand_keys, float* rois,
                            int32_t* target_class_ids, float* target_bbox, float* target_mask,
                            int32_t* roi_gt_assignment, int32_t* counts, void* stream);

/* ---- 16-bit matrix-core path (BASELINE.json configs[4]; stage 1: the convolutions of the ROI heads) ------------
 * Operands float16 / bfloat16, accumulation + bias + frozen-BN affine + activation float32, one rounding of the
 * result.  Shapes: Cin % 32 == 0, Cout % 128 == 0, dense NHWC output, no residual (the mask / class head layers).
 * w_t is the transposed weight image [Cout][KH*KW*Cin] written by mrcnn_weights_to_h16 (wt_fwd); its second
 * output wt_dgrad [Cin][KH*KW*Cout] (taps rotated by 180 degrees) is the operand of the data gradient, which is
 * the same convolution applied to dz with Cin/Cout swapped and padding (k-1)/2.  Either output may be NULL.   */
#define MRCNN_DTYPE_F16 0
#define MRCNN_DTYPE_BF16 1
int mrcnn_conv2d_fwd_h16(const mrcnn_conv_desc* d, int dtype, const void* x, const void* w_t, const float* bias,
                         const float* scale, const float* shift, void* out, void* z_out, void* stream);
/* The same with a 16-bit residual `res` (shape and strides of out; d->res_mode must be MRCNN_RES_SAME exactly when res is
 * given) added before the activation -- the shortcut of a bottleneck block (mrcnn/model.py:99-131), or the accumulating
 * input of a data gradient -- and with arbitrary output strides (a stride-2 1x1 data gradient scatters into a zeroed
 * tensor).  Shapes: as above, or the small-tile kernel for the trunk's layers: Cin % 64 == 0, Cout % 64 == 0, plain NHWC
 * (strided allowed), the only one with the residual port.  mrcnn_conv2d_fwd_h16_supported() tells whether a descriptor
 * (with / without residual) has a 16-bit kernel.                                                                     */
int mrcnn_conv2d_fwd_h16_res(const mrcnn_conv_desc* d, int dtype, const void* x, const void* w_t, const float* bias,
                             const float* scale, const float* shift, const void* res, void* out, void* z_out, void* stream);
int mrcnn_conv2d_fwd_h16_supported(const mrcnn_conv_desc* d, int has_res);
/* mrcnn_conv2d_dgrad_ep in 16 bits (small-tile kernel: Cin % 64 == 0, Cout % 64 == 0, stride 1, dense output): the data
 * gradient y = conv(dz, w_t) (+ res), fused with the epilogue backward of the layer below -- stored is
 * dz_below = y * act'(out_below) * scale_below (and dy = y * act' when asked); dbeta / dgamma / dbias accumulate in
 * float32, multiplied by grad_multiplier (1 / loss scale).  MRCNN_ERR_UNSUPPORTED for other shapes.                */
typedef struct mrcnn_bwd_epilogue_h16 {
    const void* out; const void* z;              /* 16-bit activated output / pre-BN value of the layer below */
    const float* scale; const float* mean; const float* rstd;
    float* dgamma; float* dbeta; float* dbias;
    int32_t act;                                 /* MRCNN_ACT_NONE or MRCNN_ACT_RELU */
    void* dy;                                    /* optional second output (16 bit) */
    float grad_multiplier;
} mrcnn_bwd_epilogue_h16;
int mrcnn_conv2d_dgrad_ep_h16(const mrcnn_conv_desc* d, int dtype, const void* dz, const void* w_t, const void* res,
                              void* dz_below, const mrcnn_bwd_epilogue_h16* ep, void* stream);
/* Host-only query: what mrcnn_conv2d_fwd_h16_res (ep == NULL) or mrcnn_conv2d_dgrad_ep_h16 (ep != NULL; x = dz, out = dz_below)
 * would launch for these arguments, and the status it would return.  Launches nothing and never dereferences a tensor pointer:
 * only nullness and 16-byte alignment are looked at, so it runs without a GPU (the rules that count CUs then assume the MI355X's
 * 256).  Reads the same switches as the launch -- per call: MRCNN_H16_SMALL, MRCNN_H16_TILE, MRCNN_H16_RING, MRCNN_H16P_NO_SPLIT,
 * MRCNN_H16P_GRID, MRCNN_H16W_DBG, MRCNN_H16P_TRACE and the tuning keys "h16_phase" / "h16_slab"; once per process:
 * MRCNN_H16_SLAB, MRCNN_H16S_EP_VEC.  *plan is written only with MRCNN_OK.                                                   */
#define MRCNN_H16_S64 0            /* conv_fwd_h16s_kernel: 64 x 64 tiles (residual port, strided output, backward epilogue) */
#define MRCNN_H16_T128 1           /* conv_fwd_h16_kernel<T, 2, 2, 2>: 256 x 128, double buffered */
#define MRCNN_H16_RING 2           /* <T, 3, 2, 2>: the same with a 3-slot ring */
#define MRCNN_H16_BIG 3            /* <T, 4, 2, 4>: 256 x 256, 4-stage ring */
#define MRCNN_H16_WAVE128 4        /* <T, 4, 2, 2, 4>: 256 x 256, four waves of 128 x 128 */
#define MRCNN_H16_PHASE 5          /* conv_fwd_h16p_kernel<T, zout, false>: persistent phased 256 x 256 tiles */
#define MRCNN_H16_PHASE_DECONV 6   /* conv_fwd_h16p_kernel<T, false, true>: the same with the pixel-shuffle store */
#define MRCNN_H16_SLAB 7           /* conv_fwd_h16q_kernel<T, zout>: the phased tile with slab-plus-halo staging */
typedef struct mrcnn_h16_plan {
    int32_t kernel, zout;          /* MRCNN_H16_*; the kernel's ZOUT template argument (phased kernels with a z_out) */
    int32_t grid, threads;         /* workgroups and threads per workgroup of the (first) launch */
    int32_t ptiles, mtile0;        /* ConvH16Args of that launch: tiles a persistent launch owns (0 otherwise); MRCNN_H16W_DBG */
    int32_t rem_grid, rem_mtile0;  /* the small-tile launch for a partial last round: workgroups (0 = none), its first 64-row tile */
    int32_t ep_vec, dense, fused_ep;   /* 16-byte epilogue of the small tile; plain NHWC output; ep given */
    int32_t reserved;
    uint64_t trace;                /* MRCNN_H16P_TRACE: the address the phased kernel stamps (0 = none) */
} mrcnn_h16_plan;
int mrcnn_conv2d_fwd_h16_plan(const mrcnn_conv_desc* d, int dtype, const void* x, const void* w_t, const float* bias,
                              const float* scale, const float* shift, const void* res, const void* out, const void* z_out,
                              const mrcnn_bwd_epilogue_h16* ep, mrcnn_h16_plan* plan);
int mrcnn_weights_to_h16(const float* w_hwio, void* wt_fwd, void* wt_dgrad, int KH, int KW, int Cin, int Cout,
                         int dtype, void* stream);
/* All 16-bit weight images of a model in one launch.  table: n_layers records {int64 offset of the float32 HWIO kernel in
 * `params` (floats); uint64 W^T image pointer; uint64 data-gradient image pointer or 0; int32 KH, KW, Cin, Cout, first_tile,
 * pad} (48 bytes each), first_tile = running sum of KH*KW*ceil(Cin/32)*ceil(Cout/32); total_tiles = the sum over all layers. */
int mrcnn_weights_to_h16_batched(const float* params, const void* table, int n_layers, int total_tiles, int dtype, void* stream);
/* Weight gradient with 16-bit operands x [N,H,W,Cin], dy [N,OH,OW,Cout]: dw (float32, HWIO) = multiplier * sum
 * (or dw += ... with beta_acc); float32 accumulation, slabs per pixel split summed in a fixed order.
 * Cin % 256 == 0, Cout % 128 == 0.  The workspace also holds a per-pixel offset / tap-mask table.           */
size_t mrcnn_conv2d_wgrad_h16_workspace(const mrcnn_conv_desc* d);
int mrcnn_conv2d_wgrad_h16(const mrcnn_conv_desc* d, int dtype, const void* x, const void* dy, float* dw,
                           void* workspace, size_t workspace_bytes, int beta_acc, float multiplier, void* stream);
/* Host-only query, as mrcnn_conv2d_fwd_h16_plan: what mrcnn_conv2d_wgrad_h16 would launch and the status it would return.
 * Switches: MRCNN_WGRAD_H16_PHASE (per call), MRCNN_WGRAD_XCD (once per process).                                        */
#define MRCNN_H16_WGRAD_TABLE 0    /* pixel_table_kernel + conv_wgrad_h16_kernel: 256 x 128 tiles, table driven */
#define MRCNN_H16_WGRAD_PHASE 1    /* conv_wgrad_h16p_kernel: phased 256 x 256 tiles */
#define MRCNN_H16_RED_SCALAR 0     /* wgrad_h16_reduce_kernel */
#define MRCNN_H16_RED_VEC 1        /* wgrad_h16_reduce_vec_kernel: n % 4 == 0, slabs and dw 16-byte aligned */
typedef struct mrcnn_h16_wgrad_plan {
    int32_t kernel;                /* MRCNN_H16_WGRAD_* */
    int32_t splits, chunk;         /* pixel splits (= slabs) and rows per split */
    int32_t nk, itiles, ntiles;    /* phased kernel: K-steps of 64 rows per split, 256-row tiles of KH*KW*Cin, 256-column tiles */
    int32_t grid;                  /* workgroups of the gradient kernel */
    int32_t reduce, reduce_grid;   /* MRCNN_H16_RED_* and its workgroups */
    int32_t xcd_order;             /* MRCNN_WGRAD_XCD */
    int64_t table_bytes, slab_bytes;   /* workspace: pixel table (reserved for either kernel), then 256-byte aligned the slabs */
    int64_t workspace_bytes;       /* what mrcnn_conv2d_wgrad_h16_workspace answers: room for either kernel's slabs */
} mrcnn_h16_wgrad_plan;
int mrcnn_conv2d_wgrad_h16_plan(const mrcnn_conv_desc* d, int dtype, const void* x, const void* dy, const float* dw,
                                const void* workspace, size_t workspace_bytes, mrcnn_h16_wgrad_plan* plan);
/* mrcnn_epilogue_bwd on 16-bit tensors (act NONE / RELU, C a power of two >= 16): dz_out 16 bit; the float32 channel
 * sums dgamma / dbeta / dbias are multiplied by grad_multiplier (1 / loss scale) before they are added.          */
int mrcnn_epilogue_bwd_h16(int dtype, const void* dout, const void* out, const void* z, const float* scale,
                           const float* mean, const float* rstd, void* dz_out, float* dgamma, float* dbeta,
                           float* dbias, int64_t M, int C, int act, float grad_multiplier, void* stream);
/* The same with a second output dy_out = dout * act'(out) (before the BatchNorm scale): what the shortcut of a bottleneck
 * block receives when the block's last convolution is differentiated (mrcnn/model.py:128-130, Add + Activation).      */
int mrcnn_epilogue_bwd_h16_dy(int dtype, const void* dout, const void* out, const void* z, const float* scale,
                              const float* mean, const float* rstd, void* dz_out, void* dy_out, float* dgamma, float* dbeta,
                              float* dbias, int64_t M, int C, int act, float grad_multiplier, void* stream);
/* Output stage of the mask head on a 16-bit deconvolution output `up` [M,H,W,Cd] (mrcnn_conv2d_fwd_h16 with out_mode
 * MRCNN_OUT_DECONV2 writes it): mask_out [M,H,W,C] float32 = sigmoid(up . w_mask + b_mask); and the one-pass backward
 * of mrcnn_mask_out_bwd with dzg written in 16 bits times loss_scale (the sums dw_mask / db_mask / db_deconv stay
 * float32 and unscaled).  Cd % 256 == 0 (forward), C <= 16.  MRCNN_MASK_OUT_BWD_V8=0 (read once per process, with the
 * other switches of the 16-bit file) keeps the backward off its 16-byte form.                                        */
int mrcnn_mask_out_fwd_h16(int dtype, const void* up, const float* w_mask, const float* b_mask, float* mask_out,
                           int64_t npix, int Cd, int C, void* stream);
int mrcnn_mask_out_bwd_h16(int dtype, const float* d_mask_out, const float* mask_out, const void* up, const float* w_mask,
                           void* dzg, float* dw_mask, float* db_mask, float* db_deconv, int64_t M, int H, int W, int Cd,
                           int C, float loss_scale, void* stream);
int mrcnn_cast_to_h16(const float* src, void* dst, int64_t n, int dtype, float multiplier, void* stream);
int mrcnn_cast_from_h16(const void* src, float* dst, int64_t n, int dtype, float multiplier, void* stream);
/* dst[i] += multiplier * src[i]: a 16-bit data gradient (scaled by the loss scale) added to a float32 accumulator, e.g.
 * the RPN's contribution to the pyramid gradients the ROI heads have already written (fan-out of P2..P5, model.py:2040). */
int mrcnn_axpy_from_h16(const void* src, float* dst, int64_t n, int dtype, float multiplier, void* stream);

/* build_rpn_targets (mrcnn/model.py:1536-1644), the per-image RPN target builder of the CPU input
 * pipeline, for one batch on the device.  anchors [A,4] float64 pixels (utils.generate_pyramid_anchors);
 * gt_class_ids [B,G] (>0 instance, <0 crowd, 0 padding); gt_boxes [B,G,4] int32 pixels; rand_keys [B,A]
 * uniform floats replace the two np.random.choice draws: when more than n_train/2 positives (or more than
 * n_train - positives negatives) exist, the surplus with the SMALLEST keys is reset to neutral (ties ->
 * lower anchor index).  Outputs: rpn_match [B,A] in {-1,0,1}; rpn_bbox [B,n_train,4] = deltas of the
 * positives in ascending anchor order / bbox_std_dev, zero padded.  IoUs are float64 in the reference's
 * operation order, so rpn_match is bit-exact.  G <= 512.                                              */
typedef struct mrcnn_rpntarget_desc {
    int32_t B, A, G, n_train;    /* n_train = RPN_TRAIN_ANCHORS_PER_IMAGE */
    double bbox_std_dev[4];      /* RPN_BBOX_STD_DEV (float64 in the reference) */
} mrcnn_rpntarget_desc;
size_t mrcnn_rpn_targets_workspace(const mrcnn_rpntarget_desc* d);
int mrcnn_rpn_targets(const mrcnn_rpntarget_desc* d, const double* anchors, const int32_t* gt_class_ids,
                      const int32_t* gt_boxes, const float* rand_keys, int32_t* rpn_match, float* rpn_bbox,
                      void* workspace, size_t workspace_bytes, void* stream);

/* DetectionLayer / refine_detections_graph (mrcnn/model.py:770-909): detections [B, max_inst, 6]. */
typedef struct mrcnn_detection_desc {
    int32_t B, R, C, max_instances;
    float min_confidence, nms_threshold;
    float bbox_std_dev[4];
} mrcnn_detection_desc;
size_t mrcnn_detection_workspace(const mrcnn_detection_desc* d);
int mrcnn_detection_fwd(const mrcnn_detection_desc* d, const float* rois, const float* probs,
                        const float* deltas, const float* windows, float* detections,
                        void* workspace, size_t workspace_bytes, void* stream);

/* The five losses and their gradients w.r.t. the network outputs (mrcnn/model.py:1098-1270).
 * losses[5] = rpn_class, rpn_bbox, mrcnn_class, mrcnn_bbox, mrcnn_mask (each already the batch mean).
 * loss_weights scale the gradients (LOSS_WEIGHTS * USE_LOSSES).  Gradients are written dense.        */
typedef struct mrcnn_loss_desc {
    int32_t B, A, T, C, mask_h, mask_w, max_rpn_pos;   /* max_rpn_pos = rows of input_rpn_bbox */
    int32_t mask_loss_dice;
    float w[5];
} mrcnn_loss_desc;
size_t mrcnn_losses_workspace(const mrcnn_loss_desc* d);
int mrcnn_losses_fwd_bwd(const mrcnn_loss_desc* d, const int32_t* rpn_match, const float* rpn_bbox_t,
                         const float* rpn_class_logits, const float* rpn_bbox,
                         const int32_t* target_class_ids, const float* target_bbox,
                         const float* target_mask, const int32_t* active_class_ids,
                         const float* mrcnn_class_logits, const float* mrcnn_bbox,
                         const float* mrcnn_mask, float* losses, float* d_rpn_class_logits,
                         float* d_rpn_bbox, float* d_mrcnn_class_logits, float* d_mrcnn_bbox,
                         float* d_mrcnn_mask, void* workspace, size_t workspace_bytes, void* stream);
/* The same with class weights on the three head losses.  class_weights: device, [C] positive finite floats,
 * index 0 the background; NULL = unweighted, which is mrcnn_losses_fwd_bwd.  Every ROI row r carries
 * u_r = class_weights[target_class_ids[r]]:
 *   mrcnn_class = sum(u ce pa) / sum(pa)            mrcnn_bbox = sum_pos(u smooth_l1) / (4 npos)
 *   mrcnn_mask  = sum_pos(u sum_pix bce) / (npos npix), or with mask_loss_dice
 *                 1 - (2 sum(u y q) + s) / (sum(u y) + sum(u q) + s)
 * The normalisers stay plain counts, the two RPN losses and their gradients do not change, and weights of one give the
 * unweighted result bit for bit.  target_class_ids in [0, C) is the caller's precondition, as it is for the class logits. */
int mrcnn_losses_fwd_bwd_weighted(const mrcnn_loss_desc* d, const int32_t* rpn_match, const float* rpn_bbox_t,
                                  const float* rpn_class_logits, const float* rpn_bbox,
                                  const int32_t* target_class_ids, const float* target_bbox,
                                  const float* target_mask, const int32_t* active_class_ids,
                                  const float* mrcnn_class_logits, const float* mrcnn_bbox,
                                  const float* mrcnn_mask, const float* class_weights, float* losses,
                                  float* d_rpn_class_logits, float* d_rpn_bbox, float* d_mrcnn_class_logits,
                                  float* d_mrcnn_bbox, float* d_mrcnn_mask, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* keras.optimizers.SGD(lr, momentum, clipnorm) + L2/numel regulariser (mrcnn/model.py:2255-2291) on
 * flat buffers of n floats (n % 64 == 0).  gran_coef[n/64] describes each 64-float granule (every
 * tensor starts on a granule): >= 0 trainable with that L2 gradient coefficient (2*WEIGHT_DECAY/numel,
 * 0 for gamma/beta); < 0 frozen tensor or alignment padding (gradient forced to 0, parameter kept).
 *   mrcnn_grad_prepare: grads = grads*grad_scale + coef*params (grad_scale = 1/world averages the
 *     data-parallel sum) and *sumsq_out = sum(grads^2), reduced in a fixed order so that every rank
 *     derives the same clip factor;
 *   mrcnn_sgd_momentum: g *= clipnorm/norm if norm >= clipnorm; v = momentum*v - lr*g; w += v.       */
int mrcnn_grad_prepare(float* grads, const float* params, float grad_scale, const float* gran_coef,
                       int64_t n, float* sumsq_out, void* stream);
int mrcnn_sumsq(const float* g, int64_t n, float* out_scalar, void* stream);
int mrcnn_sgd_momentum(float* params, float* momentum_buf, const float* grads, const float* sumsq,
                       float clipnorm, float lr, float momentum, const float* gran_coef, int64_t n,
                       void* stream);
/* Mixed-precision form (BASELINE configs[4]; no counterpart in the float32 reference): when *sumsq is not finite -- a
 * float16 gradient overflowed under the loss scale -- the update is skipped on the device (weights and momentum untouched,
 * no host synchronisation) and *skipped_steps (device, 32-bit) is incremented.                                              */
int mrcnn_sgd_momentum_guarded(float* params, float* momentum_buf, const float* grads, const float* sumsq,
                               float clipnorm, float lr, float momentum, const float* gran_coef, int64_t n,
                               unsigned* skipped_steps, void* stream);

/* ---- Winograd F(m x n, 3x3), m, n = 2 or 4, for the stride-1 "same" 3x3 convolutions of the mask head
 * (KL.Conv2D(256, (3, 3), padding="same"), mrcnn/model.py:1058-1082), the FPN smoothing and the shared RPN convolution, float32:
 * (m + 2)(n + 2) multiplications per m x n outputs and channel pair instead of 9 m n -- 16 per 4 (2 x 2) or 36 per 16 (4 x 4).
 * A layer is covered by GROUPS of tiles: th_n x tw_n tiles per map of oth x otw outputs each, the first at output (oh0, ow0).  A
 * uniform tiling is one group at (0, 0) (edge tiles may hang over the map: their inputs read as zero, their outputs are dropped);
 * a map whose extent is not a multiple of 4 is covered without overhang by several: 14 x 14 = 3 x 3 tiles of 4 x 4, 3 x 1 of
 * 4 x 2 (columns 12..13), 1 x 3 of 2 x 4 (rows 12..13), one of 2 x 2: 484 multiplications per map and channel pair instead of 576
 * (uniform 4 x 4 with overhang) or 784 (uniform 2 x 2).  Three launches per group -- input transform, the (oth + 2)(otw + 2)
 * transform-domain GEMMs as ONE launch, output transform with the layer's epilogue (or, for a data gradient, the epilogue backward
 * of the layer below) -- and one weight transform U = G_oth g G_otw^T per group shape and weight update.  C % 4 == 0 (GEMM:
 * K % 16 == 0, Cout % 128 == 0).  Every group has its own V / Mt of mrcnn_winograd_group_floats floats each:
 * [(oth + 2)(otw + 2)][rows][C], rows = tiles rounded up to whole 128-row tiles.  The groups of a map write disjoint outputs;
 * their channel sums (output_bwd) and weight gradients (dw with accumulate) add up.  2 x 2 tiles use +-1 and 1/2 only: the result
 * differs from the direct kernels by float32 summation order (measured 2e-6 of the output maximum); 4 x 4 tiles have constants up
 * to 8 and cost about one more decimal digit (measured 1e-5).                                                                   */
typedef struct mrcnn_wino_group {
    int oth, otw;      /* outputs per tile, rows / columns: 2 or 4 */
    int th_n, tw_n;    /* tiles per map */
    int oh0, ow0;      /* output row / column of the first tile */
} mrcnn_wino_group;
size_t mrcnn_winograd_group_floats(const mrcnn_wino_group* g, int N, int C);
/* the uniform tiling of `tile` x `tile` outputs (2: H, W even; 4: any extent) as one group: its floats, its weight transform */
size_t mrcnn_winograd_buffer_floats(int N, int H, int W, int C, int tile);
int mrcnn_winograd_weights(const float* w_hwio, float* U, int Cin, int Cout, int tile, void* stream);   /* U [(tile + 2)^2][Cin][Cout] */
int mrcnn_winograd_weights_g(const float* w_hwio, float* U, int Cin, int Cout, int oth, int otw, void* stream);
int mrcnn_winograd_input_g(const float* x, float* V, int N, int H, int W, int C, const mrcnn_wino_group* g, void* stream);
int mrcnn_gemm_batched_f32(const float* V, const float* U, float* Mt, int nb, int rows, int K, int Cout, void* stream);
/* the same product by persistent workgroups (next tile's first stage in flight under the current tile's stores): what the layers use */
int mrcnn_winograd_gemm(const float* V, const float* U, float* Mt, int nb, int rows, int K, int Cout, void* stream);
int mrcnn_winograd_output_g(const float* Mt, float* out, float* z_out, const float* bias, const float* scale, const float* shift,
                            int N, int H, int W, int C, int act, const mrcnn_wino_group* g, void* stream);
/* Two 3 x 3 layers in a row, mixed tiling (H, W = 2 mod 4, > 4: H/4 x W/4 tiles of 4 x 4, H/4 of 4 x 2, W/4 of 2 x 4, one 2 x 2): the
 * output transform and epilogue of the first layer (mrcnn_winograd_output_g of all four groups: z_out = y + bias, stored unless
 * NULL; activated = act(scale z + shift)) and the input transform of the second (mrcnn_winograd_input_g of all four groups) as ONE
 * launch -- the activated output stays in LDS and is not written anywhere.  Mt and V_next hold the four groups end to end in the
 * order above, each of mrcnn_winograd_group_floats(g, N, C) floats.  z_out and V_next equal the separate calls' bit for bit.
 * MRCNN_ERR_UNSUPPORTED, nothing launched: another tiling (tile != MRCNN_WINO_TILE_MIXED), extents not 2 mod 4, C % 128 != 0, a
 * map of more than 2048 pixels, a group of 4 GiB or more -- use the separate calls. */
#define MRCNN_WINO_TILE_MIXED 6
int mrcnn_winograd_chain(const float* Mt, float* z_out, const float* bias, const float* scale, const float* shift, float* V_next,
                         int N, int H, int W, int C, int act, int tile, void* stream);
/* Data gradient: output transform of a group + epilogue backward of the layer below: g = y * act'(out_below), dz_below = g * scale.
 * Channel sums (of g, of g (z_below - mean) rstd when mean / rstd are given, of dz) leave as partials: the launch writes
 * mrcnn_winograd_output_bwd_rows(g, N, C) rows of [3][C] floats (one per workgroup, plain stores; partials may be NULL: no sums).
 * The groups of a layer write their rows one after the other into one buffer; mrcnn_winograd_output_bwd_sums then ADDS the
 * column sums of all `rows` rows to dbeta / dgamma / dbias (each may be NULL), in a fixed order: the same inputs give the same bits. */
int mrcnn_winograd_output_bwd_rows(const mrcnn_wino_group* g, int N, int C);
int mrcnn_winograd_output_bwd_g(const float* Mt, float* dz_below, const float* below_out, const float* below_z, const float* scale,
                                const float* mean, const float* rstd, float* partials, int N, int H, int W, int C, int act,
                                const mrcnn_wino_group* g, void* stream);
/* The same when the layer below is a ReLU layer with a frozen-BN affine (forward epilogue out = max(scale * z + shift, 0)): the
 * ReLU mask is recomputed from the stored z with the forward's own expression, so the activated output is not read. */
int mrcnn_winograd_output_bwd_zmask_g(const float* Mt, float* dz_below, const float* below_z, const float* scale, const float* shift,
                                      const float* mean, const float* rstd, float* partials, int N, int H, int W, int C,
                                      const mrcnn_wino_group* g, void* stream);
int mrcnn_winograd_output_bwd_sums(const float* partials, int rows, int C, float* dgamma, float* dbeta, float* dbias, void* stream);
/* The backward twin of mrcnn_winograd_chain, between the data gradients of two 3 x 3 layers (mixed tiling): ONE launch does
 * mrcnn_winograd_output_bwd_zmask_g of all four groups (Mt: the groups end to end), and from the dz it keeps in LDS both
 * mrcnn_winograd_input_g (V_next, for the next data gradient) and mrcnn_winograd_dy_g (dM, for the weight gradient of the layer
 * below) of all four groups, end to end as Mt.  dM may be NULL (not written); dz_out may be NULL, else dz is stored too.  dz, V_next
 * and dM equal the separate calls' bit for bit.  partials (may be NULL: no sums): N rows of [3][C], one per map, plain stores;
 * mrcnn_winograd_output_bwd_sums(partials, N, C, ...) adds them up.
 * MRCNN_ERR_UNSUPPORTED, nothing launched: the shapes mrcnn_winograd_chain refuses, or a layer below without z / scale / shift
 * (no ReLU mask from z) -- use the separate calls. */
int mrcnn_winograd_bwd_chain(const float* Mt, const float* below_z, const float* scale, const float* shift, const float* mean,
                             const float* rstd, float* partials, float* V_next, float* dM, float* dz_out, int N, int H, int W, int C,
                             int tile, void* stream);
/* weight gradient: dM = A dy A^T (adjoint of the output transform) [(oth + 2)(otw + 2)][rows][C]; dU[xi] = V[xi]^T . dM[xi] are
 * 1 x 1 weight gradients (mrcnn_conv2d_wgrad on the first `tiles` rows of each matrix); dW = G^T dU G (accumulate != 0: added to dW). */
int mrcnn_winograd_dy_g(const float* dy, float* dM, int N, int H, int W, int C, const mrcnn_wino_group* g, void* stream);
int mrcnn_winograd_dw_g(const float* dU, float* dw_hwio, int Cin, int Cout, int accumulate, int oth, int otw, void* stream);

/* KL.Conv2DTranspose(256, (2, 2), strides=2, activation="relu") of build_fpn_mask_graph (mrcnn/model.py:1084-1086) as one product
 * [N H W x Cin] . [Cin x 4 Cd] on the persistent GEMM (mrcnn_winograd_gemm's kernel) with bias, activation and the pixel-shuffle
 * store in its epilogue: K is a single filter tap deep, where the persistent form beats the one-tile-per-workgroup kernel
 * (2.15 -> 1.75 ms at 2048 ROIs).  w_gemm [Cin][(a, b, co)] (the layout mrcnn_conv2d_fwd takes for MRCNN_OUT_DECONV2);
 * out [N][2 H][2 W][Cd].  Cin % 16 == 0, Cd % 32 == 0, 4 Cd % 128 == 0, act NONE or RELU; else MRCNN_ERR_UNSUPPORTED.          */
int mrcnn_deconv2x2_gemm(const float* x, const float* w_gemm, const float* bias, float* out, int N, int H, int W, int Cin, int Cd,
                         int act, void* stream);

/* The mask head's output stage (model.py:1084-1088) in one launch: the product above on the 128 x 256 tile, and in the same
 * epilogue KL.Conv2D(num_classes, (1, 1), activation="sigmoid") over the 256 channels the tile holds for each of its output pixels:
 * mask_out[n][y][x][k] = sigmoid(b_mask[k] + sum_co up[n][y][x][co] w_mask[co][k]) -- the deconvolution's output is not read back.
 * up [N][2 H][2 W][Cd] is written as mrcnn_deconv2x2_gemm writes `out` (same bits), or not at all when NULL (inference);
 * w_mask [Cd][C], b_mask [C] or NULL, mask_out [N][2 H][2 W][C].  The sum has a fixed order (no atomics).
 * Cin % 16 == 0, Cd == 256, 1 <= C <= 16, act NONE or RELU; else MRCNN_ERR_UNSUPPORTED. */
int mrcnn_deconv2x2_mask_gemm(const float* x, const float* w_gemm, const float* bias, float* up, const float* w_mask,
                              const float* b_mask, float* mask_out, int N, int H, int W, int Cin, int Cd, int C, int act, void* stream);

/* ---- data-parallel gradient exchange over RCCL / xGMI ---------------------------------------------------------------
 * Replaces the in-graph tower aggregation of mrcnn/parallel_model.py:54-104 (weights shared between towers, gradients
 * summed implicitly by TF, scalar losses averaged :97-99): one process per GPU, each rank sums contiguous ranges
 * [start, end) of its flat float32 gradient buffer with all peers, in place, on `stream`; the division by the world size
 * happens in mrcnn_grad_prepare (grad_scale = 1 / world).  RCCL is bound at run time:
 *   mrcnn_allreduce_load(path)   dlopen + dlsym; path = the librccl the process already uses (PyTorch's), or NULL for
 *                                the default search.  MRCNN_ERR_UNSUPPORTED when no RCCL can be loaded.
 *   mrcnn_allreduce_unique_id    rank 0 creates the 128-byte rendezvous id; the caller hands it to every rank (any
 *                                side channel: a torch.distributed broadcast, a file, MPI).
 *   mrcnn_allreduce_init         ncclCommInitRank on the calling thread's current HIP device; collective over all ranks.
 *   mrcnn_allreduce_grad         algo MRCNN_ALLREDUCE_RCCL: ncclAllReduce(sum);  MRCNN_ALLREDUCE_DIRECT: reduce-scatter +
 *                                all-gather as grouped point-to-point transfers, one per xGMI link, chunks summed in rank
 *                                order by the owner (bitwise identical on every rank); needs mrcnn_allreduce_scratch()
 *                                bytes of device scratch.  Enqueues only; never synchronises.
 * Calls on one communicator must be issued in the same order on every rank (RCCL's rule).                          */
#define MRCNN_UNIQUE_ID_BYTES 128
#define MRCNN_ALLREDUCE_RCCL 0
#define MRCNN_ALLREDUCE_DIRECT 1
int mrcnn_allreduce_load(const char* librccl_path);
int mrcnn_allreduce_unique_id(void* id_128_bytes);
int mrcnn_allreduce_init(void** comm, const void* id_128_bytes, int rank, int world);
size_t mrcnn_allreduce_scratch(int world, int64_t max_range_floats, int algo);
int mrcnn_allreduce_grad(void* comm, float* grads, int64_t start, int64_t end, int algo, float* scratch,
                         size_t scratch_bytes, void* stream);
/* The direct form as data (no GPU, no RCCL needed): plan[p*4 .. p*4+3] = (send_off, send_len, recv_off, recv_len) of `rank`'s
 * transfer with peer p in phase 0 (reduce-scatter: sends index the gradient buffer, receives the scratch buffer) or phase 1
 * (all-gather: both index the gradient buffer); zeros for p == rank.  own_off / own_len: the chunk `rank` sums, slot_stride:
 * floats between scratch slots.  mrcnn_allreduce_grad walks the same function.                                            */
int mrcnn_allreduce_direct_plan(int world, int rank, int64_t start, int64_t end, int phase, int64_t* plan, int64_t* own_off,
                                int64_t* own_len, int64_t* slot_stride);
/* Test entry: the direct exchange among `world` fabricated ranks that all live on the calling GPU (grads[r], scratch[r]:
 * host arrays of device pointers); transfers become device-to-device copies after the send / receive lengths of every pair
 * have been checked against each other, the sums run the real kernel.  2 <= world <= 64.                                 */
int mrcnn_allreduce_direct_simulate(float* const* grads, float* const* scratch, size_t scratch_bytes, int world, int64_t start,
                                    int64_t end, void* stream);
int mrcnn_allreduce_destroy(void* comm);
const char* mrcnn_allreduce_last_error(void);

/* ---- source catalogue: cut-out windows, member lists, window flags, ordered NaN fill (csrc/catalog.hip) ----------------------
 * The geometry and the pixel bookkeeping of the source classifier (mrcnn/classifier.py:167-260, utils.crop_img :1211-1227) for a
 * whole catalogue at once.  All pointers are device pointers; nothing is allocated, nothing synchronises, no atomic
 * read-modify-write: every result is bitwise the same from run to run.
 *
 * S sources as six float64 columns x0, y0, xmin, xmax, ymin, ymax (centre and box), a cut-out of dx x dy pixels:
 *   window of i    (xmin, xmax, ymin, ymax)_i = (int)(x0 - dx / 2), (int)(x0 + dx / 2), (int)(y0 - dy / 2), (int)(y0 + dy / 2): float64
 *                  arithmetic, truncation toward zero.  Supported coordinates: every x0 -/+ dx / 2 and y0 -/+ dy / 2 finite and of
 *                  magnitude below 2^31 (the CALLER checks this: the conversion is undefined outside it).
 *   members of i   every j != i, ascending, with x0_j > xmin_i && x0_j < xmax_i && y0_j > ymin_i && y0_j < ymax_i;
 *   cut flag       xmin_j <= xmin_i || xmax_j >= xmax_i || ymin_j <= ymin_i || ymax_j >= ymax_i.
 * mrcnn_catalog_count writes windows [S][4] int32 and counts [S] int32; the caller scans the counts into offsets [S + 1] int64
 * (exclusive, offsets[S] = total) and mrcnn_catalog_fill writes members [total] int32 and cut [total] uint8, row i at offsets[i].
 * A row is written in ascending j by ballot + prefix popcount of the wavefront that owns it.  S <= 0, dx or dy <= 0 or not
 * finite, a missing pointer: MRCNN_ERR_ARG.  S above the cap (2^18, "catalog_max_sources" of mrcnn_tuning_set) or total above
 * 2^31 - 1: MRCNN_ERR_UNSUPPORTED -- nothing launched (use the host statement).  mrcnn_catalog_check: the status
 * mrcnn_catalog_count would return for S (launches nothing).                                                                      */
#define MRCNN_CATALOG_MAX_SOURCES (1 << 18)
int mrcnn_catalog_check(int S);
int mrcnn_catalog_count(const double* x0, const double* y0, int S, double dx, double dy, int* windows, int* counts, void* stream);
int mrcnn_catalog_fill(const double* x0, const double* y0, const double* xmin, const double* xmax, const double* ymin,
                       const double* ymax, int S, double dx, double dy, const long long* offsets, long long total, int* members,
                       unsigned char* cut, void* stream);
/* T windows (xmin, xmax, ymin, ymax) of a resident float32 plane [NY][NX], clipped to the plane at the far edges as NumPy slicing
 * clips: flags [T][2] int32 = (pixels that are finite, pixels that are NaN).  A window with a negative corner or without a pixel
 * gets (0, 0).  One launch, one workgroup per window.  T <= 0, NY or NX <= 0: MRCNN_ERR_ARG.                                     */
int mrcnn_catalog_window_flags(const float* plane, int NY, int NX, const int* windows, int T, int* flags, void* stream);
/* crop_img's in-place NaN fill for K windows IN TABLE ORDER: for k = 0 .. K - 1 the non-NaN minimum of window k of the plane AS
 * IT IS THEN (earlier fills included) goes into the window's NaN pixels; a window without a finite pixel at its turn (or with a
 * negative corner, or empty) is left as it is.  alive [K] int32 = 1 where the window had a finite pixel at its turn, else 0.
 * form 0: one launch of one workgroup that walks the table with a workgroup barrier between windows; form 1: one launch of one
 * workgroup per window, in stream order.  Both write the same plane.  K == 0 launches nothing; K < 0, NY or NX <= 0, another
 * form: MRCNN_ERR_ARG.                                                                                                          */
int mrcnn_catalog_nan_fill(float* plane, int NY, int NX, const int* windows, int K, int form, int* alive, void* stream);

/* Process-wide tuning values, read by the host side of later launches.  Keys: "wgrad_lds_pad" (0..32768 bytes of extra
 * LDS per workgroup of the large weight-gradient kernel: 8192 caps it at four workgroups per CU so that kernels of another
 * stream find a free slot on every CU); "h16_phase" (0 / 1); "h16_slab" (-1 = MRCNN_H16_SLAB decides, default off; 0 / 1: the slab form of the phased 16-bit kernel off /
 * on -- tests and A/B timing); "sk16" (0 / 1: the 16 x 16-tile single-launch kernel for layers of a few hundred pixels may be
 * picked -- the engine sets it while it issues the inference graph); "proposal_skip_zero" (tests only, fault injection: 1 suppresses
 * the counter reset of mrcnn_proposal_fwd's multi-workgroup selection); "outline_lds_segs" (0..1536, default 1536: mrcnn_outline_emit
 * ranks the segments of a source in LDS up to this many and in its global workspace above; 0 = always the global form -- tests);
 * "catalog_max_sources" (1..2^18, default 2^18: mrcnn_catalog_count / _fill refuse a longer catalogue -- tests reach the refusal
 * at a size whose host statement is cheap).  MRCNN_ERR_UNSUPPORTED for an unknown key.                                                                          */
int mrcnn_tuning_set(const char* key, long long value);

const char* mrcnn_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MRCNN_HIP_H */
