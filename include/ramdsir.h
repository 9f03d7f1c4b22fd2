/* ramdsir.h -- C ABI of libramdsir_hip.so: the MI355X (gfx950) hot path of RAM-DSIR training.
 *
 * The reference (zzzqzhou/RAM-DSIR) is pure Python on top of PyTorch; it has no FFI.  The boundary a
 * maintainer binds is therefore the set of ATen/cuDNN operators its nn.Modules dispatch to
 *  plus the numpy RAM trio.  Every entry point below names the reference site(s) it
 * replaces (paths relative to the reference checkout).  INTEGRATION.md shows the ctypes stub that
 * plugs them under code/networks/unet.py and code/dataset/fundus.py.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in _host; the library never allocates
 *     tensors (the caller owns all memory; workspaces are passed in);
 *   - activations/gradients are NHWC, element type `dtype` (RD_F32 or RD_BF16); parameters, BN
 *     statistics, losses and Adam state are always fp32, OIHW like torch;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), returns 0 or a
 *     hipError_t value, and is hipGraph-capturable (no allocation, no sync inside);
 *   - a "group" is a set of consecutive images that share BatchNorm statistics: the two encoder /
 *     seg-decoder passes of one step (img, img_freq) are two groups of one launch; the per-domain
 *     slices of the restoration decoder are one group per domain (DomainSpecificBatchNorm2d).
 */
#ifndef RAMDSIR_H
#define RAMDSIR_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RD_F32 0
#define RD_BF16 1
#define RD_MAX_GROUPS_C 16
/* BatchNorm sums are accumulated with atomics; to keep thousands of workgroups off the same few addresses
 * every statistics buffer has RD_STAT_SLOTS copies, [G][RD_STAT_SLOTS][C][2]; a workgroup adds into slot
 * (its tile index mod RD_STAT_SLOTS) and the finalize kernels sum the slots.
 * Numerics (ATen's batch_norm uses a mean-then-deviation / Welford reduction, never E[x^2]-E[x]^2 in fp32): a workgroup
 * sums its tile in fp32, but (a) the forward sums are those of the conv result WITHOUT its bias (the bias -- the one
 * structural source of |mean| >> sigma -- is added back to the mean by rd_bn_finalize_fwd), and (b) everything across
 * workgroups -- the slot atomics, the slot sum, var = E[x^2]-E[x]^2 and sum g*z - mean * sum g -- is fp64. */
#define RD_STAT_SLOTS 64
/* A launch may be told to spread its sums over the FIRST n of the RD_STAT_SLOTS copies only (rd_conv_t.stat_slots, the stat_slots
 * arguments of rd_up_stats / rd_pool_bwd; 0 = all): the persistent kernels of the training step add once per workgroup, not once per
 * tile, so 8 copies keep them apart -- and a consumer that derives the BatchNorm coefficients itself (rd_src_t.fin below) then reads 8
 * copies per channel instead of 64.  The layout [G][RD_STAT_SLOTS][C][2] does not change; unused copies stay zero, and the explicit
 * finalize launches sum all of them. */
#define RD_STAT_SLOTS_FOLD 8

/* rd_src_t.fin_flags */
enum {
    RD_FIN_OWNER = 1   /* this launch also does what happens once per BatchNorm call: saved mean / invstd, running statistics and
                          num_batches_tracked (forward); dgamma / dbeta (backward) */
};

/* how a conv reads one of its (virtual) input tensors -- the producer's BatchNorm + activation
 * (+ max-pool / bilinear x2) are applied while the tile is staged into LDS ("normalise on read") */
enum {
    RD_SRC_RAW = 0,    /* v = x                                             (image, dlogits)             */
    RD_SRC_AFF = 1,    /* v = x*scale+shift                                 (ConvD.bn1: no activation)   */
    RD_SRC_AFFACT = 2, /* v = act(x*scale+shift)                            (BN+ReLU, unet.py:64-70)     */
    RD_SRC_POOL = 3,   /* v = max2x2(act(x*scale+shift)), stored at 2H x 2W (unet.py:56 MaxPool2d(2))    */
    RD_SRC_UP = 4,     /* v = act(bilerp2x(x)*scale+shift), stored at H/2 x W/2 (unet.py:84-86, 1x1 conv
                          commuted below the upsample: conv1x1(up(a)) == up(conv1x1(a)))                 */
    RD_SRC_BNBWD = 5   /* v = P*g + Q*z + R  (BatchNorm backward folded into the read; ptr=g, ptr2=z)    */
};

typedef struct {
    const void* ptr;     /* NHWC tensor [N][Hs][Ws][C]                                   */
    const void* ptr2;    /* RD_SRC_BNBWD: the raw forward tensor z                        */
    const float* scale;  /* [G][C]  (BNBWD: P)                                            */
    const float* shift;  /* [G][C]  (BNBWD: R)                                            */
    const float* q;      /* [G][C]  BNBWD only                                            */
    void* out;           /* NULL, or a tensor of ptr's shape: the launch also WRITES the values it stages from this source --
                          * act(scale x + shift), or dz = P g + Q z + R -- there (storage dtype), every pixel once.  Honoured by
                          * the launches for which rd_conv_honours_src_out() returns 1, ignored by all others.  The weight
                          * gradient of the same layer then reads stored operands (RD_SRC_RAW) instead of repeating the
                          * transform in its loader, which is what bounds it                          */
    int32_t mode;
    int32_t C;
    float slope;         /* 0 = ReLU, 0.01 = LeakyReLU (unet.py:47-50)                    */
    int32_t n_off;       /* image offset into ptr (rec decoder reads images 8.. of x5)    */
    int32_t g_fixed;     /* >=0: use this group row of scale/shift instead of the image's */
    int32_t fin_flags;   /* RD_FIN_* when fin != NULL */
    const void* fin;     /* NULL, or the rd_bn_fwd_t (modes AFF / AFFACT / POOL / UP: it produces scale / shift) resp. rd_bn_bwd_t
                          * (RD_SRC_BNBWD: P / Q / R) that describes the BatchNorm finalize of this source (a HOST struct like this
                          * one, read when the entry point is called): the launch runs it as its own prologue -- every workgroup derives
                          * the coefficient vectors from the statistic slots and writes them where the descriptor says, which is
                          * where scale / shift / q of this source must point -- instead of an rd_bn_finalize_* launch in front of it
                          * (training mode, BatchNorm only, at most 8 groups, one such source per launch).  Launches that read the same
                          * coefficients LATER in stream order need no fin; launches that may run CONCURRENTLY (another stream) each
                          * carry the fin, exactly one of them with RD_FIN_OWNER.  Honoured by rd_conv, rd_wgrad (dz only) and
                          * rd_conv_bwd_fused (the gradient descriptor's source); -3 for a fin the launch cannot take */
} rd_src_t;

/* where a dgrad launch puts the gradient w.r.t. its (virtual) input, i.e. w.r.t. the producer's
 * BN output: masks by the activation, scatters through max-pool, and accumulates the two
 * per-channel BN-backward sums (sum g, sum g*z) */
enum { RD_DST_PLAIN = 0, RD_DST_POOL = 1, RD_DST_UPY = 2, RD_DST_NONE = 3 };

typedef struct {
    void* g;             /* gradient tensor to write, NHWC [*][Hd][Wd][Cd]                          */
    const void* z;       /* producer's raw tensor (PLAIN/POOL: same dims as g; UPY: t_lo, half res) */
    const float* scale;  /* producer BN scale/shift [G][Cd] (mask needs the sign of the BN output)  */
    const float* shift;
    double* bstats;      /* [G][RD_STAT_SLOTS][Cd][2] += (sum g, sum g*z)  or NULL                  */
    int32_t kind;
    int32_t act;         /* 1: an activation follows the producer BN                                */
    int32_t accumulate;  /* 1: g += (skip connection / second consumer)                             */
    int32_t Cd;
    float slope;
    int32_t n_off;       /* image offset into g / z                                                 */
    int32_t g_fixed;     /* >=0: producer group row                                                 */
    int32_t pad_;
} rd_dst_t;

/* rd_conv: replaces F.conv2d forward (unet.py:37-43,81-88,124-131,281,307) and, with flipped /
 * transposed packed weights, cudnn's dgrad; fused: bias add, BN batch statistics of the output
 * (nn.BatchNorm2d train mode), and on the read side the producer's BN+act+pool/upsample+concat. */
typedef struct {
    rd_src_t src[2];     /* 2 sources = torch.cat([prev, y], 1) (unet.py:110), never materialised */
    int32_t nsrc;
    int32_t taps;        /* 9 (3x3, pad 1) or 1 (1x1) */
    const void* w;       /* packed weights [CinPad/CK][taps][CoutPad][CK] (CK = 64 B of channels), dtype, zero padded */
    const float* bias;   /* [Cout] or NULL */
    int32_t CinPad, CoutPad;
    int32_t N, H, W, Cin, Cout;
    int32_t G;
    int32_t gstart[RD_MAX_GROUPS_C + 1];
    int32_t emode;       /* 0 forward: write out (+stats); 1 gradient: write through dst[] */
    void* out;           /* forward: NHWC [N][H][W][Cout] */
    double* stats;       /* forward: [G][RD_STAT_SLOTS][Cout][2] += (sum, sum of squares) of the result BEFORE the bias, or NULL */
    rd_dst_t dst[2];     /* gradient: channels [0,c_split) -> dst[0], [c_split,Cout) -> dst[1] */
    int32_t c_split;
    int32_t cu_limit;    /* >0: compute-unit budget of the launch where the kernel is persistent (the small-channel kernel, the
                          * warp-specialised 64-wide kernel): a conv of a side lane leaves the rest of the GPU to the main
                          * chain; 0: the whole device */
    int32_t w_tap_rows;  /* rows per tap of the packed array `w` points into when that is MORE than CoutPad: a launch over a 32-row
                          * block of a wider pack (w = pack + first_row * CK elements; honoured by the small-channel kernels, which is
                          * where such launches go); 0: CoutPad */
    int32_t stat_slots;  /* >0: `stats` and dst[].bstats are spread over the first stat_slots copies only (RD_STAT_SLOTS_FOLD); 0: all.
                            0..RD_STAT_SLOTS (else -2), and never MORE than the nslots of the consumer that finalizes these sums */
} rd_conv_t;

int rd_conv(const rd_conv_t* p, int dtype, void* stream);
/* 1 if rd_conv(p, dtype) will write the src[i].out tensors it is given (a pure function of the descriptor and the device) */
int rd_conv_honours_src_out(const rd_conv_t* p, int dtype);

/* rd_wgrad: replaces cudnn's wgrad for the same convs.  partial is a caller workspace of
 * rd_wgrad_workspace() bytes; the result is accumulated (beta=1) or stored (beta=0) into dW, fp32
 * OIHW [Cout][Cin][kh][kw]. */
typedef struct {
    rd_src_t a[2];       /* the conv's forward input, described exactly as for rd_conv */
    int32_t na;
    int32_t taps;
    rd_src_t dz;         /* gradient w.r.t. the conv output (RD_SRC_BNBWD or RD_SRC_RAW) */
    int32_t N, H, W, Cin, Cout;
    int32_t G;
    int32_t gstart[RD_MAX_GROUPS_C + 1];
    float* partial;
    float* dW;
    float beta;
    int32_t cu_limit;    /* >0: workgroup budget of the (persistent) launch in compute units -- a launch that runs on a side
                          * stream beside the dgrad chain leaves the rest of the GPU to it; 0: the whole device.  Enters
                          * rd_wgrad_workspace() (one partial per workgroup).  The 16-channel layers ignore it. */
} rd_wgrad_t;

int64_t rd_wgrad_workspace(const rd_wgrad_t* p, int dtype);
int rd_wgrad(const rd_wgrad_t* p, int dtype, void* stream);
/* The split reduction that ends rd_wgrad and rd_conv_bwd_fused_reduce, on its own: dW[n][c][tap] = (beta ? beta * dW : 0) +
 * the sum over s < nsplit of partial[s][tap][n < CoutPadW][c < CinPadW], fp32, in a fixed order that does not depend on the load
 * width the launch picks.  CinPadW is a multiple of 16 (else -1).  16-byte loads are used when Cin % 4 == 0, `partial` is
 * 16-byte aligned and the launch has 8 split lanes per output (fewer than 128 splits, or more than 16384 outputs); in every other
 * case, a misaligned `partial` included, the 4-byte form runs without notice -- same bits.  dW is read only when beta != 0. */
int rd_wgrad_reduce(const float* partial, float* dW, int nsplit, int taps, int Cout, int Cin, int CoutPadW, int CinPadW, float beta,
                    void* stream);

/* Backward of a small-channel 3x3 conv (<= 32 channels in and out, bf16, plain per-pixel sources and destinations: every
 * 400x400 / 200x200 layer of the U-Net) in ONE launch: cudnn's dgrad AND wgrad behind the same nn.Conv2d
 * (unet.py:37-43,81-88,124-131,281,307).  Both halves are HBM-bound and read the same tensors -- g, z and the producer's raw
 * tensor; fused they are read once, and the weight-gradient MFMAs run on matrix pipes the dgrad leaves idle.
 * `dgrad` is the rd_conv descriptor of the gradient launch (emode 1), `wgrad` the rd_wgrad descriptor of the same conv;
 * rd_conv_bwd_fused_ok() says whether the pair qualifies (else use rd_conv + rd_wgrad).  rd_conv_bwd_fused writes the input
 * gradient exactly as rd_conv would and one block of weight-gradient sums per workgroup into wgrad->partial
 * (rd_conv_bwd_fused_workspace() bytes; wgrad->cu_limit is ignored, dgrad->cu_limit sizes the launch);
 * rd_conv_bwd_fused_reduce then sums them into wgrad->dW in a fixed order (a separate call so that a caller can run it
 * on another stream than the dgrad chain). */
int rd_conv_bwd_fused_ok(const rd_conv_t* dgrad, const rd_wgrad_t* wgrad, int dtype);
int64_t rd_conv_bwd_fused_workspace(const rd_conv_t* dgrad, const rd_wgrad_t* wgrad, int dtype);
int rd_conv_bwd_fused(const rd_conv_t* dgrad, const rd_wgrad_t* wgrad, int dtype, void* stream);
int rd_conv_bwd_fused_reduce(const rd_conv_t* dgrad, const rd_wgrad_t* wgrad, int dtype, void* stream);

/* Routing queries: what rd_conv / rd_wgrad / rd_conv_bwd_fused(_reduce) WOULD launch for a descriptor, from the same host function
 * the entry points launch from.  Pure host arithmetic on the descriptor and the device's compute-unit count: nothing is launched and
 * no data pointer is dereferenced (only pointer VALUES are looked at, for the alignment rules; rd_src_t.fin is not read).
 * `kernel` is the instantiation as spelled in the source (static storage), e.g. "conv_ws_kernel<1, 1, false, true>"; iarg holds the
 * integer kernel arguments the dispatcher computes, in the kernel's argument order, 0 beyond them:
 *   conv kernels {tiles_total | arg | tiles_per_wg};  weight-gradient kernels {CoutPadW, CinPadW, total_tiles};
 *   the split reduction {nsplit, taps, Cout, Cin, CoutPadW, CinPadW};  the fused backward {tiles_per_wg}. */
typedef struct {
    const char* kernel;
    int32_t grid[3], block, lds;
    int32_t iarg[6];
    int32_t stores_sources;  /* rd_conv only: the launch honours rd_src_t.out, i.e. writes the out tensors it is given (this is
                              * what rd_conv_honours_src_out returns; the storing instantiation is chosen when a source asks) */
} rd_route_t;
/* rd_conv's own return code for the descriptor (-1 / -2); 0: *out is what rd_conv would launch */
int rd_conv_route(const rd_conv_t* p, int dtype, rd_route_t* out);
/* the number of launches (the weight-gradient kernel, then its split reduction), or rd_wgrad's return code (< 0) */
int rd_wgrad_route(const rd_wgrad_t* p, int dtype, rd_route_t out[2]);
/* 2: out[0] is rd_conv_bwd_fused's launch, out[1] rd_conv_bwd_fused_reduce's; -1 when the pair does not qualify */
int rd_conv_bwd_fused_route(const rd_conv_t* dgrad, const rd_wgrad_t* wgrad, int dtype, rd_route_t out[2]);

/* rd_pack_weights: OIHW fp32 master weights -> the packed operand rd_conv reads.
 * K-chunk-major, CK = 32 (bf16) / 16 (fp32) input channels = the 64 bytes one K step of rd_conv consumes:
 * transpose=0: forward  [CinPad/CK][tap][CoutPad][CK]  (tap = kh*3+kw)
 * transpose=1: dgrad    [CoutPad'/CK][tap'][CinPad'][CK] with tap' = 8-tap (180-degree flip), i.e. the conv
 *              that maps dz (Cout channels) to da (Cin channels). */
int rd_pack_weights(const float* w_oihw, void* packed, int Cout, int Cin, int taps, int transpose,
                    int dtype, void* stream);
int64_t rd_packed_elems(int Cout, int Cin, int taps, int transpose, int dtype);

/* every conv of the network in ONE launch (run after each optimizer step): entry e reads the OIHW
 * weight at params+src_off and owns packed elements [start, next start) at packed+dst_off. */
typedef struct {
    int64_t src_off;     /* floats into the parameter arena */
    int64_t dst_off;     /* elements into the packed arena (== start) */
    int64_t start;
    int32_t Cout, Cin, taps, transpose, RowPad, ColPad;
} rd_pack_entry_t;
int rd_pack_weights_batched(const float* params, void* packed, const rd_pack_entry_t* table_dev, int n_entries,
                            int64_t total, int dtype, void* stream);


/* ------------------------------------------------------------------------------------------------
 * BatchNorm2d (train: batch statistics; eval: running statistics) split into "finalize" launches
 * around the convs.  nn.BatchNorm2d / DomainSpecificBatchNorm2d: code/networks/unet.py:17-28,
 * code/networks/dsbn.py:24-27.  Per-group parameter pointers: the two passes of the encoder share one
 * BN (same pointers in both groups -> running stats updated twice, in order); DSBN gives each domain
 * group its own bns[d]. */
typedef struct {
    const double* stats;  /* [G][RD_STAT_SLOTS][C][2] sum, sum of squares of (conv output - conv_bias) */
    const float* conv_bias; /* [C] bias of the producing conv (its sums exclude it) or NULL            */
    float* scale;         /* [G][C] out: gamma*invstd          */
    float* shift;         /* [G][C] out: beta - mean*scale     */
    float* mean;          /* [G][C] out (saved for backward)   */
    float* invstd;        /* [G][C] out                        */
    const float* gamma[RD_MAX_GROUPS_C];
    const float* beta[RD_MAX_GROUPS_C];
    float* running_mean[RD_MAX_GROUPS_C];
    float* running_var[RD_MAX_GROUPS_C];
    int64_t* num_batches_tracked[RD_MAX_GROUPS_C];
    float count[RD_MAX_GROUPS_C];   /* elements per channel in the group: N_g*H*W */
    int32_t C, G;
    float eps, momentum;
    int32_t training;     /* 0: eval -- scale/shift from the running statistics, nothing updated */
    int32_t nslots;       /* rd_src_t.fin only: statistic copies the producers used (0 = all); a multiple of 8 up to RD_STAT_SLOTS (else -3),
                             >= every producer's stat_slots.  rd_bn_finalize_fwd sums all RD_STAT_SLOTS copies */
} rd_bn_fwd_t;
int rd_bn_finalize_fwd(const rd_bn_fwd_t* p, void* stream);

/* BatchNorm backward, second half: from (sum g, sum g*z) produce the per-channel coefficients
 * dz = P*g + Q*z + R that the next dgrad / wgrad fold into their reads, and accumulate dgamma, dbeta. */
typedef struct {
    const double* bstats; /* [G][RD_STAT_SLOTS][C][2] */
    const float* mean;    /* [G][C] */
    const float* invstd;  /* [G][C] */
    const float* gamma[RD_MAX_GROUPS_C];
    float* dgamma[RD_MAX_GROUPS_C];   /* += */
    float* dbeta[RD_MAX_GROUPS_C];    /* += */
    float* P; float* Q; float* R;     /* [G][C] out */
    float count[RD_MAX_GROUPS_C];
    int32_t C, G;
    /* rd_gn_finalize_bwd only (NULL / ignored for BatchNorm, where the bias of a conv in front of the normalisation has an identically
     * zero gradient): GroupNorm pools the mean over the channels, so the conv bias has a gradient, sum over the pixels of dz =
     * P * sum g + Q * sum z + R * count, formed here from the forward sums */
    const double* fstats;   /* [G][RD_STAT_SLOTS][C][2] the forward statistics of this site */
    const float* conv_bias; /* [C] as in rd_bn_fwd_t (NULL: the forward sums already contain it) */
    float* dbias;           /* [C] += */
    int32_t nslots;         /* rd_src_t.fin only, as in rd_bn_fwd_t */
    int32_t pad_;
} rd_bn_bwd_t;
int rd_bn_finalize_bwd(const rd_bn_bwd_t* p, void* stream);

/* nn.GroupNorm(1, planes) (code/networks/unet.py:20-21, normalization(norm='gn')): every image is its own group (gstart = 0, 1, .., N;
 * N <= RD_MAX_GROUPS_C), mean / variance pooled over (C, H, W) of the image; the descriptors and outputs are those of the BatchNorm
 * finalize launches above (running-statistics pointers are ignored, `training` is irrelevant: the statistics are always the input's),
 * gamma / beta / dgamma / dbeta of group 0 are the layer's (shared by all images; dgamma / dbeta += in image order).
 * nn.InstanceNorm2d (unet.py:22-23, norm='in') needs no entry point of its own: rd_bn_finalize_fwd / _bwd with one group per image,
 * gamma -> ones, beta -> zeros, running_* = num_batches_tracked = dgamma = dbeta = NULL, training = 1. */
int rd_gn_finalize_fwd(const rd_bn_fwd_t* p, void* stream);
int rd_gn_finalize_bwd(const rd_bn_bwd_t* p, void* stream);

/* statistics of y = bilinear_x2(t) (nn.Upsample(scale_factor=2, 'bilinear', align_corners=False),
 * unet.py:84): stats[G][slot][C][2] += (sum y, sum y^2) (each thread sums deviations from the first value it sees and
 * converts to plain sums in fp64).  t: NHWC [N][h][w][C].  y_out == NULL: y is not
 * materialised (its readers interpolate t on the fly, RD_SRC_UP / RD_DST_UPY); otherwise y is also written to
 * y_out NHWC [N][2h][2w][C] in `dtype` and the statistics are those of the STORED (rounded) values, so that
 * plain RD_SRC_AFFACT / RD_DST_PLAIN readers normalise exactly what was measured. */
int rd_up_stats(const void* t, double* stats, void* y_out, int N, int h, int w, int C, int G, const int32_t* gstart_host,
                int dtype, int stat_slots /* 0: all copies */, void* stream);

/* statistics of a plain NHWC tensor x [N][H][W][C]: stats[G][slot][C][2] += (sum x, sum x^2) -- the standalone
 * nn.BatchNorm2d / DomainSpecificBatchNorm2d.forward (code/networks/dsbn.py:24-27), where no conv produced x. */
int rd_bn_stats(const void* x, double* stats, int N, int H, int W, int C, int G, const int32_t* gstart_host, int dtype,
                void* stream);

/* backward of y = up2(t) followed by BN: dt = up2^T( P*g + Q*up2(t) + R ), g: NHWC [N][2h][2w][C],
 * dt/t: NHWC [N][h][w][C]. */
int rd_up_bwd(const void* g, const void* t, void* dt, const float* P, const float* Q, const float* R, int N, int h,
              int w, int C, int G, const int32_t* gstart_host, int dtype, const rd_bn_bwd_t* fin /* NULL, or as rd_src_t.fin: produces P, Q, R */,
              int fin_flags, void* stream);

/* nn.MaxPool2d(2) at the head of ConvD levels 2-5 (unet.py:45,56), materialised: out[N][Ho][Wo][C] = max over the 2x2 window of
 * act(z*scale+shift) (scale == NULL: identity coefficients; slope 1: no activation), z: NHWC [N][2Ho][2Wo][C].  The conv behind
 * it then reads `out` as a plain tensor in forward, dgrad and wgrad. */
int rd_pool_fwd(const void* z, const float* scale, const float* shift, float slope, void* out, int N, int Ho, int Wo, int C, int G,
                const int32_t* gstart_host, int dtype, const rd_bn_fwd_t* fin /* NULL, or as rd_src_t.fin: produces scale, shift */, int fin_flags,
                void* stream);
/* its backward: g[N][2Ho][2Wo][C] (+)= gp scattered to the FIRST maximum of each window (ATen's tie rule), times the
 * activation derivative there when act != 0; bstats (or NULL) += (sum g_new, sum g_new*z) of the scattered values. */
int rd_pool_bwd(const void* gp, const void* z, const float* scale, const float* shift, float slope, int act, void* g, int accumulate,
                double* bstats, int N, int Ho, int Wo, int C, int G, const int32_t* gstart_host, int dtype,
                int stat_slots /* 0: all copies */, void* stream);

/* Elementwise materialisation  out = act( a*x + b*x2 + c ; slope )  over NHWC [N][H][W][C] with per-(group, channel)
 * coefficients a, b, c [G][C] (b, x2 may be NULL; slope 1 = no activation):
 *   forward  : a = BN scale, c = BN shift          -> the activated tensor relu(bn(z)) (unet.py:59-70), stored once
 *   backward : a = P, x2 = z, b = Q, c = R         -> dz, the gradient w.r.t. the conv output behind the BN
 * Used for the >= 64-channel layers, whose conv kernels are instruction-bound in the loader: their many readers
 * (one workgroup per 64 output channels, forward + dgrad + wgrad) then fetch the stored tensor with RD_SRC_RAW
 * instead of each redoing the BN/ReLU arithmetic; the tensors are small (<= 20 MB) at those depths. */
int rd_bn_apply(const void* x, const void* x2, void* out, const float* a, const float* b, const float* c, float slope,
                int N, int H, int W, int C, int G, const int32_t* gstart_host, int dtype, void* stream);

/* layout / materialisation at the module boundary (torch NCHW fp32 <-> NHWC dtype) */
/* cstride: elements between pixels of y (0 or C: dense; larger: zero-initialised pad channels are left untouched) */
int rd_nchw_to_nhwc(const float* x_nchw, void* y_nhwc, int N, int C, int H, int W, int cstride, int dtype, void* stream);
/* y_nchw = act(z*scale+shift)  (act: 0 none, 1 activation with `slope`); scale==NULL -> identity */
int rd_nhwc_to_nchw(const void* z_nhwc, float* y_nchw, const float* scale, const float* shift, int act, float slope,
                    int N, int C, int H, int W, int G, const int32_t* gstart_host, int dtype, void* stream);
/* gradient entering a module from torch: g_nhwc (+)= mask(dy_nchw), bstats += (sum g, sum g*z) */
int rd_grad_in(const float* dy_nchw, const void* z_nhwc, void* g_nhwc, const float* scale, const float* shift,
               double* bstats, int act, float slope, int accumulate, int N, int C, int H, int W, int G,
               const int32_t* gstart_host, int dtype, void* stream);
/* column sums of an NHWC tensor: out[c] (+)= sum over pixels (bias gradient of the two out1 convs) */
int rd_colsum(const void* x_nhwc, float* out, float* partial_ws /* >= 8192 floats */, int64_t npix, int C, int cstride /* 0: C */,
              float beta, int dtype, void* stream);


/* ------------------------------------------------------------------------------------------------
 * Fused segmentation + consistency losses, forward and backward in two passes over the logits.
 * Fundus  (code/train.py:246-259,283): p=sigmoid(l); BCELoss + dice_loss (utils/losses.py:8-16) for
 *          both passes + 0.5*KD|MSE(p2,p1) (train.py:85-88).  mask: NCHW fp32 [B][K][H][W].
 * Prostate (train.py:412-427,451): p=softmax(l); CrossEntropyLoss + dice_loss_multi(ignore_index=0)
 *          (utils/losses.py:18-33) + 0.5*KD|MSE.  target: int64 [B][H][W].
 * logits/dlogits: NHWC [2B][H][W][K] (pass 0 = images [0,B), pass 1 = [B,2B)).
 * losses_out[8] = {seg1, dice1, seg2, dice2, consistency, seg1+seg2+dice1+dice2+w*consistency, 0, 0}. */
typedef struct {
    const void* logits;
    const void* target;     /* fundus: const float* mask NCHW; prostate: const int64_t* */
    void* dlogits;
    float* partial;         /* workspace: rd_seg_loss_workspace() bytes */
    float* losses_out;      /* [8] device */
    int32_t B, H, W, K;
    int32_t kind;           /* 0 fundus (sigmoid/BCE/dice), 1 prostate (softmax/CE/dice_multi) */
    int32_t consistency;    /* 0 none, 1 kd, 2 mse */
    float cons_weight;      /* 0.5 (train.py:283) */
    int32_t dlogits_cstride; /* elements between pixels of dlogits (0 or K: dense); the pad is never written */
} rd_seg_loss_t;
int64_t rd_seg_loss_workspace(const rd_seg_loss_t* p);
int rd_seg_loss(const rd_seg_loss_t* p, int dtype, void* stream);

/* Restoration loss (train.py:265-276): per domain group d, MSELoss(tanh(rec_logits[d]), img[d]);
 * loss += lambda_rec * mse_d.  rec_logits / target / dlogits: NHWC [B][H][W][C].  mse_out[G] device.  H*W*C < 2^24 (-1 otherwise). */
int rd_rec_loss(const void* rec_logits, const void* target, void* dlogits, float* mse_out, float* partial_ws,
                int B, int H, int W, int C, int target_cstride /* 0: C */, int dlogits_cstride /* 0: C */, int G,
                const int32_t* gstart_host, float lambda_rec, int dtype, void* stream);
int64_t rd_rec_loss_workspace(int B, int H, int W, int C);

/* ------------------------------------------------------------------------------------------------
 * Adam over the flat parameter arena (torch.optim.Adam, betas (0.9,0.999), eps 1e-8, no weight decay;
 * code/train.py:573-576) with the reference's 3 param groups (encoder at lr/2) and poly LR
 * lr*(1-iter/total)^0.9 written after the step (train.py:289-293).  `iter` is a device counter that
 * the call increments, so a captured hipGraph replays the schedule without host involvement.
 * hyper_out[4] = {lr used for group 1/2, bias_correction1, bias_correction2, iter used}. */
typedef struct {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    int64_t n;              /* total elements */
    int64_t n_half_lr;      /* the first n_half_lr elements (encoder) use lr/2 */
    int32_t* iter;          /* device, incremented */
    float* hyper_out;       /* device [4] */
    float base_lr;
    int32_t total_iters;
    float beta1, beta2, eps;
    int32_t pad_;
} rd_adam_t;
int rd_adam_step(const rd_adam_t* p, void* stream);

/* optimizer.zero_grad() (code/train.py:285,454) and the per-step reset of the BatchNorm sum buffers (stats / bstats arenas,
 * which the conv epilogues add into): n device ranges [ptrs_host[i], +bytes_host[i]) := 0, asynchronously on `stream`.
 * The two arrays are HOST arrays (read before the call returns).  Up to 8 ranges with 16-byte-aligned starts are cleared by ONE
 * kernel launch; otherwise one hipMemsetAsync per range. */
int rd_zero(void* const* ptrs_host, const int64_t* bytes_host, int n, void* stream);


/* ------------------------------------------------------------------------------------------------
 * Random Amplitude Mixup for a whole batch on the GPU.  Replaces extract_amp_spectrum /
 * low_freq_mutate_np / source_to_target_freq (code/dataset/fundus.py:13-61 == prostate.py:10-62) and
 * the call sites fundus.py:211-225 (clip [0,255], /127.5-1) and prostate.py:186-188 (clip [-1,1]).
 * src/trg: NHWC [B][H][W][3] (HWC like the PIL / .npy arrays the reference feeds the trio), fp32 or -- src_u8 != 0 --
 * uint8 (decoded PNG pixels: 1 byte per value to upload and to read); lam[B]: the per-sample ratio the reference draws
 * with random.randint(1,10)/10 (fundus.py:35); b = floor(0.1*min(H,W)) (fundus.py:26).
 * out_img = f(src), out_freq = f(clip(RAM(src,trg,lam), clip_lo, clip_hi)) with f(v) = v/div + offset when div != 0
 * (bit for bit the reference's `img /= 127.5; img -= 1.0`, fundus.py:217-218) else v*scale + offset; both NHWC `dtype`
 * [B][H][W][out_cstride] -- normally the two halves of the network input batch.
 * trg_amp != NULL: the partner is given as its amplitude spectrum [B][3][H][W] (what extract_amp_spectrum returns) instead
 * of as an image -- source_to_target_freq(src_img, amp_trg) of fundus.py:41; trg is then ignored.
 * tw_w / tw_h: (cos, -sin)(2*pi*k/N) tables of W / H entries.  H and W must factor into 2, 3 and 5 and be <= 1024; 256,
 * 384, 400 and 512 run compile-time radix plans. */
typedef struct {
    const void* src; const void* trg; const float* lam;
    void* out_img; void* out_freq;
    void* workspace;            /* rd_ram_workspace() bytes */
    const float* tw_w; const float* tw_h;
    int32_t B, H, W, C, b;
    float clip_lo, clip_hi, scale, offset;
    int32_t out_cstride;        /* elements between pixels of out_img / out_freq (0 or 3: dense; one 16-byte slot (8 bf16 /
                                 * 4 fp32): the first conv reads whole channel vectors, channels 3.. are written as zeros) */
    int32_t src_u8;             /* src / trg are uint8 */
    float div;
    int32_t pad_;
    const float* trg_amp;
    const void* dft_tables;     /* rd_ram_dft_tables() output for this (H, W, b), or NULL: see below */
} rd_ram_t;
int64_t rd_ram_workspace(int B, int H, int W, int b);
int rd_ram_mix(const rd_ram_t* p, int dtype, void* stream);
/* The mix only needs the bins |kx|, |ky| <= b of each spectrum (41 of 201 row bins at 400 x 400): with coefficient tables for the
 * geometry -- rd_ram_dft_tables_bytes() bytes of device memory filled ONCE by rd_ram_dft_tables (fp64 sincos, three bf16 terms per
 * coefficient) and passed as rd_ram_t.dft_tables -- rd_ram_mix computes exactly those bins as matrix products on the matrix cores
 * (csrc/ram_dft.hip) instead of whole FFTs on the vector units.  dft_tables == NULL, or a geometry the matrix path does not take
 * (rd_ram_dft_tables_bytes returns 0: W not a multiple of 16): the FFT kernels. */
int64_t rd_ram_dft_tables_bytes(int H, int W, int b);
int rd_ram_dft_tables(void* tables, int H, int W, int b, void* stream);

/* The reference's free functions on their own (API parity; the training step uses rd_ram_mix):
 *   rd_ram_amp     extract_amp_spectrum (fundus.py:13-19): amp[C][H][W] = |fft2(img[C][H][W])|, fp32
 *   rd_ram_mutate  low_freq_mutate_np (fundus.py:21-39) with the ratio given: out = amp_src, and inside the centred window
 *                  |ky| <= b, |kx| <= b (fftshift'ed coordinates c-b..c+b): lam*amp_src + (1-lam)*amp_trg */
int64_t rd_ram_amp_workspace(int C, int H, int W);
int rd_ram_amp(const float* img_chw, float* amp_chw, int C, int H, int W, void* workspace, const float* tw_w, const float* tw_h,
               void* stream);
int rd_ram_mutate(const float* amp_src, const float* amp_trg, float* out, int C, int H, int W, int b, float lam, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Launch lists.  The training step (code/train.py:225-296) is ~250 calls of the entry points above over three HIP streams; issued
 * one by one from the interpreter (a ctypes call + an event record / stream wait per fork) they cost the host 2.2 ms per 4.4 ms step.
 * rd_run_list walks a prepared list in C++: one call per step segment.
 *   op      which entry point (RD_OP_*), or RD_OP_FORK / RD_OP_JOIN;
 *   a[]     its arguments in declaration order WITHOUT the trailing stream: pointers and integers as they are, a float as its
 *           bit pattern in the low 32 bits.  Descriptor structs and host arrays (gstart_host, rd_zero's arrays) are referenced, not
 *           copied: they must stay alive and unchanged while the list is in use;
 *   lane    index into streams[] (0 = the caller's main stream).  An entry on lane k > 0 with wait_main != 0 first makes streams[k]
 *           wait for everything enqueued on streams[0] so far (the weight-gradient launches: each behind its place in the dgrad
 *           chain).  RD_OP_FORK: streams[lane] waits for streams[0]; RD_OP_JOIN: streams[0] waits for streams[lane] if the lane is
 *           open.  A lane is OPEN from its first fork / wait_main entry until it is joined.
 * *open_lanes (bit k = lane k; may be NULL) carries the open set in and out, so that consecutive segments can leave a lane running
 * across their boundary (the data-parallel step joins the weight-gradient lane only in front of the optimizer);
 * rd_join_lanes makes streams[0] wait for every lane in `mask`.  Works eagerly and under stream capture (events only).
 * Returns 0, the first failing entry point's error code, or -1 for a malformed entry (its index in *bad_index if not NULL). */
/* The entry points a list can hold: X(enum suffix, entry point).  THE table: the RD_OP_* codes below, the argument unpacking of
 * csrc/runlist.hip (from each function's own signature) and rd_op_code() all come from it.  The codes are ABI: rows are only appended. */
#define RD_LAUNCH_OPS(X)                                                                                                          \
    X(CONV, rd_conv) X(WGRAD, rd_wgrad) X(CONV_BWD_FUSED, rd_conv_bwd_fused) X(CONV_BWD_FUSED_REDUCE, rd_conv_bwd_fused_reduce)  \
    X(PACK_WEIGHTS_BATCHED, rd_pack_weights_batched) X(BN_FINALIZE_FWD, rd_bn_finalize_fwd) X(BN_FINALIZE_BWD, rd_bn_finalize_bwd) \
    X(GN_FINALIZE_FWD, rd_gn_finalize_fwd) X(GN_FINALIZE_BWD, rd_gn_finalize_bwd) X(UP_STATS, rd_up_stats) X(BN_STATS, rd_bn_stats) \
    X(UP_BWD, rd_up_bwd) X(POOL_FWD, rd_pool_fwd) X(POOL_BWD, rd_pool_bwd) X(BN_APPLY, rd_bn_apply) X(NCHW_TO_NHWC, rd_nchw_to_nhwc) \
    X(NHWC_TO_NCHW, rd_nhwc_to_nchw) X(GRAD_IN, rd_grad_in) X(COLSUM, rd_colsum) X(SEG_LOSS, rd_seg_loss) X(REC_LOSS, rd_rec_loss)  \
    X(ADAM_STEP, rd_adam_step) X(ZERO, rd_zero) X(RAM_MIX, rd_ram_mix)
#define RD_OP_ENUM_(suffix, fn) RD_OP_##suffix,
enum { RD_OP_FORK = 1, RD_OP_JOIN = 2, RD_OP_BEFORE_FIRST_ = 9, RD_LAUNCH_OPS(RD_OP_ENUM_) RD_OP_END_ };   /* RD_OP_CONV = 10 ... RD_OP_RAM_MIX = 33 */
#undef RD_OP_ENUM_
/* the RD_OP_* code of an entry point by its name ("rd_conv" -> 10), -1 if a list cannot hold it.  Host logic only. */
int rd_op_code(const char* entry_point);
#define RD_LAUNCH_MAX_ARGS 18
typedef struct {
    int32_t op;
    int32_t lane;
    int32_t wait_main;
    int32_t nargs;
    uint64_t a[RD_LAUNCH_MAX_ARGS];
} rd_launch_t;
int rd_run_list(const rd_launch_t* ops, int n, void* const* streams, int n_streams, uint32_t* open_lanes, int* bad_index);
int rd_join_lanes(void* const* streams, int n_streams, uint32_t mask);
/* enable != 0: rd_run_list enqueues the entries of every lane k > 0 from a worker thread of the library (one per lane, started on first
 * use), in parallel with the calling thread's lane 0: a launch costs the host ~2.4 us inside the HIP runtime whoever issues it, so ONE
 * thread needs ~0.85 ms for the step's ~305 kernels and three need ~0.4.  Same per-stream order, same events between the streams: the
 * GPU executes the same graph.  Not used while the main stream is being captured.  Returns the previous setting.  Process-wide;
 * rd_run_list itself must still be called from one thread at a time. */
int rd_run_list_threads(int enable);
/* enable != 0 (the default): a lane fork that directly follows a launch of the main stream takes its event from that launch's own
 * dispatch packet (hipExtLaunchKernelGGL stop event) instead of a hipEventRecord behind it: a record is a packet of its own between two
 * dependent kernels and costs the main stream ~3 us per fork (scripts/probe/ext_event.hip), ~40 times per training step.  The
 * dependency is the same one -- the lane waits for that launch and everything before it on the main stream.  Never under stream
 * capture, single-threaded walk only (an entry that launches no kernel of the library leaves the fork to a record).  Returns the previous setting.  Process-wide. */
int rd_run_list_bind_fork_events(int enable);
/* forks of the single-threaded walk since the library was loaded: served by a bound event / by a recorded one (tests, diagnostics) */
void rd_run_list_fork_counts(long long* bound, long long* recorded);
/* carries[i] = 1 for the entries of lane 0 that rd_run_list would launch with a fork's event bound to them (a RD_OP_FORK of a lane > 0,
 * or a lane entry with wait_main, follows before the main stream is given anything else or joins a lane).  Host logic only. */
int rd_run_list_fork_plan(const rd_launch_t* ops, int n, unsigned char* carries);
/* The walk of rd_run_list without streams and without launches: what it would do with a list over n_streams distinct streams, step by
 * step and in order -- launch entry `index` on `lane` (carries: with a fork's event bound to it, as rd_run_list_fork_plan says), make
 * streams[lane] wait for the main stream's position (RD_STEP_FORK: a fork, or the edge in front of a wait_main entry), make the main
 * stream wait for streams[lane] (RD_STEP_JOIN).  steps has room for 2 * n; *open_lanes, *bad_index and the return value are the walk's
 * (-1 with the index of a malformed entry: lane, nargs, unknown op, nargs other than the entry point's).  Host logic only. */
enum { RD_STEP_LAUNCH = 0, RD_STEP_FORK = 1, RD_STEP_JOIN = 2 };
typedef struct {
    int32_t kind;
    int32_t lane;
    int32_t index;      /* RD_STEP_LAUNCH: the entry; -1 otherwise */
    int32_t carries;
} rd_step_t;
int rd_run_list_schedule(const rd_launch_t* ops, int n, int n_streams, uint32_t* open_lanes, int* bad_index, rd_step_t* steps, int* n_steps);

/* ------------------------------------------------------------------------------------------------
 * GPU-resident training data (train.py --gpu_data, ramdsir/gpu_data.py): the decoded pixels of every image training can touch
 * stay in device memory, the host only draws the random numbers, and ONE launch per step does all the per-sample pixel work of
 * the host path's DataLoader workers -- for the whole step's batch, all domains concatenated, on the caller's stream, with no
 * host-device synchronisation.
 *
 * rd_fundus_batch replaces Resize(256) + RandomScaleCrop(256) (code/dataset/transform.py:163-204) and the per-sample work of
 * Fundus_Multi.__getitem__ (code/dataset/fundus.py:197-240): image -> bilinear S x S -> (with the drawn factors) bilinear sw x sh
 * -> crop (cx, cy, S x S); the mask through the same geometry with nearest sampling, then [cup = g <= 50, disc = g <= 200]; the
 * partner -> bilinear S x S; lam.  The arithmetic is Pillow's 8-bit resampling (Resample.c), integer only, so the result is BIT-
 * IDENTICAL to the host path: per axis a table (ramdsir/resample.py axis_table) at an int32 offset of `tables`:
 *   [n_in, n_out, ksize, 0] xmin[n_out] cnt[n_out] k[n_out][ksize] nearest[n_out]
 * out[i] = clamp((2^21 + sum_{t < cnt[i]} in[xmin[i] + t] * k[i][t]) >> 22, 0, 255), the horizontal pass first and rounded to
 * uint8, nearest[i] the source index Image.resize(NEAREST) takes.  "No scaling" is sw = sh = S with the identity tables of S -> S
 * (which reproduce their input exactly).  One workgroup per (sample, band of band_rows output rows, image / partner); the stage-1
 * rows a band needs live in LDS: (src_rows + 2 mid_rows) * S * 3 bytes, bounds the caller derives from the tables
 * (ramdsir/resample.py max_window).
 * Outputs: src, trg uint8 [B][S][S][3]; lam fp32 [B]; mask fp32 [B][2][S][S] -- what train.py's on_device() makes of the host
 * path's batches. */
typedef struct {
    int64_t off;                /* byte offset of the HWC RGB pixels in rd_fundus_batch_t.pixels */
    int64_t mask_off;           /* byte offset of the gray mask (H x W) in .masks, -1: none (partner-only images) */
    int32_t h, w;
    int32_t tab_x, tab_y;       /* tables w -> S (x) and h -> S (y) */
} rd_aug_image_t;

typedef struct {
    int32_t img, partner;       /* image slots */
    int32_t tab_x, tab_y;       /* tables S -> sw (x) and S -> sh (y) */
    int32_t sw, sh;             /* the scaled size (S, S: the coin said no) */
    int32_t cx, cy;             /* crop offset, 0 <= cx <= sw - S, 0 <= cy <= sh - S */
    float lam;
    int32_t pad_;
} rd_fundus_sample_t;

typedef struct {
    const uint8_t* pixels;
    const uint8_t* masks;
    const rd_aug_image_t* images;   /* device array [n_images] */
    const int32_t* tables;
    uint8_t* src;
    uint8_t* trg;
    float* lam;
    float* mask;
    int32_t n_images;
    int32_t S;                  /* output size (256) */
    int32_t id_x, id_y;         /* tables S -> S (partner's second stage) */
    int32_t band_rows, src_rows, mid_rows;
    int32_t pad_;
} rd_fundus_batch_t;
/* samples_host: B HOST records (read before the call returns: they travel as kernel arguments, RD_AUG_CHUNK per launch).  Returns
 * -1 for an invalid descriptor or record. */
#define RD_AUG_CHUNK 48
int rd_fundus_batch(const rd_fundus_batch_t* p, const rd_fundus_sample_t* samples_host, int B, void* stream);

/* rd_prostate_batch replaces the per-sample work of Prostate_Multi.__getitem__ (code/dataset/prostate.py:167-188): gathers the
 * resident fp32 (S, S, 3) slices of the images and partners and the masks (uint8 labels, widened to int64), and writes lam --
 * exactly what the host path's collated batches hold: src, trg fp32 [B][S][S][3], lam fp32 [B], mask int64 [B][S][S]. */
typedef struct {
    int32_t img, partner;       /* slice slots (img must have a mask) */
    float lam;
    int32_t pad_;
} rd_prostate_sample_t;

typedef struct {
    const float* slices;        /* [n_slices][S][S][3] */
    const uint8_t* masks;       /* [n_slices][S][S] */
    float* src;
    float* trg;
    float* lam;
    int64_t* mask;
    int32_t n_slices, S;
} rd_prostate_batch_t;
int rd_prostate_batch(const rd_prostate_batch_t* p, const rd_prostate_sample_t* samples_host, int B, void* stream);

/* In-training Fundus validation after the forward pass (train.py --gpu_val; code/train.py:91-132, code/utils/utils.py:19-28,45-96),
 * csrc/val_post.hip.  Images have their own native sizes; each owns two planes (0 cup, 1 disc) of h x w bytes, stored back to back.
 * All three take B HOST records (read before the call returns: they travel as kernel arguments, RD_VAL_CHUNK per launch), launch on
 * `stream`, never synchronise and return -1 for an invalid record or a buffer too small for it.
 *   rd_val_threshold  mask = F.interpolate(sigmoid(logits), (h, w), mode='bilinear', align_corners=False) > 0.75 as 0 / 1 bytes at
 *                     mask + off, for image b of logits fp32 [B][2][Sh][Sw] (contiguous NCHW).  fp32 throughout: scale = (float)S / out,
 *                     src = max(scale * (dst + 0.5f) - 0.5f, 0), i0 = (int)src, i1 = min(i0 + 1, S - 1), weight src - i0, the horizontal
 *                     pairs first, then the vertical one, every operation rounded on its own (ramdsir/gpu_val.py resize_threshold_model).
 *   rd_val_post       per plane: keep the largest 8-connected component of mask (ties: the one whose first pixel in raster order comes
 *                     first; an empty plane stays empty), then turn every background pixel that is not 4-connected to the image border
 *                     into foreground -> post (bit-identical to utils.metrics.postprocess_binary; ramdsir/gpu_val.py postprocess_model).
 *                     mask and post are distinct buffers with the same layout.  With gt (0 / non-0 bytes, the image's planes at gt_off)
 *                     and counts (int32 [n_slots][2][3], zeroed by the caller before a pass) it adds |post|, |gt|, |post & gt| of every
 *                     plane to counts[slot][plane]; gt and counts are given together or both NULL.  Integer atomics only: the result does
 *                     not depend on scheduling.  workspace: rd_val_post_workspace(images, B) bytes, 16-byte aligned, contents irrelevant. */
typedef struct {
    int64_t off;                /* byte offset of the image's (2, h, w) planes in mask and post */
    int64_t gt_off;             /* byte offset of its (2, h, w) target planes in gt */
    int32_t h, w;
    int32_t slot;               /* row of counts the image adds to */
    int32_t pad_;
} rd_val_image_t;
#define RD_VAL_CHUNK 32
int rd_val_threshold(const float* logits, int B, int Sh, int Sw, const rd_val_image_t* images_host, uint8_t* mask, int64_t mask_bytes,
                     void* stream);
int64_t rd_val_post_workspace(const rd_val_image_t* images_host, int B);
int rd_val_post(const uint8_t* mask, uint8_t* post, int64_t mask_bytes, const uint8_t* gt, int64_t gt_bytes, int32_t* counts, int n_slots,
                void* workspace, int64_t workspace_bytes, const rd_val_image_t* images_host, int B, void* stream);

/* In-training Prostate validation around the forward pass (train.py --gpu_val_volumes; code/train.py:134-192,
 * code/utils/utils.py:30-42), csrc/val_volume.hip.  A volume is (D, H, W) in raster order; its fp32 voxels, normalised on the host at
 * preload, stay on the device.  frames_host: B HOST frame indices (read before the call returns: they travel as kernel arguments,
 * RD_VAL_CHUNK per launch), -1 for an empty slot, otherwise 1 <= jj <= D - 2 and increasing.  All entry points launch on `stream`,
 * never synchronise and return -1 for an invalid argument or record or a buffer too small for it, before anything is launched.
 *   rd_vol_stack   the 2.5-D batch of code/train.py:161-168: out fp32 [B][3][H][W] (contiguous), channel c of slot b = slice
 *                  frames[b] - 1 + c of `volume`; an empty slot is all zeros.  A pure copy.
 *   rd_vol_argmax  code/train.py:170-176: slice jj = frames[b] of `pred` (0 / 1 bytes, (D, H, W)) := argmax over the two classes of
 *                  logits fp32 [B][2][H][W] (contiguous NCHW), the first maximum winning (1 iff l1 > l0) -- or zeros where
 *                  gt_empty[jj] != 0 (D bytes: the slices whose ground truth sums to 0).  Empty slots write nothing; slices that no
 *                  call reaches keep what the caller cleared them to (rd_zero, once per pass).
 *   rd_vol_post    code/utils/utils.py:30-42 `_connectivity_region_analysis`: per volume, keep the largest 6-connected (face)
 *                  component of pred (ties: the one whose first voxel in (z, y, x) raster order comes first); an EMPTY prediction
 *                  becomes all ones, as the reference's `keep == 0` does -> post (bit-identical to
 *                  utils.metrics.connectivity_region_analysis; ramdsir/gpu_val_volumes.py largest_component_model).  pred and post are
 *                  distinct buffers with the same layout.  With gt (0 / non-0 bytes, the volume at gt_off) and counts (int32
 *                  [n_slots][3], zeroed by the caller before a pass) it adds |post|, |gt|, |post & gt| to counts[slot]; gt and counts
 *                  are given together or both NULL.  Integer atomics only: the result does not depend on scheduling.
 *                  workspace: rd_vol_post_workspace(volumes, B) bytes, 16-byte aligned, contents irrelevant. */
typedef struct {
    int64_t off;                /* byte offset of the volume's (d, h, w) bytes in pred and post */
    int64_t gt_off;             /* byte offset of its ground truth in gt */
    int32_t d, h, w;
    int32_t slot;               /* row of counts the volume adds to */
} rd_val_volume_t;
int rd_vol_stack(const float* volume, int D, int H, int W, const int32_t* frames_host, int B, float* out, void* stream);
int rd_vol_argmax(const float* logits, int B, int H, int W, const int32_t* frames_host, const uint8_t* gt_empty, int D, uint8_t* pred,
                  void* stream);
int64_t rd_vol_post_workspace(const rd_val_volume_t* volumes_host, int B);
int rd_vol_post(const uint8_t* pred, uint8_t* post, int64_t pred_bytes, const uint8_t* gt, int64_t gt_bytes, int32_t* counts, int n_slots,
                void* workspace, int64_t workspace_bytes, const rd_val_volume_t* volumes_host, int B, void* stream);

/* The fused validation forward (train.py --fused_val, ramdsir/infer.py EvalForward), csrc/infer.hip: what a forward-only launch list
 * with frozen BatchNorm (engine.Plan frozen_bn: rd_conv and rd_pool_fwd entries only) needs around it.  The network input and the
 * logits are NHWC in the storage dtype (RD_F32 / RD_BF16) with a channel stride `cstride` in elements; a stored value is widened to
 * fp32 exactly.  All four launch on `stream`, never wait for work on any stream, and return -1 for an invalid argument or record
 * before anything is launched.  No reference counterpart beyond the lines the NCHW forms above cite.
 *   rd_bn_eval_coeffs      scale / shift of ALL n_sites BatchNorm sites in one launch, from the running statistics: the eval branch of
 *                          rd_bn_finalize_fwd (invstd = 1 / sqrt(running_var + eps), scale = gamma * invstd,
 *                          shift = beta - running_mean * scale; the same device function, so the same bits).  sites_dev: a DEVICE
 *                          table, written once when the plan is built and complete in memory before the call; max_C: the largest C
 *                          in it.  The call reads the table back through a stream of its own to check it (the host waits for that
 *                          copy of n_sites records, not for `stream`): a null pointer or C < 1 or C > max_C in a site returns -1.
 *   rd_val_threshold_nhwc  rd_val_threshold on logits [B][Sh][Sw][cstride], channel 0 the cup and 1 the disc (cstride >= 2): the same
 *                          operation sequence on the widened values, records, return codes and chunking.
 *   rd_vol_stack_nhwc      rd_vol_stack straight into the plan's input: out[b][y][x][c] = slice frames[b] - 1 + c for c < 3 (fp32 ->
 *                          storage dtype rounded to nearest even, what rd_nchw_to_nhwc does to rd_vol_stack's output), zeros in
 *                          channels 3 .. cstride - 1 (cstride >= 3) and in every channel of an empty slot.
 *   rd_vol_argmax_nhwc     rd_vol_argmax on logits [B][H][W][cstride] (cstride >= 2): 1 iff l1 > l0 on the widened values; gt_empty
 *                          and empty slots as there. */
typedef struct {
    const float* gamma;
    const float* beta;
    const float* running_mean;
    const float* running_var;
    float* scale;               /* [C] */
    float* shift;               /* [C] */
    int32_t C;
    int32_t pad_;
} rd_bn_eval_site_t;
int rd_bn_eval_coeffs(const rd_bn_eval_site_t* sites_dev, int n_sites, int max_C, float eps, void* stream);
int rd_val_threshold_nhwc(const void* logits, int dtype, int cstride, int B, int Sh, int Sw, const rd_val_image_t* images_host,
                          uint8_t* mask, int64_t mask_bytes, void* stream);
int rd_vol_stack_nhwc(const float* volume, int D, int H, int W, const int32_t* frames_host, int B, void* out, int dtype, int cstride,
                      void* stream);
int rd_vol_argmax_nhwc(const void* logits, int dtype, int cstride, int B, int H, int W, const int32_t* frames_host,
                       const uint8_t* gt_empty, int D, uint8_t* pred, void* stream);

/* TensorBoard image summaries (train.py --tb_images, ramdsir/tb_images.py), csrc/tb_grid.hip: replaces the make_grid(...) +
 * writer.add_image(...) blocks of code/train.py:306-329 (Fundus) and :475-496 (Prostate) -- the slicing, sigmoid / tanh / argmax,
 * decode_seg_map_sequence (code/utils/utils.py:285-336), torchvision.utils.make_grid and tensorboardX's float -> uint8 conversion --
 * for ALL grids of one logging iteration in at most two launches.  torchvision and tensorboardX are not dependencies; their semantics
 * are RESTATED here (parity unpinned) and modelled in numpy by ramdsir/tb_images.py grid_model:
 *   selection   samples sample[0..n) (1 <= n <= 3) of the source, channels c0 .. c0 + nc (nc = 3, or nc = 1: replicated to three);
 *               element (s, c, y, x) is src[s * stride_n + c * stride_c + y * stride_h + x * stride_w] (strides in ELEMENTS: the step's
 *               NHWC buffers with a padded channel slot and contiguous NCHW tensors are both covered), bf16 widened to fp32;
 *   transform   identity | sigmoid 1 / (1 + exp(-x)) | tanh | RD_TB_ARGMAX: argmax over the nc (= K <= RD_TB_PALETTE) channels from c0,
 *               the lowest index winning a tie, then the palette | RD_TB_LABEL: the source is int64 [s][y][x] class labels, then the
 *               palette.  Palette: the 21 "pascal" colours of decode_segmap, value float32(double(colour) / 255.0); a class outside it
 *               stays black.  A Fundus target (fp32 0 / 1 planes) is RD_TB_F32 + identity without normalize;
 *   normalize   make_grid(normalize=True): lo, hi = min, max over the whole selection after the transform;
 *               v = (x - lo) / float32(max(double(hi) - double(lo), 1e-5)), an IEEE division (torchvision's norm_ip:
 *               clamp_(low, high).sub_(low).div_(max(high - low, 1e-5)));
 *   grid        make_grid(nrow=3, padding=2, pad_value=0): n == 1 -> the image itself, H x W; otherwise (H + 4) x (n (W + 2) + 2),
 *               zero filled, tile k at rows [2, 2 + H), columns [k (W + 2) + 2, k (W + 2) + 2 + W);
 *   pixel       add_image: uint8(trunc(v * 255.0f)), v in [0, 1] by construction;
 *   dst         uint8 HWC [grid rows][grid columns][3] in a caller-owned device buffer.
 * grids_host: n_grids (1 .. RD_TB_MAX_GRIDS) HOST records (read before the call returns: they travel as kernel arguments).  workspace:
 * rd_tb_grids_workspace(n_grids) bytes, 8-byte aligned, contents irrelevant before and after (one (min, max) pair per workgroup of the
 * first launch: no atomics, nothing to initialise; the launch is skipped when no grid normalises).  Launches on `stream`, never
 * synchronises or copies (the caller reads dst with its own copy); -1 for an invalid record, before anything is launched.  The
 * extents of src and dst are the caller's to guarantee. */
enum { RD_TB_F32 = 0, RD_TB_BF16 = 1, RD_TB_I64 = 2 };
enum { RD_TB_IDENTITY = 0, RD_TB_SIGMOID = 1, RD_TB_TANH = 2, RD_TB_ARGMAX = 3, RD_TB_LABEL = 4 };
#define RD_TB_MAX_GRIDS 8
#define RD_TB_PARTS 64
#define RD_TB_PALETTE 21
typedef struct {
    const void* src;
    uint8_t* dst;
    int64_t stride_n, stride_c, stride_h, stride_w;   /* elements */
    int32_t etype;              /* RD_TB_F32 / RD_TB_BF16; RD_TB_I64 with RD_TB_LABEL */
    int32_t H, W;
    int32_t n;                  /* selected samples, 1 .. 3 */
    int32_t sample[3];
    int32_t c0, nc;
    int32_t transform;          /* RD_TB_* */
    int32_t normalize;          /* not with RD_TB_ARGMAX / RD_TB_LABEL */
    int32_t slot;               /* set by the library (whole 16-byte channel-slot loads apply); ignored on input */
} rd_tb_grid_t;
int64_t rd_tb_grids_workspace(int n_grids);
int rd_tb_grids(const rd_tb_grid_t* grids_host, int n_grids, void* workspace, int64_t workspace_bytes, void* stream);

/* Per-step record stream (train.py --tb_every_iter / --tb_health, ramdsir/step_log.py), csrc/step_log.hip: the reference writes its
 * seven scalars -- lr, loss/loss_{bce,ce}_1, loss/loss_dice_1, loss/loss_{bce,ce}_2, loss/loss_dice_2, loss/loss_consistency,
 * loss/loss_rec -- at EVERY iteration (code/train.py:298-304 Fundus, :467-473 Prostate), reading each loss with .item().  Here one call
 * behind a step appends one row of RD_LOG_ROW floats to a device-resident ring and the host drains the ring where it synchronises
 * anyway.  Row layout (float32 words):
 *   [0, 8)    losses[8]   (rd_seg_loss's losses_out)
 *   [8, 12)   hyper[4]    (rd_adam_step's hyper_out: word 8 is the lr of the step, word 11 its iteration number)
 *   [12, 28)  rec_mse[n_rec], the remaining slots 0 (n_rec <= RD_LOG_MAX_REC)
 *   [28, 31)  gradient norms of the three Adam groups (code/train.py:573-576: encoder, seg decoder, rec decoder), elements
 *             [range[g], range[g + 1]) of `grads`: (float)sqrt(sum of g * g), the sum in fp64 over the FINITE elements
 *   [31]      the number of non-finite (NaN, +-Inf) elements of [range[0], range[3]), as a float (exact: range[3] - range[0] <= 2^24)
 * grads == NULL: no health pass, words 28..31 are 0 and `partial` is not used.  The row goes to ring + row * RD_LOG_ROW; the caller
 * owns the row counter.  The health pass has no reference counterpart.  It is a pure function of the data: group g is cut into chunks
 * of RD_LOG_CHUNK elements from range[g] on, chunk c of the call (groups in order) is summed by workgroup c in a fixed order into
 * partial[c] = {double sum, int64 count}; a second launch of one workgroup adds the partials of a group, each lane of a wave its
 * indices lane, lane + 64, ... in ascending order, then the 64 lanes in a fixed tree -- no atomics, nothing depends on which
 * workgroup finishes first.  Wide loads are used on the 16-byte-aligned part of a chunk, whatever the alignment of grads + range[g].
 * partial: rd_step_log_workspace(range[3] - range[0]) bytes, 8-byte aligned, contents irrelevant before and after.  At most two
 * launches on `stream`; allocates nothing, synchronises nothing, copies nothing.  Returns, before anything is launched: -1 a null
 * descriptor / losses / rec_mse / hyper / ring (or partial, with grads), -2 row outside [0, rows), -3 n_rec outside
 * [0, RD_LOG_MAX_REC], -4 a negative or decreasing range or one of more than 2^24 elements. */
#define RD_LOG_ROW 32
#define RD_LOG_MAX_REC 16
#define RD_LOG_CHUNK 4096
typedef struct {
    const float* losses;        /* device [8] */
    const float* rec_mse;       /* device [n_rec] */
    const float* hyper;         /* device [4] */
    const float* grads;         /* device arena, or NULL */
    int64_t range[4];           /* element offsets into grads */
    float* ring;                /* device [rows][RD_LOG_ROW] */
    int32_t rows, row;
    int32_t n_rec;
    int32_t pad_;
    void* partial;
} rd_step_log_t;
int rd_step_log(const rd_step_log_t* p, void* stream);
int64_t rd_step_log_workspace(int64_t n);

/* Training-state snapshot (train.py --ckpt_every / --resume, ramdsir/ckpt.py), csrc/snapshot.hip: copies n device ranges to
 * (direction 0, gather) or from (direction 1, scatter) ONE contiguous staging buffer and leaves two 64-bit checksums per range.  No
 * reference counterpart: the reference writes its three state_dicts with torch.save (code/train.py:342-360) and never reads one back
 * into a trainer.  Range i is [ptr, ptr + bytes) on the device and [staging + offset, staging + offset + bytes) in the staging buffer;
 * bytes is a multiple of 4, ptr, offset and staging are 4-byte aligned, the offsets ascend in table order without overlap and stay
 * inside staging_bytes.  bytes == 0 is allowed (its sums are 0).  The device ranges of a scatter must not overlap each other (not
 * checked).  With the little-endian uint32 words w[0 .. bytes / 4) of a range -- the words READ from the range by a gather, the words
 * WRITTEN to it by a scatter --
 *     sums[S i] = sum w[k],   sums[S i + 1] = sum (k + 1) w[k]      (both mod 2^64; S = RD_SNAP_SUM_STRIDE: one 128-byte line per
 * range, of which only these two words are ever written -- same-address atomics are served one after the other, so the pairs of
 * different ranges sit in different lines; sums_dev holds n * S words)
 * each workgroup reduces its part and issues one pair of 64-bit integer atomic adds: integer addition commutes, so the sums are the
 * same bits on every run; no floating point.  Work decomposition (csrc/range_walk.h: the ONE text of this walk, which rd_avg_step,
 * rd_guard_sync and rd_optim_step share): range i is cut into chunks of RD_SNAP_CHUNK bytes from its start
 * (the last one ragged), chunk0 = the number of chunks of the ranges in front of it; the grid is flat over the total_chunks chunks and
 * a workgroup finds its range by binary search over chunk0 in table_dev -- the SAME n entries in device memory, uploaded once by the
 * caller, as rd_pack_weights_batched's table_dev.  table_host is read for validation only; nothing on the device is dereferenced by
 * the host.  Within a chunk the part where source and destination are both 16-byte aligned moves with 16-byte loads and stores, the
 * words in front of and behind it (or the whole chunk, when the two sides are aligned differently) with 4-byte accesses.
 * At most two launches on `stream`, both kernels through the library's one launch site: a clear of the 2 n sums, then the copy (none
 * at all for n == 0, which succeeds; the clear alone when every range is empty).  No hipMemcpyAsync / hipMemsetAsync; allocates
 * nothing, synchronises nothing; the caller owns every buffer.  Returns, before anything is launched: -1 n < 0 (or > 2^24) or a null
 * table / staging / sums, -2 a byte count that is negative or not a multiple of 4, -3 a misaligned range start, offset, staging or
 * sums pointer (or a null start with bytes > 0), -4 offsets that overlap, descend or leave staging_bytes, -5 a chunk0 column or
 * total_chunks that does not match the byte counts, -6 a direction other than 0 or 1. */
#define RD_SNAP_CHUNK 65536
#define RD_SNAP_SUM_STRIDE 16
typedef struct {
    void* ptr;                  /* device start of the range */
    int64_t bytes;
    int64_t offset;             /* byte offset in the staging buffer */
    int64_t chunk0;             /* first chunk of the range in the flat grid */
} rd_snap_range_t;
int rd_snapshot(const rd_snap_range_t* table_host, const rd_snap_range_t* table_dev, int n, int64_t total_chunks, void* staging,
                int64_t staging_bytes, uint64_t* sums_dev, int direction, void* stream);

/* Weight averaging along the training trajectory (train.py --avg_weights, ramdsir/avg.py), csrc/avg.hip: one pass over n pairs of
 * device ranges, src the live model (parameters, BatchNorm buffers), dst the averaged copy.  No reference counterpart: the reference
 * keeps the last iterate only.  Range i is [src, src + bytes) and [dst, dst + bytes); bytes is a multiple of 4, src and dst are
 * 4-byte aligned, bytes == 0 is allowed.  The src and dst ranges must not overlap each other (not checked); src is only read.
 * The number of completed steps s is READ from *iter_dev by the kernel (rd_adam_step leaves it there: `*p.iter = it + 1`), never passed:
 * every argument is the same at every step.  With k = s - 1 - start, per 32-bit word p of src and a of dst:
 *     kind 1 (non-float words, e.g. the int64 num_batches_tracked):  a = p, always
 *     kind 0 (fp32), k <= 0:                                          a = p   (the average IS the live model until averaging starts, and
 *                                                                             the first averaged point is a copy; the bits are moved as they are)
 *     kind 0 (fp32), k > 0:    d = p - a;  t = w * d;  a = a + t      three separately rounded fp32 operations (round to nearest even,
 *                                                                     denormals kept), never an fma;
 *                              w = one_minus_decay (mode 0, exponential moving average) or 1.0f / (float)(k + 1) (mode 1, the uniform
 *                              average of the iterates start + 1, ..., s), the division correctly rounded
 * -- numpy float32 reproduces it bit for bit (ramdsir/avg.py model()).  Work decomposition: the walk of csrc/range_walk.h as
 * described for rd_snapshot above, over chunks of RD_AVG_CHUNK bytes -- chunk0, total_chunks, table_dev (the SAME n entries in
 * device memory, uploaded once by the caller), table_host (read for validation only; nothing on the device is dereferenced by the
 * host) and the 16-byte / 4-byte split of a chunk between src and dst mean what they mean there.
 * Exactly ONE launch on `stream`, through the library's one launch site (none for n == 0 or when every range is empty, which
 * succeed).  No hipMemcpyAsync / hipMemsetAsync; allocates nothing, synchronises nothing; the caller owns every buffer.  Returns,
 * before anything is launched: -1 n < 0 (or > 2^24), a null iter_dev, or (n > 0) a null table; -2 a byte count that is negative or not
 * a multiple of 4; -3 a misaligned src, dst or iter_dev (or a null src / dst with bytes > 0); -4 a kind other than 0 or 1; -5 a chunk0
 * column or total_chunks that does not match the byte counts; -6 a mode other than 0 or 1; -7 mode 0 with one_minus_decay outside
 * (0, 1) (NaN included); -8 start < 0. */
#define RD_AVG_CHUNK 16384
typedef struct {
    const void* src;            /* device start of the live range */
    void* dst;                  /* device start of the averaged range */
    int64_t bytes;
    int64_t chunk0;             /* first chunk of the range in the flat grid */
    int32_t kind;               /* 0 fp32 (averaged), 1 other words (copied) */
    int32_t pad_;
} rd_avg_range_t;
int rd_avg_step(const rd_avg_range_t* table_host, const rd_avg_range_t* table_dev, int n, int64_t total_chunks,
                const int32_t* iter_dev, int mode, float one_minus_decay, int32_t start, void* stream);

/* BatchNorm re-estimation of the averaged model (train.py --avg_bn_recal, ramdsir/avg_bn.py), csrc/bn_recal.hip: the cumulative
 * average of the batch statistics of ALL n_sites BatchNorm sites of a forward plan in one launch -- what
 * torch.optim.swa_utils.update_bn leaves in a BatchNorm with momentum=None.  No reference counterpart.  Called once per batch,
 * behind the forward launch list of a plan whose finalize launches leave the running statistics alone (rd_bn_fwd_t with
 * running_mean = running_var = num_batches_tracked = NULL, as for InstanceNorm above; engine.Plan recal_bn), with k = 0, 1, ... the
 * index of the batch.  Per site and channel c: (s1, s2) = the sums over the first nslots copies of the site's statistic slots,
 * then the finalize's own arithmetic (csrc/bn_fin.h fwd_stat, contraction off): mean = (float)(s1 / count + conv_bias[c]) -- the
 * bits of rd_bn_fwd_t.mean of the same launch list --, var = max(s2 / count - (s1 / count)^2, 0) in fp64,
 * unb = (float)(var * count / (count - 1)) for count > 1, (float)var otherwise.  With x the batch value (mean resp. unb):
 *     k == 0:  running = x                                       a plain store, the old content is not read
 *     k > 0:   d = x - running;  t = w * d;  running = running + t      three separately rounded fp32 operations, never an fma;
 *                                                                w = 1.0f / (float)(k + 1), the division correctly rounded
 * and num_batches_tracked = k + 1 (int64).  numpy reproduces it bit for bit (ramdsir/avg_bn.py model()).
 * sites_dev: the table in device memory, uploaded once by the caller; sites_host: the SAME n_sites records, read for validation
 * only (rd_avg_step's convention: nothing on the device is dereferenced by the host); max_C: the largest C in the table.  Grid:
 * (blocks over max_C, n_sites), as rd_bn_eval_coeffs'.  Exactly ONE launch on `stream`, through the library's one launch site; no
 * hipMemcpyAsync / hipMemsetAsync; allocates nothing, synchronises nothing.  Returns, before anything is launched: -1 a null table,
 * n_sites outside 1 .. RD_BN_RECAL_MAX_SITES or max_C < 1; -2 k < 0; -3 a site with a null stats, running_mean, running_var or
 * num_batches_tracked, or a misaligned pointer (stats 16, num_batches_tracked 8, the others 4 bytes); -4 a site with C < 1 or
 * C > max_C; -5 a site whose count is not >= 1 (NaN included); -6 a site whose nslots is not a multiple of 8 in 8 .. RD_STAT_SLOTS;
 * -7 eps negative or NaN. */
#define RD_BN_RECAL_MAX_SITES 4096
typedef struct {
    const double* stats;            /* [1][RD_STAT_SLOTS][C][2] sum, sum of squares of one statistics group */
    const float* conv_bias;         /* [C] bias of the producing conv (its sums exclude it) or NULL (rd_up_stats sums y itself) */
    float* running_mean;            /* [C] */
    float* running_var;             /* [C] */
    int64_t* num_batches_tracked;   /* [1] */
    float count;                    /* elements per channel of a batch: N * H * W */
    int32_t C;
    int32_t nslots;                 /* statistic copies the producers used: a multiple of 8 up to RD_STAT_SLOTS */
    int32_t pad_;
} rd_bn_recal_site_t;
int rd_bn_recal(const rd_bn_recal_site_t* sites_host, const rd_bn_recal_site_t* sites_dev, int n_sites, int max_C, int32_t k, float eps,
                void* stream);

/* Guarded optimizer step (train.py --clip_grad_norm / --skip_nonfinite, ramdsir/guard.py), csrc/guard.hip + csrc/loss.hip: what
 * stands in front of the reference's `loss.backward(); optimizer.step()` (code/train.py:285-287) when the user asks for it -- the
 * gradient of the whole arena is clipped by its global norm (torch.nn.utils.clip_grad_norm_ over the one optimizer), and a step whose
 * gradient is not finite leaves no trace in the model state.  No reference counterpart: the reference steps on whatever it gets.
 * Everything is decided on the device: the three entry points communicate through ONE device-resident rd_guard_state_t, which every
 * launch below reads or writes through its device pointer; the host reads it only where it synchronises anyway.
 *
 * rd_grad_guard: two launches, the decomposition of rd_step_log's health pass over ONE group.  (1) the n elements of `grad` are cut
 * into chunks of RD_LOG_CHUNK from its start; workgroup c sums g * g in fp64 over the FINITE elements of chunk c in a fixed order and
 * counts the others into partial[c] = {double sum, int64 count}; 16-byte loads on the aligned part of a chunk with a scalar head and
 * tail, for any 4-byte alignment of grad.  (2) one workgroup: lane l of wave 0 adds partials l, l + 64, ... in ascending order, then
 * the 64 lanes in the fixed xor tree (offsets 32, 16, ..., 1) -- no atomics -- and thread 0 writes
 *     norm      = (float)sqrt(sum)                       (the fp64 square root, rounded once to fp32)
 *     nonfinite = the count                              (n <= 2^24: it fits)
 *     skip      = nonfinite > 0 || !isfinite(norm)       (squares that overflow fp32 but not fp64 give a norm that is +Inf as a float)
 *     scale     = skip ? 1 : max_norm > 0 ? fminf(max_norm / (norm + 1e-6f), 1) : 1      separately rounded fp32 operations
 *     steps += 1;  clipped += (scale < 1 && !skip);  skipped += skip
 * ramdsir/guard.py model() is the same arithmetic in numpy, bit for bit.  The gradient is only read.  workspace:
 * rd_grad_guard_workspace(n) bytes, 8-byte aligned, contents irrelevant before and after.  Returns, before anything is launched:
 * -1 a null descriptor / grad / workspace / state or a misaligned one (grad 4, workspace and state 8 bytes), -2 n < 1 or n > 2^24
 * (rd_step_log's bound), -3 a max_norm that is negative or not finite (0: clipping off).
 *
 * rd_adam_step_guarded: rd_adam_step with two differences.  Its prepare launch forms the bias corrections from the number of updates
 * APPLIED, t = max(1, iter + 1 - guard->skipped) (the state['step'] of a skipped optimizer.step()); lr, hyper_out[0], hyper_out[3]
 * and `*iter += 1` are exactly rd_adam_step's -- the reference's lr is a function of iter_num (code/train.py:289).  Its update launch
 * returns at once when guard->skip is set (nothing is stored), and otherwise uses g = grad[i] * guard->scale (one rounded fp32
 * multiplication; scale == 1 is the identity) in rd_adam_step's arithmetic.  Returns -1 for a null descriptor or state, or n < 1.
 *
 * rd_guard_sync: ONE launch over n range pairs {live, shadow, bytes, chunk0}: with guard->skip set, live <- shadow (the BatchNorm
 * buffers the forward pass of the skipped step has moved are rolled back); otherwise shadow <- live (the last good step is
 * remembered).  A byte copy: int64 ranges and NaN bit patterns pass through untouched.  Work decomposition (csrc/range_walk.h) and
 * validation codes are rd_avg_step's, with RD_GUARD_CHUNK for RD_AVG_CHUNK: -1 n < 0 (or > 2^24), a null guard_dev, or (n > 0) a null table; -2 a byte
 * count that is negative or not a multiple of 4; -3 a misaligned live / shadow / guard_dev (or a null live / shadow with bytes > 0);
 * -5 a chunk0 column or total_chunks that does not match the byte counts.  The live and shadow ranges must not overlap (not checked).
 * None of the three allocates, synchronises or copies anything; every launch goes through the library's one launch site. */
#define RD_GUARD_CHUNK 16384
typedef struct {
    float norm;                 /* global gradient norm of the last guarded step (finite elements) */
    float scale;                /* what that step multiplied its gradient by */
    int32_t skip;               /* 1: that step was skipped */
    int32_t nonfinite;          /* its number of non-finite gradient elements */
    int64_t steps;              /* guarded steps so far */
    int64_t clipped;            /* of these, steps with scale < 1 */
    int64_t skipped;            /* of these, skipped steps */
} rd_guard_state_t;
typedef struct {
    const float* grad;          /* device arena */
    int64_t n;                  /* elements */
    float max_norm;             /* 0: no clipping */
    int32_t pad_;
    void* workspace;            /* device */
    rd_guard_state_t* state;    /* device */
} rd_grad_guard_t;
typedef struct {
    void* live;                 /* device start of the live range */
    void* shadow;               /* device start of its shadow copy */
    int64_t bytes;
    int64_t chunk0;             /* first chunk of the range in the flat grid */
} rd_guard_range_t;
int64_t rd_grad_guard_workspace(int64_t n);
int rd_grad_guard(const rd_grad_guard_t* p, void* stream);
int rd_adam_step_guarded(const rd_adam_t* p, const rd_guard_state_t* guard_dev, void* stream);
int rd_guard_sync(const rd_guard_range_t* table_host, const rd_guard_range_t* table_dev, int n, int64_t total_chunks,
                  const rd_guard_state_t* guard_dev, void* stream);

/* Grouped Adam (train.py --weight_decay / --wd_mode / --lr_schedule / --warmup_iters / --enc_lr_mult, ramdsir/optim.py),
 * csrc/optim.hip: torch's param_groups as a device table of contiguous ranges of the arena, each with its own learning-rate
 * multiplier and weight decay, and a schedule chosen by a field and evaluated on the device from the iteration counter.  The
 * reference's optimizer (code/train.py:573-576, 289-293; rd_adam_step) is the special case schedule poly, no warm-up and the table
 * {[0, n_half_lr): 0.5, 0}, {[n_half_lr, n): 1, 0}: with it rd_optim_step leaves the bits rd_adam_step leaves (guard_dev null) or
 * rd_adam_step_guarded leaves (guard_dev set), for any values, non-finite ones included -- the three update kernels share ONE source
 * text of the per-element arithmetic (csrc/adam_body.h).
 *
 * The table: n_ranges <= 4096 entries {first, count, lr_mult, weight_decay, chunk0}, sorted, contiguous, covering [0, n) exactly,
 * count >= 1.  Range starts have any 4-byte alignment (the arena packs tensors back to back).  Work decomposition: the walk of
 * csrc/range_walk.h (see rd_snapshot) over chunks of RD_OPT_CHUNK ELEMENTS, the grid flat over all chunks (not capped), with a
 * lookup of its own: a workgroup finds its range by a search over the chunk0 column of the device table (one load per thread and a
 * count over the workgroup, behind binary steps only above 256 ranges) -- per workgroup, never per element -- and moves the part of
 * its chunk that starts at a 16-byte boundary of all four arenas with 16-byte accesses, the words in front of and behind it one by one.
 *
 * Two launches.  (1) prepare, one thread, all in fp64, each word rounded once to fp32: with it = *iter,
 *     s(it) = schedule 0 (poly):     it == 0 ? 1 : (1 - (it - 1) / total_iters) ^ 0.9      rd_adam_step's expression, the reference's
 *                                                                                            one-iteration lag included
 *             schedule 1 (cosine):   0.5 * (1 + cos(pi * min(it, total_iters) / total_iters))      no lag
 *             schedule 2 (constant): 1
 *     w(it) = warmup_iters > 0 ? min(1, (it + 1) / warmup_iters) : 1
 *     hyper_out[0] = (float)(base_lr * s * w);  hyper_out[1..3] and *iter += 1 as rd_adam_step; with guard_dev the bias
 *     corrections count the updates applied, t = max(1, it + 1 - guard->skipped), as rd_adam_step_guarded.
 * (2) update: for element i of a range with multiplier M and decay D, separately rounded fp32 operations:
 *     lr_g = M * hyper_out[0]                                 (M = 0.5 and M = 1 give the bits of rd_adam_step's two rates)
 *     g = grad[i];  with guard_dev: nothing at all is stored when guard->skip is set, otherwise g = g * guard->scale
 *     D > 0, wd_mode 0 (decoupled):  param[i] = param[i] * (1 - lr_g * D)     torch.optim.AdamW's param.mul_(1 - lr * wd), first
 *     D > 0, wd_mode 1 (L2):         g = fma(D, param[i], g)                  torch.optim.Adam(weight_decay), behind the guard's
 *                                                                             scale as clip_grad_norm_ precedes optimizer.step()
 *     D == 0: neither operation is executed;  then rd_adam_step's update of exp_avg[i], exp_avg_sq[i], param[i] at rate lr_g.
 * ramdsir/optim.py schedule_model / decay_model are the same arithmetic in numpy.
 *
 * Returns, before anything is launched: -1 a null descriptor / arena / iter / hyper_out / table, n < 1 or n_ranges outside
 * 1..4096; -4 an unknown schedule or wd_mode, warmup_iters < 0 or >= total_iters; -2 a range with count < 1, ranges that are not
 * contiguous or do not cover [0, n); -3 an lr_mult that is not finite or <= 0, a weight_decay that is negative or not finite; -5 a
 * chunk0 column or total_chunks that does not match the counts.  Nothing is allocated, synchronised or copied; both launches go
 * through the library's one launch site.  rd_adam_t, rd_adam_step and rd_adam_step_guarded are unchanged. */
#define RD_OPT_CHUNK 4096
#define RD_OPT_MAX_RANGES 4096
typedef struct {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;     /* device arenas */
    int64_t n;              /* total elements */
    int32_t* iter;          /* device, incremented */
    float* hyper_out;       /* device [4]: rd_adam_step's layout */
    float base_lr;
    int32_t total_iters;
    float beta1, beta2, eps;
    int32_t schedule;       /* 0 poly, 1 cosine, 2 constant */
    int32_t warmup_iters;   /* 0: none */
    int32_t wd_mode;        /* 0 decoupled (AdamW), 1 L2 (Adam(weight_decay)) */
} rd_optim_t;
typedef struct {
    int64_t first;          /* first element of the range in the arena */
    int64_t count;          /* elements, >= 1 */
    float lr_mult;          /* the range's rate is lr_mult * hyper_out[0] */
    float weight_decay;     /* 0: none */
    int64_t chunk0;         /* first chunk of the range in the flat grid */
} rd_optim_range_t;
int rd_optim_step(const rd_optim_t* p, const rd_optim_range_t* table_host, const rd_optim_range_t* table_dev, int n_ranges,
                  int64_t total_chunks, const rd_guard_state_t* guard_dev /* may be NULL */, void* stream);

/* Gradient accumulation (train.py --accum_steps N, ramdsir/accum.py), csrc/accum.hip: the optimizer tail of the fused step runs on
 * every N-th iteration only, on the MEAN of the N micro-batch gradients.  The writers of the gradient arena overwrite (and rd_zero at
 * the head of every step is part of the contract of the ones that add), so the running sum lives in a second fp32 arena `acc` of the
 * same length and ONE launch per iteration stands between the encoder backward and the tail.  No reference counterpart: the
 * reference's batch sizes are its tables (code/train.py:35-45).
 *
 * grad = the step's gradient arena, n elements; k = the position of this micro-batch in its window of `steps`; per element, every
 * operation a separately rounded fp32 operation (never an fma):
 *     steps == 1:          returns 0, launches nothing
 *     k == 0:              acc = grad                          a word copy -- the bits, NaN payloads included; grad is not written
 *     0 < k < steps - 1:   acc = acc + grad                    grad is not written
 *     k == steps - 1:      grad = (acc + grad) * inv_steps     in place in the gradient arena; acc is not written
 * so rd_adam_step, rd_grad_guard + rd_adam_step_guarded and rd_optim_step read the arena they always read.  inv_steps is
 * (float)(1.0 / steps), formed once by the caller; another bit pattern is refused.  ramdsir/accum.py model() is the same arithmetic
 * in numpy.  (The payload of a NaN that an addition PRODUCES -- inf + -inf -- is the hardware's; every other bit is the model's.)
 *
 * Elementwise: no LDS, no atomics, no reduction.  One range, so rd_adam_step's grid-stride form (at most 1024 workgroups of 256
 * threads).  Where grad and acc share a 16-byte phase the part behind the first 16-byte boundary moves with 16-byte accesses and
 * the (at most six) words in front of and behind it one by one; arenas of different phase go word by word throughout.  Every load
 * of a thread's batch is issued before its first store.
 *
 * Returns, before anything is launched: -1 a null grad or acc; -2 a pointer that is not 4-byte aligned; -3 n < 1 (or above
 * RD_ACCUM_MAX_N); -4 steps outside 1..RD_ACCUM_MAX_STEPS; -5 k outside [0, steps); -6 an inv_steps whose bits are not those of
 * (float)(1.0 / steps); -7 [grad, grad + n) and [acc, acc + n) overlap.  Nothing is allocated, synchronised or copied; the launch goes
 * through the library's one launch site. */
#define RD_ACCUM_MAX_STEPS 65536
#define RD_ACCUM_MAX_N (1ll << 40)
int rd_grad_accum(float* grad, float* acc, int64_t n, int32_t k, int32_t steps, float inv_steps, void* stream);

/* Per-tensor histograms (train.py --tb_hist, ramdsir/tb_hist.py), csrc/hist.hip: what TensorBoard's histogram dashboard shows of the
 * four arenas -- one histogram and one statistics record per range of a table, computed where the arenas live.  No reference
 * counterpart: the reference writes scalars and images only (code/train.py:298-329).
 *
 * The table: n <= RD_HIST_MAX_RANGES records {src, count, chunk0} in the convention of csrc/range_walk.h (see rd_snapshot): the same
 * records on the host (read for validation only) and in device memory (uploaded once), range i cut into chunks of RD_HIST_CHUNK
 * ELEMENTS from its start, chunk0 the number of chunks of the ranges in front of it.  src is an absolute device pointer of any
 * 4-byte alignment, so one table spans several arenas; count may be 0.  The limits: n_limits doubles, strictly ascending and finite,
 * 2 <= n_limits <= RD_HIST_MAX_LIMITS, the same values at limits_host (validation) and limits_dev (the kernel): they are data, not
 * code, so the kernel compares against the very doubles the caller's numpy holds.
 *
 * A finite element v falls into bucket b = min(#{i : limits[i] <= (double)v}, n_limits - 1): TensorFlow's upper_bound rule, bucket b
 * has the upper edge limits[b], there are n_limits buckets; the comparison is between the widened float and the double limit, exact,
 * == np.searchsorted(limits, v.astype(float64), side='right') clamped.  Per range i: counts[i][n_limits] (uint32) and stats[i] =
 * {min, max, sum, sum_squares over the finite elements in fp64; num = their number; nonfinite = the number of NaN and +-Inf elements,
 * which enter nothing else}.  An empty range, or one without a finite element, gives all-zero counts and num = min = max = sum =
 * sum_squares = 0.
 *
 * Three launches on `stream`: (1) counts <- 0 (the caller's contents are irrelevant); (2) a flat grid over the chunks of all ranges,
 * one workgroup per chunk: an LDS histogram under integer LDS atomics, its non-empty bins added to counts[i] with uint32 global vector
 * atomics (integer addition: the bits do not depend on the order), the statistics of the chunk -> partial[chunk] without atomics, in
 * an order fixed by the indices; (3) one wave per range adds the partials of its chunks (lane l takes l, l + 64, ... ascending, then
 * the fixed xor tree) -- rd_step_log's decomposition.  ramdsir/tb_hist.py model() is the numpy model: counts, num, nonfinite, min,
 * max equal on any data; sum and sum_squares bit for bit where the sums are exact in fp64, otherwise within the bound of the
 * summation length.  workspace: rd_hist_workspace(total_chunks) bytes, 8-byte aligned, non-null, contents irrelevant before and after.
 *
 * Returns, before anything is launched and without dereferencing a device pointer: -1 a null table / limits / counts / stats /
 * workspace, n outside 1..RD_HIST_MAX_RANGES, or a misaligned pointer (table_dev, limits_dev, stats, workspace 8 bytes, counts 4);
 * -2 n_limits outside 2..RD_HIST_MAX_LIMITS, limits not strictly ascending or not finite; -3 a range with a null or non-4-byte-aligned
 * src, or a count that is negative or above 2^31 - 1; -5 a chunk0 column or total_chunks that does not match the counts.  Nothing is
 * allocated, synchronised or copied; every launch goes through the library's one launch site. */
#define RD_HIST_CHUNK 16384
#define RD_HIST_MAX_LIMITS 4096
#define RD_HIST_MAX_RANGES 4096
typedef struct {
    const float* src;           /* device start of the range (absolute) */
    int64_t count;              /* elements */
    int64_t chunk0;             /* first chunk of the range in the flat grid */
} rd_hist_range_t;
typedef struct {
    double min, max, sum, sum_squares;      /* over the finite elements */
    int64_t num;                /* finite elements */
    int64_t nonfinite;          /* NaN and +-Inf elements */
} rd_hist_stats_t;
int64_t rd_hist_workspace(int64_t total_chunks);
int rd_hist(const rd_hist_range_t* table_host, const rd_hist_range_t* table_dev, int n, int64_t total_chunks,
            const double* limits_host, const double* limits_dev, int n_limits, uint32_t* counts, rd_hist_stats_t* stats,
            void* workspace, void* stream);

/* crc32c (Castagnoli) of n HOST bytes, continuing from `seed` (the crc of the bytes in front; 0 for none) -- the checksum of the
 * TFRecord framing of utils/tfevents.py, whose pure-Python loop runs at about a megabyte per second against image records of hundreds
 * of kilobytes.  Plain table-driven C++ on the host (csrc/crc32c.hip): no GPU involved.  No reference counterpart (tensorboardX's crc32c). */
uint32_t rd_crc32c(const void* data, size_t n, uint32_t seed);

/* Measurement only (bench.py `box`): what this box's GPU sustains on two fixed micro-kernels, so that a bench line can be compared across
 * boxes of a pool whose clocks differ by a few per cent.  No reference counterpart (the reference publishes no throughput: BASELINE.md).
 *   which 0: streaming copy of n bytes (n % 16 == 0) from a to b, 16 B per lane, 8 workgroups of 256 threads per CU;
 *   which 1: n iterations of four independent v_mfma_f32_32x32x16_bf16 per wave, 8 waves on every CU (a: >= 4 bytes of device scratch, b unused):
 *            flops = CUs x 8 x n x 4 x 32768.
 *   which 2: stamps {shader-clock counter, 100 MHz counter} of every compute unit that one of 4096 small workgroups lands on, into
 *            a[2 * unit + 0..1] (2048 units x two 8-byte words, unit = XCC_ID << 8 | SE_ID << 5 | SH_ID << 4 | CU_ID; untouched slots
 *            keep their contents), in stream order (b, n unused): two launches around a stretch of work on one stream give its
 *            average shader clock per unit = 100 MHz x d(a[2u]) / d(a[2u + 1]) (counters of different XCDs are not aligned).
 * The caller times the launch with events on `stream`. */
int rd_box_probe(int which, void* a, void* b, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
