/*
 * bayesnn_fpga_amd.h — C ABI of libbayesnn_fpga_amd.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE path of os-hxfan/BayesNN_FPGA: the Monte-Carlo-dropout /
 * Masksembles multi-exit inference forward pass and its T-sample per-exit moment
 * reduction.  The reference has no FFI of its own: its boundary is the
 * Python API of Software_Artifact/software (abbreviated SA/), so every entry point below
 * cites the reference code it replaces:
 *
 *   bmi_create / bmi_plan      the layer graph that SA/models/resnet18/resnet18.py:260-300
 *                              (ResNet18MCEarlyExit.__init__), :212-244 (ResNet18MC) and
 *                              SA/models/vgg19/vgg19.py:327-382 build as nn.Modules
 *   bmi_forward_mcd            the T-pass loop of FullAnalysis._get_output,
 *                              SA/train/results_analyzer.py:236-246: `for i in range(mc_passes):
 *                              output = self.model(b_x)` + per-exit softmax, i.e. T x
 *                              ResNet18MCEarlyExit.forward (resnet18.py:302-346) with
 *                              MCDropout.forward (:207-210) / Masksembles*.forward
 *                              (SA/utils.py:156-169, :218-231) at every stochastic site
 *   bmi_finalize               np.average over the T passes, results_analyzer.py:247-248, plus
 *                              the build-defined T-sample variance (ddof = 0)
 *   bmi_philox_mask            the RNG primitive under F.dropout (resnet18.py:210), replaced by
 *                              the counter-based Philox convention of csrc/philox.h
 *   bmi_stem_conv_fwd, bmi_conv_igemm_fwd   conv+BN(+residual)(+ReLU) of BasicBlock.forward
 *                              (resnet18.py:32-48) and of the exit heads (:306-308,:318-319,:329)
 *   bmi_mask_apply, bmi_mask_bits   MCDropout / Masksembles2D on a stage output (:278-280)
 *   bmi_head_fused             one exit head end to end: F.avg_pool2d(F.relu(.),4) + flatten + exit dropout (:309-313),
 *                              ex{1,2,3}linear / linear (:314,:325,:335,:344), softmax (results_analyzer.py:242) and
 *                              the accumulation behind np.average over the passes (:247-248)
 *   bmi_dense_f32              hidden Dense layers of the VGG-11 classifier stack (Keras definition, see below)
 *
 * Conventions: plain pointers and sizes only; every function returns 0 or a negative
 * errno-style code (no exceptions cross the ABI); all device buffers are owned by the
 * caller; every launch is asynchronous on the caller's hipStream_t (passed as void*);
 * no allocation or synchronisation happens inside a launch function, so a caller may
 * capture bmi_forward_mcd into a hipGraph.
 *
 * Threading: one host thread per engine handle at a time (a handle carries the state of the call in flight); different handles —
 * one per GPU, or the two / three "batches in flight" of one GPU — may be driven from different threads concurrently.  The
 * kernel-selection switches of bmi_set_option are process DEFAULTS that bmi_create copies into the handle: a live engine is not
 * affected by later bmi_set_option calls from any thread (bmi_engine_set_option edits one engine's copy).
 *
 * Data layout in HBM: activations are NHWC fp16 ([image][y][x][channel]); conv weights
 * fp16 [Cout][ky][kx][Cin]; folded-BN scale/bias fp32 [Cout]; classifier weights fp32
 * [ceil32(C)][K] (rows >= C zero); with bmi_model_desc.dtype = BMI_DTYPE_BF16 "fp16" reads
 * bfloat16 throughout; the network input is fp32 NCHW exactly as the reference
 * receives it; moment accumulators are float64 [E][B][C].
 */
#ifndef BAYESNN_FPGA_AMD_H
#define BAYESNN_FPGA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BMI_VERSION 600

#define BMI_OK 0
#define BMI_ERR_INVALID (-22)      /* EINVAL: bad descriptor / argument            */
#define BMI_ERR_NOMEM (-12)        /* ENOMEM: workspace too small                  */
#define BMI_ERR_HIP (-5)           /* EIO: a HIP runtime call or launch failed     */
#define BMI_ERR_UNSUPPORTED (-95)  /* EOPNOTSUPP: shape outside the kernels' range */

typedef struct bmi_engine_s* bmi_handle;
typedef void* bmi_stream; /* hipStream_t */

/* stochastic-site kinds */
#define BMI_SITE_NONE 0
#define BMI_SITE_ELEMENTWISE 1 /* MCDropout: x * keep / (1-p), one Bernoulli per element      */
#define BMI_SITE_CHANNEL 2     /* dropout2d semantics: one Bernoulli per (image, channel)      */
#define BMI_SITE_MASKSEMBLE 3  /* x * masks[(cnt0 + t) mod M][channel], no rescale             */

#define BMI_SITE_POS_OUTER 0 /* after scale/bias/residual/ReLU (HEAD: on the pooled features) */
#define BMI_SITE_POS_INNER 1 /* between the layer and what follows it (see bmi_op_desc)       */

typedef struct bmi_site {
    int32_t kind;        /* BMI_SITE_*                                                  */
    int32_t site_id;     /* call-order index of the stochastic layer inside one forward */
    float p;             /* drop probability (ELEMENTWISE / CHANNEL)                    */
    int32_t num_masks;   /* MASKSEMBLE: M                                               */
    const float* masks;  /* MASKSEMBLE: device fp32 [M][C] of 0/1                       */
} bmi_site;

/* op kinds */
#define BMI_OP_STEM 1  /* direct conv on the fp32 NCHW network input (Cin <= 4)        */
#define BMI_OP_CONV 2  /* implicit-GEMM conv (Cin % 64 == 0, Cout % 64 == 0)           */
#define BMI_OP_MASK 3  /* stand-alone stochastic site on a tensor                      */
#define BMI_OP_HEAD 4  /* global avg-pool + site + Linear + softmax + moment sums -> exit `out` (Cin % 32 == 0) */
#define BMI_OP_MAXPOOL 5 /* 2x2 stride-2 max-pool                                      */
#define BMI_OP_DENSE 6 /* hidden fully-connected layer on a flattened [1][1][K] tensor, fp32 weights,
                          accumulation and OUTPUT (the tensor `out` is then fp32 in the workspace and may
                          only feed another DENSE or a HEAD): out = relu?(in . weight^T + bias) (site)   */

typedef struct bmi_tensor_desc {
    int32_t h, w, c; /* per-image NHWC extent; tensor 0 is the network input */
} bmi_tensor_desc;

typedef struct bmi_op_desc {
    int32_t kind;
    int32_t in;        /* input tensor id                                              */
    int32_t out;       /* output tensor id; HEAD: exit index                           */
    int32_t residual;  /* CONV: tensor added before the ReLU, or -1                    */
    int32_t in2;       /* CONV 3x3 stride-1: input of a fused 1x1 strided shortcut conv (the BasicBlock
                          downsample path, resnet18.py:42-45) whose result is added before the ReLU, or -1.
                          With in2 both BN scales must be folded into the fp16 weights (scale = NULL)
                          and `bias` is the sum of the two BN biases.  Split engines only: `scale` may carry
                          one per-channel factor common to both weight sets (the host's power-of-two lift). */
    int32_t ksize, stride, pad;
    int32_t relu;      /* apply ReLU after scale/bias(+residual)                       */
    const void* weight;  /* device; CONV fp16 [Cout][k][k][Cin]; STEM fp32 [Cout][k][k][Cin];
                            HEAD fp32 [ceil32(out_dim)][Cin]; DENSE fp32 [Cout][Cin]   */
    const void* weight2;       /* CONV with in2: device fp16 [Cout][Cin2] (BN scale folded in)          */
    const float* scale;  /* device fp32 [Cout] folded BN scale (NULL = 1)              */
    const float* bias;   /* device fp32 [Cout] folded BN bias / Linear bias            */
    bmi_site site;       /* CONV/STEM/MASK: applied to the op's output; HEAD: applied to
                            the pooled features before the Linear                      */
    /* "inner" sites — the converter/pytorch insertion rule (Hardware_Artifact/converter/pytorch/nn2bnn.py:32-45,
     * Dropouts.py:25-56) wraps the layer itself, so the mask lands BEFORE a following BatchNorm / on the logits:
     *   CONV/STEM/MASK, site_pos = BMI_SITE_POS_INNER:
     *       out = relu?( (conv * scale + bias) * mask + bias_post (+ residual) )
     *       (scale/bias: the BN scale and scale * conv.bias; bias_post: the BN shift; no outer site then)
     *   HEAD, site_pos = BMI_SITE_POS_INNER: logits = (Linear(pool(x))) * mask  (dropout after the last layer) */
    const float* bias_post; /* device fp32 [Cout] or NULL (only read with BMI_SITE_POS_INNER)      */
    int32_t site_pos;       /* BMI_SITE_POS_*                                                      */
} bmi_op_desc;

/* element type of the 16-bit activations and conv weights of an engine */
#define BMI_DTYPE_F16 0  /* IEEE half: v_mfma_f32_*_f16 (default; meets the 1e-3 parity bar)            */
#define BMI_DTYPE_BF16 1 /* bfloat16:  v_mfma_f32_16x16x32_bf16 (8 mantissa bits: measured error in DESIGN.md) */
#define BMI_DTYPE_F32 2  /* the EXACT engine, for parity: fp32 activations in the workspace, fp32 conv weights (`weight`
                            fp32 [Cout][k][k][Cin]), every conv on v_mfma_f32_32x32x2_f32 in one generic per-tap kernel
                            (csrc/conv_exact.hip) — the arithmetic of the reference's fp32 CPU path, 1/16 of the fp16 MFMA
                            rate.  Graph features that exist for speed only are not built (in2 is BMI_ERR_UNSUPPORTED; no
                            pair / pooling / lazy-site fusion); bmi_forward_mcd_exit is BMI_ERR_UNSUPPORTED.              */

#define BMI_DTYPE_F16X2 3  /* the SPLIT engines, parity at speed (csrc/conv_split.hip): every conv operand a 16-bit head + tail pair, v = hi + lo
                             (hi = rn16(v), lo = rn16(v - hi)) — `weight` is 16-bit [2][Cout][k][k][Cin], plane 0 = the heads, plane 1 = the
                             tails, split ONCE by the host; the activations live in the workspace in the same form ("pair32": per pixel,
                             32-channel blocks [hi x 32 | lo x 32], 4 bytes per element: csrc/conv_epilogue.h), encoded once by the
                             kernel that produces a tensor — and
                             w.x = w_lo.x_hi + w_hi.x_lo + w_hi.x_hi on v_mfma_f32_32x32x16_f16 (fp32 accumulate; lo.lo dropped): three MFMAs
                             per K-step instead of the exact engine's sixteen.  Precision of an operand: 22 significant bits while its tail is a
                             NORMAL fp16 number, i.e. |v| >= 2^-3; below that the tail is an fp16 subnormal (ulp 2^-24) and the operand carries
                             an ABSOLUTE error floor of ~2^-25 = 3e-8 (|v| = 1e-3: ~15 bits; |v| < 6e-8 is lost).  For WEIGHTS the host removes
                             the floor: bayesnn_fpga_amd/engine.py splits each output channel's weights after an exact power-of-two scale that
                             brings max|w| of the channel to [2^7, 2^8) and folds 2^-k into the channel's BN scale (exact); activations are
                             O(1) behind BatchNorm and keep the floor.  The reference's fp32 arithmetic to ~1e-6 where plain fp16 is at
                             1e-4..2e-3 (peaky logits of trained / converted nets, Hardware_Artifact/converter/pytorch/nn2bnn.py:32-45 on
                             SA/models/vgg19/vgg19.py:256-324).  |values| < 65504.
                             Graph support: what the 16-bit engines take, bmi_forward_mcd_exit included (row tables in conv_split) — in2 (the fused 1x1 shortcut) of any conv geometry with Cin2 % 32 == 0 (extra
                             K-steps of the same kernel), pair launches and split-K are taken; channel counts Cin % 32 == 0, Cout % 64 == 0;
                             no lazy first site, no pooled epilogue (the tensors are materialised).                                     */
#define BMI_DTYPE_BF16X3 4 /* the same on v_mfma_f32_32x32x16_bf16: bf16 head + tail (16 significant bits, fp32's exponent range), three
                             bf16 MFMAs per K-step — BASELINE configs[1] ("bf16") inside north_star's 1e-3 on the bf16 matrix pipe      */

typedef struct bmi_model_desc {
    int32_t n_tensors;
    const bmi_tensor_desc* tensors;
    int32_t n_ops;
    const bmi_op_desc* ops;
    int32_t n_exits;
    int32_t out_dim;
    int32_t dtype; /* BMI_DTYPE_*: conv weights (`weight`, `weight2`) must be in this type (F32: fp32; F16X2 / BF16X3: 16-bit head
                      and tail planes [2][Cout][k][k][Cin]) */
} bmi_model_desc;

/* per-op-kind device time, filled by bmi_profile_read */
#define BMI_PROFILE_SLOTS 8 /* index = BMI_OP_* (the exit heads' slot includes the moment sums) */
#define BMI_PROFILE_ENSEMBLE 7 /* the ensemble.hip launches of bmi_forward_mcd_adaptive_ensemble / bmi_forward_mcd_exit_staged_ensemble */

int bmi_version(void);
const char* bmi_error_string(int code);

/* Process-wide switches: kernel selection (used for same-process A/B measurement and by the tests to cover both code
 * paths) and the element type of the unit-test entry points.  Results are equal TO ROUNDING across them, not always bit for
 * bit: "mfma_shape_*", "epilogue_lite", "conv_seam", "split_tile" and "split_shx" leave every bit alone; "conv_pw", "conv_s2", "conv_stream" and "conv_wide" move a
 * conv to a kernel family that sums its K dimension in another order, "splitk" adds nine fp32 partial sums separately,
 * "dense_exact" swaps the split-fp16 product for the exact-f32 MFMA.  (Kernel selection itself looks at the conv's shape
 * and the engine's planned batch x chunk only, so two runs of one engine — whole, t-sharded, image-sharded, partial chunks —
 * agree bit for bit: the float64 moment sums of an image's 32-sample groups are joined in group order.)  Returns BMI_ERR_INVALID for an unknown
 * name / value.  Names:
 *   "mfma_shape_patch", "mfma_shape_wide"   16 | 32: MFMA instruction shape of conv3x3_patch / conv_igemm_wide
 *                                           (v_mfma_f32_16x16x32_f16 | v_mfma_f32_32x32x16_f16); 0 = built-in default
 *   "xcd_split"                             0 | 1 | 2 | 4: channel-tile classes of the XCD-aware tile order (0 = chosen from
 *                                           the conv's weight bytes so that one XCD's weights stay L2-resident)
 *   "conv_pw"                               0 | 1 | 2 (= 1 without the minimum-grid rule: tests): 3x3 stride-1 convs on 8x8 / 4x4 maps with Cout % 256 == 0 run in conv3x3_pw (256 x 256
 *                                           tile, 8 waves) instead of conv3x3_patch (128 x 128, 2 workgroups per CU); 3 | 4 (= 1 | 2 with the four-wave,
 *                                           software-pipelined conv3x3_pw4 where it applies: measurement reference, the same bits)
 *   "conv_stream"                           0 | 1 | 2 (= 1 without the minimum-grid rule and for plain launches too: tests) | 3 (= 1 with the
 *                                           256-pixel tile: A/B): HBM-bound 1x1 convs (Cin <= 512; with a residual, or Cout % 256 != 0) run
 *                                           in conv1x1_stream (128 x 128 tile, three or four workgroups per CU) instead of conv_igemm_wide
 *   "split_shx"                             0 | 1: the split engines' 3x3 stride-1 convs fetch the pixel tile of a tap row once for its three taps (the same
 *                                           bits; 0: once per tap)
 *   "split_tile"                            0 | 1: the split engines' conv kernel narrows its channel tile (256 -> 128 -> 64) while a launch of the planned
 *                                           batch x chunk would be fewer than two workgroups per CU (the same bits; 0: always the widest tile)
 *   "conv_seam"                             0 | 1 | 2 | 3, read by bmi_create and per launch: conv3 + BN + shortcut add + ReLU of one Bottleneck and conv1 + BN +
 *                                           ReLU of the next (128 narrow channels; 2 | 3: 256 too, no minimum grid — tests; 3: the unpipelined loop) run
 *                                           as one conv1x1_seam launch, the wide tensor fed to the second conv from LDS; 0: the two launches
 *   "conv_s2"                               0 | 1 | 2 (= 1 without the minimum-grid rule: tests): 3x3 stride-2 convs with a BN + ReLU epilogue on
 *                                           32x32 / 16x16 / 8x8 maps with Cout % 256 == 0 (a pair's channels together) run in conv3x3_s2 (input
 *                                           patch resident in LDS as four parity planes, persistent) instead of conv_igemm_wide
 *   "conv_pool"                             0 | 1 | 2: a 3x3 conv whose 4x4 output map feeds one exit head and nothing else writes fp32 means over the
 *                                           map (ReLU + avg_pool2d(4) fused into the epilogue) instead of the map: the plain stride-2 convs in
 *                                           conv3x3_s2 (1, 2) and the stride-1 conv in front of the final head in conv3x3_pw (1)
 *   "mask_lazy"                             0 | 1: the elementwise site that expands the once-per-batch prefix (32x32 maps) to the folded batch writes
 *                                           keep bits + one scaled copy of the B images; conv3x3_s2 / conv3x3_patch (fused shortcut input) clear the
 *                                           dropped elements in LDS, any other consumer makes the masked tensor appear first (1, default), or the
 *                                           masked tensor is always written (0); the same bits either way
 *   "pw_persist"                            0 | 1: plain-epilogue launches of conv3x3_pw (BN + ReLU, with or without the fused shortcut) run in its
 *                                           persistent form — one workgroup per CU walks the tiles, the last chunk of a tile prefetches the next tile's
 *                                           first weight stages and sub-patch, the epilogue stages through 64 KB beside them (1, default: -3..-5 % per
 *                                           launch) — or one workgroup per tile (0); the same bits either way
 *   "pw_pad_skip"                           0 | 1: conv3x3_pw on 4x4 maps takes an MFMA pixel tile to be ONE output position across the tile's 16 images,
 *                                           so a (position, tap) pair that reads the zero-padding ring is a whole tile that is neither fetched, read
 *                                           nor multiplied (1, default), or a 4 x 4 block of one image with the ring in LDS (0); the same bits either way
 *   "pw_pad_skip8"                          0 | 1: the same on 8x8 maps, persistent conv3x3_pw launches only: a workgroup tile is 16 images x one 4x4
 *                                           quadrant of the map, its sub-patch the quadrant's 5 x 5 real input cells (1, default), or four whole
 *                                           images in 4 x 4 blocks with the ring in LDS (0); the same bits either way
 *   "s2_pad_skip"                           0 | 1: the same for conv3x3_s2 on 8x8 -> 4x4 maps (plain, pair and pooled launches; row-table launches keep
 *                                           the 4 x 4 blocks): the parity planes keep their size and refill schedule, a plane's cells are stored
 *                                           position-major with the image fastest, and the 23 of 144 (position, tap) pairs that read only the
 *                                           padding row / column are never read or multiplied (1, default), or 4 x 4 blocks of one image (0); the
 *                                           same bits either way
 *   "lazy_planar"                           0 | 1: a lazy site whose readers are all stride-2 consumers (conv3x3_s2 on 32x32 maps, the fused 1x1
 *                                           stride-2 shortcut of conv3x3_patch) stores its scaled copy and keep bits as 32-channel planes with
 *                                           the even columns of a row in front of the odd ones — what such a reader DMAs is then contiguous,
 *                                           whole 128-byte lines (1, default) — or in NHWC (0); the same bits either way
 *   "conv_wide"                             0 | 1: 0 skips conv_igemm_wide (A/B against the per-tap kernel)
 *   "splitk"                                0 | 1, read by bmi_plan: 3x3 convs of the once-per-batch prefix whose grid is <= 64 tiles (VGG's convs on
 *                                           2x2 maps) run split-K: one workgroup per (tile, tap), fp32 partial sums, a finishing pass
 *   "dense_exact"                           0 | 1: hidden dense layers (BMI_OP_DENSE / bmi_dense_f32) on the exact-f32 MFMA (1) or as
 *                                           fp16 head + tail products on the fp16 MFMA with fp32 accumulation (0, default: fp32-equivalent
 *                                           to a few 1e-7, 2.5x faster)
 *   "lazy_order"                            0 | 1: the kernels that read a deterministic tensor through a lazy site's keep bits walk their
 *                                           tiles sample-minor — the samples of one activation tile back to back on one XCD, which finds it
 *                                           in its L2 (1, default) — or in the plain order (0).  Placement only: the same bits
 *   "epilogue_lite"                         0 | 1 | 2: BN + residual + ReLU + 2-bit elementwise-site launches finish on the accumulator
 *                                           registers with one fp16 trip through LDS (1, default; 2: without the forms that have the
 *                                           site kind and the residual compiled in) or in the general two-round fp32 epilogue (0);
 *                                           the same bits every way
 *   "wide_persist_min_x10"                  10..1000: conv_igemm_wide runs persistent (one workgroup per CU walking the tiles)
 *                                           when tiles * 10 > value * CUs
 *   "unit_entry_dtype"                      BMI_DTYPE_*: how the single-kernel entry points below (unit tests) interpret
 *                                           their 16-bit buffers; engines carry their own dtype in bmi_model_desc.  BMI_DTYPE_F32:
 *                                           bmi_conv_igemm_fwd / bmi_stem_conv_fwd (output) / bmi_mask_apply / bmi_maxpool2 take fp32
 *                                           buffers (and fp32 conv weights) and run the exact engine's kernels; BMI_DTYPE_F16X2 / BF16X3: the
 *                                           activation buffers of those entry points (and of bmi_head_fused / bmi_dense_f32 with in_is_f32 = 0)
 *                                           are pair32 tensors, bmi_conv_igemm_fwd takes the 16-bit head / tail weight planes and runs conv_split
 *   "ws_no_reuse"                           0 | 1, read by bmi_plan: every suffix tensor keeps its own workspace range (per-layer
 *                                           traces through bmi_tensor_info; the workspace grows to the sum of the activations)
 *   "conv_patch64"                          0 | 1: 3x3 stride-1 convs with Cout % 128 == 64 on 32-wide maps (the 64 -> 64 BasicBlocks behind the stem) run in
 *                                           conv3x3_patch's 64-channel tile (1, default) or in the per-tap conv_igemm (0); another K order (64- vs
 *                                           32-channel chunks): equal to rounding
 *   "splitk_tiles"                          0..1024, read by bmi_plan: the largest grid (128 x 128 tiles at the planned batch) of a deterministic 3x3 conv
 *                                           with Cin >= 256 that still runs split-K (default 64: a quarter of the CUs)
 *   "pair_prefix"                           0 | 1, read by bmi_create: pair fusion (two plain convs on one input as one launch) also in the once-per-batch
 *                                           prefix (1, default: the exit-only step +3 %, profiles/experiments/r6_exit_only_variants.txt) or in the suffix only (0)
 *   "patch_direct"                          0 | 1 | 2: conv3x3_patch's BasicBlock tails on 16x16 maps (residual, residual + 2-bit site) finish on the accumulator
 *                                           registers and store straight to HBM (1, default; 2: its plain launches too — measured slower in the network) or
 *                                           take the epilogues through LDS (0).  The same bits every way
 *   "head_batch"                            0 | 1: consecutive exit heads of the sample-folded suffix run as ONE launch (1, default) — with exit-only
 *                                           dropout, the configuration of every run of the paper (journal_script.sh:10-63), the suffix is nothing but
 *                                           the four / five heads — or one launch per head (0).  The same bits either way
 * Initial values come from the environment (BMI_MFMA_SHAPE, BMI_MFMA_SHAPE_WIDE, BMI_XCD_SPLIT).
 *
 * SCOPE (C-ABI 600).  bmi_set_option edits the PROCESS DEFAULTS: what the single-kernel entry points read, and what bmi_create COPIES into
 * the handle it returns.  An engine runs every later call (bmi_plan, bmi_forward_*) under its own copy, so a live engine never changes
 * kernels because another host thread (see "Threading" at the top) changed a default; bmi_engine_set_option edits the copy
 * of ONE engine (same names and ranges; switches read by bmi_create / bmi_plan take effect at the next bmi_plan at the latest, the
 * graph-merging one — "conv_seam" — only at launch time: an op merged at bmi_create falls back to its two launches). */
int bmi_set_option(const char* name, int32_t value);
int bmi_engine_set_option(bmi_handle h, const char* name, int32_t value);

/* Host-only: validates and copies the graph, marks which tensors are stochastic, splits a
 * conv that carries a site but has only deterministic inputs into conv + MASK (so the
 * deterministic prefix runs once per batch).  No HIP call. */
int bmi_create(const bmi_model_desc* desc, bmi_handle* out);
int bmi_destroy(bmi_handle h);

/* Host-only: lays the activation buffers out for batches of up to `max_batch` images and
 * chunks of up to `chunk_samples` Monte-Carlo samples folded into the GEMM M dimension. */
int bmi_plan(bmi_handle h, int32_t max_batch, int32_t chunk_samples, size_t* workspace_bytes);

/* MACs (conv + linear) per image of the deterministic prefix and per (image, sample) of the
 * stochastic suffix; and the op counts after the split. */
int bmi_query(bmi_handle h, int64_t* prefix_macs, int64_t* suffix_macs, int32_t* n_prefix_ops, int32_t* n_suffix_ops);

/* Traces (tools/layer_trace.py): where tensor `id` (1 .. n_tensors-1 of the descriptor) of a PLANNED engine lives in the caller's
 * workspace: byte offset, bytes per element (2: the engine's 16-bit type, 4: fp32 or pair32), per_sample bit 0: it holds one image set per
 * Monte-Carlo sample of the chunk ([chunk*B][h][w][c], image = t_local*B + b) rather than the once-per-batch B images; bit 1: the tensor
 * is in the split engines' pair32 layout (per pixel, 32-channel blocks of 32 heads + 32 tails, 16-bit each); and its extent.
 * Suffix tensors share workspace ranges by live range unless the engine was planned under bmi_set_option("ws_no_reuse", 1);
 * a fused launch may leave a tensor unwritten (set "mask_lazy" = 0, "conv_pool" = 0 for a full trace).  Keep-bit tensors and
 * tensors nothing reads are BMI_ERR_UNSUPPORTED.  No reference counterpart (a forward hook on an nn.Module). */
int bmi_tensor_info(bmi_handle h, int32_t id, int64_t* offset, int32_t* elem_bytes, int32_t* per_sample, int32_t* th, int32_t* tw,
                    int32_t* tc);

/* Runs samples t_begin .. t_begin+t_count-1 for one batch and ADDS, per exit e, image b and
 * class c:  S1 += softmax_p, S2 += softmax_p^2, SL += logit   (float64 [E][B][C]). */
int bmi_forward_mcd(bmi_handle h, const float* x_nchw, int32_t batch, int32_t t_begin, int32_t t_count,
                    uint64_t seed, int32_t mask_cnt0, double* S1, double* S2, double* SL, void* workspace,
                    size_t workspace_bytes, bmi_stream stream);

/* The same for images image_offset .. image_offset+batch-1 of a LARGER batch: `x_nchw` and S1/S2/SL hold this share only
 * ([batch] rows), while every dropout mask is drawn at the image's index in the whole batch — so the shares of a batch
 * partitioned by IMAGES over several GPUs (the fallback of SURVEY.md §8.5 when there are fewer Monte-Carlo samples than
 * ranks: every rank runs all T samples on its images, nobody idles) reproduce the rows of the one-GPU run bit for bit when
 * the engine is planned for the whole batch (kernel selection looks at the planned batch, not at the call's).
 * A site's index offset must be a whole number of Philox calls (image_offset x elements per image % 64 == 0: true for every
 * tensor of the CNN families here), else BMI_ERR_UNSUPPORTED — bmi_image_offset_ok (host-only) tells beforehand, so that the
 * ranks of a group can refuse a partition TOGETHER instead of one rank failing while the others wait in the all-reduce.
 * Masksembles masks do not depend on the image.  No reference counterpart (single device: SA/train/train_utils.py:10-11). */
int bmi_image_offset_ok(bmi_handle h, int32_t image_offset);
int bmi_forward_mcd_images(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_begin,
                           int32_t t_count, uint64_t seed, int32_t mask_cnt0, double* S1, double* S2, double* SL,
                           void* workspace, size_t workspace_bytes, bmi_stream stream);

/* Per-sample outputs of the folded path — what the reference's evaluate() consumes pass by pass (SA/train/evaluate.py:8-22 ->
 * SA/train/train_utils.py:32-38 -> _MultiExitAccuracy._metrics, SA/train/loss/base_classes.py:39-66: the logits of every exit of every
 * stochastic forward): samples t_begin .. t_begin+t_count-1 of the batch as in bmi_forward_mcd, and
 *     logits[(t - t_begin)][e][b][c]   fp32 [t_count][E][batch][C]
 * written by the fused head kernel beside the moment sums (S1 / S2 / SL as in bmi_forward_mcd), or instead of them (all three NULL).
 * mask_stride: the Masksembles mask of sample t is (mask_cnt0 + (t - t_begin) * mask_stride) mod M — the reference's layers count
 * their forward calls (SA/utils.py:165-169), so when its evaluate() walks a loader of n batches T times, pass i of batch k is call
 * i * n + k: the T passes of batch k folded into ONE call here take mask_cnt0 = cnt + k, mask_stride = n.  mask_cnt0 is the mask of the
 * call's FIRST sample whatever t_begin (mask_stride = 1 and t_begin = 0: the masks of bmi_forward_mcd, which indexes (mask_cnt0 + t) mod M
 * with the global sample index t).  MC-dropout masks depend on the sample index t alone, as everywhere.  Captures into a hipGraph like
 * bmi_forward_mcd. */
int bmi_forward_mcd_samples(bmi_handle h, const float* x_nchw, int32_t batch, int32_t t_begin, int32_t t_count, uint64_t seed,
                            int32_t mask_cnt0, int32_t mask_stride, float* logits, double* S1, double* S2, double* SL, void* workspace,
                            size_t workspace_bytes, bmi_stream stream);

/* Uncertainty decomposition of the folded path: bmi_forward_mcd_images (same arguments, same S1 / S2 / SL, the same bits in them), and
 * the fused head also ADDS the softmax entropy of every sample it evaluates into the float64 [E][batch] buffer SH:
 *     SH[e][b] += sum_t H(softmax(logits_t[e][b])),   H(p) = -sum_c p_c log p_c in nats,
 * computed per sample where the softmax is (never stored) in log-softmax form, log(sum) - sum_c p_c (l_c - max): no log of an underflowed
 * probability.  Per-sample values do not depend on the chunking; the float64 sums join in group order like S1's.  SH of a share
 * (image_offset) covers rows 0 .. batch-1 of that share.  With bmi_finalize_uncertainty it gives the expected entropy E_t H[p_t] (the
 * aleatoric part) and the mutual information H[p_mean] - E_t H[p_t] (the epistemic part, "BALD") that MC dropout and Masksembles exist to
 * produce; the paper's hardware evaluation reports the predictive entropy H[p_mean] of random-noise inputs as aPE
 * (Hardware_Artifact/bayes_hw/metric_utils.py:3-6, used at hls4ml_pred.py:86-119 on the inputs of data_utils.py:73-88).
 * No allocation and no synchronisation: captures into a hipGraph like bmi_forward_mcd. */
int bmi_forward_mcd_entropy(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_begin,
                            int32_t t_count, uint64_t seed, int32_t mask_cnt0, double* S1, double* S2, double* SL, double* SH,
                            void* workspace, size_t workspace_bytes, bmi_stream stream);

/* The exit ensemble as a predictor of its own.  What the paper ships is the mean of the softmax outputs of exits 0..e; the reference forms
 * it from the T-mean probabilities (FullAnalysis._get_output, SA/train/results_analyzer.py:260-269: `ensemble_output_sm`) and per
 * stochastic pass (_MultiExitAccuracy._metrics, SA/train/loss/base_classes.py:41,54,58: `ensemble += softmax(logits)` inside one forward).
 * Its variance and its mutual information need the PER-SAMPLE ensemble: the exits of one pass share the trunk's dropout draw, so
 * E_t[q q] holds cross-exit terms that S1 / S2 do not.  Per sample t, exit e, image b, class c, in float64 from the fp32 per-sample
 * logits l of the fused head (the plane bmi_forward_mcd_samples writes), without fused multiply-adds:
 *     z_te = (double) fl32(l_te * inv_e)        inv_e = float32(1 / tau_e) (bmi_engine_set_temperature), the head's own z; 1 when off
 *     p_te = softmax_c(z_te)                    max-subtracted
 *     q_te = (p_t0 + ... + p_te) / (e + 1)      summed in exit order, divided once
 *     Q1[e][b][c] += q     Q2[e][b][c] += q * q     QH[e][b] += -sum_c q log q   (0 log 0 = 0, class order)
 * Row e = 0 is exit 0 itself.  For every (e, b, c) the samples of a call are added IN SAMPLE ORDER ONTO THE RUNNING SUM (load, add, store;
 * no floating-point atomics): the sums are the same bits however the samples were split into chunks, launches or calls.
 *
 * bmi_forward_mcd_ensemble: bmi_forward_mcd_entropy with the same arguments and the same bits in S1 / S2 / SL / SH; per planned chunk the
 * heads also write their logits into `scratch` (device, bmi_ensemble_scratch_bytes(h, batch) = planned chunk x E x batch x C x 4 bytes;
 * 0 for a handle that is not planned or a batch it does not take) and one launch of ensemble.hip follows the chunk's heads.  Q1 / Q2
 * [E][batch][C] and QH [E][batch] are device float64, ADDED TO like S1; rows 0 .. batch-1 of a share (image_offset).  The planned
 * workspace is that of every other entry point.  BMI_ERR_NOMEM: scratch too small; BMI_ERR_UNSUPPORTED: more than 32 exits, more than
 * 128 classes or n_exits * (C | 1) > 3456.  No allocation and no synchronisation: captures into a hipGraph like bmi_forward_mcd.  Under
 * adaptive sampling and staged early exit: bmi_forward_mcd_adaptive_ensemble and bmi_forward_mcd_exit_staged_ensemble below. */
size_t bmi_ensemble_scratch_bytes(bmi_handle h, int32_t batch);
int bmi_forward_mcd_ensemble(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_begin, int32_t t_count,
                             uint64_t seed, int32_t mask_cnt0, double* S1, double* S2, double* SL, double* SH, double* Q1, double* Q2,
                             double* QH, void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, bmi_stream stream);

/* The same sums from a caller's per-sample logits: device fp32 [T][E][B][C] (bmi_forward_mcd_samples' layout), tau: HOST [E], every entry
 * finite and > 0 (rounded like bmi_engine_set_temperature: inv_e = float32(1.0 / (double)tau_e)), or NULL = ones.  Q1 / Q2 / QH are ADDED
 * TO; two calls on the halves of T leave the bits of one call.  BMI_ERR_UNSUPPORTED (never a wrong number) for a shape the kernel does
 * not take: E > 32, C > 128 or E * (C | 1) > 3456. */
int bmi_ensemble_moments(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const float* tau, double* Q1, double* Q2, double* QH,
                         bmi_stream stream);

/* bmi_ensemble_moments of the WEIGHTED exit ensembles (bmi_engine_set_ensemble_weights states the arithmetic): W_device is device
 * float64 [E][E], row-major, used as given.  BMI_ERR_INVALID for a NULL W_device as well. */
int bmi_ensemble_moments_weighted(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const float* tau, const double* W_device,
                                  double* Q1, double* Q2, double* QH, bmi_stream stream);

/* Per (exit, image) from the sums of t_total samples, float64: ens_mean = Q1 / T and ens_var = max(Q2 / T - ens_mean^2, 0) (ddof 0 like
 * bmi_finalize's var), [E][batch][C]; pred_entropy = H[ens_mean], exp_entropy = QH / T, mutual_info = max(pred - exp, 0), [E][batch]
 * (0 log 0 = 0).  nonfinite (NULL: not counted) as in bmi_finalize_checked: ADDS the number of non-finite Q1 / Q2 / QH inputs. */
int bmi_finalize_ensemble(int32_t n_exits, int32_t batch, int32_t out_dim, int32_t t_total, const double* Q1, const double* Q2, const double* QH,
                          double* ens_mean, double* ens_var, double* pred_entropy, double* exp_entropy, double* mutual_info, int32_t* nonfinite,
                          bmi_stream stream);

/* bmi_finalize_ensemble with a per-image sample count t_used[b] (device int32 [batch], every entry >= 1) in place of t_total, as
 * bmi_finalize_per_image is to bmi_finalize_checked / bmi_finalize_uncertainty: row (e, b) of every output divides by t_used[b] (the sums of
 * bmi_forward_mcd_adaptive_ensemble). */
int bmi_finalize_ensemble_per_image(int32_t n_exits, int32_t batch, int32_t out_dim, const int32_t* t_used, const double* Q1, const double* Q2,
                                    const double* QH, double* ens_mean, double* ens_var, double* pred_entropy, double* exp_entropy,
                                    double* mutual_info, int32_t* nonfinite, bmi_stream stream);

/* Confidence-threshold early exiting ON the device — what the reference only models after the fact
 * (FullAnalysis.confidence_exiting / is_confident / flop_saver, SA/train/results_analyzer.py:606-630, :638-677, :725-733):
 * runs samples 0 .. t_count-1 of the batch stage by stage; after the head of exit e (first_exit <= e < n_exits-1; the
 * reference's loop starts at exit 1) an image whose confidence max_c mean_t softmax[e][b][c] exceeds `threshold` is
 * assigned exit_of_image[b] = e and takes no part in the later stages: the following launches cover only the still-active
 * images (compact tile grid, tensors keep their original rows, masks keep their original element indices, so every value
 * that IS computed equals the full run's bit for bit).  Images that never pass get n_exits-1.
 * S1/S2/SL [E][batch][C] must be ZERO on entry; on return the rows of exits an image did not reach hold no samples.
 * active_after[e] (host, [n_exits]) = images still active after exit e's test.  Needs t_count <= the planned chunk;
 * synchronises the stream once per tested exit (the host sizes the next stage's grids), so it cannot be graph-captured.
 * Graphs with MASK / MAXPOOL / DENSE ops behind the first tested exit are BMI_ERR_UNSUPPORTED. */
int bmi_forward_mcd_exit(bmi_handle h, const float* x_nchw, int32_t batch, int32_t t_count, uint64_t seed, int32_t mask_cnt0,
                         double threshold, int32_t first_exit, double* S1, double* S2, double* SL, int32_t* exit_of_image,
                         int32_t* active_after, void* workspace, size_t workspace_bytes, bmi_stream stream);

/* Adaptive (sequential) Monte-Carlo sampling with a per-image stopping rule, on the folded path.  The prefix runs once; samples
 * then run in steps of t_step (<= the planned chunk) up to t_max.  After each step the stop rule is tested at exit test_exit on
 * the running sums of every still-active image; images that pass retire with t_used[b] = the samples they got, and later steps
 * cover only the images still active: compact grids, original tensor rows, original mask element indices — so every sample keeps
 * its global index t (Philox counter, Masksembles row (mask_cnt0 + t) mod M) and image b's sums are those of bmi_forward_mcd
 * truncated at t_used[b].  A step in which no image has retired yet runs exactly bmi_forward_mcd's kernels.
 * Rules, float64, with t = samples so far, m = S1/t, v = max(S2/t - m^2, 0), both at test_exit:
 *   BMI_STOP_SEM    (0): stat = max_c sqrt(v_c / t);                                          stop when stat <= threshold
 *   BMI_STOP_MARGIN (1): c1 = argmax m (lowest index on ties), c2 = argmax over c != c1;
 *                        stat = (m_c1 - m_c2) / sqrt((v_c1 + v_c2) / t), +inf when the denominator is 0 and the margin > 0,
 *                        0 when both are 0;                                                    stop when stat >= threshold
 * S1 / S2 / SL [E][batch][C] (and SH [E][batch] when not NULL: per-sample entropies as in bmi_forward_mcd_entropy) must be ZERO on
 * entry; on return every exit's rows of image b hold exactly its first t_used[b] samples.  t_used (device int32 [batch]) is
 * required; converged (device uint8 [batch], NULL: not written) = whether the rule holds at t_used[b] (an image at t_max may or may
 * not pass).  active_after_step (host, [ceil(t_max / t_step)]) = images still active after each step (0 after the last step that
 * ran).  image_offset as in bmi_forward_mcd_images.  Synchronises the stream once per step (the host sizes the next step's
 * grids), so it cannot be graph-captured.  A first MC site that is lazy in the full run is materialised in steps that carry a row
 * table.  BMI_ERR_INVALID: a NULL required pointer, batch / t_max < 1, t_step < 1, mask_cnt0 < 0, an unknown rule, test_exit
 * outside [0, E), batch > max_batch; BMI_ERR_UNSUPPORTED: t_step > the planned chunk, the exact engine (BMI_DTYPE_F32), keep-bit
 * consumers (BMI_MASK_BITS=1) in the suffix. */
#define BMI_STOP_SEM 0
#define BMI_STOP_MARGIN 1
int bmi_forward_mcd_adaptive(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_max,
                             int32_t t_step, uint64_t seed, int32_t mask_cnt0, int32_t rule, double threshold,
                             int32_t test_exit, double* S1, double* S2, double* SL, double* SH, int32_t* t_used,
                             uint8_t* converged, int32_t* active_after_step, void* workspace, size_t workspace_bytes,
                             bmi_stream stream);

/* Adaptive sampling that also keeps the exit-ensemble sums, and can stop on them.  The ensemble is the predictor the paper ships — the
 * reference forms it from the T-mean probabilities (FullAnalysis._get_output, SA/train/results_analyzer.py:260-269: `ensemble_output_sm`)
 * and per stochastic pass (_MultiExitAccuracy._metrics, SA/train/loss/base_classes.py:41,54,58) — and its standard error holds cross-exit
 * covariance that no per-exit sum contains.  bmi_forward_mcd_adaptive with the same arguments plus stop_on, Q1 / Q2 [E][batch][C],
 * QH [E][batch] (device float64, ZERO on entry like S1) and the scratch of bmi_forward_mcd_ensemble (bmi_ensemble_scratch_bytes(h, batch):
 * one step of [t_step][E][batch][C] logits fits, t_step <= the planned chunk).  Per step the heads also write their logits into
 * `scratch` — at the ORIGINAL image row under a row table; rows of retired images are stale and never read — and one launch of
 * ensemble.hip follows them: over every image while none has retired, over the list of active images afterwards (same arithmetic per
 * row, one running sum per (exit, image, class) continued in sample order).  The decision follows that launch.
 *   BMI_STOP_ON_EXIT     (0): the rule reads S1 / S2 at test_exit: t_used, converged, active_after_step, S1 / S2 / SL / SH are
 *                             bmi_forward_mcd_adaptive's bits.
 *   BMI_STOP_ON_ENSEMBLE (1): the SAME rule (BMI_STOP_SEM / BMI_STOP_MARGIN, float64) reads Q1 / Q2 at row test_exit: the sums of the
 *                             ensemble of exits 0..test_exit (row 0 is exit 0 itself).
 * On return image b's rows of Q1 / Q2 / QH, like those of S1, hold exactly its first t_used[b] samples: bmi_forward_mcd_ensemble's bits
 * truncated there (bmi_finalize_ensemble_per_image reads them out).  Errors: bmi_forward_mcd_adaptive's, BMI_ERR_INVALID for a NULL Q1 /
 * Q2 / QH / scratch or an unknown stop_on, BMI_ERR_NOMEM for a scratch too small, BMI_ERR_UNSUPPORTED for a shape ensemble.hip does not
 * take (bmi_forward_mcd_ensemble's list); in every error case nothing is written.  Synchronises once per step. */
#define BMI_STOP_ON_EXIT 0
#define BMI_STOP_ON_ENSEMBLE 1
int bmi_forward_mcd_adaptive_ensemble(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_max, int32_t t_step,
                                      uint64_t seed, int32_t mask_cnt0, int32_t rule, double threshold, int32_t test_exit, int32_t stop_on,
                                      double* S1, double* S2, double* SL, double* SH, double* Q1, double* Q2, double* QH, void* scratch,
                                      size_t scratch_bytes, int32_t* t_used, uint8_t* converged, int32_t* active_after_step, void* workspace,
                                      size_t workspace_bytes, bmi_stream stream);

/* Adaptive sampling that also keeps the vote counts (see bmi_vote_counts below), and can stop on them.  bmi_forward_mcd_adaptive_ensemble
 * with the same arguments plus V (device int32 [2][E][batch][C], ZERO on entry) and nonfinite (device int32, ADDED to; NULL: not counted).
 * Per step one launch of votes_rows.hip follows the ensemble launch on the same scratch, under the handle's calibration map and ensemble
 * weights: over every image while none has retired, over the list of active images afterwards.  On return image b's rows of V hold exactly
 * the votes of its first t_used[b] samples — bmi_forward_mcd_votes' counts truncated there — and S1 / S2 / SL / SH / Q1 / Q2 / QH hold
 * bmi_forward_mcd_adaptive_ensemble's bits.  With BMI_STOP_SEM / BMI_STOP_MARGIN the decisions are bmi_forward_mcd_adaptive_ensemble's, bit
 * for bit.  This entry point alone also takes
 *   BMI_STOP_VOTES (2): integer arithmetic on row test_exit of V[0] (stop_on = BMI_STOP_ON_EXIT: the exit's votes) or of V[1]
 *                       (BMI_STOP_ON_ENSEMBLE: the votes of the ensemble of exits 0..test_exit).  With t = samples so far,
 *                           c1   = the lowest class with the largest count
 *                           lead = min over c != c1 of (V[c1] - V[c] - (c < c1 ? 1 : 0)), INT32_MAX when C == 1
 *                           r    = max(0, t_max - t - slack),  slack = threshold: a whole number >= 0 (at most INT32_MAX)
 *                       stop when lead >= r.  A class below c1 wins a tie (the lowest index), hence the 1.  With slack = 0 no class can
 *                       reach the leader in the t_max - t samples still to come, whatever they vote: vote_class at the tested row is
 *                       EXACTLY that of the full t_max run (a pass casts at most one vote).  slack > 0 stops earlier and gives the
 *                       guarantee up.  r = 0 at t_max, so converged is 1 for every image under this rule.
 * The vote launches are not recorded in the profile table (it has no free slot; bmi_forward_mcd_votes' are not either).
 * Errors: bmi_forward_mcd_adaptive_ensemble's, BMI_ERR_INVALID for a NULL V, a rule outside 0..2, BMI_STOP_VOTES with a threshold that is
 * negative, fractional, not finite or above INT32_MAX; BMI_ERR_UNSUPPORTED for a shape votes.hip does not take (bmi_forward_mcd_votes'
 * list); in every error case nothing is written.  Synchronises once per step. */
#define BMI_STOP_VOTES 2
int bmi_forward_mcd_adaptive_votes(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_max, int32_t t_step,
                                   uint64_t seed, int32_t mask_cnt0, int32_t rule, double threshold, int32_t test_exit, int32_t stop_on,
                                   double* S1, double* S2, double* SL, double* SH, double* Q1, double* Q2, double* QH, int32_t* V,
                                   int32_t* nonfinite, void* scratch, size_t scratch_bytes, int32_t* t_used, uint8_t* converged,
                                   int32_t* active_after_step, void* workspace, size_t workspace_bytes, bmi_stream stream);

/* Early exit by stages that also skips the deterministic trunk (the paper's exit-only dropout: every trunk and exit-branch conv is in
 * the once-per-batch prefix).  Every op, prefix and suffix, has a stage: the smallest exit index of any head downstream of its outputs
 * (a pair- or seam-fused op: the smaller of its two members'); stages <= rule->first_exit fold into stage 0.  Stage 0 runs on the whole
 * batch exactly as bmi_forward_mcd would; after stage k the rule is tested at exit e = first_exit + k (e < n_exits-1) on the device, and
 * stage k+1 runs on the images still active only: its prefix ops once over the Bc active images (one row-table entry per image), its
 * suffix ops over t_count x Bc rows.  Tensors keep their original rows and masks their original element indices, and a launch under a
 * row table takes the full run's kernel, so every row that is computed equals bmi_forward_mcd's (same seed, mask_cnt0) bit for bit:
 * S1 / S2 / SL, and SH when not NULL (as bmi_forward_mcd_entropy).  Split-K launches (conv_igemm, conv_split) and the pooled epilogues run
 * compacted; a prefix op whose full-run kernel has no row-table form (a 1x1 conv that conv1x1_stream takes at the planned batch) runs
 * over the whole batch, and bmi_query_exit_stages reports those ops.
 * The rule, float64 on the active images' sums at exit e, p_c = S1[e][b][c] / t_count, or with ensemble = 1
 * p_c = (sum_{e'=0..e} S1[e'][b][c] / t_count) / (e + 1), summed in exit order (the reference's exit ensembles):
 *   BMI_EXIT_CONFIDENCE (0): stat = max_c p_c          (is_confident)
 *   BMI_EXIT_MARGIN     (1): stat = p_(1) - p_(2)      (top-1 minus top-2: confident(diff=True))
 * an image leaves when stat > threshold: exit_of_image[b] = e (device int32 [batch]); images that never leave get n_exits-1.
 * S1 / S2 / SL [E][batch][C] (and SH [E][batch]) must be ZERO on entry; rows of exits an image never reached stay zero.
 * active_after[e] (host, [n_exits]) = images still active after exit e's test (exits before first_exit and the last: the images that
 * ran it; 0 for exits nobody reached).  Synchronises the stream once per decision (the host sizes the next stage's grids), so it cannot
 * be graph-captured.  BMI_ERR_INVALID: a NULL required pointer, an unknown criterion, ensemble not 0 / 1, a NaN threshold, first_exit
 * outside [0, E), batch / t_count < 1, mask_cnt0 < 0, batch > max_batch; BMI_ERR_UNSUPPORTED: t_count > the planned chunk, the exact
 * engine (BMI_DTYPE_F32), keep-bit consumers (BMI_MASK_BITS=1) behind a decision, a staged suffix order that the workspace packing
 * cannot hold (never seen on the bundled models). */
#define BMI_EXIT_CONFIDENCE 0
#define BMI_EXIT_MARGIN 1
typedef struct bmi_exit_rule {
    int32_t criterion;   /* BMI_EXIT_* */
    int32_t ensemble;    /* 1: the mean of exits 0..e decides */
    double threshold;
    int32_t first_exit;  /* the first exit tested */
} bmi_exit_rule;
int bmi_forward_mcd_exit_staged(bmi_handle h, const float* x_nchw, int32_t batch, int32_t t_count, uint64_t seed, int32_t mask_cnt0,
                                const bmi_exit_rule* rule, double* S1, double* S2, double* SL, double* SH, int32_t* exit_of_image,
                                int32_t* active_after, void* workspace, size_t workspace_bytes, bmi_stream stream);

/* Staged early exit that also keeps the exit-ensemble sums of the exits every image reached (the per-pass ensemble of
 * _MultiExitAccuracy._metrics, SA/train/loss/base_classes.py:41,54,58; FullAnalysis._get_output, SA/train/results_analyzer.py:260-269).
 * bmi_forward_mcd_exit_staged with the same arguments — the rule is NOT changed: its ensemble = 1 stays the mean of the T-means — plus
 * Q1 / Q2 [E][batch][C], QH [E][batch] (device float64, ZERO on entry) and the scratch of bmi_forward_mcd_ensemble
 * (bmi_ensemble_scratch_bytes(h, batch); t_count <= the planned chunk).  Every stage's heads also write their logits into the one
 * [t_count][E][batch][C] scratch, active images only; behind the last stage that ran — also when every image has left early — ONE launch
 * of ensemble.hip walks all images with n_e[b] = exit_of_image[b] + 1 exits each: the running exit sum is cut there, so rows
 * e <= exit_of_image[b] of Q1 / Q2 / QH are bmi_forward_mcd_ensemble's (samples 0 .. t_count-1) bit for bit, and rows of exits an image
 * never reached stay zero, like S1's.  S1 / S2 / SL / SH, exit_of_image and active_after are bmi_forward_mcd_exit_staged's bits.
 * Errors: bmi_forward_mcd_exit_staged's, BMI_ERR_INVALID for a NULL Q1 / Q2 / QH / scratch, BMI_ERR_NOMEM for a scratch too small,
 * BMI_ERR_UNSUPPORTED for a shape ensemble.hip does not take; in every error case nothing is written. */
int bmi_forward_mcd_exit_staged_ensemble(bmi_handle h, const float* x_nchw, int32_t batch, int32_t t_count, uint64_t seed, int32_t mask_cnt0,
                                         const bmi_exit_rule* rule, double* S1, double* S2, double* SL, double* SH, double* Q1, double* Q2,
                                         double* QH, void* scratch, size_t scratch_bytes, int32_t* exit_of_image, int32_t* active_after,
                                         void* workspace, size_t workspace_bytes, bmi_stream stream);

/* Staged early exit that also keeps the vote counts of the exits every image reached.  bmi_forward_mcd_exit_staged_ensemble with the same
 * arguments — the exit rule is NOT changed: there is no vote-based exit rule — plus V (device int32 [2][E][batch][C], ZERO on entry) and
 * nonfinite (device int32, ADDED to; NULL: not counted).  Behind the one ensemble launch, one launch of votes_rows.hip walks all images
 * with the same n_e[b] = exit_of_image[b] + 1 exits each: rows e <= exit_of_image[b] of V[0] and V[1] are bmi_forward_mcd_votes' counts
 * (samples 0 .. t_count-1), rows of exits an image never reached stay zero.  Every other output holds
 * bmi_forward_mcd_exit_staged_ensemble's bits.  Not recorded in the profile table.  Errors: bmi_forward_mcd_exit_staged_ensemble's,
 * BMI_ERR_INVALID for a NULL V, BMI_ERR_UNSUPPORTED for a shape votes.hip does not take; in every error case nothing is written. */
int bmi_forward_mcd_exit_staged_votes(bmi_handle h, const float* x_nchw, int32_t batch, int32_t t_count, uint64_t seed, int32_t mask_cnt0,
                                      const bmi_exit_rule* rule, double* S1, double* S2, double* SL, double* SH, double* Q1, double* Q2,
                                      double* QH, int32_t* V, int32_t* nonfinite, void* scratch, size_t scratch_bytes, int32_t* exit_of_image,
                                      int32_t* active_after, void* workspace, size_t workspace_bytes, bmi_stream stream);

/* The stage plan of bmi_forward_mcd_exit_staged for first_exit (host only; needs bmi_plan).  *n_stages = n_exits - first_exit; with
 * capacity 0 only that is written, else capacity must be >= it.  Per stage k (each array NULL: not written): prefix_macs[k] (MACs per
 * image), suffix_macs[k] (per image and sample), n_ops[k] (prefix + suffix ops), and of those the prefix ops that run over the whole
 * batch because their kernel has no row-table form: whole_batch_macs[k] (per image, also counted in prefix_macs[k]) and
 * n_whole_batch_ops[k] (0 in stage 0).  Summed over the stages the MACs equal bmi_query's. */
int bmi_query_exit_stages(bmi_handle h, int32_t first_exit, int32_t capacity, int32_t* n_stages, int64_t* prefix_macs, int64_t* suffix_macs,
                          int32_t* n_ops, int64_t* whole_batch_macs, int32_t* n_whole_batch_ops);
/* The same plan per op (host only): one entry per output of every op (a pair- or seam-fused op lists both outputs), in the engine's
 * order: out[i] = the tensor id (a head: -1 - its exit index), stage[i] its stage for first_exit, whole_batch[i] = 1 for a prefix op
 * behind a decision without a row-table form.  *count = the number of entries; capacity 0 writes only that, else capacity must be >= it. */
int bmi_query_op_stages(bmi_handle h, int32_t first_exit, int32_t capacity, int32_t* count, int32_t* out, int32_t* stage, int32_t* whole_batch);

/* bmi_finalize_checked and bmi_finalize_uncertainty with a per-image sample count t_used[b] (device int32 [batch], every entry >= 1)
 * in place of t_total: mean / var / logit_mean [E][batch][C]; pred_entropy / exp_entropy / mutual_info [E][batch] when SH and
 * the three outputs are all non-NULL (all NULL: skipped).  nonfinite (NULL: not counted) as in bmi_finalize_checked. */
int bmi_finalize_per_image(int32_t n_exits, int32_t batch, int32_t out_dim, const int32_t* t_used, const double* S1,
                           const double* S2, const double* SL, const double* SH, double* mean, double* var,
                           double* logit_mean, double* pred_entropy, double* exp_entropy, double* mutual_info,
                           int32_t* nonfinite, bmi_stream stream);

/* mean = S1/T, var = S2/T - mean^2 (clamped at 0), logit_mean = SL/T; n = E*B*C. */
int bmi_finalize(int64_t n, int32_t t_total, const double* S1, const double* S2, const double* SL, double* mean,
                 double* var, double* logit_mean, bmi_stream stream);
/* The same, and ADDS to *nonfinite (device int32, caller-zeroed) the number of elements whose sums are not finite: the 16-bit engines
 * saturate at 65 504 (fp16) — an overflowing activation becomes inf, then NaN in the softmax, and would otherwise travel into the
 * reference's np.average (SA/train/results_analyzer.py:247-248) unnoticed.  No synchronisation: read the counter with the results. */
int bmi_finalize_checked(int64_t n, int32_t t_total, const double* S1, const double* S2, const double* SL, double* mean,
                         double* var, double* logit_mean, int32_t* nonfinite, bmi_stream stream);

/* Per (exit, image), float64 [E][batch] each, from the S1 [E][batch][C] and SH [E][batch] sums of t_total samples
 * (bmi_forward_mcd_entropy): m = S1 / T, pred_entropy = -sum_c m_c log m_c (0 log 0 = 0; the reference's entropy() adds 1e-8
 * inside the log instead), exp_entropy = SH / T, mutual_info = max(pred_entropy - exp_entropy, 0).  nonfinite (NULL: not counted) as
 * in bmi_finalize_checked: ADDS the number of non-finite S1 / SH inputs. */
int bmi_finalize_uncertainty(int32_t n_exits, int32_t batch, int32_t out_dim, int32_t t_total, const double* S1, const double* SH,
                             double* pred_entropy, double* exp_entropy, double* mutual_info, int32_t* nonfinite, bmi_stream stream);

/* Temperature scaling, one scalar per exit (host only, no HIP call).  tau: host [n_exits], every entry finite and > 0, or NULL = off;
 * all ones is off as well.  The heads multiply by inv_e = float32(1.0 / (double)tau_e): behind the bias and a site on the logits, in
 * front of the running max, every sample's logits become z = l * inv_e in fp32; the softmax, S1, S2 and the per-sample entropy (SH) are
 * those of z.  SL and the per-sample logits of bmi_forward_mcd_samples stay the RAW l — the logit mean does not depend on tau, and a
 * fit that reads per-sample logits never depends on the temperature currently set.  Every bmi_forward_mcd* entry point honours it (the
 * decision kernels of _exit / _exit_staged / _adaptive read the tempered sums); bmi_head_fused does not.  Off, the launches are the
 * untempered kernels and every output keeps its bits.  The value is read at launch: a captured hipGraph keeps what was set at capture.
 * BMI_ERR_INVALID: wrong count, a non-finite or non-positive entry, capacity < n_exits.  get returns ones when nothing was set. */
int bmi_engine_set_temperature(bmi_handle h, const float* tau, int32_t n_exits);
int bmi_engine_get_temperature(bmi_handle h, float* tau, int32_t capacity);

/* The objective of a temperature fit on per-sample logits, for G candidate temperatures per exit in one launch.  logits: device fp32
 * [T][E][B][C] (bmi_forward_mcd_samples' layout), labels: device int32 [B], every entry in [0, C) (the CALLER checks: an out-of-range
 * label is not read but makes that image's term meaningless), tau_grid: device fp32 [E][G], every entry finite and > 0; nll: device
 * float64 [E][G], ADDED TO (a walk over a loader accumulates).  All in float64, no fused multiply-add in the statistic:
 *     z_tc = (double)l_tebc * (1.0 / (double)tau_eg),   a_t = z_{t,y_b} - max_c z_tc - log sum_c exp(z_tc - max_c z_tc),
 *     nll[e][g] += sum_b -( logsumexp_t a_t - log T )
 * — the negative log-likelihood of the T-mean softmax at temperature tau_eg, in log-sum-exp form: no clip (the reference's NLL clips
 * at 1e-256, SA/train/results_analyzer.py:497-505), finite for any finite logits.  Bit-reproducible: the per-image terms go to
 * `scratch` ([E][G][B] float64, bmi_nll_temperature_scratch_bytes) and a second kernel sums them over the images in a fixed order; no
 * floating-point atomics.  BMI_ERR_NOMEM: scratch too small.  No allocation, no synchronisation. */
size_t bmi_nll_temperature_scratch_bytes(int32_t E, int32_t B, int32_t G);
int bmi_nll_temperature_grid(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const int32_t* labels, const float* tau_grid,
                             int32_t G, double* nll, void* scratch, size_t scratch_bytes, bmi_stream stream);

/* The objective of a JOINT temperature fit of the exit ensembles on per-sample logits: row e is the NLL of the mean over exits 0..e and
 * over the T samples of the tempered softmax (the row bmi_forward_mcd_ensemble forms, as a likelihood), for G candidate temperatures
 * in one launch.  logits / labels as bmi_nll_temperature_grid's; tau: device fp32 [E], the current temperature vector; vary_mask: bit i
 * set = exit i takes the candidate; tau_cand: device fp32 [G]; every temperature finite and > 0:
 *     tau_i(g) = bit i of vary_mask ? tau_cand[g] : tau[i]
 * — one bit is a coordinate step, all E bits one shared "ensemble temperature", no bit with G = 1 evaluates the vector tau.  nll: device
 * float64 [E][G], ADDED TO; ALL E rows are written for every candidate (the rows below the lowest varied exit hold the same bits for
 * every g).  All in float64, no fused multiply-add in the statistic, y = labels[b]:
 *     z_c        = (double)l[t][i][b][c] * (1.0 / (double)tau_i(g))
 *     a[t][i][b] = (z_y - max_c z) - log sum_c exp(z_c - max_c z)
 *     L[i][b]    = logsumexp_t a[t][i][b]
 *     R[0][b]    = L[0][b],   R[e][b] = logaddexp(R[e-1][b], L[e][b])        (m + log(exp(x - m) + exp(y - m)), m = max(x, y))
 *     nll[e][g] += sum_b -( R[e][b] - log(T * (e + 1)) )
 * — the float64 product bmi_nll_temperature_grid uses, not the heads' fp32 product, so a fit never depends on the temperature set on an
 * engine; log-sum-exp form, no clip, finite for any finite logits.  The logits of a run of (image, sample) rows, all E exits, are
 * staged once; an exit outside the mask costs C exponentials per row, an exit in the mask C per (candidate, row): a candidate of a
 * coordinate step costs C per row, not E * C.  Bit-reproducible: per-image terms go to `scratch` ([E][G][B] float64,
 * bmi_nll_ensemble_temperature_scratch_bytes = E * G * B * 8, 0 for a count below 1) and are summed over the images in a fixed order;
 * no floating-point atomics.  No allocation, no synchronisation.  A sample count whose T * E rows exceed
 * min(BMI_NLL_ENS_ROWS, BMI_NLL_ENS_SLAB / (C | 1)) runs in chunks of samples.
 * BMI_ERR_INVALID (decided before any HIP call): a null pointer, a count below 1, a mask bit at or above E.  BMI_ERR_UNSUPPORTED: E > 32,
 * or one sample's E rows do not fit the staging buffer, E * (C | 1) > BMI_NLL_ENS_SLAB.  BMI_ERR_NOMEM: scratch too small.  An error
 * writes nothing. */
#define BMI_NLL_ENS_SLAB 9216 /* floats of staged logits per workgroup */
#define BMI_NLL_ENS_ROWS 192  /* (sample, exit, image) rows per staged chunk, at most */
size_t bmi_nll_ensemble_temperature_scratch_bytes(int32_t E, int32_t B, int32_t G);
int bmi_nll_ensemble_temperature_grid(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const int32_t* labels, const float* tau,
                                      uint32_t vary_mask, const float* tau_cand, int32_t G, double* nll, void* scratch, size_t scratch_bytes,
                                      bmi_stream stream);

/* Weighted exit ensembles.  W_device: DEVICE float64 [n_exits][n_exits], row-major, owned by the caller and alive for as long as it is
 * set; row e is the weight vector of the ensemble of exits 0..e (W[e][i] >= 0, W[e][i] == 0 for i > e, every row sums to 1).  NULL: off.
 * The contents are used AS GIVEN — no check and no renormalisation on the device; validating them is the caller's job (the Python layer
 * does).  With weights set, per sample, in float64 without fused multiply-adds, p_te the tempered softmax of bmi_forward_mcd_ensemble:
 *     q_te = ((W[e][0] * p_t0 + W[e][1] * p_t1) + ...) + W[e][e] * p_te         every product rounded, added in exit order from 0.0
 * and Q1 / Q2 / QH are accumulated from q exactly as before: bmi_forward_mcd_ensemble, bmi_forward_mcd_adaptive_ensemble (so
 * BMI_STOP_ON_ENSEMBLE decides on the weighted ensemble) and bmi_forward_mcd_exit_staged_ensemble all read it; an image with n exits
 * reads rows e < n of W only.  The rule of bmi_forward_mcd_exit_staged with ensemble = 1 becomes
 *     p_c = sum_{i<=e} W[e][i] * (S1[i][b][c] / t_count)                        in exit order, from 0.0
 * (bmi_forward_mcd_exit, the older entry, keeps the equal mean).  S1 / S2 / SL / SH never depend on it.  Off, the launches are the
 * unweighted kernels and every output keeps its bits.  The pointer is read at launch: a captured hipGraph keeps what was set at capture.
 * BMI_ERR_INVALID: a NULL handle, n_exits other than the engine's.  bmi_finalize_ensemble* need no change: they read the sums. */
int bmi_engine_set_ensemble_weights(bmi_handle h, const double* W_device, int32_t n_exits);

/* Vector scaling (Guo et al. 2017): a per-class scale and bias per exit in place of the one scalar of bmi_engine_set_temperature.
 * scale_device / bias_device: DEVICE fp32 [n_exits][out_dim], owned by the caller and alive for as long as they are set; every value
 * finite, no sign constraint (used AS GIVEN: validating them is the caller's job, the Python layer does).  scale_device NULL: off.  At the
 * place the temperature acts — behind the classifier bias and a site on the logits, in front of the running max — every sample's logits
 * become
 *     z_c = fl32( fl32(l_c * scale[e][c]) + bias[e][c] )                         two rounded fp32 operations, never one fused multiply-add
 * and the max, the softmax, S1, S2 and the per-sample entropy (SH) are those of z.  SL and the per-sample logits of
 * bmi_forward_mcd_samples stay the RAW l, as under a temperature.  Every bmi_forward_mcd* entry point honours it, the ensemble launches
 * of the *_ensemble entry points included (their z is the number above, in place of fl32(l * inv_e)); the decision kernels read the
 * scaled sums; bmi_head_fused does not.  Off, the launches are the kernels they were and every output keeps its bits.  The pointers are
 * read at launch: a captured hipGraph keeps what was set at capture.
 * Temperature and vector scaling are mutually exclusive; clearing one is how to switch.  BMI_ERR_INVALID: a NULL handle, a NULL
 * bias_device with a scale, n_exits / out_dim other than the engine's, or a temperature other than all ones in force; and
 * bmi_engine_set_temperature returns BMI_ERR_INVALID for a temperature other than all ones while a vector scaling is set. */
int bmi_engine_set_vector_scaling(bmi_handle h, const float* scale_device, const float* bias_device, int32_t n_exits, int32_t out_dim);

/* bmi_ensemble_moments_weighted with tau replaced by the two device arrays of bmi_engine_set_vector_scaling (fp32 [E][C]):
 *     z_te,c = (double) fl32( fl32(l * scale[e][c]) + bias[e][c] )
 * and everything behind it unchanged.  W_device may be NULL (the equal-weight mean).  BMI_ERR_INVALID: a null pointer otherwise, a count
 * below 1; BMI_ERR_UNSUPPORTED as bmi_ensemble_moments. */
int bmi_ensemble_moments_vector(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const float* scale_device, const float* bias_device,
                                const double* W_device, double* Q1, double* Q2, double* QH, bmi_stream stream);

/* Value and gradient of a vector-scaling fit on per-sample logits, all E exits in one call.  logits / labels as
 * bmi_nll_temperature_grid's; scale / bias: device float64 [E][C]; nll: device float64 [E], grad_scale / grad_bias: device float64
 * [E][C], all three ADDED TO (a walk over a loader accumulates in call order).  All in float64, no fused multiply-add, y = labels[b]:
 *     z_tc = (double)l_tebc * scale[e][c] + bias[e][c]                              (the optimiser's smooth objective: the fp32 rounding of
 *                                                                                    the head happens once, when a result is applied)
 *     A_t  = (z_ty - max_c z_tc) - log sum_c exp(z_tc - max_c z_tc),    nll[e] += sum_b -( logsumexp_t A_t - log T )
 *     p_tc = softmax_c(z_t),   r_t = exp(A_t) / sum_t' exp(A_t')
 *     grad_bias[e][c]  += sum_b sum_t r_t (p_tc - [c == y])
 *     grad_scale[e][c] += sum_b sum_t r_t (p_tc - [c == y]) * l_tebc
 * One workgroup per (image, exit) stages min(64, 3456 / (C | 1)) samples at a time; a larger T runs in chunks of samples with the running
 * log-sum-exp state carried.  Bit-reproducible: per-image terms go to `scratch` ([E][B][2C + 1] float64,
 * bmi_nll_vector_scratch_bytes, 0 for a count below 1) and a second kernel sums them over the images in a fixed order; no floating-point
 * atomics.  No allocation, no synchronisation.  BMI_ERR_INVALID (decided before any HIP call): a null pointer, a count below 1.
 * BMI_ERR_UNSUPPORTED: C > 256 or E > 65535.  BMI_ERR_NOMEM: scratch too small.  An error writes nothing. */
size_t bmi_nll_vector_scratch_bytes(int32_t E, int32_t B, int32_t C);
int bmi_nll_vector_scaling_grad(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const int32_t* labels, const double* scale,
                                const double* bias, double* nll, double* grad_scale, double* grad_bias, void* scratch, size_t scratch_bytes,
                                bmi_stream stream);

/* Matrix scaling (Guo et al. 2017): a full [out_dim][out_dim] matrix and a bias per exit, the one calibration map that moves probability
 * mass between classes; temperature and vector scaling are its special cases.  matrix_device: DEVICE fp32 [n_exits][out_dim][out_dim],
 * row-major, row = OUTPUT class; bias_device: DEVICE fp32 [n_exits][out_dim]; both owned by the caller and alive for as long as they are
 * set, every value finite (used AS GIVEN: validating them is the caller's job, the Python layer does).  matrix_device NULL: off.  At the
 * place the temperature acts — behind the classifier bias and a site on the logits, in front of the running max — every sample's logits
 * become
 *     acc = fl32(M[c][0] * l_0)
 *     acc = fl32(acc + fl32(M[c][j] * l_j))          j = 1 .. C-1, ascending
 *     z_c = fl32(acc + b[c])
 * every product and every sum rounded to fp32, never a fused multiply-add, no matrix instruction (its accumulation order is not this
 * one): a float32 numpy loop reproduces z exactly, and a diagonal matrix gives the bits of bmi_engine_set_vector_scaling (the off-diagonal
 * products are +-0 for finite logits).  The max, the softmax, S1, S2 and the per-sample entropy (SH) are those of z.  SL and the
 * per-sample logits of bmi_forward_mcd_samples stay the RAW l.  Every bmi_forward_mcd* entry point honours it, the ensemble launches of
 * the *_ensemble entry points included; the decision kernels read the scaled sums; bmi_head_fused does not.  Off, the launches are the
 * kernels they were and every output keeps its bits.  The pointers are read at launch: a captured hipGraph keeps what was set at capture.
 * One calibration map at a time.  BMI_ERR_INVALID: a NULL handle, a NULL bias_device with a matrix, n_exits / out_dim other than the
 * engine's, or a temperature other than all ones or a vector scaling in force; and bmi_engine_set_temperature (other than all ones) and
 * bmi_engine_set_vector_scaling return BMI_ERR_INVALID while a matrix is set. */
int bmi_engine_set_matrix_scaling(bmi_handle h, const float* matrix_device, const float* bias_device, int32_t n_exits, int32_t out_dim);

/* bmi_ensemble_moments_vector with the two device arrays of bmi_engine_set_matrix_scaling (fp32 [E][C][C] and [E][C]):
 *     z_te,c = (double) fl32( (..(fl32(M[e][c][0] * l_0) + fl32(M[e][c][1] * l_1)) + ..) + bias[e][c] )         the head's number above
 * formed once per (sample, exit, image) row, and everything behind it unchanged.  W_device may be NULL (the equal-weight mean).
 * BMI_ERR_INVALID: a null pointer otherwise, a count below 1; BMI_ERR_UNSUPPORTED as bmi_ensemble_moments. */
int bmi_ensemble_moments_matrix(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const float* matrix_device, const float* bias_device,
                                const double* W_device, double* Q1, double* Q2, double* QH, bmi_stream stream);

/* Value and gradient of a matrix-scaling fit on per-sample logits, all E exits in one call.  logits / labels as
 * bmi_nll_temperature_grid's; matrix: device float64 [E][C][C] (row = output class), bias: device float64 [E][C]; nll: device float64
 * [E], grad_matrix [E][C][C], grad_bias [E][C], all three ADDED TO (a walk over a loader accumulates in call order).  All in float64, no
 * fused multiply-add, y = labels[b]:
 *     z_tc = ((0.0 + (double)l_t0 * M[c][0]) + (double)l_t1 * M[c][1] + ...) + b[c]          j ascending, every operation rounded
 *     A_t  = (z_ty - max_c z_tc) - log sum_c exp(z_tc - max_c z_tc),    nll[e] += sum_b -( logsumexp_t A_t - log T )
 *     r_t  = exp(A_t) / sum_t' exp(A_t'),   d_tc = r_t (softmax_c(z_t) - [c == y])
 *     grad_bias[e][c]      += sum_b sum_t d_tc
 *     grad_matrix[e][c][j] += sum_b sum_t d_tc * (double)l_tj
 * One workgroup per (image, exit) stages min(64, 3456 / (C | 1)) samples at a time; a larger T runs in chunks of samples with the running
 * log-sum-exp state carried.  Bit-reproducible: per-image terms go to `scratch` ([E][B][C * C + C + 1] float64,
 * bmi_nll_matrix_scratch_bytes — 80 MB at E = 4, B = 250, C = 100; 0 for a count below 1) and a second kernel sums them over the images
 * in a fixed order; no floating-point atomics.  No allocation, no synchronisation.  BMI_ERR_INVALID (decided before any HIP call): a null
 * pointer, a count below 1.  BMI_ERR_UNSUPPORTED: C > 128 (the head's own limit) or E > 65535.  BMI_ERR_NOMEM: scratch too small.  An
 * error writes nothing. */
size_t bmi_nll_matrix_scratch_bytes(int32_t E, int32_t B, int32_t C);
int bmi_nll_matrix_scaling_grad(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const int32_t* labels, const double* matrix,
                                const double* bias, double* nll, double* grad_matrix, double* grad_bias, void* scratch, size_t scratch_bytes,
                                bmi_stream stream);

/* Per-pass multi-exit accuracy on per-sample logits: the top-k hit counts of every exit and of every exit ensemble of every stochastic
 * pass, and every exit's summed max-probability, in two launches — the read-out of the reference's _MultiExitAccuracy._metrics
 * (SA/train/loss/base_classes.py:39-66) for ALL 2 E rows, not only the two its row-0 overwrite keeps.  logits: device fp32 [T][E][B][C]
 * (bmi_forward_mcd_samples' layout, the RAW logits: no calibration map acts here), labels: device int32 [B]; tops: HOST int32 [K], each
 * >= 1, read during the call (a value > C always hits on a valid row).  For pass t and image b, y = labels[b], all in float64, no fused
 * multiply-add:
 *     rank(score) = #{c : score_c > score_y} + #{c < y : score_c == score_y}      the label loses ties to lower class indices: a stable
 *                                                                                  descending sort, the project's "lowest index on ties"
 *     rank_clf[e] = rank(l_te)                                                     comparisons of the fp32 logits as given
 *     p_te = softmax_c((double)l_te)   (max-subtracted),   s_te = p_t0 + ... + p_te   in exit order from exit 0 (the reference's
 *                                                                                  unnormalised `ensemble += softmax(logits)`)
 *     rank_ens[e] = rank(s_te),        m_te = 1 / sum_c exp((double)l_tec - max_c)   (the row's max-probability)
 *     hits[t][0][e][i] = #{b : rank_clf[e] < tops[i]},   hits[t][1][e][i] = #{b : rank_ens[e] < tops[i]}        int32 [T][2][E][K]
 *     maxprob[t][e]    = sum_b m_te, added in image order b = 0, 1, ... from 0.0                                 float64 [T][E]
 * Both outputs are OVERWRITTEN (the caller points at the row of its own table).  A row (t, e, b) with a non-finite logit is a miss for
 * every k in clf[e] and in ens[e' >= e] of that (t, b), contributes 0.0 to maxprob[t][e] and adds 1 to *nonfinite (device int32, ADDED
 * TO; NULL: not counted).  A label outside [0, C) makes the image a miss everywhere: nothing is read outside the row, and the row is not
 * counted as non-finite.  No NaN reaches an output.  Exact and bit-reproducible: the counts are integers, the max-probability sum has one
 * order whatever the launch geometry, no floating-point atomics; the per-(pass, exit, image) ranks and max-probabilities go through
 * `scratch` (bmi_pass_accuracy_scratch_bytes = T * E * B * 16, 0 for a count below 1).  No allocation, no synchronisation: capturable.
 * BMI_ERR_INVALID (decided before any HIP call): a null pointer other than nonfinite, a count below 1, a tops[i] < 1.
 * BMI_ERR_UNSUPPORTED: C > 128 (the head's own limit), E > 32, K > 8, T * B >= 2^25 or T * E >= 2^31 (the launch grids).
 * BMI_ERR_NOMEM: scratch too small.  An error writes nothing. */
size_t bmi_pass_accuracy_scratch_bytes(int32_t T, int32_t E, int32_t B);
int bmi_pass_accuracy(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const int32_t* labels,
                      const int32_t* tops /* host, [K], each >= 1; a value > C always hits on a valid row */, int32_t K, int32_t* hits,
                      double* maxprob, int32_t* nonfinite /* device, ADDED to; NULL: not counted */, void* scratch, size_t scratch_bytes,
                      bmi_stream stream);

/* Vote counts: the variation ratio and the majority-vote prediction, the third MC-dropout uncertainty measure beside the predictive
 * entropy and the mutual information.  A vote is the arg-max of ONE stochastic pass, so it cannot be recovered from the sums over the
 * passes (S1 / S2 / SL, Q1 / Q2 / QH): it is taken where the per-sample logits exist.  For pass t, image b and exit e, with the raw fp32
 * logits l_te of length C and no fused multiply-add wherever a number is formed:
 *     z_te  the calibrated fp32 logits, formed exactly as the fused head and the ensemble launches form them — no map: z = l;
 *           temperature: fl32(l * inv_e), inv_e = float32(1 / tau_e); vector scaling: fl32(fl32(l * a_c) + b_c); matrix scaling: the number
 *           of bmi_engine_set_matrix_scaling (products rounded one by one, added for j ascending, then the bias).  One map at a time.
 *     bad   row (t, e, b) is bad if any z_tec, c < C, is not finite
 *     classifier vote    k = min{c : z_c == max_c z} (fp32 comparisons, the lowest index on ties):  V[0][e][b][k] += 1; a bad row casts none
 *     p_te = softmax_c((double) z_te), max-subtracted, float64 — the member of bmi_forward_mcd_ensemble
 *     q_te = (p_t0 + ... + p_te) / (e + 1), summed in exit order and divided once; with weights (bmi_engine_set_ensemble_weights)
 *            ((W[e][0] p_t0 + W[e][1] p_t1) + ...) + W[e][e] p_te, every product rounded, added from 0.0 — what bmi_forward_mcd_ensemble forms
 *     ensemble vote      k = min{c : q_c == max_c q}:  V[1][e][b][k] += 1; none if any row i <= e of that (t, b) is bad
 *     *nonfinite (device int32, ADDED to; NULL: not counted) gains 1 per bad row
 * V is device int32 [2][E][B][C] and is ADDED to, like S1.  The counts are integers (integer atomic adds, no floating-point atomics):
 * the same whatever the launch geometry and however the samples are split into chunks, launches, calls or ranks.
 *
 * bmi_forward_mcd_votes: bmi_forward_mcd_ensemble with the same arguments, the same bits in S1 / S2 / SL / SH / Q1 / Q2 / QH and the same
 * scratch (bmi_ensemble_scratch_bytes); behind every chunk's ensemble launch one launch of votes.hip reads the same per-sample logits,
 * under the handle's calibration map and ensemble weights.  V covers rows 0 .. batch-1 of a share (image_offset).  No allocation and no
 * synchronisation: capturable.  BMI_ERR_INVALID: a null pointer other than nonfinite, what bmi_forward_mcd_ensemble refuses;
 * BMI_ERR_UNSUPPORTED: more than 32 exits or 128 classes (and bmi_forward_mcd_ensemble's limits); BMI_ERR_NOMEM: scratch or workspace
 * too small.  Decided before any HIP call; an error writes nothing. */
int bmi_forward_mcd_votes(bmi_handle h, const float* x_nchw, int32_t batch, int32_t image_offset, int32_t t_begin, int32_t t_count,
                          uint64_t seed, int32_t mask_cnt0, double* S1, double* S2, double* SL, double* SH, double* Q1, double* Q2, double* QH,
                          int32_t* V, int32_t* nonfinite /* device, ADDED to; NULL: not counted */, void* scratch, size_t scratch_bytes,
                          void* workspace, size_t workspace_bytes, bmi_stream stream);

/* The same counts from a caller's per-sample logits: device fp32 [T][E][B][C] (bmi_forward_mcd_samples' layout).  Every map is optional
 * and at most one may be given: tau HOST [E], every entry finite and > 0 (rounded like bmi_engine_set_temperature), or NULL; scale_device
 * + bias_device device fp32 [E][C] (bmi_engine_set_vector_scaling's); matrix_device [E][C][C] + bias_device [E][C]
 * (bmi_engine_set_matrix_scaling's).  bias_device belongs to the scale or to the matrix: it is given exactly when one of them is.
 * W_device: device float64 [E][E] row-major, used as given, or NULL (the equal-weight mean).  V is ADDED to: two calls on the halves of T
 * leave the counts of one call.  BMI_ERR_INVALID (decided before any HIP call): a null logits or V, a count below 1, more than one map,
 * a bias without its map or a map without its bias, a tau entry that is not finite and > 0.  BMI_ERR_UNSUPPORTED (never a wrong
 * number): C > 128, E > 32 or T * B >= 2^25 (the launch grid).  An error writes nothing. */
int bmi_vote_counts(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const float* tau /* host [E] or NULL */,
                    const float* scale_device, const float* bias_device, const float* matrix_device, const double* W_device, int32_t* V,
                    int32_t* nonfinite, bmi_stream stream);

/* bmi_vote_counts over a list of images and a per-image number of exits (the kernel of bmi_forward_mcd_adaptive_votes and
 * bmi_forward_mcd_exit_staged_votes).  list: device int32 [list_count], image indices in [0, B), each at most once, or NULL (every image;
 * list_count is then ignored).  n_e: device int32 [B], or NULL (all E): of image b only the exits e < n_e[b] are read, and only those cast
 * votes, exit or ensemble — the running exit sum is cut there.  logits and V keep the batch stride B: image b's rows sit at index b whether
 * or not a list is given.  Every count that is added is the one bmi_vote_counts adds for that row; images not in the list and exits
 * >= n_e[b] are neither read nor written (their logits may be stale or NaN, *nonfinite does not see them).  Errors: bmi_vote_counts', and
 * BMI_ERR_INVALID for a list with list_count outside [1, B].  An error writes nothing. */
int bmi_vote_counts_rows(const float* logits, int32_t T, int32_t E, int32_t B, int32_t C, const float* tau /* host [E] or NULL */,
                         const float* scale_device, const float* bias_device, const float* matrix_device, const double* W_device,
                         const int32_t* list, int32_t list_count, const int32_t* n_e, int32_t* V, int32_t* nonfinite, bmi_stream stream);

/* The decided-vote stop rule (BMI_STOP_VOTES of bmi_forward_mcd_adaptive_votes) on counts the caller holds: V device int32 [2][E][B][C],
 * non-negative; the rule reads row V[kind][test_exit][b] (kind 0: the exit, 1: the exit ensemble) of every image b of in_list (device
 * int32 [in_count], or NULL: images 0 .. in_count-1) after t of t_max samples.  Every tested image gets t_used[b] = t (device int32 [B]);
 * the images that are NOT decided go to out_list (device int32, room for in_count entries, not in_list itself) in their order, their
 * number to *count (device int32).  Integer arithmetic only.  BMI_ERR_INVALID (decided before any HIP call): a NULL V / out_list / count
 * / t_used, a count below 1, kind outside 0..1, test_exit outside [0, E), t < 1, t_max < t, slack < 0, in_count outside [1, B],
 * out_list == in_list.  An error writes nothing. */
int bmi_vote_decide(const int32_t* V, int32_t E, int32_t B, int32_t C, int32_t kind, int32_t test_exit, int32_t t, int32_t t_max, int32_t slack,
                    const int32_t* in_list, int32_t in_count, int32_t* out_list, int32_t* count, int32_t* t_used, bmi_stream stream);

/* The read-out of V [2][E][batch][C], per kind, exit and image, all three outputs [2][E][batch] and OVERWRITTEN:
 *     n = sum_c V_c (the votes cast),   m = max_c V_c
 *     vote_class      = the lowest c with V_c == m                                    int32
 *     variation_ratio = 1.0 - (double)m / (double)n                                   float64
 *     vote_entropy    = -sum_{c : V_c > 0} f_c log f_c,  f_c = (double)V_c / (double)n, subtracted in class order from 0.0, in nats
 *     n == 0:  vote_class = -1, variation_ratio = 1.0, vote_entropy = 0.0             no NaN reaches an output
 * BMI_ERR_INVALID: a null pointer, a count below 1; BMI_ERR_UNSUPPORTED: 2 * n_exits * batch >= 2^25 (the launch grid). */
int bmi_finalize_votes(int32_t n_exits, int32_t batch, int32_t out_dim, const int32_t* V, int32_t* vote_class, double* variation_ratio,
                       double* vote_entropy, bmi_stream stream);

/* Reliability tables: per exit and per exit ensemble the confidence histogram behind the top-label ECE (equal-mass bins as the reference's
 * hist-ECE takes them, SA/train/results_analyzer.py:446-495, or fixed edges) and the NLL and Brier sums (:497-503), from the T-mean
 * probabilities on the device.  R = 2 E rows r = kind * E + e: kind 0 is exit e's mean[e], kind 1 the exit ensemble
 * q_e = (p_0 + ... + p_e) / (e + 1), added in exit order from exit 0 onto 0.0 and divided once.  Per row and image, v = the row's C values,
 * y = labels[b], float64 and no fused multiply-add wherever a number is formed:
 *     pc_c = max(v_c, 1e-256),   s = ((0.0 + pc_0) + pc_1) + ...  (ascending class order),   pred = the lowest c with pc_c = max_c pc
 *     conf = (float)(pc_pred / s),   key = the float32 bit pattern of conf (uint32: for positive floats the unsigned order is the float order)
 *     hit = (pred == y),   nll = -log(pc_y),   brier = ((0.0 + d_0^2) + d_1^2) + ...,   d_c = v_c - [c == y]  (the unclipped v)
 * An image whose label is outside [0, C): key 0, hit 0, nll = brier = 0.0 in all R rows and counters[1] += 1 (nothing of it is read).
 * Otherwise a (row, image) with a non-finite v_c: key 0, hit 0, nll = brier = 0.0 and counters[0] += 1.  No NaN reaches an output.
 *
 * The record call writes the records of the B images of one batch at columns n0 .. n0 + B - 1 of the caller's record buffers, each
 * [R][N_cap]: keys uint32, hit uint8, nll and brier float64 (21 bytes per row and image).  mean: device float64 [E][B][C] (bmi_finalize's
 * mean), labels: device int32 [B]; counters: device int32 [2], ADDED to, or NULL (not counted).  One launch; capturable.
 * BMI_ERR_INVALID (decided before any HIP call): a null pointer other than counters, a count below 1, n0 < 0, n0 + B > N_cap.
 * BMI_ERR_UNSUPPORTED: C > 128, E > 32, B >= 2^25 (the launch grid).  An error writes nothing. */
int bmi_reliability_record(const double* mean, int32_t E, int32_t B, int32_t C, const int32_t* labels, int32_t n0, int32_t N_cap, uint32_t* keys,
                           uint8_t* hit, double* nll, double* brier, int32_t* counters /* device [2], ADDED to; NULL: not counted */,
                           bmi_stream stream);

/* The table of columns 0 .. N-1 of the records, every output OVERWRITTEN:
 *     edges    float32 [R][n_bins + 1].  edges_in NULL: by mass — per = N / n_bins (integer), edges[0] = 0, edges[i + 1] = the order statistic
 *              of rank min((i + 1) * per, N - 1) (0-based, ascending) of the row's N keys (radix select: exact under duplicates), edges[n_bins]
 *              = 1.  Otherwise edges_in: HOST float32 [n_bins + 1], finite and non-decreasing, read during the call, copied to every row.
 *     count, hits, conf_fix   int64 [R][n_bins]: image n is in the one bin i with edges[i] < conf <= edges[i + 1] (a zero-width bin stays
 *              empty, key 0 is in none); conf_fix = sum (int64)(conf * 2^40), exact for C <= 128, where conf >= 2^-8 is a multiple of 2^-40
 *     sums     float64 [R][2]: the nll and the brier records, each added in image order n = 0, 1, ... from 0.0
 * Integer (LDS) atomics only, no floating-point atomics: the same bits on every run, however the N images were cut into record calls.
 * Four launches, no allocation, no synchronisation: capturable.  scratch: the per-chunk integer tables, bmi_reliability_scratch_bytes
 * = R * ceil(N / 4096) * 3 * n_bins * 8 (0 for arguments the table call refuses).
 * BMI_ERR_INVALID (decided before any HIP call): a null pointer other than edges_in, a count below 1, N > N_cap, n_bins outside [1, 64],
 * an edges_in entry that is not finite or is below its predecessor.  BMI_ERR_UNSUPPORTED: R > 64, N >= 2^22.  BMI_ERR_NOMEM: scratch too
 * small.  An error writes nothing. */
size_t bmi_reliability_scratch_bytes(int32_t R, int32_t N, int32_t n_bins);
int bmi_reliability_table(const uint32_t* keys, const uint8_t* hit, const double* nll, const double* brier, int32_t R, int32_t N, int32_t N_cap,
                          int32_t n_bins, const float* edges_in /* host [n_bins + 1] or NULL */, float* edges_out, int64_t* count, int64_t* hits,
                          int64_t* conf_fix, double* sums, void* scratch, size_t scratch_bytes, bmi_stream stream);

/* The KDE-ECE of columns 0 .. N-1 of the records — the one calibration error the reference prints (the `ECE` column of
 * FullAnalysis.all_experiments: ece_eval_binary -> ece_kde_binary, SA/train/results_analyzer.py:351-443) —, per row, from the float32
 * confidences (keys) and the hit bits alone, with the densities evaluated exactly (no binning).  Float64, no fused multiply-add, correctly
 * rounded division and sqrt, no other library function; per row r, every sum from 0.0 in image order (the contract, operation by operation,
 * is the header comment of csrc/reliability_kde.hip; train.reliability.reliability_kde_numpy restates it):
 *     data     the images with keys[r][n] != 0, d = (double) conf;  n of them, n1 with the hit bit set
 *     bw       sd = sqrt(sum (d - mu)^2 / n1) over the hit data, mu = sum d / n1 (two passes; n1 = 0: sd = 0);
 *              bw = (sd != 0 ? sd : 1e-16) * bw_scale, h = 3 bw.  bw_scale: the reference's is (2 N)^-0.2, formed by the caller
 *     grid     x_i = i * (2.2 / (G - 1)) + (-0.6), i < G
 *     sums     S1 (hit data) and S2 (all data): per datum the centres d and its mirror (-d if d < 0.5, else 2 - d), per centre
 *              u = (x_i - c) / h, t = 1 - u u, the term t t t where t > 0
 *     density  [R][2][G] = pp1, pp2:  pp2_i = S2_i * (35 / 32) / (h * 2 n) * 2 where 0 < x_i < 1, else 0;  pp1 with S1 and n1
 *     ece_kde  a / b, the trapezoids over 0 <= x_i <= 1 of I and of pp2:  where max(pp1_i, pp2_i) > 1e-6,
 *              I_i = |x_i - min(n1 / n * pp1_i / pp2_i, 1)|^order * pp2_i, elsewhere the last such I below i (the reference's carry-forward), else 0
 *     degenerate  1 where n = 0 or b == 0 (no hit, one hit or equal hit confidences: sd = 0, the reference's NaN), with ece_kde = 0.0
 * Every output is OVERWRITTEN (density holds S1, S2 between the second and the third launch); no floating-point atomics: the same bits on every run and
 * for every cut of the images into record calls.  Three launches, no allocation, no synchronisation: capturable.
 * BMI_ERR_INVALID (decided before any HIP call): a null pointer, a count below 1, N > N_cap, G outside [BMI_KDE_MIN_GRID, BMI_KDE_MAX_GRID],
 * order not 1 or 2, bw_scale not finite and positive.  BMI_ERR_UNSUPPORTED: R > 64, N >= 2^22, bw_scale outside [2^-100, 2^100] (inside,
 * every quotient above is finite: no NaN reaches an output).  An error writes nothing. */
#define BMI_KDE_MIN_GRID 16
#define BMI_KDE_MAX_GRID 65536
int bmi_reliability_kde(const uint32_t* keys, const uint8_t* hit, int32_t R, int32_t N, int32_t N_cap, int32_t G, int32_t order, double bw_scale,
                        double* ece_kde /*[R]*/, double* bw /*[R]*/, double* sd /*[R]*/, int64_t* n_data /*[R]*/, int64_t* n_hit /*[R]*/,
                        int32_t* degenerate /*[R]*/, double* density /*[R][2][G]*/, bmi_stream stream);

/* Classwise reliability tables: the confidence histogram behind the classwise ECE (Kull et al. 2019) per exit, per exit ensemble AND PER
 * CLASS — what the top-label calls above drop: the other C - 1 probabilities of every image.  Rows as above (R = 2 E, r = kind * E + e, the
 * ensemble added in exit order from 0.0 and divided once).  Per row and image, v = the row's C values, float64 and no fused multiply-add
 * (the contract, operation by operation, is the header comment of csrc/reliability_classwise.hip; train.reliability.classwise_numpy restates it):
 *     pc_c = max(v_c, 1e-256),   s = ((0.0 + pc_0) + pc_1) + ...  (ascending class order: the s of bmi_reliability_record)
 *     q_c = pc_c / s for EVERY class,   conf_c = 0.0f if q_c < 2^-126 (an explicit compare on the double), else (float) q_c;  conf_c <= 1.0f
 *     key_c = the float32 bit pattern of conf_c;  at the arg-max class it is bit for bit the key bmi_reliability_record writes
 * An image whose label is outside [0, C): all R C keys of it INVALID (0xFFFFFFFF), label record -1, counters[1] += 1.  Otherwise a (row,
 * image) with a non-finite v_c: that row's C keys INVALID, counters[0] += 1.  Key 0 is a VALID key here (confidence zero).
 *
 * The record call writes the B images of one batch at columns n0 .. n0 + B - 1 of pkeys uint32 [R][C][N_cap] (the image index fastest) and
 * labels_rec int32 [N_cap]: 4 R C bytes per image — 32 MB at E = 4, C = 100, N = 10 000.  mean: device float64 [E][B][C], labels: device
 * int32 [B]; counters: device int32 [2], ADDED to, or NULL (not counted).  One launch, no allocation, no synchronisation: capturable.
 * BMI_ERR_INVALID (decided before any HIP call): a null pointer other than counters, a count below 1, n0 < 0, n0 + B > N_cap.
 * BMI_ERR_UNSUPPORTED: C > 128, E > 32, B >= 2^25 (the launch grid).  An error writes nothing. */
int bmi_classwise_record(const double* mean, int32_t E, int32_t B, int32_t C, const int32_t* labels, int32_t n0, int32_t N_cap, uint32_t* pkeys,
                         int32_t* labels_rec, int32_t* counters /* device [2], ADDED to; NULL: not counted */, bmi_stream stream);

/* The classwise table of columns 0 .. N-1 of the records, every output OVERWRITTEN:
 *     edges    float32 [R][C][n_bins + 1].  edges_in NULL: by mass, per (row, class) — per = N / n_bins (integer), edges[0] = 0, edges[i + 1]
 *              = the order statistic of rank min((i + 1) * per, N - 1) (0-based) of that line's N keys in unsigned order (radix select: exact
 *              under duplicates; INVALID keys sort last, a selected INVALID key gives 1.0f), edges[n_bins] = 1.  Otherwise edges_in: HOST
 *              float32 [n_bins + 1], finite and non-decreasing, read during the call, copied to every (row, class).
 *     count, hits, conf_fix   int64 [R][C][n_bins]: a valid pair (image n, class c) with conf >= edges[0] is in the lowest bin j with
 *              conf <= edges[j + 1]; below edges[0] or above edges[n_bins] in none.  Bin 0 is CLOSED at its lower edge (confidence 0 is
 *              counted: the other classes' confidences are data) — the top-label table's is open; edges_in[0] > 0 ignores the
 *              negligible probabilities.  hits: the pairs with labels_rec[n] == c.  conf_fix = sum (int64)((double) conf * 2^40),
 *              truncating: an exact integer definition within count * 2^-40 of the sum (a classwise conf can lie below 2^-8)
 *     valid    int64 [R]: the images of the row whose keys are not INVALID
 * Integer (LDS) atomics only and no floating-point sum: the same bits on every run, however the N images were cut into record calls.  Two
 * launches, no scratch, no allocation, no synchronisation: capturable.
 * BMI_ERR_INVALID (decided before any HIP call): a null pointer other than edges_in, a count below 1, N > N_cap, n_bins outside [1, 64], an
 * edges_in entry that is not finite or is below its predecessor.  BMI_ERR_UNSUPPORTED: C > 128, R > 64, N >= 2^22.  An error writes nothing. */
int bmi_classwise_table(const uint32_t* pkeys, const int32_t* labels_rec, int32_t R, int32_t C, int32_t N, int32_t N_cap, int32_t n_bins,
                        const float* edges_in /* host [n_bins + 1] or NULL */, float* edges_out, int64_t* count, int64_t* hits,
                        int64_t* conf_fix, int64_t* valid, bmi_stream stream);

/* Rank quality of the per-image uncertainty scores: do the wrong predictions — or out-of-distribution inputs — carry the high uncertainty?
 * Per row the stable order of the images by a score key, the risk-coverage curve of selective prediction and the Mann-Whitney count of the
 * AUROC, as exact integers on the device (csrc/ranking.hip; train.ranking.score_keys_numpy / rank_quality_numpy restate both calls).  The
 * reference's hardware evaluation prints the mean predictive entropy of random-noise inputs (Hardware_Artifact/bayes_hw/data_utils.py:72-90,
 * metric_utils.py:3-6); these two calls read the same data per image.
 *
 * bmi_score_record turns non-negative scores into 32-bit keys whose ascending unsigned order is "most certain first": score float64 [R][B]
 * (device) -> columns n0 .. n0 + B - 1 of ukeys uint32 [R][N_cap].  Per (row, image):
 *     f = (float) score (round to nearest)
 *     valid_keys given (uint32 [R][N_cap], the same columns: the reliability records' keys) and valid_keys[r][n] == 0:
 *                                   ukey = 0xFFFFFFFF (INVALID: the image is in no count), not counted
 *     otherwise f NaN, infinite or below zero:   ukey = 0xFFFFFFFF and *counter += 1 (device int32, ADDED to, or NULL: not counted)
 *     otherwise b = the bit pattern of f + 0.0f (-0.0 becomes +0.0; b <= 0x7F7FFFFF):
 *                                   direction +1 (an uncertainty): ukey = b;   direction -1 (a confidence): ukey = 0x7F7FFFFF - b
 * One launch; capturable.  BMI_ERR_INVALID (decided before any HIP call): a NULL score or ukeys, R / B / N_cap below 1, n0 < 0,
 * n0 + B > N_cap, direction not +1 or -1.  BMI_ERR_UNSUPPORTED: R > BMI_RANK_MAX_ROWS, B > BMI_RANK_MAX_IMAGES.  An error writes nothing.
 *
 * bmi_rank_quality reads columns 0 .. N-1 of ukeys and of positive uint8 [R][N_cap] (1 where the image is what the score should flag: a
 * wrong prediction, a noise image).  The valid images of row r are those with ukey != 0xFFFFFFFF (a ukey above 0x7F7FFFFF, which no
 * record call writes, is read as INVALID), m of them, in the STABLE ascending order: by ukey, ties by image index.  Every output is
 * OVERWRITTEN in columns 0 .. N-1; columns >= N are not touched:
 *     rank         int32 [R][N_cap]    the image's position 0 .. m-1 in that order, -1 for an invalid image
 *     sorted_keys  uint32 [R][N_cap]   position k: the ukey of the image ranked k; positions m .. N-1: 0xFFFFFFFF
 *     curve        int32 [R][N_cap]    position k: the positive images at positions 0 .. k; positions m .. N-1: n_pos
 *     counts       int64 [R][3]        m, n_pos (valid and positive), U2 = the sum over the pairs (positive i, negative j), both valid, of
 *                                      2 [ukey_j < ukey_i] + [ukey_j == ukey_i]:  AUROC = U2 / (2 n_pos n_neg), ties counted half
 *     aurc_sum     float64 [R]         ((0.0 + curve[0] / 1) + curve[1] / 2) + ... + curve[m-1] / m: ascending k from 0.0, each quotient the
 *                                      correctly rounded float64 division of the two integers converted exactly, no fused multiply-add,
 *                                      added by one wave in order; 0.0 when m = 0.  AURC = aurc_sum / m is formed on the host.
 * Ranking by counting, O(N^2) compare steps per row and no sort: exact and stable by construction.  No floating-point atomics (integer
 * LDS atomics only): the same bits on every run and for every cut of the images into record calls; no NaN reaches an output.  Two
 * launches, no allocation, no synchronisation: capturable.  scratch: the per-tile integer partials, bmi_rank_scratch_bytes = R *
 * ceil(N / BMI_RANK_TILE_I) * 3 * 8 (0 for arguments the call refuses).
 * BMI_ERR_INVALID (decided before any HIP call): a null pointer, R / N below 1, N > N_cap.  BMI_ERR_UNSUPPORTED: N > BMI_RANK_MAX_IMAGES
 * (2^17: a radix sort for longer rows is not built), R > BMI_RANK_MAX_ROWS (1024).  BMI_ERR_NOMEM: scratch too small.  An error writes
 * nothing. */
#define BMI_RANK_TILE_I 512         /* images whose keys one workgroup of the counting kernel keeps in registers */
#define BMI_RANK_TILE_J 2048        /* images whose keys it stages in LDS per step */
#define BMI_RANK_MAX_IMAGES 131072
#define BMI_RANK_MAX_ROWS 1024
int bmi_score_record(const double* score /*[R][B]*/, int32_t R, int32_t B, int32_t direction, const uint32_t* valid_keys /*[R][N_cap] or NULL*/,
                     int32_t n0, int32_t N_cap, uint32_t* ukeys /*[R][N_cap]*/, int32_t* counter /* device [1], ADDED to; NULL: not counted */,
                     bmi_stream stream);
size_t bmi_rank_scratch_bytes(int32_t R, int32_t N);
int bmi_rank_quality(const uint32_t* ukeys, const uint8_t* positive, int32_t R, int32_t N, int32_t N_cap, int32_t* rank, uint32_t* sorted_keys,
                     int32_t* curve, int64_t* counts /*[R][3]*/, double* aurc_sum /*[R]*/, void* scratch, size_t scratch_bytes,
                     bmi_stream stream);

/* Exit-policy sweep: for many thresholds at once, where every image would leave under the staged engine's rule and what the predictions
 * taken there are worth — the trade-off table of the reference's get_confidence_exiting_values (SA/train/results_analyzer.py:543-566:
 * confidence_exiting, flop_saver, flop_saver_ensembled over eleven thresholds) from per-image records that stay on the device
 * (csrc/exit_policy.hip; train.exit_policy.exit_stat_numpy / exit_policy_numpy restate both calls).
 *
 * bmi_exit_stat_record writes the decision statistics of a batch: S1 float64 [E][B][C] (device: the sums of t_count samples'
 * probabilities, as every forward call leaves them) -> columns n0 .. n0 + B - 1 of stat float64 [2][E][N_cap].  stat[ens][e][n0 + b] is the
 * number bmi_forward_mcd_exit_staged compares with its threshold at exit e under (criterion, ensemble = ens) — compiled from the same
 * function (csrc/exit_rule.h), so the same bits: float64, no fused multiply-add,
 *     p_c = S1[e][b][c] / t                                                 (ens 0)
 *     p_c = (((0.0 + S1[0][b][c] / t) + S1[1][b][c] / t) + ... ) / (e + 1)   (ens 1, weights NULL)
 *     p_c = ((0.0 + w[e][0] * (S1[0][b][c] / t)) + w[e][1] * (S1[1][b][c] / t)) + ...   up to exit e   (ens 1, weights device [E][E])
 *     BMI_EXIT_CONFIDENCE: max_c p_c;   BMI_EXIT_MARGIN: top-1 minus top-2 (0 on a tie; top-1 alone when C = 1)
 * A NaN statistic is stored as it is: the rule's stat > threshold is false for it, here as there.  One launch, no allocation, no
 * synchronisation: capturable.  BMI_ERR_INVALID (decided before any HIP call): a NULL S1 or stat, E / B / C / t_count / N_cap below 1,
 * n0 < 0, n0 + B > N_cap, an unknown criterion.  BMI_ERR_UNSUPPORTED: E > 32, C > 128.  An error writes nothing.
 *
 * bmi_exit_policy_sweep reads columns 0 .. N-1 of stat [E][N_cap] — ONE plane of the record (ens 0: the record's base; ens 1: base +
 * E * N_cap) —, G thresholds (device float64, any order, repeats allowed) and the outcome rows keys / hit / nll / brier [E][N_cap] each: the
 * reliability records (bmi_reliability_record) offset to row kind * E — kind 0 for the exits' own predictions, kind 1 for the equal-mean
 * exit ensembles'.  Per threshold g and image n:
 *     e* = the lowest e in [first_exit, E-2] with stat[e][n] > thresholds[g] (strict, float64), E-1 if there is none.  The statistic decides
 *          alone: e* is the exit_of_image bmi_forward_mcd_exit_staged assigns under that threshold.  A NaN threshold lets nobody leave
 *          early (it is on the device and cannot be refused before a HIP call).
 *     exit_of[g][n] = e*                                     uint8 [G][N_cap], or NULL
 *     keys[e*][n] == 0 (a bad label, a non-finite row):      invalid[g] += 1; the selected record is all zeros, which the table and KDE
 *                                                            calls skip
 *     otherwise  count[g][e*] += 1,  hits[g][e*] += hit[e*][n] != 0,  and the selected records sel_keys / sel_hit / sel_nll / sel_brier
 *                [G][N_cap] (all four or none; G <= BMI_POLICY_MAX_RECORD_ROWS) are copies of the four records at (e*, n): a valid R = G
 *                record set for bmi_reliability_table, bmi_reliability_kde and bmi_score_record(valid_keys =) — the ECE, KDE-ECE, NLL and
 *                Brier of the exited predictions, with the bit contracts of those calls.
 * count, hits int64 [G][E] and invalid int64 [G] are OVERWRITTEN; exit_of and the selected records in columns 0 .. N-1 only.  Integer
 * LDS atomics and integer partial sums only, no floating-point atomics: the same bits on every run and for every cut of the images into
 * record calls.  Two launches, no allocation, no synchronisation: capturable.  scratch: bmi_exit_policy_scratch_bytes = min(ceil(N / 128),
 * 128) * G * (2 E + 1) * 4 (0 for arguments the call refuses).
 * BMI_ERR_INVALID (decided before any HIP call): a NULL required pointer, some but not all of the four sel_ pointers, E / N / G below 1,
 * N > N_cap, first_exit outside [0, E).  BMI_ERR_UNSUPPORTED: E > 32, G > BMI_POLICY_MAX_THRESHOLDS, N >= 2^22, selected records with
 * G > BMI_POLICY_MAX_RECORD_ROWS.  BMI_ERR_NOMEM: scratch too small.  An error writes nothing. */
#define BMI_POLICY_MAX_THRESHOLDS 1024
#define BMI_POLICY_MAX_RECORD_ROWS 64      /* = what bmi_reliability_table takes as R */
int bmi_exit_stat_record(const double* S1 /*[E][B][C]*/, int32_t E, int32_t B, int32_t C, int32_t t_count,
                         int32_t criterion /*BMI_EXIT_CONFIDENCE | BMI_EXIT_MARGIN*/, const double* weights /*device [E][E] or NULL*/, int32_t n0,
                         int32_t N_cap, double* stat /*[2][E][N_cap]*/, bmi_stream stream);
size_t bmi_exit_policy_scratch_bytes(int32_t E, int32_t N, int32_t G);
int bmi_exit_policy_sweep(const double* stat /*[E][N_cap]*/, int32_t E, int32_t N, int32_t N_cap, int32_t first_exit,
                          const double* thresholds /*device [G]*/, int32_t G, const uint32_t* keys, const uint8_t* hit, const double* nll,
                          const double* brier /*outcome rows: [E][N_cap] each*/, int64_t* count /*[G][E]*/, int64_t* hits /*[G][E]*/,
                          int64_t* invalid /*[G]*/, uint8_t* exit_of /*[G][N_cap] or NULL*/, uint32_t* sel_keys, uint8_t* sel_hit,
                          double* sel_nll, double* sel_brier /*[G][N_cap] each, all four or none*/, void* scratch, size_t scratch_bytes,
                          bmi_stream stream);

/* Per-op-kind HIP-event timing of bmi_forward_mcd (off by default; adds two event records per
 * launch).  bmi_profile_read synchronises the recorded events and resets the accumulators. */
int bmi_profile_enable(bmi_handle h, int32_t enable);
int bmi_profile_read(bmi_handle h, double ms[BMI_PROFILE_SLOTS], int64_t launches[BMI_PROFILE_SLOTS]);
/* The BMI_OP_CONV slot of the LAST bmi_profile_read, split by the kernel that took each launch, with the
 * algorithmic FLOPs (2 * MACs) and algorithmic HBM bytes (every operand tensor and the weights read once, the output
 * written once) of those launches: what bench.py prices against the MFMA and the HBM roofline. */
#define BMI_CONV_FAMILY_PATCH 0 /* conv3x3_patch_kernel  */
#define BMI_CONV_FAMILY_WIDE 1  /* conv_igemm_wide_kernel */
#define BMI_CONV_FAMILY_IGEMM 2 /* conv_igemm_kernel */
#define BMI_CONV_FAMILY_PW 3    /* conv3x3_pw_kernel */
#define BMI_CONV_FAMILY_STREAM 4 /* conv1x1_stream_kernel */
#define BMI_CONV_FAMILY_S2 5    /* conv3x3_s2_kernel */
#define BMI_CONV_FAMILY_SPLIT 6 /* conv_split_kernel (the split engines; FLOPs = algorithmic, i.e. one third of the MFMA work) */
#define BMI_CONV_FAMILY_SEAM 7  /* conv1x1_seam_kernel (two 1x1 convs of neighbouring Bottlenecks in one launch; FLOPs and bytes of both) */
#define BMI_CONV_FAMILIES 8
int bmi_profile_conv_families(bmi_handle h, double ms[BMI_CONV_FAMILIES], int64_t launches[BMI_CONV_FAMILIES],
                              double flops[BMI_CONV_FAMILIES], double bytes[BMI_CONV_FAMILIES]);

/* The individual launches behind the most recent bmi_profile_read, in launch order: op kind (BMI_OP_*), conv family (-1 for
 * non-conv ops), the op's output tensor id (identifies the op in the graph), images carried, device milliseconds, algorithmic
 * FLOPs and HBM bytes (conv ops).  *count = number of launches recorded; at most `capacity` entries are written; any array
 * may be NULL.  (tools/per_launch.py prints the table: which launch of a model sits where against its roofline.) */
int bmi_profile_launches(bmi_handle h, int32_t capacity, int32_t* count, int32_t* kind, int32_t* family, int32_t* out_tensor,
                         int32_t* images, double* ms, double* flops, double* bytes);

/* ---- single-kernel entry points (unit parity tests) -------------------------------------- */

/* keep bits (0/1 bytes) of elements 0..n-1 of stream (seed, site, t). */
int bmi_philox_mask(uint8_t* keep, int64_t n, uint64_t seed, int32_t site, int32_t t, float p, bmi_stream stream);

int bmi_stem_conv_fwd(const float* x_nchw, const float* weight, const float* scale, const float* bias, void* out_nhwc,
                      int32_t n, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t ksize, int32_t stride,
                      int32_t pad, int32_t relu, bmi_stream stream);

/* out[n] = conv(in[n % in_mod]) * scale + bias (+ res[n % res_mod]) (ReLU) (site); `batch` is
 * the per-sample image count B used by the site's element index (n = t_local*B + b). */
/* keep bits (1 bit per element, byte g = elements 8g..8g+7) of an elementwise site for the folded batch
 * n = samples*batch images of hw pixels x c channels */
int bmi_mask_bits(void* bits, int32_t n, int32_t hw, int32_t c, const bmi_site* site, int32_t batch, int32_t t0,
                  uint64_t seed, bmi_stream stream);

/* in_keep_bits (or NULL): input-side MC-dropout — image n reads in[n % in_mod] with the dropped elements of
 * folded image n zeroed while staging; out_mul multiplies the BN scale (pass 1/(1-p) then, else 1). */
int bmi_conv_igemm_fwd(const void* in, const void* in_keep_bits, float out_mul, const void* weight,
                       const float* scale, const float* bias, const void* res, void* out,
                       int32_t n, int32_t in_mod, int32_t res_mod, int32_t h, int32_t w, int32_t cin, int32_t cout,
                       int32_t ksize, int32_t stride, int32_t pad, int32_t relu, const bmi_site* site,
                       int32_t batch, int32_t t0, uint64_t seed, int32_t mask_cnt0, bmi_stream stream);

/* out = relu?( conv3x3_s1_p1(in; weight) + conv1x1_stride2(in2; weight2) + bias ), the fused BasicBlock tail
 * with downsample (both BN scales folded into the weights); in2 is [n][2h][2w][cin2]. */
int bmi_conv3x3_shortcut_fwd(const void* in, const void* weight, const void* in2, const void* weight2, const float* bias,
                             void* out, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t cin2,
                             int32_t relu, bmi_stream stream);

/* The seam between two Bottleneck blocks as one launch (csrc/conv1x1_seam.hip): out_wide = relu(bn3(conv1x1(in; weight3)) + res) [n][h][w][cw] and
 * out_narrow = relu1?(bn1(conv1x1(out_wide; weight1))) [n][h][w][cn], the second conv fed from the tile the first has just produced (out_wide
 * is written, not read back).  cmid % 64 == 0, cmid <= 512, cw % 128 == 0, cn = 128 (256 too under "conv_seam" >= 2: slower than the
 * two launches, kept for the tests); anything else, and launches under the kernel's minimum grid, run as the two launches.  Bit-identical
 * to bmi_conv_igemm_fwd twice.  Replaces conv3 + bn3 + shortcut add + ReLU of one Bottleneck and conv1 + bn1 + ReLU of the next (the
 * Bottleneck form of SA/models/resnet18/resnet18.py:51-85; BASELINE configs[4]). */
int bmi_conv1x1_seam_fwd(const void* in, const void* weight3, const float* scale3, const float* bias3, const void* res, void* out_wide,
                         const void* weight1, const float* scale1, const float* bias1, void* out_narrow, int32_t n, int32_t h, int32_t w,
                         int32_t cmid, int32_t cw, int32_t cn, int32_t relu1, bmi_stream stream);

/* Two convolutions that read the SAME input with the same geometry, as one launch of the 256 x 256-tile kernel:
 * out_a = relu?(bn_a(conv(in; weight_a))) [..][cout_a], out_b likewise [..][cout_b].  cout_a % 128 == 0,
 * (cout_a + cout_b) % 256 == 0, cin % 64 == 0.  Replaces the pair layerN[0].conv1 / ex{N-1}conv1 of
 * ResNet18MCEarlyExit.forward (SA/models/resnet18/resnet18.py:306, :318, :329 next to :280-299). */
int bmi_conv_pair_fwd(const void* in, const void* weight_a, const float* scale_a, const float* bias_a, void* out_a,
                      const void* weight_b, const float* scale_b, const float* bias_b, void* out_b, int32_t n,
                      int32_t in_mod, int32_t h, int32_t w, int32_t cin, int32_t cout_a, int32_t cout_b, int32_t ksize,
                      int32_t stride, int32_t pad, int32_t relu, bmi_stream stream);

int bmi_mask_apply(const void* in, void* out, int32_t n, int32_t in_mod, int32_t hw, int32_t c, const bmi_site* site,
                   int32_t batch, int32_t t0, uint64_t seed, int32_t mask_cnt0, bmi_stream stream);

int bmi_maxpool2(const void* in, void* out, int32_t n, int32_t h, int32_t w, int32_t c, bmi_stream stream);

/* One exit head for samples t0 .. t0+tc-1 of `batch` images, fused (csrc/head_fused.hip):
 *   feat[n][k]   = mean_hw(relu(in[n % in_mod][hw][k])) (site)          n = t_local*batch + b, in_mod = batch or batch*tc
 *   logits[n][c] = feat[n] . weight_pad[c] + bias[c]  (site_logits: ELEMENTWISE dropout on the [batch, out_dim] logits, the
 *                  converter/pytorch rule wraps the last Linear too, nn2bnn.py:33-45; NULL = none)
 *   S1[b][c] += sum_t softmax(logits)[c], S2 += sum_t softmax^2, SL += sum_t logits        (float64 [batch][out_dim])
 * `in` is fp16 / bf16 (in_is_f32 = 0, per unit_entry_dtype) or fp32; weight_pad fp32 [ceil32(out_dim)][k], rows >= out_dim
 * zero; k % 32 == 0, out_dim <= 128.  No per-sample probabilities are materialised. */
int bmi_head_fused(const void* in, int32_t in_is_f32, int32_t in_mod, int32_t hw, int32_t k, const float* weight_pad,
                   const float* bias, int32_t out_dim, const bmi_site* site, const bmi_site* site_logits, int32_t batch, int32_t t0,
                   int32_t tc, uint64_t seed, int32_t mask_cnt0, double* S1, double* S2, double* SL, bmi_stream stream);

/* One exit head with everything the fused kernel's launchers take (csrc/kernels.h, HeadArgs), and packs of them: bmi_head_fused reaches the
 * plain form only.  Fields as bmi_head_fused's arguments, then:
 *   SH              [batch] float64 accumulator of the per-sample softmax entropies in nats, or NULL (S1 / S2 / SL all NULL with `logits`
 *                   given: logits only, no accumulator is touched)
 *   image_map       device int32 [n_mapped]: the launch covers these images only (any order, no repeats), or NULL: all `batch` images
 *   image_offset    batch index of this launch's image 0 in the sites' index space (bmi_forward_mcd_images): the logits site adds it to the
 *                   image index, a stochastic feature site gets the element offset image_offset * k, which must be a multiple of 64
 *                   (BMI_ERR_UNSUPPORTED otherwise, bmi_image_offset_ok's rule)
 *   logits          per-sample raw logits out, sample tl of the launch, class c of image b -> logits[tl * logits_tstride + b * out_dim + c]
 *                   (float32; logits_tstride in elements, >= batch * out_dim: BMI_ERR_INVALID otherwise), or NULL
 *   scratch         float64 [ceil(tc / 32)][3][batch][out_dim], plus [ceil(tc / 32)][batch] behind it when SH is given: the partial sums
 *                   of a launch with tc > 32, joined in group order (bit-reproducible); NULL: hardware float64 atomics for tc > 32.  Every
 *                   head of a pack needs its own.
 *   inv_tau         float32(1 / tau) of temperature scaling, or 0: off
 *   vec_scale / vec_bias     device float32 [out_dim] of vector scaling (both or neither), or NULL
 *   mat / mat_bias  device float32 [out_dim][out_dim] (row = output class) and [out_dim] of matrix scaling (both or neither), or NULL
 * At most one of inv_tau, vec_*, mat* (BMI_ERR_INVALID).  S1 / S2 / SH are those of the mapped logits z, SL and `logits` stay raw. */
typedef struct bmi_head_ex {
    const void* in;
    int32_t in_is_f32, in_mod, hw, k;
    const float* weight_pad;
    const float* bias;
    int32_t out_dim;
    const bmi_site* site;
    const bmi_site* site_logits;
    int32_t batch, t0, tc;
    uint64_t seed;
    int32_t mask_cnt0;
    double *S1, *S2, *SL, *SH;
    const int32_t* image_map;
    int32_t n_mapped, image_offset;
    float* logits;
    size_t logits_tstride;
    double* scratch;
    float inv_tau;
    const float *vec_scale, *vec_bias, *mat, *mat_bias;
} bmi_head_ex;

/* n_heads == 1: one launch of heads[0].  2 <= n_heads <= 8: the heads in ONE launch (the engine's pack, csrc/head_fused_body.h); they must
 * agree in out_dim, input kind, batch, tc and in which of S1 / SH / scratch / the calibration maps they carry, and none may have an
 * image_map (BMI_ERR_UNSUPPORTED; the engine launches such heads one by one).  Returns the launcher's code; nothing is written on an error. */
int bmi_head_fused_ex(const bmi_head_ex* heads, int32_t n_heads, bmi_stream stream);

/* Hidden dense layer in fp32 (BMI_OP_DENSE): out[n][c] = relu?(in[n % in_mod] . weight[c] + bias[c]) (site on the
 * [batch, cout] tensor, sample index n / batch + t0).  `in` is fp16 (in_is_f32 = 0) or fp32 [.][k]; weight fp32 [cout][k];
 * k % 32 == 0, cout % 64 == 0.  Replaces the Dense 512 layers of the VGG-11 classifier stack
 * (Hardware_Artifact/bayes_hw/models/models.py:262-281) with their dropout (:268-281). */
int bmi_dense_f32(const void* in, int32_t in_is_f32 /* 0: 16-bit (unit_entry_dtype), 1: fp32 */, const float* weight, const float* bias, float* out, int32_t n,
                  int32_t in_mod, int32_t k, int32_t cout, int32_t relu, const bmi_site* site, int32_t batch, int32_t t0,
                  uint64_t seed, int32_t mask_cnt0, bmi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYESNN_FPGA_AMD_H */
