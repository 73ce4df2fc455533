/*
 * pointdsc_hip.h -- C ABI of libpointdsc_hip.so (gfx950 / MI355X).
 *
 * The reference (XuyangBai/PointDSC) has no FFI of its own: its hot path is the Python method
 * PointDSC.forward(data) in testing mode (reference models/PointDSC.py:128-197) built from stock ATen
 * calls.  This header is the boundary a maintainer binds with ctypes: one entry
 * point per reference stage (so each stage can be parity-checked on its own) plus one whole-path call.
 * Every entry point cites the reference lines it replaces.
 *
 * Two tiers (r05):
 *   PRODUCT BOUNDARY -- what a caller of the reference's module needs: pdsc_forward (one call struct: testing forward, uniform or
 *     ragged, on one or two streams; validation forward; range probe); the weight packers pdsc_wpack_floats / _offset,
 *     pdsc_wsplit_bytes / _offset / _build; the workspace queries pdsc_workspace_bytes / _offset; pdsc_version / pdsc_last_error; and, for the callers either
 *     side of the path (SURVEY.md section 8 f-2 .. f-4), pdsc_match_* / pdsc_select_correspondences / pdsc_build_corr_pos,
 *     pdsc_sm_baseline*, pdsc_pmc_*, pdsc_cal_confidence, pdsc_eval_stats, pdsc_*_loss*, pdsc_pointwise_train_*, pdsc_optim_*, pdsc_icp_*, pdsc_information_*, pdsc_voxel_*, pdsc_cloud_*.
 *   STAGE LEVEL -- one entry point per reference stage (sections a-1 .. a-11 below), the plan / size queries that go with them,
 *     pdsc_selftest_* and the diagnostic hooks.  The forward does not go through them (it calls the same launchers directly); they
 *     exist so that every stage can be parity-checked on its own (tests/test_gpu_parity.py), for the tools, and for a maintainer
 *     who keeps the reference's module and swaps single stages.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HIP, fp32 unless stated), caller-owned, never retained;
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it: no host
 *     synchronisation, no allocation (graph-capturable).  Results depend on the arguments only.  Process-global
 *     state is limited to: the per-(kernel, device) dynamic-LDS opt-in table (mutex-protected), the per-device event that orders
 *     opt-in register-resident spectral-matching launches (mutex-protected), the error string
 *     (thread-local), and the opt-in DIAGNOSTIC hooks -- pdsc_profile_* event timing, pdsc_attention_trace,
 *     pdsc_layer_trace -- which are process-wide switches and not thread-safe: use them from one thread.
 *     The product library reads NO environment variable: everything that selects a kernel or changes arithmetic is a field
 *     of pdsc_config or an argument.  The PDSC_* tuning / A-B knobs DESIGN.md lists exist in experiments builds only
 *     (-DPDSC_EXPERIMENTS, `python -m pointdsc_amd.build --experiments` -> libpointdsc_hip_exp.so; pdsc_experiments_enabled());
 *   - tensors are dense row-major; `bs` = number of correspondence sets (pairs), `N` = correspondences
 *     per pair, `C` = 128 channels, `S` = number of seeds, `k` = neighbours per seed;
 *   - bs > 1 means bs independent pairs, i.e. the reference called once per pair (the reference's
 *     testing mode asserts bs == 1, models/PointDSC.py:210,414);
 *   - return value 0 = enqueued, < 0 = rejected (pdsc_last_error() tells why); nothing is enqueued
 *     on rejection.
 */
#ifndef POINTDSC_HIP_H
#define POINTDSC_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDSC_VERSION 10
#define PDSC_CHANNELS 128        /* num_channels of every released PointDSC model */
#define PDSC_MAX_K 64            /* neighbours per seed handled by one wavefront   */
#define PDSC_MAX_POWER_ITERS 32

enum pdsc_status {
    PDSC_OK = 0,
    PDSC_ERR_ARG = -1,           /* bad argument (null pointer, unsupported size) */
    PDSC_ERR_WORKSPACE = -2,     /* workspace too small                           */
    PDSC_ERR_LAUNCH = -3         /* HIP launch error                              */
};

/* Constructor arguments of reference PointDSC.__init__ (models/PointDSC.py:81-91) that the path uses. */
typedef struct pdsc_config {
    int in_dim;              /* 6 (1..16: datasets/ThreeDMatch.py:299-312 builds 6 / 9 / 12) */
    int num_layers;          /* 12 in the released snapshots                   */
    int num_channels;        /* must be PDSC_CHANNELS                          */
    int num_iterations;      /* power-iteration cap, 10                        */
    int k;                   /* neighbours per seed, 40                        */
    int refine_iters;        /* 20 (models/PointDSC.py:416-418)                */
    float inlier_threshold;  /* hypothesis-scoring threshold (:328,:335)       */
    float nms_radius;        /* NMS radius R (:174)                            */
    float refine_threshold;  /* 0.10 if inlier_threshold == 0.10 else 1.2 (:415-418) */
    int attention_precision; /* enum pdsc_attention_precision: how the two N x N x C contractions are evaluated */
    int compat_format;       /* enum pdsc_compat_format: how the forward stores the N x N spatial-consistency matrix  */
    int layer_gemm;          /* enum pdsc_layer_gemm: arithmetic of the fc_message / PointCN GEMMs in the fused layer kernel */
    int att_leaves;          /* enum pdsc_att_leaves: summation tree of the attention's key dimension (split-precision modes) */
    int value_fold;          /* enum pdsc_value_fold: fc_message's first conv folded into the value projection                */
} pdsc_config;

/* fc_message's first conv (+ its BatchNorm, W1f / b1f) folded into the value projection (models/PointDSC.py:12-20,36-44).  Each
 * softmax row sums to 1, so  W1f (sum_j p_ij (Wv f_j + bv)) + b1f = sum_j p_ij (W1f Wv) f_j + (W1f bv + b1f)  exactly in real
 * arithmetic: the head projects V' = (W1f Wv) f with C/2 = 64 channels, the attention contracts P V' over 64 channels instead
 * of 128 (half the P V MFMAs, half the V^T planes and partials), and the layer kernel adds b' = W1f bv + b1f to the merged
 * 64-channel message and goes straight to ReLU -> fc2 (no fc1 GEMM).  Same three-MFMA split arithmetic per product; only the
 * association order of an fp32-class computation changes.  W1f Wv is formed in fp64 from the packed fp32 matrices and rounded
 * once to fp32 (pdsc_wsplit_build).
 *   OFF (0): the 128-channel value path, layouts and bits of library version 8.
 *   ON  (1): valid with a split-precision attention and layer_gemm = PDSC_LAYER_GEMM_H3 only (config check).  pdsc_forward
 *            folds on the point-fragment hand-offs (leaf form, and key splits of 2..8) of calls with N <= PDSC_VALUE_FOLD_MAX_N
 *            (N = the longest pair of a ragged batch); a per-launch plan whose key split is 1 or more than 8, and larger N, keep
 *            the 128-channel path.                                                             [default of the Python module]
 * The size bound: at the multiway evaluation size (N = 20000) the reference's recorded outputs pin a golden pair whose winning
 * seed has its k-th and (k+1)-th neighbour distances 1.2e-7 apart, resolved by the last bit of the fp32 feature Gram; the
 * fold's association order resolves it to the other side (both inside the contract).  The calls beyond the bound keep the
 * 128-channel results that record was made with. */
enum pdsc_value_fold { PDSC_VALUE_FOLD_OFF = 0, PDSC_VALUE_FOLD_ON = 1 };
#define PDSC_VALUE_FOLD_MAX_N 16384

/* How the N keys of a query are summed (models/PointDSC.py:41-42: one softmax-weighted sum per query) when the key range is
 * cut so that one pair can fill the chip.  A LEAF is a run of 32-key tiles accumulated from a fresh online-softmax state;
 * the fused layer kernel merges the partials (O, m, l) in order (weights exp2(m - max m), one reciprocal) while it loads them.
 *   PER_LAUNCH (0): one partial per key split, the split planned per launch from (batch, N): the bits of a pair depend on how
 *                   many pairs share its launch (all within the contract; the r01-r04 results).
 *   CANONICAL  (1): pdsc_attention_leaf_count(N) leaves, a function of N alone; the launch plan only decides WHICH workgroup
 *                   computes a leaf (the key split is a divisor of the leaf count), never the arithmetic -- a pair's result is
 *                   bit-identical at every batch size, on one GPU or sharded over eight.  Split-precision attention with the
 *                   H3 layer kernel only (the other arithmetic modes keep PER_LAUNCH).        [default of the Python module]
 *   2 .. 8        : that many leaves (tuning). */
enum pdsc_att_leaves { PDSC_LEAVES_PER_LAUNCH = 0, PDSC_LEAVES_CANONICAL = 1 };

/* Arithmetic of the point-wise GEMMs whose results land on the residual stream (fc1..fc3 of fc_message, PointCN;
 * models/PointDSC.py:12-23,56-61) inside the fused layer kernel (split-precision attention modes).  H3 runs on
 * layer_h3_kernel, or on the bit-identical layer_h3_coop_kernel for launches of at most 2560 tiles
 * (pdsc_layer_h3_uses_coop(bs, N) == 1); F32 on layer_wave_kernel, or on the workgroup-per-tile kernel for small problems
 * (pdsc_layer_prefers_block(bs, N) == 1):
 *   F32: v_mfma_f32_32x32x2_f32, exact fp32 products (600 MFMAs x 64 matrix-pipe cycles per 32-point tile).
 *   H3 : every fp32 operand as fp16 hi + fp16 lo' (lo' = (x - hi) * 2048), product = hi*hi + (hi*lo' + lo'*hi) / 2048 on
 *        v_mfma_f32_32x32x16_f16 with fp32 accumulation: ~2^-21 relative error per product (as the fp16 hi/lo split of the
 *        attention operands), 216 MFMAs x 32 cycles per tile.  Operands must stay inside the fp16 range
 *        (|x| < 65504); the network's activations and weights are O(1). */
enum pdsc_layer_gemm { PDSC_LAYER_GEMM_F32 = 0, PDSC_LAYER_GEMM_H3 = 1 };

/* Order of the [rows][C] fp32 matrices handed from the attention to the fused layer kernel (key-split partials) and from
 * one fused layer launch to the next (featB = the residual): plain rows, or point-fragment order (PF) -- rows in tiles of 32,
 * a tile = [q = 0..15][lane = 0..63][4 floats] with lane (l31 = lane & 31, h = lane >> 5) holding channels 8q + 4h .. + 3 of
 * row l31: exactly the registers of the producing and of the consuming wavefront, so every store / load instruction moves
 * 1 KiB of consecutive memory and neither side transposes through LDS.  PF buffers are padded to whole tiles per pair
 * (ceil(N / 32) * 32 rows); padding rows hold copies of the pair's last row.  Only the H3 layer kernel reads / writes PF. */
enum pdsc_partial_layout { PDSC_PARTIALS_ROWS = 0, PDSC_PARTIALS_PF = 1 };
enum pdsc_layer_io { PDSC_IO_PARTIALS_PF = 1, PDSC_IO_RES_PF = 2, PDSC_IO_FEATB_PF = 4 };

/* Storage of the spatial-consistency matrix between its build and the 12 attention launches that stream it
 * (the split-precision modes only; PDSC_ATT_FP32 always uses fp32 storage):
 *   U16: unorm16, value = round(c * 65535) / 65535 with c evaluated on the hardware's 1-ulp square root (r03: the exact
 *        sqrt / divide of the fp32 matrix made the build instruction-bound) -- within 2 units (3e-5) of the fp32 matrix,
 *        the diagonal exactly 1, symmetric bit for bit (r05: with the attention operands as fp16 pairs this is the largest
 *        arithmetic difference left between the default and the exact-fp32 configuration); half the HBM stream (2 N^2 instead of 4 N^2 bytes per layer per pair), half the workspace; +4.6 % pairs/s
 *        at N=5000 (tools/ab_forward.py).
 *   F32: the fp32 matrix of pdsc_spatial_compat, bit-identical to the reference's.
 * The Python module defaults to U16 (parity census equal to F32's); the C struct has no default. */
enum pdsc_compat_format { PDSC_COMPAT_F32 = 0, PDSC_COMPAT_U16 = 1 };

/* Arithmetic of the attention contractions (models/PointDSC.py:39,42).  Softmax, accumulation, outputs: fp32 in both.
 *   FP16X3: every fp32 operand split into fp16 hi + fp16 lo (lo = x - hi, unscaled: 22 significant bits down to fp16's
 *           denormal floor, which the gfx950 f16 MFMA honours), three v_mfma_f32_32x32x16_f16 per operand pair
 *           (hi*hi + hi*lo + lo*hi) into one fp32 accumulator: ~2^-21 relative error per product.  Operands must stay inside the
 *           fp16 range (|q|, |k|, |v| < 65504; the softmax weights are kept in (0, 32768] by construction): the Python module
 *           probes the first forward of a checkpoint and falls back to FP32 outside it (pdsc_forward, PDSC_FORWARD_PROBE).
 *           Also used for the q|k|v projection (its results only feed the attention); the GEMMs whose results
 *           land on the residual stream (PointCN, fc_message) follow pdsc_config.layer_gemm.           [default]
 *           Rounds 1-4 split into bf16 pairs (2^-16 per product, fp32's range): on trained-like KITTI weights, whose
 *           confidence logits reach 33, that left the logits up to 0.27 from the reference's; the fp16 pairs leave 0.04
 *           (exact fp32: 0.017) for 1.7 % of the pairs/s (same-box A/B, profiles/r05_j_ab_split16_summary.txt).
 *   FP32  : v_mfma_f32_32x32x2_f32, exact fp32 products, 16/3 x the matrix-pipe time.
 *   FP16X3_ALL: the point-wise GEMMs too (PDSC_LAYER_KERNEL_X3): their error lands on the residual stream un-averaged.
 *           A/B record: accepted by experiments builds only.
 * BREAKING in PDSC_VERSION 8: the names PDSC_ATT_BF16X3 / PDSC_ATT_BF16X3_ALL of rounds 1-4 are GONE (they were aliases of values 0 / 2
 * in version 7).  Those modes split into bf16 pairs and had fp32's range; values 0 / 2 split into fp16 pairs and do not -- a C caller
 * that still spells the old name must not compile into different arithmetic silently.  Range contract of FP16X3: every forward
 * carries a device-side sentinel (workspace entry "range_flag", [bs] u32, pdsc_workspace_offset): a pair any of whose activations
 * reached 65504 on its way into an fp16 pair has a non-zero word there after the call AND its final_trans is returned as NaN. */
enum pdsc_attention_precision { PDSC_ATT_FP16X3 = 0, PDSC_ATT_FP32 = 1, PDSC_ATT_FP16X3_ALL = 2 };
/* (A testing forward can also leave the range words in pinned host memory: pdsc_forward_call.range_report.) */

/* ---- packed weights --------------------------------------------------------------------------
 * One flat fp32 buffer holding the model with BatchNorm (eval) folded into the preceding conv and
 * log2(e)/sqrt(C) folded into the Q projection.  Offsets (in floats) come from pdsc_wpack_offset so
 * that the host packer (pointdsc_amd/model.py) and the kernels cannot disagree.
 * All matrices are [out][in] row-major exactly like Conv1d.weight[:, :, 0]. */
enum pdsc_wsection {
    PDSC_W_LAYER0_W = 0,  /* [C][16]  in_dim (<= 16) zero-padded to 16 (encoder.layer0)       */
    PDSC_W_LAYER0_B,      /* [C]                                                             */
    PDSC_W_PCN_W,         /* per layer [C][C]     PointCN conv + BN folded                   */
    PDSC_W_PCN_B,         /* per layer [C]                                                   */
    PDSC_W_QKV_W,         /* per layer [3C][C]    rows: q (pre-scaled), k, v                 */
    PDSC_W_QKV_B,         /* per layer [3C]                                                  */
    PDSC_W_FC1_W,         /* per layer [C/2][C]   fc_message.0 + BN .1 folded                */
    PDSC_W_FC1_B,         /* per layer [C/2]                                                 */
    PDSC_W_FC2_W,         /* per layer [C/2][C/2] fc_message.3 + BN .4 folded                */
    PDSC_W_FC2_B,         /* per layer [C/2]                                                 */
    PDSC_W_FC3_W,         /* per layer [C][C/2]   fc_message.6                               */
    PDSC_W_FC3_B,         /* per layer [C]                                                   */
    PDSC_W_CLS1_W,        /* [32][C]   classification.0                                      */
    PDSC_W_CLS1_B,        /* [32]                                                            */
    PDSC_W_CLS2_W,        /* [32][32]  classification.2                                      */
    PDSC_W_CLS2_B,        /* [32]                                                            */
    PDSC_W_CLS3_W,        /* [32]      classification.4                                      */
    PDSC_W_CLS3_B,        /* [1]                                                             */
    PDSC_W_SIGMA,         /* [1]  learned feature-compat sigma   (models/PointDSC.py:97)     */
    PDSC_W_SIGMA_SPAT,    /* [1]  spatial sigma_d                (models/PointDSC.py:98)     */
    PDSC_W_NUM_SECTIONS
};

int         pdsc_version(void);
const char* pdsc_last_error(void);
/* 1 in experiments builds (A/B knobs and the opt-in record kernels compiled in), 0 in the product library */
int         pdsc_experiments_enabled(void);

/* total floats of the packed buffer / offset of a section (layer ignored for per-model sections);
 * returns -1 on bad arguments */
long long pdsc_wpack_floats(const pdsc_config* cfg);
long long pdsc_wpack_offset(const pdsc_config* cfg, int section, int layer);

/* leading dimension (floats) the compat matrix rows must have for N correspondences */
long long pdsc_compat_ld(int N);

/* bytes of scratch pdsc_forward needs (compat matrix included) */
size_t pdsc_workspace_bytes(const pdsc_config* cfg, int bs, int N, int num_seeds);

/* ---- a-1  spatial-consistency matrix -----------------------------------------------------------
 * replaces models/PointDSC.py:150-153.
 *   src_dist[i][j] = ||src_i - src_j||_2 ,  compat[i][j] = max(0, 1 - (src_dist - tgt_dist)^2 / sigma_spat^2)
 * compat: [bs][N][ld] (ld >= N, multiple of 4; columns N..ld-1 are written as 0).
 * src_dist: optional (may be NULL) [bs][N][ld]; the fused path never materialises it. */
int pdsc_spatial_compat(const float* src_keypts, const float* tgt_keypts, const float* sigma_spat,
                        float* compat, float* src_dist, long long ld, int bs, int N, void* stream);

/* Partials only (no merge: the fused layer kernel merges while it loads), compat in either storage format, partials in
 * either order (enum pdsc_partial_layout); nsplit as above (0 = the plan's), must come out > 1. */
int pdsc_sc_attention_split_partials(const void* q_split, const void* kv_tiles, const void* compat, int compat_format,
                                     long long ld, void* scratch, size_t scratch_bytes, int bs, int N, int nsplit,
                                     int partial_layout, void* stream);

/* unorm16 variant (enum pdsc_compat_format): compat_u16 [bs][N][ld] uint16, ld = pdsc_compat_ld(N) (multiple of 32),
 * value u = round(compat * 65535); inside every group of 32 columns, column 8g + 4h + e is stored at position
 * 16h + 4g + e (the order the attention kernel's accumulator holds the keys); columns >= N are 0.
 * Consumed by pdsc_sc_attention_split_u16 only. */
int pdsc_spatial_compat_u16(const float* src_keypts, const float* tgt_keypts, const float* sigma_spat,
                            unsigned short* compat_u16, long long ld, int bs, int N, void* stream);

/* Self-test hook for the two hand-rolled exact primitives of the compat kernel (correctly rounded sqrt, division
 * by a loop-invariant): sqrt_out[i] = sqrt(x[i]), div_out[i] = x[i] / divisor, both must equal the IEEE results. */
int pdsc_selftest_exact_math(const float* x, float divisor, float* sqrt_out, float* div_out, long long n, void* stream);
/* Test infrastructure: launches `workgroups` x 256 threads of a synthetic kernel that interleaves bf16 MFMAs with ordinary vector
 * work for `iters` loop iterations (2500 ~ 1 ms) -- the co-resident neighbour beside which packed fp32 instructions with operand
 * selects return wrong lanes (tools/pk_f32_repro.hip "mix").  The library ships no such instruction; the GPU
 * tests keep this neighbour on the chip while they check the entry points bit for bit.  sink: >= 1 float, never written. */
int pdsc_selftest_mfma_valu_neighbour(float* sink, int workgroups, int iters, void* stream);

/* ---- a-2  point-wise layers --------------------------------------------------------------------
 * replaces every Conv1d(kernel_size=1)[+BatchNorm1d(eval)][+ReLU] of models/PointDSC.py:12-23,54-61,107-113.
 *   Y[m][n] = act( sum_k X[m][k] * W[n][k] + bias[n] ) (+ residual[m][n])
 * X [M][ldx], W [Nout][K], Y [M][ldy]; K multiple of 8 and <= 128; ldx, ldy, ldr multiples of 4.
 * bias / residual may be NULL.  relu applies before the residual add (fc_message has no final ReLU). */
int pdsc_linear(const float* X, long long ldx, const float* W, const float* bias,
                const float* residual, long long ldr, float* Y, long long ldy,
                int M, int K, int Nout, int relu, void* stream);

/* encoder.layer0 (models/PointDSC.py:54,73): feat[m][c] = sum_d corr_pos[m][d] * W0[c][d] + b0[c];
 * corr_pos [M][in_dim] dense, W0 [C][8] (zero-padded), feat [M][C]. */
int pdsc_layer0(const float* corr_pos, int in_dim, const float* W0, const float* b0, float* feat,
                int M, void* stream);

/* Fused point-wise chain between two attention calls (one launch instead of five pdsc_linear calls):
 *   tail (msg or the partials given): feat = res + fc3(relu(fc2(relu(fc1(msg)))))    models/PointDSC.py:43-45
 *   head (featB_out given):           featB = relu(pcn(feat)); qkv = Wqkv featB + bqkv models/PointDSC.py:75,36-38
 * tail only -> feat_out required; head only -> feat_in required.  Rows are bs pairs of N points (a 32-point tile never
 * straddles two pairs); a caller with one run of M independent rows passes bs = 1, N = M.  Buffers must not alias.
 * One call, pdsc_layer_run, takes one struct; a zero-initialised field means "absent".  The weights come in ONE of two forms:
 *   natural layout: [out][in] fp32 matrices, BN folded (sections PDSC_W_FC1..FC3 of layer i, PDSC_W_PCN / QKV of layer i+1);
 *   fragment streams: 8 KiB chunks in exactly the order the wavefront-resident kernels consume them, so every weight load of
 *     a wave is 1 KiB of consecutive memory -- what pdsc_forward uses by default.  Built by pdsc_wfrag_build_tail / _head:
 *       tail stream: pdsc_wfrag_tail_bytes() bytes from (fc1 [C/2][C], fc2 [C/2][C/2], fc3 [C][C/2]) fp32 and their biases;
 *       head stream: pdsc_wfrag_head_bytes() bytes from (pcn [C][C], qkv [3C][C] fp32 -> fp16 hi / lo) and their biases
 *                    (the bias of an output tile is one more k-step of its GEMM: A = bias, B = 1);
 *     gemm_format (enum pdsc_layer_gemm) chooses the format of the fc1..fc3 / pcn chunks (the q|k|v chunks are fp16 hi / lo in
 *     both), and the layer call must be told the format its streams were built in.
 * Giving weights in both forms is PDSC_ERR_ARG.
 * BREAKING in PDSC_VERSION 9: the six fused-layer entry points of version 8 (one per weight form: natural, with split streams, all
 * split, fragment streams, with a format, with io flags) are GONE.  pdsc_layer_run does what each did when the struct's fields of
 * the same names hold the same values (the M-rows form: bs = 1, N = M; the all-split form: kernel = PDSC_LAYER_KERNEL_X3).
 * pdsc_wfrag_build_tail / _head take gemm_format: PDSC_LAYER_GEMM_F32 is what they built before, and their format-suffixed twins
 * are gone. */
enum pdsc_layer_kernel {
    PDSC_LAYER_KERNEL_AUTO = 0,  /* natural layout: BLOCK if pdsc_layer_prefers_block(bs, N), else WAVE.  Fragment streams: H3 if
                                  * io_flags != 0; else H3 if gemm_format = PDSC_LAYER_GEMM_H3 and the H3 kernel serves the output
                                  * set (head: the split streams only, no qkv_out; tail + head: no feat_out), else WAVE */
    PDSC_LAYER_KERNEL_BLOCK,     /* one 4-wave workgroup per 32-point tile, natural layout; merges up to 8 partials */
    PDSC_LAYER_KERNEL_WAVE,      /* one wavefront per tile, natural layout or fragment streams; merges up to 4 partials */
    PDSC_LAYER_KERNEL_H3,        /* the pipelined kernel over PDSC_LAYER_GEMM_H3 streams (layer_h3_coop_kernel for few tiles); up to 8 */
    PDSC_LAYER_KERNEL_X3         /* every GEMM as three f16 MFMAs per operand pair (PDSC_ATT_FP16X3_ALL); never chosen by AUTO;
                                  * up to 4 partials; experiments builds only, PDSC_ERR_ARG in the product library */
};
/* A kernel other than AUTO that the arguments do not fit is PDSC_ERR_ARG. */
typedef struct pdsc_layer_call {
    const float* msg;        /* [bs*N][C] tail input: the merged attention output, or NULL when the partials below are given */
    const float* part_o;     /* tail input, un-merged: the key-split partials exactly as pdsc_sc_attention_split leaves them in its */
    const float* part_ml;    /*   scratch when called with msg == NULL, part_o [bs][nsplit][Npad][C], part_ml [bs][nsplit][Npad][2]; */
    int nsplit, Npad;        /*   the merge happens while the tile is loaded (no combine launch, no round trip of msg through HBM) */
    const float* res;        /* [bs*N][C] tail residual (featB of this layer) */
    const float* feat_in;    /* [bs*N][C] head-only input */
    float* feat_out;         /* [bs*N][C] tail result; required when there is no head, optional otherwise */
    float* featB_out;        /* [bs*N][C] head result; NULL = no head */
    float* qkv_out;          /* [bs*N][3C] head, fp32 (q|k|v) rows; optional when the split streams below are given */
    void* q_split;           /* head, optional, both or neither: the fp16 hi/lo operand streams of the split-precision attention */
    void* kv_tiles;          /*   (pointdsc_amd/csrc/split_layout.h): q_split [bs*N][256] fp16 (hi | lo), pdsc_split_q_bytes(bs, N)
                              *   bytes; kv_tiles [bs][ceil(N/32)][37 KiB] (a 32 KiB image per tile of 32 keys, images 37 KiB
                              *   apart), pdsc_split_kv_bytes(bs, N) bytes */
    const void* w1; const float* b1;     /* natural layout: fc1 [C/2][C], fc2 [C/2][C/2], fc3 [C][C/2] (tail), pcn [C][C], */
    const void* w2; const float* b2;     /*   qkv [3C][C] (head) as fp32 [out][in] and their fp32 biases.  PDSC_LAYER_KERNEL_X3: */
    const void* w3; const float* b3;     /*   the five matrices are those of the split-weight buffer instead (fp16 [out][in] hi, */
    const void* wp; const float* bp;     /*   then [out][in] lo, at 16-bit element pdsc_wsplit_offset(cfg, section, layer)); */
    const void* wq; const float* bq;     /*   the biases stay fp32 */
    const void* wq_split;    /* optional, natural layout: the q|k|v weights as fp16 hi [3C][C] | lo [3C][C] (section PDSC_W_QKV_W of
                              * the split-weight buffer) -> that one GEMM runs in split precision; q, k, v only feed the attention,
                              * whose own operand split has an error of the same order, and never touch the residual stream */
    const void* wfrag_tail;  /* fragment streams (pdsc_wfrag_build_tail / _head) instead of the natural-layout weights; the */
    const void* wfrag_head;  /*   q|k|v projection then runs in split precision */
    int gemm_format;         /* enum pdsc_layer_gemm: the format the fragment streams were built in */
    int io_flags;            /* OR of enum pdsc_layer_io: which of part_o / res / featB_out are in point-fragment order.  Non-zero
                              * needs gemm_format = PDSC_LAYER_GEMM_H3 and the forward's output set (head: split streams only, no
                              * qkv_out; tail + head: no feat_out), PDSC_ERR_ARG otherwise; PF res / featB_out buffers hold
                              * bs * ceil(N / 32) * 32 rows */
    int bs, N;
    int kernel;              /* enum pdsc_layer_kernel */
} pdsc_layer_call;
int pdsc_layer_run(const pdsc_layer_call* call, void* stream);

/* The split-weight buffer: pdsc_wsplit_bytes(cfg) bytes, filled once per model by pdsc_wsplit_build(cfg, wpack, wsplit, stream);
 *   matrix of `section` (PDSC_W_PCN_W, _QKV_W, _FC1_W, _FC2_W, _FC3_W) of `layer` starts at 16-bit element
 *   pdsc_wsplit_offset(cfg, section, layer): [out][in] hi, then [out][in] lo.  Biases stay fp32 (packed buffer).
 * pdsc_wsplit_build also stores the fragment streams per layer, in both formats, at 16-bit element
 * pdsc_wsplit_offset(cfg, PDSC_WS_FRAG_TAIL / PDSC_WS_FRAG_HEAD (_H3), layer). */
size_t    pdsc_wsplit_bytes(const pdsc_config* cfg);
long long pdsc_wsplit_offset(const pdsc_config* cfg, int section, int layer);
int       pdsc_wsplit_build(const pdsc_config* cfg, const float* wpack, void* wsplit, void* stream);
#define PDSC_WS_FRAG_TAIL 100
#define PDSC_WS_FRAG_HEAD 101
#define PDSC_WS_FRAG_TAIL_H3 102   /* the same streams built with gemm_format = PDSC_LAYER_GEMM_H3 */
#define PDSC_WS_FRAG_HEAD_H3 103
/* value_fold = 1 only (pdsc_wsplit_offset returns -1 otherwise), per layer after the streams above:
 *   PDSC_WS_FOLD_TAIL_H3: H3 tail stream of the folded layer (fc2, fc3: 6 chunks, their biases, then b' = W1f bv + b1f, 64 fp32)
 *   PDSC_WS_FOLD_HEAD_H3: H3 head stream (pcn, q, k, v' = W1f Wv: 28 chunks, biases; the v' rows carry no bias)
 *   PDSC_WS_FOLD_W      : W1f Wv [C/2][C] fp32, then b' [C/2] fp32 (what the streams were built from) */
#define PDSC_WS_FOLD_TAIL_H3 104
#define PDSC_WS_FOLD_HEAD_H3 105
#define PDSC_WS_FOLD_W 106
size_t pdsc_wfrag_fold_tail_bytes(void);
size_t pdsc_wfrag_fold_head_bytes(void);
int pdsc_layer_prefers_block(int bs, int N);   /* 1: with layer_gemm = F32, pdsc_forward takes the workgroup-per-tile kernel for this size */
int pdsc_layer_h3_uses_coop(int bs, int N);    /* 1: with layer_gemm = H3, a launch over bs x N points takes layer_h3_coop_kernel (four
                                                * wavefronts per 32-point tile: at most 2560 tiles), 0: layer_h3_kernel */
size_t pdsc_wfrag_tail_bytes(void);
size_t pdsc_wfrag_head_bytes(void);
int pdsc_wfrag_build_tail(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                          const float* b3, void* out, int gemm_format, void* stream);
int pdsc_wfrag_build_head(const float* wp, const float* bp, const float* wq, const float* bq, void* out,
                          int gemm_format, void* stream);

/* ---- a-3  spatial-consistency guided non-local attention ---------------------------------------
 * replaces models/PointDSC.py:39-42 (both einsums and the softmax; N x N scores never materialised).
 *   msg[o][:] = sum_i softmax_i( compat[o][i] * <Q_o, K_i> / sqrt(C) ) * V_i
 * qkv [bs*N][3C] rows = (q | k | v) with q PRE-SCALED by log2(e)/sqrt(C) (see PDSC_W_QKV_W);
 * compat [bs][N][ld]; msg [bs*N][C].  `scratch` holds split-key partials, size from
 * pdsc_attention_scratch_bytes; nsplit <= 0 lets the library choose. */
size_t pdsc_attention_scratch_bytes(int bs, int N, int nsplit);
int    pdsc_attention_default_split(int bs, int N);
int    pdsc_sc_attention(const float* qkv, const float* compat, long long ld, float* msg,
                         void* scratch, size_t scratch_bytes, int bs, int N, int nsplit, void* stream);

/* Split-precision variant (PDSC_ATT_FP16X3): same contract, operands as fp16 hi/lo streams.
 * pdsc_pack_qkv_split converts fp32 (q|k|v) rows [bs*N][3C] into the two streams (the fused layer kernel emits
 * them directly; the packer serves stage tests and callers with their own projections). */
size_t pdsc_split_q_bytes(int bs, int N);
size_t pdsc_split_kv_bytes(int bs, int N);
int    pdsc_pack_qkv_split(const float* qkv, void* q_split, void* kv_tiles, int bs, int N, void* stream);
size_t pdsc_attention_split_scratch_bytes(int bs, int N, int nsplit);
int    pdsc_attention_split_default_split(int bs, int N);
/* leaf form (enum pdsc_att_leaves >= PDSC_LEAVES_CANONICAL): canonical leaf count of N; the plan (key split = workgroups per query
 * block, leaves per pair) the forward uses for (bs, N, leaves_mode); bytes of its scratch (the leaf partials).  A key split of 1
 * with more than one leaf: the workgroup merges its leaves itself and the pair's leaf-0 slot holds the ONE partial the layer
 * launch loads (un-normalised sum, m = 0, l = the merge's denominator). */
int    pdsc_attention_leaf_count(int N);
int    pdsc_attention_leaf_plan(int bs, int N, int leaves_mode, int* nsplit, int* nleaf);
size_t pdsc_attention_leaf_scratch_bytes(int bs, int N, int leaves_mode);
int    pdsc_sc_attention_split(const void* q_split, const void* kv_tiles, const float* compat, long long ld,
                               float* msg, void* scratch, size_t scratch_bytes, int bs, int N, int nsplit,
                               void* stream);
/* same, streaming the unorm16 matrix of pdsc_spatial_compat_u16 (ld: uint16 elements per row) */
int    pdsc_sc_attention_split_u16(const void* q_split, const void* kv_tiles, const unsigned short* compat_u16, long long ld,
                                   float* msg, void* scratch, size_t scratch_bytes, int bs, int N, int nsplit,
                                   void* stream);
/* msg == NULL (only when the key split is > 1): the partials are left un-merged in `scratch` for pdsc_layer_run:
 * part_o = scratch as [bs][nsplit][Npad][C] floats, Npad = N rounded up to 256, part_ml right behind it as
 * [bs][nsplit][Npad][2]. */

/* Diagnostics hook of the split-precision kernel: when a device buffer of (#workgroups * 8 waves * 8) int64 is set,
 * the 8-wave kernel variant is replaced by an instrumented build that accumulates per-wave shader-clock sums of its
 * phases (0 prologue, 1 first tile, 2 own-DMA wait, 3 barrier, 4 DMA issue, 5 phase A, 6 phase B, 7 rest) there.
 * NULL (default) switches it off.  Used by tools/attention_trace.py only. */
int pdsc_attention_trace(long long* device_buffer);

/* Diagnostics hook of the leaf form: workgroups per query block of every later leaf-form attention launch of this process.
 * 0 (default): the planner decides (a function of bs and N).  Otherwise d must divide the launch's leaf count -- the call that
 * plans a launch (pdsc_attention_leaf_plan, the forwards) fails where it does not.  The key split decides speed only: with d = 1
 * every workgroup merges the leaves of its query block itself, with d > 1 the layer kernel merges them, same arithmetic, same
 * bits.  Used by the tests and the A/B tools; process-wide, not thread-safe against running forwards. */
int pdsc_attention_leaf_split_override(int d);

/* Same for the fused layer kernel: buffer of (#workgroups * 4 waves * 16) int64 receiving raw shader-clock stamps at the
 * stage boundaries of layer_fused_kernel (tools/layer_trace.py); NULL switches it off. */
int pdsc_layer_trace(long long* device_buffer);

/* ---- a-4  first two layers of the confidence head in one launch ------------------------------------------------
 * replaces classification.0 .. classification.3 (models/PointDSC.py:107-111, called at :171):
 *   h2[m][0:32] = relu(W2 relu(W1 feat[m][0:128] + b1) + b2),  W1 [32][128], W2 [32][32] row-major fp32.
 * Exact fp32 MFMA; every output element goes through the same fma chain as
 *   pdsc_linear(feat, 128, W1, b1, ..., relu) followed by pdsc_linear(h1, 32, W2, b2, ..., relu)   -- bit-identical --
 * without the [M][32] hidden layer going through HBM.  pdsc_forward calls this since r04. */
int pdsc_classifier_hidden(const float* feat, const float* W1, const float* b1, const float* W2, const float* b2, float* h2,
                           int M, void* stream);

/* ---- a-4  L2 normalisation + last classifier layer --------------------------------------------
 * replaces F.normalize (models/PointDSC.py:156) and classification.4 (:112,171).
 *   normed[m][:] = feat[m][:] / max(||feat[m]||_2, 1e-12);  conf[m] = <h2[m][0:32], w3> + b3 */
int pdsc_normalize_confidence(const float* feat, const float* h2, const float* w3, const float* b3,
                              float* normed, float* conf, int M, void* stream);

/* ---- a-5  NMS seed selection -------------------------------------------------------------------
 * replaces pick_seeds (models/PointDSC.py:199-217).
 *   keys[i] = conf[i] * [ for all j: conf[i] >= conf[j]  or  ||src_i - src_j|| >= radius ]
 *   seeds   = first num_seeds indices by descending key, equal keys by ascending index. */
int pdsc_nms_keys(const float* src_keypts, const float* conf, float radius, float* keys,
                  int bs, int N, void* stream);
/* the same keys, bit for bit, from ~1 % of the pair evaluations: points counting-sorted into a 2-D cell grid of width >=
 * radius, the predicate evaluated against the 3 x 3 neighbouring cells only (what the forward calls; workspace from
 * pdsc_nms_workspace_bytes; radius <= 0 / NaN / NULL workspace fall back to pdsc_nms_keys) */
size_t pdsc_nms_workspace_bytes(int bs, int N);
int pdsc_nms_keys_grid(const float* src_keypts, const float* conf, float radius, float* keys, void* workspace,
                       size_t workspace_bytes, int bs, int N, void* stream);
int pdsc_rank_select(const float* keys, int* seeds, int bs, int N, int num_seeds, void* stream);

/* ---- a-6  feature-space kNN of the seeds -------------------------------------------------------
 * replaces knn(..., ignore_self=True, normalized=True) + the seed gather
 * (models/common.py:48-69, models/PointDSC.py:250-252); only the seed rows are computed.
 *   dist[s][j] = 2 - 2 * <normed[seed_s], normed[j]>;  knn_idx[s][0:k] = ranks 1..k of ascending
 *   (dist, index) order (rank 0 dropped exactly like `[:, :, 1:]`).  A NaN distance (a NaN in a feature row) ranks after every
 *   number whatever its sign, as torch.sort orders it: as long as a seed keeps k + 1 finite distances both forms return the
 *   same finite neighbours; with fewer the remaining slots are unspecified.
 * dist_scratch: [bs][S][ldd] floats, ldd = pdsc_compat_ld(N).  knn_idx: [bs][S][k] int32.
 * NOTE: pdsc_knn_seeds = pdsc_knn_seeds_form(form 0): for large batches (bs * ceil(S / 32) >= 384) the library takes the fused
 * form, which never writes dist_scratch -- its contents are then UNDEFINED.  A caller that wants the S x N distances back calls
 * pdsc_knn_seeds_form(..., form = 1). */
int pdsc_knn_seeds(const float* normed, const int* seeds, float* dist_scratch, int* knn_idx,
                   int bs, int N, int S, int k, void* stream);
/* form: 0 = the library's choice, 1 = two launches through the S x N distance matrix (Gram rows, then a selection launch),
 * 2 = fused (r05: 32 seeds per workgroup, the distances never leave the chip -- only candidates below a per-seed bound reach an
 * LDS list; needs k + 1 <= 48 and N >= 256; dist_scratch unused).  Same distance bits, same (dist, index) order: the neighbour
 * indices of the two forms are identical.  form 0 takes the fused form when bs * ceil(S / 32) >= 384 workgroups.
 * normed_pf (optional, fused form): the same normalised rows in point-fragment order, [bs][ceil(N / 32) * 32][128]
 * (pdsc_normalize_confidence_pf writes both) -- the kernel then loads its column operand 1 KiB per instruction; NULL = gathered
 * from `normed` (32 pieces of 32 bytes per instruction: 2 x slower, same results). */
int pdsc_knn_seeds_form(const float* normed, const float* normed_pf, const int* seeds, float* dist_scratch, int* knn_idx,
                        int bs, int N, int S, int k, int form, void* stream);
/* pdsc_normalize_confidence per pair (feat [bs][N][128] ...), additionally leaving the normalised rows in point-fragment order */
int pdsc_normalize_confidence_pf(const float* feat, const float* h2, const float* w3, const float* b3, float* normed,
                                 float* normed_pf, float* conf, int bs, int N, void* stream);

/* ---- a-7/a-8  per-seed compatibility + power iteration ----------------------------------------
 * replaces models/PointDSC.py:257-281 and cal_leading_eigenvector (:347-358).
 * Every iterate is stored: eig_iters [bs][S][num_iterations][PDSC_MAX_K]; conv_mask[b] bit i is set iff
 * every seed of pair b satisfied the allclose test at iteration i (the reference's early exit is global
 * over the S seeds).  seed_M (optional, may be NULL): [bs][S][k][k]. */
int pdsc_seed_power_iteration(const float* normed, const float* src_keypts, const float* tgt_keypts,
                              const int* knn_idx, const float* sigma, const float* sigma_spat,
                              float* eig_iters, unsigned int* conv_mask, float* seed_M,
                              int bs, int N, int S, int k, int num_iterations, void* stream);

/* ---- a-9  seed-wise weighted Procrustes --------------------------------------------------------
 * replaces models/PointDSC.py:282-320 (weight normalisation + rigid_transform_3d on the k neighbours).
 * Picks iterate `first set bit of conv_mask, else num_iterations-1`.  seed_trans [bs][S][16]. */
int pdsc_seed_transforms(const float* src_keypts, const float* tgt_keypts, const int* knn_idx,
                         const float* eig_iters, const unsigned int* conv_mask, float* seed_trans,
                         float* seed_weights /* optional [bs][S][k] */,
                         int bs, int N, int S, int k, int num_iterations, void* stream);

/* ---- a-7 + a-8 + a-9: the launches of the testing forward ------------------------------------------
 * Launch 1: pdsc_seed_power_iteration and, for the LAST iterate, the Procrustes sums of pdsc_seed_transforms by the same
 * wavefront that owns the seed.  Launch 2 (one wavefront per 64 consecutive seeds of the flattened bs * S list) re-solves the
 * seeds of a pair whose global early exit (conv_mask) selected an earlier iterate, then turns every slot into its 4x4; with
 * num_iterations = 0 it is the plain decomposition launch.  Same bits as pdsc_seed_power_iteration + pdsc_seed_transforms.
 * seed_weights / seed_M may be NULL.  seed_trans == NULL: launch 1 alone (this is then pdsc_seed_power_iteration). */
int pdsc_seed_solve(const float* normed, const float* src_keypts, const float* tgt_keypts, const int* knn_idx,
                    const float* sigma, const float* sigma_spat, float* eig_iters, unsigned int* conv_mask, float* seed_M,
                    float* seed_trans, float* seed_weights, int bs, int N, int S, int k, int num_iterations, void* stream);

/* rigid_transform_3d(A, B, weights, weight_threshold) (models/common.py:7-45 + utils/SE3.py:73-96):
 * A,B [bs][n][3], weights [bs][n] or NULL (=1), T [bs][16] row-major 4x4 with p_B = R p_A + t.
 * weights are NOT modified (the reference zeroes weights < threshold in place). */
int pdsc_rigid_transform_3d(const float* A, const float* B, const float* weights, float weight_threshold,
                            float* T, int bs, int n, void* stream);

/* ---- a-10  hypothesis scoring ------------------------------------------------------------------
 * replaces models/PointDSC.py:325-335.  counts[b][s] = #{n : ||R_s src_n + t_s - tgt_n|| < thr};
 * best = first argmax; initial_trans = seed_trans[best]; labels[n] = residual_best[n] < thr (0/1 fp32). */
int pdsc_score_hypotheses(const float* seed_trans, const float* src_keypts, const float* tgt_keypts,
                          float inlier_threshold, int* counts, int bs, int N, int S, void* stream);
int pdsc_select_best(const int* counts, const float* seed_trans, const float* src_keypts,
                     const float* tgt_keypts, float inlier_threshold, int* best, float* initial_trans,
                     float* labels, int bs, int N, int S, void* stream);

/* ---- a-11  post refinement ---------------------------------------------------------------------
 * replaces post_refinement (models/PointDSC.py:403-438) incl. transform (utils/SE3.py:43-57): the whole
 * <=max_iters loop runs on the device.  solves (optional) [bs] = number of re-solves performed. */
int pdsc_post_refinement(const float* initial_trans, const float* src_keypts, const float* tgt_keypts,
                         float threshold, int max_iters, float* final_trans, int* solves,
                         int bs, int N, void* stream);

/* ---- whole path --------------------------------------------------------------------------------
 * One call, pdsc_forward, takes one struct; a zero-initialised field means "absent".  `mode` says which forward runs:
 *
 * PDSC_FORWARD_TESTING replaces PointDSC.forward(data) with 'testing' in data (models/PointDSC.py:128-197).
 *   corr_pos [bs][N][in_dim], src/tgt [bs][N][3]  ->  final_trans [bs][16], final_labels [bs][N] (0/1).
 *   num_seeds = int(N * ratio) computed by the caller in double precision like the reference (:174).
 *
 *   Ragged batch (num_corr, num_seeds_per_pair, n_min given).  The reference's real evaluation feeds every pair with its own number
 *   of correspondences (evaluation/test_3DMatch.py:126 `num_node='all'`, datasets/ThreeDMatch.py:271-276) and therefore one pair
 *   per call (models/PointDSC.py:210); its own batching crops every pair to the shortest (datasets/dataloader.py:6-31).  Here a
 *   batch may mix sizes: the inputs are padded to the longest pair, [bs][N][.] with N = max_b num_corr[b] (padding rows: any
 *   finite values, e.g. zeros), num_seeds = max_b num_seeds_per_pair[b].  Pair b's results are those of a uniform call on its own
 *   num_corr[b] rows (same stages on the same data; only the launch plans, i.e. fp32 summation orders, are the batch's):
 *   final_trans [bs][16], final_labels [bs][N] with rows >= num_corr[b] zero.  Workspace: pdsc_workspace_bytes(cfg, bs, N,
 *   num_seeds).  Split-precision attention modes only.
 *
 *   Two streams (tail_stream, fork_event, join_event given; throughput loops with several forwards in flight,
 *   pointdsc_amd/pipeline.py).  Same result as on one stream, uniform or ragged.  The encoder (compat build, 12 attention + layer
 *   launches) is enqueued on `stream`; everything after it -- classifier, NMS, seed ranking, kNN, per-seed solver, scoring,
 *   refinement: a sequential chain of ~15 small launches -- on `tail_stream`, which the caller creates with a HIGHER priority:
 *   while forward i's tail runs, forward i+1's encoder (another stream) keeps the chip full, and the tail's few workgroups are
 *   dispatched ahead of the attention launch's queued ones instead of behind them.  fork_event / join_event: caller-owned
 *   hipEvent_t (no timing needed), recorded on stream / tail_stream; on return `stream` waits for join_event, so work enqueued on
 *   `stream` afterwards is ordered after the results.  Nothing is allocated; capturable in a hipGraph.  Measured with two forwards
 *   in flight (profiles/r03_h_inflight_ab.txt, r03_i_inflight_ab.txt): -2.6 % per step at 32 pairs of N = 5000, -6 % at 4 pairs,
 *   -13 % for one pair of N = 10000 against one stream; two plain streams without it: +-0.
 *
 * PDSC_FORWARD_VALIDATION replaces PointDSC.forward(data) WITHOUT the 'testing' key on a module in
 *   eval() mode (libs/trainer.py:158-222 calls it so): models/PointDSC.py:158-163 (feature similarity matrix M), :176 (seeds = top
 *   int(N*ratio) by confidence, no NMS), :182 (per-seed hypotheses; the power iteration's allclose exit is taken over the whole
 *   batch), no post refinement, :190-191 (the returned labels are the confidence logits).  Forward only (no autograd).
 *   final_trans [bs][16] = best seed hypothesis; final_labels [bs][N] = the logits; M [bs][N][ldM].  Uniform batches, one stream.
 *
 * PDSC_FORWARD_PROBE: range probe for layer_gemm = PDSC_LAYER_GEMM_H3.  The H3 arithmetic carries every operand of the
 *   fc_message / PointCN GEMMs as fp16 hi + lo, so every activation of the 12-layer chain -- hidden ones included -- must stay
 *   below 65504.  This mode runs the ENCODER (compat, layer0, 12 x {PointCN, q|k|v, attention, fc1, fc2, fc3 + residual};
 *   models/PointDSC.py:48-77) once with the fp32 GEMMs, one launch per conv, and leaves in absmax[kind] (enum pdsc_range_kind) the
 *   largest |value| of each activation kind over all layers (a NaN anywhere reads back as NaN).  No pose, no labels: final_trans,
 *   final_labels and M are not written.  The module calls it on the first forward after packing weights and falls back to
 *   PDSC_LAYER_GEMM_F32 with a warning when a value is out of range.  Same inputs and workspace as the testing forward. */
enum pdsc_forward_mode { PDSC_FORWARD_TESTING = 0, PDSC_FORWARD_VALIDATION = 1, PDSC_FORWARD_PROBE = 2 };
enum pdsc_range_kind { PDSC_RANGE_LAYER0 = 0, PDSC_RANGE_POINTCN = 1, PDSC_RANGE_QKV = 2, PDSC_RANGE_MESSAGE = 3, PDSC_RANGE_FC1 = 4,
                       PDSC_RANGE_FC2 = 5, PDSC_RANGE_FEATURE = 6, PDSC_RANGE_NUM_KINDS = 8 };
typedef struct pdsc_forward_call {
    int mode;                        /* enum pdsc_forward_mode */
    const pdsc_config* cfg;
    const float* wpack;              /* packed weights (pdsc_wpack_floats) */
    const void* wsplit;              /* split-weight buffer (pdsc_wsplit_build); NULL iff PDSC_ATT_FP32 */
    const float* corr_pos;           /* [bs][N][in_dim] */
    const float* src_keypts;         /* [bs][N][3] */
    const float* tgt_keypts;         /* [bs][N][3] */
    int bs, N, num_seeds;            /* ragged batch: N and num_seeds are those of the longest pair */
    float* final_trans;              /* [bs][16]; required except by the probe */
    float* final_labels;             /* [bs][N]: 0/1 labels (testing) or the confidence logits (validation); required except by the probe */
    float* M;                        /* [bs][N][ldM] feature similarity matrix: validation only, and required there */
    long long ldM;                   /*   >= N */
    void* workspace;                 /* pdsc_workspace_bytes(cfg, bs, N, num_seeds) bytes */
    size_t workspace_bytes;
    const int* num_corr;             /* ragged batch (testing only; both arrays or neither): [bs] int32, DEVICE: correspondences of pair b
                                      * (2 <= num_corr[b] <= N) */
    const int* num_seeds_per_pair;   /*   [bs] int32, DEVICE: int(num_corr[b] * ratio) >= 1, computed by the caller in double precision (:174) */
    int n_min;                       /*   min_b num_corr[b] (host copy), 2 <= n_min <= N.  It must leave every pair at least one 32-key tile
                                      *   per attention key split: ceil(n_min / 32) >= pdsc_attention_split_default_split(bs, N), and
                                      *   n_min > min(cfg->k, N - 1): the reference clamps k per pair, k = min(k, num_corr - 1)
                                      *   (models/PointDSC.py:250), one launch has one k -- a pair of at most k rows is its own call;
                                      *   PDSC_ERR_ARG otherwise */
    void* tail_stream;               /* two streams (testing only): hipStream_t of the tail, different from `stream`; needs both events */
    void* fork_event;                /*   hipEvent_t recorded on `stream` behind the encoder; tail_stream waits for it */
    void* join_event;                /*   hipEvent_t recorded on tail_stream behind the last launch; `stream` waits for it */
    float* absmax;                   /* probe only, and required there: [PDSC_RANGE_NUM_KINDS] floats, DEVICE; zeroed by the call's first launch */
    unsigned int* range_report;      /* optional (testing only): where the forward also leaves its range words -- [bs] u32 of pinned,
                                      * device-mapped HOST memory (hipHostMalloc; checked: anything else is PDSC_ERR_ARG), written by the
                                      * forward's last launch: a caller that waits for the stream anyway reads them without a
                                      * device-to-host copy of its own */
} pdsc_forward_call;
/* Every field is checked before the first launch, event record or fill: a rejected call (< 0) has enqueued nothing, and
 * pdsc_last_error() names the call and its mode, "pdsc_forward(validation): ...".
 * BREAKING in PDSC_VERSION 10: the five whole-path entry points of version 9 (testing, ragged, on two streams, validation, encoder
 * range probe) and the thread-local range-report setter are GONE.  pdsc_forward does what each did when the struct's fields of the
 * same names hold the same values. */
int pdsc_forward(const pdsc_forward_call* call, void* stream);

/* M[b][i][j] = clamp(1 - (1 - <normed_i, normed_j>) / sigma^2, 0, 1), M[b][i][i] = 0   (models/PointDSC.py:158-163);
 * normed [bs*N][C], sigma: device pointer to the learned sigma, M [bs][N][ld >= N]. */
int pdsc_feature_compat(const float* normed, const float* sigma, float* M, long long ld, int bs, int N, void* stream);

/* AND of the per-pair convergence masks of pdsc_seed_power_iteration into every entry: the reference's
 * power-iteration exit (models/PointDSC.py:347-358) is global over all matrices of one call. */
int pdsc_conv_mask_all_pairs(unsigned int* conv_mask, int bs, void* stream);

/* ---- correspondence construction: the step in front of the hot path -----------------
 * replaces datasets/ThreeDMatch.py:283-290,305-308 / demo_registration.py:101-108 (numpy on the host in the reference):
 *   distance = sqrt(2 - 2 * src_desc @ tgt_desc^T + 1e-6);  nn_idx[i] = argmin_j distance[i][j] (first index among equal
 *   distances, NaN first -- np.argmin);  nn_dist[i] (optional) = that distance.  The Ns x Nt matrix is never stored.
 * src_desc [Ns][D], tgt_desc [Nt][D] fp32 (L2-normalised descriptors, D <= 64); scratch: pdsc_match_scratch_bytes. */
size_t pdsc_match_scratch_bytes(int Ns, int Nt);
int pdsc_match_descriptors(const float* src_desc, const float* tgt_desc, int Ns, int Nt, int D, int* nn_idx,
                           float* nn_dist, void* scratch, size_t scratch_bytes, void* stream);
/* the 3DLoMatch caller's form (evaluation/test_3DLoMatch.py:45-46): nn_idx[i] = argmax_j <src_desc_i, tgt_desc_j> (torch.argmax:
 * first index among equal maxima, NaN counts as the maximum); nn_dot[i] (optional) = that inner product.  Same scratch. */
int pdsc_match_descriptors_ip(const float* src_desc, const float* tgt_desc, int Ns, int Nt, int D, int* nn_idx,
                              float* nn_dot, void* scratch, size_t scratch_bytes, void* stream);
/* corr[c] = (i, src2tgt[i]) for i ascending; with tgt2src != NULL only the mutual nearest neighbours
 * (tgt2src[src2tgt[i]] == i, ThreeDMatch.py:286-288) are kept.  corr [Ns][2] (capacity), *count = rows written. */
int pdsc_select_correspondences(const int* src2tgt, const int* tgt2src, int Ns, int* corr, int* count, void* stream);
/* src_sel[c] = src_keypts[corr[c][0]], tgt_sel[c] = tgt_keypts[corr[c][1]], corr_pos[c] = (src_sel | tgt_sel) - column mean
 * over the *count rows (in_dim = 6, ThreeDMatch.py:299-308).  Outputs have capacity for every row of corr. */
int pdsc_build_corr_pos(const float* src_keypts, const float* tgt_keypts, const int* corr, const int* count,
                        float* corr_pos, float* src_sel, float* tgt_sel, void* stream);

/* ---- correspondence construction for a batch of pairs over a pool of clouds ----------------
 * replaces, for P pairs in one call, what Dataset.__getitem__ runs once per pair on the host: datasets/ThreeDMatch.py:283-290
 * (distance, argmin, mutual check), :293-297 (the ground-truth label), :300-308 (gather, corr_pos = concat - column mean), the
 * same lines of datasets/KITTI.py:80-105, and with metric 1 the matching of evaluation/test_3DLoMatch.py:45-48.
 *
 * POOL: desc [total][D] and keypts [total][3] fp32 hold the clouds one after the other.  TABLE [W][5] int32 on the device, one row
 * per work item: { source offset, source count, target offset, target count, first source tile } -- offsets and counts in rows of
 * the pool, counts >= 1; the first tile of item w is the sum of ceil(source count / 128) over the items before it, and total_tiles
 * that sum over all of them.  mutual = 0: W = P, item p is pair p.  mutual = 1: W = 2 P, item 2p is pair p (source -> target) and
 * item 2p + 1 the same pair with the roles swapped.  A cloud may serve any number of pairs, as source and as target, also of
 * itself.  max_tgt = the largest target count of the table, cap = the row capacity of the outputs (LIMIT: cap >= the largest
 * source count of the pairs; the caller builds the table from shapes it knows and answers for its consistency -- the call reads
 * nothing back).
 *
 * OUTPUTS, pair p at row p * cap:  corr [P][cap][2] int32 = (i, nearest target of i) for the kept source rows i ascending (all of
 * them, or with mutual = 1 those whose target's nearest source is i), num_corr [P] int32 = rows kept, written on the device;
 * src_sel / tgt_sel [P][cap][3] the two endpoints, corr_pos [P][cap][6] = (src_sel | tgt_sel) - column mean over the num_corr rows
 * (fp64 column sums, added in a fixed order).  Rows from num_corr[p] up to cap are ZERO in every output.
 * TIES AND NaN are those of pdsc_match_descriptors / _ip: the distance (inner product) of a (source, target) row pair is the same
 * bits as there (one tile body, csrc/match_tile.h), the first index wins among equal values, NaN orders first.
 * LABEL (gt_trans != NULL, then gt_labels != NULL too): gt_trans [P][4][4] fp64 row-major, x = src_sel, y = tgt_sel taken to fp64,
 *   gt_labels[p][c] = sqrt(sum_d (R_p x + t_p - y)_d^2) < inlier_threshold ? 1 : 0      fp64 throughout, as numpy promotes
 * ThreeDMatch.py:295-297 (np.linalg.inv hands over a float64 gt_trans); gt_labels [P][cap] fp32.
 * Launches only (key fill, matcher, select, gather, centre) on `stream`: nothing is read on the host or allocated.
 * The target range is split over workgroups by pdsc_match_descriptors' rule applied to total_tiles (about 1024 workgroups, whole
 * 128-row target tiles per split): a large batch runs with one split.  _ex: splits = 0 keeps that rule, 1 .. ceil(max_tgt / 128)
 * overrides it (tests; the outputs do not depend on it).
 * workspace: pdsc_corr_batch_workspace_bytes(P, total_tiles, cap) (0 for a non-positive argument).
 * ERRORS, nothing enqueued: PDSC_ERR_ARG with the text "pdsc_build_correspondences_batch: ..." for a null pointer, P outside
 * 1 .. 65535, D outside 1 .. 64, mutual or metric not 0 / 1, total_tiles < W, max_tgt < 1 or > 65535 * 128, cap < 1, gt_trans
 * without gt_labels or the reverse, a NaN threshold, splits out of range; PDSC_ERR_WORKSPACE for a short workspace. */
size_t pdsc_corr_batch_workspace_bytes(int P, int total_tiles, int cap);
int pdsc_build_correspondences_batch(const float* desc, const float* keypts, const int* table, int P, int D, int mutual, int metric,
                                     int total_tiles, int max_tgt, int cap, const double* gt_trans, double inlier_threshold,
                                     float* corr_pos, float* src_sel, float* tgt_sel, int* corr, int* num_corr, float* gt_labels,
                                     void* workspace, size_t workspace_bytes, void* stream);
int pdsc_build_correspondences_batch_ex(const float* desc, const float* keypts, const int* table, int P, int D, int mutual, int metric,
                                        int total_tiles, int max_tgt, int cap, const double* gt_trans, double inlier_threshold,
                                        float* corr_pos, float* src_sel, float* tgt_sel, int* corr, int* num_corr, float* gt_labels,
                                        void* workspace, size_t workspace_bytes, int splits, void* stream);

/* ---- spectral-matching baseline: the N x N power iteration ------------------------------
 * replaces SM() of baseline_scripts/baseline_3DMatch.py:19-53:  M = max(0, 4.5 - d^2 / 2 / sigma^2) (zero diagonal,
 * d = |corr_i[0:3] - corr_j[0:3]| - |corr_i[3:6] - corr_j[3:6]|, sigma = inlier_threshold / 3);  v = 1, num_iterations x
 * { v = M v; v /= |v| + 1e-6 };  pred_labels = 1 for the num_top = int(N * top_ratio) largest entries of v (equal
 * entries by ascending index);  pred_trans = rigid_transform_3d(src_keypts, tgt_keypts, v * pred_labels).
 * corr_pos [bs][N][6] (the centred coordinates the reference passes as `corr`), src/tgt [bs][N][3];
 * pred_trans [bs][16], pred_labels [bs][N], leading_eig (optional) [bs][N]; workspace: pdsc_sm_workspace_bytes
 * (holds M: 4 N ld bytes per pair).  bs > 1 = independent pairs (the reference asserts bs == 1).
 * Non-finite coordinates behave as in the reference: an entry of M whose d is NaN is NaN (torch.clamp(min=0) keeps it), so
 * leading_eig and pred_trans of that pair are NaN; the selection ranks NaN as the largest value (torch.sort's order), NaNs among
 * themselves by ascending index -- an all-NaN vector labels the indices 0 .. num_top - 1.  Other pairs of the batch are untouched.
 * 2 <= N <= 40 896 (see the forms below), 0 <= num_top <= N, num_iterations >= 1; else PDSC_ERR_ARG. */
size_t pdsc_sm_workspace_bytes(int bs, int N);
int pdsc_sm_baseline(const float* corr_pos, const float* src_keypts, const float* tgt_keypts, float inlier_threshold,
                     int num_top, int num_iterations, float* pred_trans, float* pred_labels, float* leading_eig,
                     void* workspace, size_t workspace_bytes, int bs, int N, void* stream);
/* Two forms, bit-identical results (same arithmetic in the same order):
 *   streaming (form 1): the 4 N^2-byte matrix is written to the workspace once and streamed from HBM per iteration, the pairs of a
 *                       batch in one launch; any N up to 40 896 (v sits in the mat-vec's dynamic LDS, round_up(N, 64) floats of
 *                       160 KiB - 64 bytes; a larger N returns PDSC_ERR_ARG before anything is enqueued);
 *   register-resident (form 2): ONE persistent launch per pair computes the matrix straight into the chip's vector registers
 *                       (100 MB at N = 5000 of the 128 MiB the 256 compute units hold) and runs every power iteration from there;
 *                       per iteration only y crosses the chip, behind a grid barrier.  N <= 5120, 20 rows per compute unit.
 * pdsc_sm_baseline (= form 0) ALWAYS runs the streaming form (r05).  The resident form (one pair of N = 5000: 252 us against 342)
 * needs the whole chip to itself for its grid barrier, which only the caller can promise: it is opt-in (form 2), launched
 * cooperatively (the launch fails, PDSC_ERR_LAUNCH, when the runtime cannot make the grid co-resident), refused under stream
 * capture, ordered against this process's other resident launches on the same device, and every in-kernel wait is bounded --
 * a second PROCESS running it on the same GPU at the same time ends in NaN outputs after 0.5 s, never in a hang. */
int pdsc_sm_baseline_form(const float* corr_pos, const float* src_keypts, const float* tgt_keypts, float inlier_threshold,
                          int num_top, int num_iterations, float* pred_trans, float* pred_labels, float* leading_eig,
                          void* workspace, size_t workspace_bytes, int bs, int N, int form, void* stream);

/* ---- PMC baseline: exact maximum clique of the compatibility graph ----------------------------
 * replaces PMC() of baseline_scripts/baseline_3DMatch.py:56-77.  Vertices = correspondences; i and j are joined iff
 *   | ((dx*dx + dy*dy) + dz*dz)  -  ((ex*ex + ey*ey) + ez*ez) | < inlier_threshold,   d = c_i[0:3] - c_j[0:3], e = c_i[3:6] - c_j[3:6]
 * in fp32 in exactly this order (SQUARED distances, as the reference writes it; c = corr_pos, the centred coordinates the reference
 * passes as `corr`): the edge set is numpy's bit for bit.  pred_labels = 1 on a maximum clique, pred_trans =
 * rigid_transform_3d(src_keypts, tgt_keypts, pred_labels).
 *
 * pdsc_pmc_adjacency: bits [bs][N][ld_words] 64-bit words, bit (j & 63) of word (j >> 6) of row i = edge (i, j); zero diagonal,
 *   symmetric, the bits of columns >= N and the words beyond ceil(N / 64) zero.  ld_words >= ceil(N / 64).  N <= 16384.
 *
 * pdsc_pmc_baseline: adjacency, degrees, the order (degree descending, index ascending), a greedy clique from every vertex (its
 *   largest = the lower bound), branch and bound with a greedy-colouring bound, labels, Procrustes -- ten launches, no host
 *   synchronisation, nothing allocated.  The ROOT of a clique is its last member in the order; root r's subproblem (r + its neighbours
 *   earlier in the order, renumbered into a bitset of their own) is searched by one single-wave workgroup whose incumbent is private
 *   and starts at the lower bound, so nothing depends on the order in which workgroups finish: the same inputs give the same bits in
 *   every output, for a pair alone or inside a batch, with proven = 0 as well.
 *   max_nodes (1 .. 2^30, mandatory): the number of NODES one workgroup (= one root's search, but see LIMITS) may expand per launch; a node = one branching step (one vertex joins
 *     the current clique and the child's candidate set is formed).  A root that runs out keeps its best find; the call returns normally.
 *   clique_size [bs] int: size of the labelled clique.  proven [bs] int: 1 = every root was exhausted or cut by its bound, the size
 *     is the maximum; 0 = some root ran out of max_nodes (or could not be served, below) and the clique is the best one found.
 *   TIE RULE: the largest clique wins; a root's clique replaces the greedy one only when strictly larger; among roots with equally
 *     large cliques the root earliest in the order wins; inside a root the first clique of that size met by the depth-first search
 *     (branching on the later-ordered candidate first) stays; among greedy cliques of equal size the start vertex earliest in the order.
 *     A graph without edges (and N = 1) therefore labels vertex 0 alone: clique_size 1, proven 1.
 *   LIMITS: N <= 16384.  A root's candidate bitsets and their n x ceil(n / 64)-word adjacency live in 48 KiB of LDS when
 *     8 (n ceil(n / 64) + 2 ceil(n / 64) (colours of the root + 1)) bytes fit (n up to ~ 500 - 600 candidates), else in a slab of the
 *     workspace, which serves n <= 4096 candidates and 1024 stack levels; a root beyond that is not searched and makes proven 0.
 *     The slab pass has 64 workgroups per pair; workgroup g serves the roots g, g + 64, ... that did not fit, in ascending order,
 *     with ONE budget of max_nodes for all of them, a node there being charged 8 (its matrix is behind the L2, not in LDS).
 *   The workspace's first bs x 4 int64 hold, per pair, after the call: nodes expanded, roots searched, roots not exhausted, the greedy bound.
 * Bad arguments (null pointer, N < 1 or > 16384, max_nodes out of range) return PDSC_ERR_ARG, a short workspace PDSC_ERR_WORKSPACE,
 * with nothing enqueued. */
int pdsc_pmc_adjacency(const float* corr_pos, float inlier_threshold, unsigned long long* bits, long long ld_words, int bs, int N,
                       void* stream);
size_t pdsc_pmc_workspace_bytes(int bs, int N);
int pdsc_pmc_baseline(const float* corr_pos, const float* src_keypts, const float* tgt_keypts, float inlier_threshold, int max_nodes,
                      float* pred_trans, float* pred_labels, int* clique_size, int* proven, void* workspace, size_t workspace_bytes,
                      int bs, int N, void* stream);
/* The same call with two options for tools and tests.  lds_words: 0, or the number of 8-byte words (1 .. 6144) of the LDS pool the
 * first search pass may use -- a small value sends every root through the slab pass (same results where the budget allows: the
 * two passes run the same code).  stage_ms (HOST, 4 floats, or NULL): the call is bracketed by events on the stream and returns
 * the milliseconds of adjacency | ordering, greedy cliques and bound | search | labels and Procrustes; asking for them
 * synchronises the host on the last event (tools/pmc_bench.py). */
int pdsc_pmc_baseline_ex(const float* corr_pos, const float* src_keypts, const float* tgt_keypts, float inlier_threshold, int max_nodes,
                         float* pred_trans, float* pred_labels, int* clique_size, int* proven, void* workspace, size_t workspace_bytes,
                         int bs, int N, int lds_words, float* stage_ms, void* stream);

/* cal_confidence (models/PointDSC.py:366-401): confidence of a spectral-matching solution from its compatibility matrix
 * M [bs][N][ld] (ld >= N, multiple of 4) and leading eigenvector [bs][N]:
 *   method 0 'eig_value'      : Rayleigh quotient lambda1 = v^T M v / v^T v
 *   method 1 'eig_value_ratio': lambda1 / lambda2, lambda2 from num_iterations power steps on B = M - lambda1 v v^T
 *                               started at 1 (each step normalised by |.| + 1e-6), B never materialised
 *   method 2 'xMx'            : v^T M v / N
 * confidence [bs]; workspace from pdsc_cal_confidence_workspace_bytes.  One HBM-bound N x N mat-vec per step. */
size_t pdsc_cal_confidence_workspace_bytes(int bs, int N);
int pdsc_cal_confidence(const float* M, long long ld, const float* leading_eig, int method, int num_iterations,
                        float* confidence, void* workspace, size_t workspace_bytes, int bs, int N, void* stream);

/* ---- evaluation row on the device -----------------------------------------------------------
 * replaces libs/loss.py:44-51 (RE / TE / recall of TransformationLoss), :96-100 (precision / recall / F1, sklearn on the
 * host) and the stats row of evaluation/test_3DMatch.py:90-98, per pair, without a device -> host copy:
 *   stats[b][0..8] = success (RE < re_thre && TE < te_thre), RE [deg], TE [cm], #gt inliers, gt inlier ratio,
 *                    #gt inliers among the predicted inliers, precision, recall, F1       (pred > 0 is "predicted inlier")
 * trans, gt_trans [bs][16]; pred_labels, gt_labels [bs][N]; stats [bs][9].
 * A NaN pose (what the range sentinel returns for a flagged pair) stays NaN: RE = acos(clamp((trace - 1) / 2, -1, 1)) with
 * torch.clamp's NaN-keeping clamp, TE likewise, and success is 0 (both comparisons are strict and false for NaN). */
int pdsc_eval_stats(const float* trans, const float* gt_trans, const float* pred_labels, const float* gt_labels,
                    float re_thre, float te_thre, float* stats, int bs, int N, void* stream);

/* ---- ICP post-step of the evaluation (the open3d hand-off of SURVEY.md section 8 f-4) ----------
 * replaces evaluation/benchmark_utils.py:40-56 icp_refine (called by evaluation/test_3DMatch.py:79-80, test_KITTI.py:79-80,
 * multiway/test_multi.py:53-54): open3d 0.9 registration_icp with TransformationEstimationPointToPoint, per pair:
 *   fp64 throughout; T = init; P = src transformed by init (skipped when init passes Eigen's isIdentity()); evaluate(P);
 *   up to max_iteration times { U = umeyama(P[corr], tgt[corr]) (identity for an empty set); T = U T; P = U P; evaluate(P);
 *   stop when |d fitness| < relative_fitness and |d rmse| < relative_rmse };
 *   evaluate: each source point's nearest target with fp64 d2 < float(max_distance^2) (FLANN's radius test; equal distances:
 *   the lowest target index), fitness = |corr| / Ns_b, inlier_rmse = sqrt(sum d2 / |corr|) (both 0 for an empty set).
 * src [bs][Ns][3], tgt [bs][Nt][3] (fp32, widened exactly), init_trans [bs][16]; Ns_per_pair / Nt_per_pair [bs] int32
 * (DEVICE; NULL = every pair has Ns / Nt points; rows beyond a pair's count are padding and never read).
 * Outputs [bs]: out_trans_f32 [bs][16], out_trans_f64 [bs][16] (optional), fitness, inlier_rmse (double), num_corr (final
 * |corr|), iterations (loop iterations run).  max_distance <= 0 returns init with zeros (as open3d does); a non-finite init or
 * point returns a NaN pose, NaN fitness / rmse, iterations 0.  The convergence test runs on the device: pairs stop independently.
 * workspace: pdsc_icp_workspace_bytes(bs, Ns, Nt).  A pair's result does not depend on the batch it runs in.
 * Defaults of the reference (open3d 0.9 ICPConvergenceCriteria): max_distance 0.10, relative_* 1e-6, max_iteration 30. */
size_t pdsc_icp_workspace_bytes(int bs, int Ns, int Nt);
int pdsc_icp_refine(const float* src, const float* tgt, const float* init_trans, const int* Ns_per_pair, const int* Nt_per_pair,
                    double max_distance, double relative_fitness, double relative_rmse, int max_iteration, float* out_trans_f32,
                    double* out_trans_f64, double* fitness, double* inlier_rmse, int* num_corr, int* iterations, void* workspace,
                    size_t workspace_bytes, int bs, int Ns, int Nt, void* stream);

/* ---- correspondence RANSAC ---------------------------------------------------------------------
 * replaces open3d registration_ransac_based_on_correspondence as baseline_scripts/baseline_3DMatch.py:80-98 (--method RANSAC:
 * ransac_n 4, 1000 iterations, all correspondences) and evaluation/test_3DMatch.py:59-77, test_KITTI.py:59-77 (--solver RANSAC:
 * ransac_n 3, 5000 iterations, the correspondences the model labelled inliers) call it.  The contract is this project's, modelled
 * on open3d 0.9 RegistrationRANSACBasedOnCorrespondence as recalled; what cannot be checked without open3d is a named rule.
 * Per pair b: src, tgt [N][3] fp32 (row i = correspondence i; widened exactly); the candidate list L = the ascending indices
 * i < N_b with mask[i] > 0 (mask NULL: all of them), M = |L|; r = the distance threshold; I = max_iteration hypotheses.
 *   DRAW_RULE      position j < ransac_n of iteration i uses the counter c = ((pair_offset + b) * I + i) * 8 + j (64-bit, wrapping):
 *                  z = splitmix64's output for the state seed + (c + 1) * 0x9E3779B97F4A7C15, i.e. z ^= z >> 30,
 *                  z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31; position in L = (hi32(z) * M) >> 32.
 *                  Draws are with replacement (as 0.9's loop): a sample may repeat an index.  pair_offset makes a pair's draws
 *                  independent of how a driver groups pairs.  samples != NULL ([bs][I][ransac_n] int32 positions into L) replaces
 *                  the draws; a position < 0 or >= M makes that hypothesis invalid.
 *   hypothesis     Eigen's umeyama without scaling on the sample, fp64: means = sum * (1 / n), Sigma = (1 / n) sum (q - mB)(p - mA)^T,
 *                  pose from the library's one fp64 Kabsch entry (the one pdsc_icp_refine uses; its rank <= 1 fallback covers repeated
 *                  indices).  A non-finite pose is an invalid hypothesis: NaN pose, count 0, sumsq 0, never wins.
 *   SCORE_RULE     over every l in L (not the sample only): d2 = |R src_l + t - tgt_l|^2 in fp64; l is an inlier iff d2 < r * r, r * r
 *                  in fp64 (open3d compares sqrt(d2) < r: the two differ at the last ulp at most).  count = #inliers, sumsq = sum of
 *                  d2 over the inliers, DEFINED as the partial sums of the consecutive PDSC_RANSAC_CHUNK-entry chunks of L, each in list
 *                  order, added in ascending chunk order -- so that a pair's bits do not depend on the batch, the tiling or the run.
 *                  A NaN or inf coordinate compares false: never an inlier; a sample that contains one is an invalid hypothesis.
 *   SELECT_RULE    open3d's sequential update (fitness greater, or equal and rmse smaller) as an order: the largest count, then the
 *                  smallest sumsq (compared on sumsq, not on a rounded rmse), then the lowest iteration; count 0 never wins.
 *   NO_REFIT_RULE  the winner's pose is returned as solved from its sample: no refit on the inlier set (0.9 has none, as recalled).
 * Early outs, evaluated on the device where M lives: M < ransac_n, r <= 0 or r NaN: nothing wins.
 * Outputs: trans [bs][16] fp32 (the winner's pose rounded once; identity if nothing won), labels [bs][N] fp32 (1 at the winner's
 * inliers, all inside L; 0 elsewhere, padding rows included; labels sum to the winner's count exactly), fitness = count / M and
 * inlier_rmse = sqrt(sumsq / count) [bs] double (0 if nothing won), best_iter [bs] int32 (-1 if nothing won), num_candidates = M.
 * Optional (NULL = not wanted), the full hypothesis table: hyp_trans [bs][I][12] double (rows of R | t), hyp_count [bs][I] int32,
 * hyp_sumsq [bs][I] double.  counts [bs] int32 (DEVICE; NULL = every pair has N rows; rows beyond a pair's count are padding).
 * Four launches, no allocation, no host synchronisation (graph-capturable).  Limits: 1 <= bs <= PDSC_RANSAC_MAX_PAIRS,
 * 1 <= N <= PDSC_RANSAC_MAX_N, 1 <= max_iteration <= PDSC_RANSAC_MAX_ITERATIONS, 3 <= ransac_n <= 8; anything else, or a null pointer,
 * returns PDSC_ERR_ARG, a short workspace PDSC_ERR_WORKSPACE, with nothing enqueued.  workspace: pdsc_ransac_workspace_bytes(bs, N,
 * max_iteration) (0 for unsupported sizes). */
#define PDSC_RANSAC_CHUNK 512
#define PDSC_RANSAC_MAX_PAIRS 65535
#define PDSC_RANSAC_MAX_N (1 << 22)
#define PDSC_RANSAC_MAX_ITERATIONS (1 << 22)
size_t pdsc_ransac_workspace_bytes(int bs, int N, int max_iteration);
int pdsc_ransac_correspondence(const float* src, const float* tgt, const int* counts, const float* mask, const int* samples, double r,
                               int ransac_n, int max_iteration, unsigned long long seed, long long pair_offset, float* trans,
                               float* labels, double* fitness, double* inlier_rmse, int* best_iter, int* num_candidates,
                               double* hyp_trans, int* hyp_count, double* hyp_sumsq, void* workspace, size_t workspace_bytes, int bs,
                               int N, void* stream);
/* The same call for tools/ransac_bench.py: stage_ms [4] (HOST) receives the milliseconds of compact | hypothesise | score | select
 * between events on the stream.  This entry synchronises the host and cannot be captured. */
int pdsc_ransac_correspondence_stages(const float* src, const float* tgt, const int* counts, const float* mask, const int* samples,
                                      double r, int ransac_n, int max_iteration, unsigned long long seed, long long pair_offset,
                                      float* trans, float* labels, double* fitness, double* inlier_rmse, int* best_iter,
                                      int* num_candidates, double* hyp_trans, int* hyp_count, double* hyp_sumsq, void* workspace,
                                      size_t workspace_bytes, int bs, int N, float* stage_ms, void* stream);

/* ---- multiway edge step ------------------------------------------------------------------------
 * pdsc_information_matrix replaces open3d registration.get_information_matrix_from_point_clouds
 * (GetInformationMatrixFromPointClouds) as multiway/test_multi_ate.py:69-72 and :141-146 call it, per pair, fp64 throughout:
 *   P = trans * src (skipped when trans passes Eigen's isIdentity(), as in pdsc_icp_refine); the correspondence set is
 *   pdsc_icp_refine's evaluate step: each source point's nearest target with fp64 d2 < float(max_distance^2), equal distances:
 *   the lowest target index; for every correspondence with TARGET point (x, y, z) info += g g^T for the three rows
 *   g = (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1).
 * IDENTITY_RULE: open3d 0.9 is believed to start every OpenMP thread's private accumulator from the 6x6 identity (its result
 * then depends on the thread count); later versions start from zero.  Not checkable without open3d; this entry returns the
 * plain sum, so info[3][3] = info[4][4] = info[5][5] = num_corr exactly (what the driver's overlap gate reads, :147).
 * src [bs][Ns][3], tgt [bs][Nt][3] (fp32, widened exactly), trans [bs][16] fp32; Ns_per_pair / Nt_per_pair [bs] int32 (DEVICE;
 * NULL = every pair has Ns / Nt points; rows beyond a pair's count are padding and never read).
 * Outputs: info [bs][36] double (row-major 6x6, symmetric bit for bit, every entry written), num_corr [bs] int32, and
 * optionally corr [bs][Ns] int32 (NULL = not wanted): the target index of each source point, -1 = none and for padding rows.
 * max_distance <= 0 or an empty set: the zero matrix; a non-finite pose or point: a NaN matrix and num_corr 0.
 * One launch, no allocation, no host synchronisation (graph-capturable); a pair's result does not depend on its batch.
 * workspace: pdsc_information_workspace_bytes(bs, Ns, Nt). */
size_t pdsc_information_workspace_bytes(int bs, int Ns, int Nt);
int pdsc_information_matrix(const float* src, const float* tgt, const float* trans, const int* Ns_per_pair, const int* Nt_per_pair,
                            double max_distance, double* info, int* num_corr, int* corr, void* workspace, size_t workspace_bytes,
                            int bs, int Ns, int Nt, void* stream);

/* open3d PointCloud.voxel_down_sample (multiway/test_multi_ate.py:58-59) in two launches around a stable sort of the keys that
 * the caller provides: grid anchored at min - voxel_size / 2, fp64 floor((p - origin) / voxel_size) per axis, one output point per
 * occupied voxel = the fp64 mean of its points (summed in input order) rounded to fp32, output ordered by ascending voxel
 * index (ix dy + iy) dz + iz (open3d's own order is a hash-map artefact).
 *   pdsc_voxel_keys : points [bs][N][3], n_per_cloud [bs] int32 (DEVICE; NULL = N each) -> keys [bs][N] int64.  Padding rows,
 *                     and every row of a cloud with a non-finite point or a grid beyond 2^20 voxels per axis, get INT64_MAX.
 *                     voxel_size <= 0 (or not finite): PDSC_ERR_ARG.
 *   pdsc_voxel_means: sorted_keys [bs][N] = the keys of each cloud in ascending order, perm [bs][N] int64 = the STABLE permutation
 *                     that sorts them (sorted_keys[i] = keys[perm[i]]) -> out [bs][N][3] (one row per run of equal keys; rows
 *                     beyond the count are zero), counts [bs] int32.  A cloud whose keys are all INT64_MAX has count 0.  Entries
 *                     of perm outside [0, N) are skipped (nothing is read outside the cloud); a run left without a point is NaN.
 *                     Cost: a run of equal keys is summed by one thread in input order, so the time grows with the fullest voxel. */
int pdsc_voxel_keys(const float* points, const int* n_per_cloud, double voxel_size, long long* keys, int bs, int N, void* stream);
int pdsc_voxel_means(const float* points, const long long* sorted_keys, const long long* perm, float* out, int* counts, int bs,
                     int N, void* stream);

/* ---- FPFH descriptors ----------------------------------------------------------------------------
 * replaces the open3d calls of misc/cal_fpfh.py:21-26 on an already down-sampled cloud (estimate_normals with
 * KDTreeSearchParamHybrid(2 voxel, 30), compute_fpfh_feature with KDTreeSearchParamHybrid(5 voxel, 100)) and the normalisation of
 * demo_registration.py:43, f / (|f|_2 + 1e-6).  fp64 arithmetic throughout; batched over bs clouds of up to N points:
 * points [bs][N][3] fp32 (widened exactly), n_per_cloud [bs] int32 (DEVICE; NULL = N each; rows beyond a cloud's count are padding
 * and never read).  Every entry only enqueues kernels on `stream`: no allocation, no host synchronisation, graph-capturable; a
 * cloud's result does not depend on the batch it runs in.  Three named rules (open3d's own behaviour is an artefact there, or cannot
 * be checked without it):
 *   FLANN_RADIUS_RULE      a neighbour has fp64 d2 < float32(r * r), strict (as in pdsc_icp_refine);
 *   COVARIANCE_ORDER_RULE  the nine cumulants of a normal are summed in ascending neighbour INDEX order, so that two points with
 *                          the same neighbour set get bit-equal normals;
 *   NORMAL_SIGN_RULE       a normal n of point p is kept when dot(n, viewpoint - p) >= 0 and negated otherwise (open3d 0.9 leaves
 *                          the eigen-solver's arbitrary sign; orient_normals_towards_camera_location, default the origin).
 *
 * pdsc_hybrid_neighbours (KDTreeFlann::SearchHybrid): per point the at most max_nn (<= 128) nearest points of the same cloud under
 *   FLANN_RADIUS_RULE, ascending by (d2, index); the point itself is included.  idx [bs][N][max_nn] int32 (entries beyond the count:
 *   -1), d2 [bs][N][max_nn] double (optional; beyond the count: 0), count [bs][N] int32.  Padding rows have count 0; every row of a
 *   cloud with a non-finite point has count -1, which the three entries below turn into NaN rows.  d2 = (dx dx + dy dy) + dz dz.
 *   workspace: pdsc_hybrid_neighbours_workspace_bytes(bs, N) (the cell grid of icp_grid.h, built once per cloud per call).
 * pdsc_estimate_normals (open3d 0.9 EstimateNormals): from such lists (count >= 3: cumulants = means of x, y, z, xx, xy, xz, yy,
 *   yz, zz over the list under COVARIANCE_ORDER_RULE, C = E[p p^T] - E[p] E[p]^T, unit eigenvector of the smallest eigenvalue;
 *   fewer than 3 neighbours: (0, 0, 1)), then NORMAL_SIGN_RULE.  viewpoint: 3 doubles on the HOST, read before the call returns
 *   (NULL = the origin).  normals [bs][N][3] double; padding rows zero.
 * pdsc_spfh (ComputeSPFHFeature): spfh [bs][N][33] double; for count > 1 the pair features of list entries 1 .. count-1
 *   (ComputePairFeatures; a pair at distance 0 is binned as (0, 0, 0)) are counted into 3 x 11 bins and scaled by 100 / (count - 1).
 * pdsc_fpfh_from_spfh (ComputeFPFHFeature): f[j] = sum over list entries k >= 1 with d2_k != 0 of spfh[idx_k][j] / d2_k (list order),
 *   then f[j] = f[j] * (100 / sum of its block of 11, 0 when that sum is 0) + spfh[i][j].  fpfh_f64 [bs][N][33] double (optional),
 *   desc_f32 [bs][N][33] fp32 = f / (|f|_2 + 1e-6) (optional; one of the two is required).  Padding rows zero.
 * pdsc_fpfh chains the four: lists at normal_radius / normal_max_nn -> normals -> lists at feature_radius / feature_max_nn -> SPFH ->
 *   FPFH.  normals_out [bs][N][3] double is optional.  workspace: pdsc_fpfh_workspace_bytes(bs, N, normal_max_nn, feature_max_nn).
 * Bad arguments (null pointer, radius <= 0 or not finite, max_nn outside 1 .. 128, bs outside 1 .. 65535, N outside 1 .. 2^24,
 * workspace too small) return PDSC_ERR_ARG with nothing enqueued. */
#define PDSC_FPFH_DIM 33
#define PDSC_FPFH_MAX_NN 128
size_t pdsc_hybrid_neighbours_workspace_bytes(int bs, int N);
int pdsc_hybrid_neighbours(const float* points, const int* n_per_cloud, double radius, int max_nn, int* idx, double* d2, int* count,
                           void* workspace, size_t workspace_bytes, int bs, int N, void* stream);
int pdsc_estimate_normals(const float* points, const int* n_per_cloud, const int* idx, const int* count, int max_nn,
                          const double* viewpoint, double* normals, int bs, int N, void* stream);
int pdsc_spfh(const float* points, const int* n_per_cloud, const double* normals, const int* idx, const int* count, int max_nn,
              double* spfh, int bs, int N, void* stream);
int pdsc_fpfh_from_spfh(const double* spfh, const int* n_per_cloud, const int* idx, const double* d2, const int* count, int max_nn,
                        double* fpfh_f64, float* desc_f32, int bs, int N, void* stream);
size_t pdsc_fpfh_workspace_bytes(int bs, int N, int normal_max_nn, int feature_max_nn);
int pdsc_fpfh(const float* points, const int* n_per_cloud, double normal_radius, int normal_max_nn, double feature_radius,
              int feature_max_nn, const double* viewpoint, double* fpfh_f64, float* desc_f32, double* normals_out, void* workspace,
              size_t workspace_bytes, int bs, int N, void* stream);

/* ---- FPFH from raw clouds ------------------------------------------------------------------------
 * The demo's recipe (demo_registration.py:37-44, --descriptor fpfh) for clouds of any size up to 2^24 points: estimate_normals on the
 * RAW cloud (pdsc_cloud_neighbours at (2 voxel, 30) + pdsc_estimate_normals), voxel_down_sample(voxel) that also averages the normals
 * of each voxel (pdsc_cloud_voxel_keys, the caller's stable sort, pdsc_cloud_voxel_means), compute_fpfh_feature on the down-sampled
 * cloud with those normals (pdsc_hybrid_neighbours + pdsc_spfh + pdsc_fpfh_from_spfh).  The three pdsc_cloud_* entries take a
 * `path` selector, as pdsc_sm_baseline_form takes `form`:
 *   PDSC_PATH_AUTO (0)           PDSC_PATH_MANY from N >= PDSC_CLOUD_AUTO_MANY rows per cloud on, PDSC_PATH_ONE_WORKGROUP below;
 *                                PDSC_CLOUD_AUTO_MANY is 2^30, above every admissible N: no time of a raw cloud has been measured
 *                                yet, so auto is PDSC_PATH_ONE_WORKGROUP for every shape and PDSC_PATH_MANY is OPT-IN (DESIGN.md
 *                                f-9); the threshold moves down (never below 32768) once a measurement shows where path 2 wins;
 *   PDSC_PATH_ONE_WORKGROUP (1)  the kernels of f-6 / f-7: one 512-thread workgroup per cloud;
 *   PDSC_PATH_MANY (2)           chains of ordinary kernels with one workgroup per 1024 points (512 sorted keys for the means):
 *                                chunk boxes -> reduce -> keys; run heads per tile -> scan -> means; chunk boxes -> grid -> bucket
 *                                histogram -> scan -> scatter.  No kernel waits for another workgroup.
 * Both paths give bit-identical results: min / max are order-free, a key depends on its point and the box alone, a run of equal keys
 * is summed by one thread in input order either way, and the neighbour search ranks its candidates by (d2, index), whatever their
 * order inside a hash bucket.  pdsc_hybrid_neighbours and pdsc_fpfh behave as PDSC_PATH_AUTO (their workspace holds the chunk boxes);
 * pdsc_voxel_keys / pdsc_voxel_means have no workspace and stay on one workgroup per cloud.
 * Two named rules:
 *   VOXEL_NORMAL_RULE  the normal of a voxel is sum(n_i) / count over its points (fp64, summed in input order), NOT renormalised.
 *                      This restates open3d 0.9's AccumulatedPoint::GetAverageNormal from memory: open3d is not available where this
 *                      was written, so the text here is the contract.  Later open3d versions normalise the average, hence the flag:
 *                      renormalize = 1 gives n / |n| (|n| = sqrt((x x + y y) + z z)), and a zero mean stays (0, 0, 0).  The pair
 *                      features of pdsc_spfh use whatever comes out, as open3d's do.
 *   CAPACITY_RULE      out_capacity = output rows per cloud.  A cloud with more occupied voxels than out_capacity gets count -1 and
 *                      out_capacity zero rows; nothing is ever written beyond out_capacity rows.  (pdsc_hybrid_neighbours, pdsc_spfh,
 *                      ... read a negative n_per_cloud entry as an empty cloud.)
 * pdsc_cloud_voxel_keys : pdsc_voxel_keys with a path.
 * pdsc_cloud_voxel_means: pdsc_voxel_means (same keys, same stable-sort contract, same output order, bit-equal mean points) that also
 *   averages normals [bs][N][3] double -> out_points [bs][out_capacity][3] fp32, out_normals [bs][out_capacity][3] double (rows beyond
 *   the count: zero), counts [bs] int32.
 * pdsc_cloud_neighbours : pdsc_hybrid_neighbours with a path; workspace: pdsc_hybrid_neighbours_workspace_bytes(bs, N).
 * workspace of the two voxel entries: pdsc_cloud_voxel_workspace_bytes(bs, N) (chunk boxes and head counts; required on every path).
 * Enqueue-only, graph-capturable.  Bad arguments (null pointer, bs outside 1 .. 65535, N outside 1 .. 2^24, out_capacity < 1,
 * renormalize not 0 / 1, path outside 0 .. 2, workspace too small) return PDSC_ERR_ARG with nothing enqueued. */
#define PDSC_PATH_AUTO 0
#define PDSC_PATH_ONE_WORKGROUP 1
#define PDSC_PATH_MANY 2
#define PDSC_CLOUD_AUTO_MANY 1073741824
size_t pdsc_cloud_voxel_workspace_bytes(int bs, int N);
int pdsc_cloud_voxel_keys(const float* points, const int* n_per_cloud, double voxel_size, long long* keys, void* workspace,
                          size_t workspace_bytes, int bs, int N, int path, void* stream);
int pdsc_cloud_voxel_means(const float* points, const double* normals, const long long* sorted_keys, const long long* perm,
                           float* out_points, double* out_normals, int* counts, int out_capacity, int renormalize, void* workspace,
                           size_t workspace_bytes, int bs, int N, int path, void* stream);
int pdsc_cloud_neighbours(const float* points, const int* n_per_cloud, double radius, int max_nn, int* idx, double* d2, int* count,
                          void* workspace, size_t workspace_bytes, int bs, int N, int path, void* stream);

/* ---- pose-graph optimisation ---------------------------------------------------------------------
 * pdsc_global_optimization replaces o3d.registration.global_optimization(pose_graph, GlobalOptimizationLevenbergMarquardt(),
 * GlobalOptimizationConvergenceCriteria(), option) as multiway/test_multi_ate.py:166-174 and :217-224 call it, for a ragged batch
 * of graphs, fp64 throughout.  open3d cannot be consulted here: this text (open3d 0.9's algorithm restated) is the contract.
 *   graph: node poses [4][4] (fragment -> world); edges (s, t, X [4][4] source -> target, Lambda [6][6], uncertain).
 *   residual of an edge: A = X^-1 pose_t^-1, e = lin6(A pose_s), lin6(M) = ((M21 - M12) / 2, (M02 - M20) / 2, (M10 - M01) / 2,
 *     M03, M13, M23);  column k of Js = lin6(A G_k pose_s), G_k the generators (alpha: G12 = -1, G21 = 1; beta: G02 = 1,
 *     G20 = -1; gamma: G01 = -1, G10 = 1; a, b, c: G03, G13, G23 = 1);  Jt = -Js.
 *   line process: w = preference_loop_closure * max_correspondence_distance^2 * mean over the live edges of Lambda[5][5] (0 without
 *     live edges); confidence of an uncertain edge = (w / (w + e^T Lambda e))^2, 1 before the first update; its weight l in the
 *     system is the confidence, a certain edge's is 1.
 *   objective: sum over uncertain edges of l e^T Lambda e + w (sqrt(l) - 1)^2, plus sum over certain edges of e^T Lambda e.
 *   system: per live edge H[s][s] += l Js^T Lambda Js, H[s][t] += l Js^T Lambda Jt, H[t][s] += l Jt^T Lambda Js, H[t][t] += l Jt^T
 *     Lambda Jt, b[s] -= l Js^T Lambda e, b[t] -= l Jt^T Lambda e; every entry is summed over its incident edges in ascending
 *     edge index.
 *   one pass: w; residuals; cur = objective; update the confidences; H, b; lambda = 1e-5 max diag H; nu = 2; stop = max b < 1e-6;
 *     x = mat2vec of every pose; for (iter = 0; !stop; iter++) { lm = 0; do { delta = solve((H + lambda I) delta = b);
 *     stop |= |delta| < 1e-6 (|x| + 1e-6); if (!stop) { pose'_i = vec2mat(delta_i) pose_i; new = objective of pose' (same
 *     confidences); rho = (cur - new) / (delta . (lambda delta + b) + 1e-3); if (rho > 0) { stop |= cur - new < 1e-6 cur; if
 *     (stop) break; lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)); nu = 2; accept pose', cur = new, x; update the confidences;
 *     rebuild H, b; stop |= max b < 1e-6; if (stop) break; } else { lambda *= nu; nu *= 2; } } lm++; stop |= lm >= 20; } while
 *     (!(rho > 0 || stop)); stop |= iter >= 100 || cur < 1e-6; }  finally every pose is multiplied from the left by
 *     pose_ref(at the start of the pass) pose_ref(now)^-1 (open3d does not fix the reference node in the solve).
 *     vec2mat(v): R = Rz(v2) Ry(v1) Rx(v0), t = v[3:6];  mat2vec(T) (used for |x| only): sy = hypot(R00, R10); sy not < 1e-6:
 *     (atan2(R21, R22), atan2(-R20, sy), atan2(R10, R00)), otherwise (atan2(-R12, R11), atan2(-R20, sy), 0).
 *   global optimisation: pass 1 on the live edges; an edge stays live when it is certain or its confidence > edge_prune_threshold;
 *     pass 2 on the survivors from pass 1's poses and confidences (w over the survivors); prune again.  Pruning is a mask.
 * Named rules:
 *   INVERSE_RULE  the inverse of a pose is [R^-1, -R^-1 t; 0 0 0 1] with R^-1 = adj(R) / det(R), not R^T (the forward's fp32
 *                 rotations are orthogonal to about 1e-7 only, and open3d takes the general inverse);
 *   SOLVE_RULE    open3d solves with Eigen's ldlt(); here a blocked Cholesky with fused multiply-adds (H + lambda I is positive
 *                 definite; any backward-stable factorisation agrees within the tolerance of tests/test_posegraph.py).
 * Validity (this library's rule, not open3d's ValidatePoseGraph): a graph with a non-finite entry, an index outside [0, F) or
 * s == t in a live edge, a non-finite node pose, reference_node >= F, or more nodes / edges than max_nodes / max_edges returns
 * NaN poses, its input mask, confidences of 1 and status 1; nothing else in the batch is affected.  A graph without live edges
 * returns its nodes unchanged with status 0.
 * nodes [sum F][16], source / target [sum E] int32 (node index inside the edge's graph), X [sum E][16], info [sum E][36],
 * uncertain [sum E] u8, live_in [sum E] u8 (NULL = all live), node_offset / edge_offset [num_graphs + 1] int32 (DEVICE; graph g owns
 * nodes node_offset[g] .. node_offset[g + 1]), total_nodes / total_edges = the arrays' lengths (offsets beyond them: status 1,
 * nothing else of that graph is written).  Outputs: nodes_out [sum F][16] (must not alias nodes), confidence [sum E] (1 for an
 * edge that never was live or is certain), live_out [sum E] u8, record [num_graphs][PDSC_POSEGRAPH_RECORD] double: [0] status,
 * [1..4] pass 1's outer iterations, solves, final objective and w, [5..8] pass 2's, [9..11] live edges at the start, after the first
 * pruning, at the end; ticks [num_graphs][3] int64 (optional, NULL = not wanted; tools/posegraph_bench.py): the workgroup's time in
 * residuals + assembly, in the solves and in the whole graph, in ticks of the constant 100 MHz device clock.  One launch of one persistent workgroup per graph; graphs exit independently; no allocation, no host
 * synchronisation (graph-capturable); a graph's bits do not depend on its batch.  workspace: pdsc_posegraph_workspace_bytes.
 * pdsc_posegraph_nodes: the driver's node chain (:129-130) per graph: node 0 = I, odometry = I; per live certain edge in order
 *   odometry = X odometry, the next node = odometry^-1 (INVERSE_RULE); nodes the chain does not reach are NaN; a graph whose offsets
 *   leave the arrays is not written at all.
 * Bad arguments (null pointer, counts out of range, NaN option, workspace too small) return PDSC_ERR_ARG with nothing enqueued. */
#define PDSC_POSEGRAPH_MAX_NODES 128
#define PDSC_POSEGRAPH_RECORD 12
size_t pdsc_posegraph_workspace_bytes(int num_graphs, int max_nodes, int max_edges);
int pdsc_posegraph_nodes(const double* X, const unsigned char* uncertain, const unsigned char* live, const int* node_offset,
                         const int* edge_offset, double* nodes, int num_graphs, int total_nodes, int total_edges, void* stream);
int pdsc_global_optimization(const double* nodes, const int* source, const int* target, const double* X, const double* info,
                             const unsigned char* uncertain, const unsigned char* live_in, const int* node_offset,
                             const int* edge_offset, double max_correspondence_distance, double edge_prune_threshold,
                             double preference_loop_closure, int reference_node, double* nodes_out, double* confidence,
                             unsigned char* live_out, double* record, long long* ticks, void* workspace, size_t workspace_bytes,
                             int num_graphs, int max_nodes, int max_edges, int total_nodes, int total_edges, void* stream);

/* Named views into the workspace of the last layout computed for (cfg, bs, N, num_seeds): lets the
 * parity tests read intermediates after pdsc_forward.  Returns byte offset or -1. */
long long pdsc_workspace_offset(const pdsc_config* cfg, int bs, int N, int num_seeds, const char* name);

/* ---- opt-in kernel timing (bench.py's roofline leg) ----------------------------------------------
 * When enabled, the two roofline kernels are bracketed by hipEvents recorded on the caller's stream:
 * kind 0 = sc_attention_kernel (MFMA roofline), kind 1 = compat_kernel (HBM roofline).  Disabled by
 * default: then no event is created or recorded.  pdsc_profile_read synchronises on the recorded events
 * (host side, call it after the timed region) and returns total milliseconds + number of launches. */
enum pdsc_profile_kind { PDSC_PROF_ATTENTION = 0, PDSC_PROF_COMPAT = 1, PDSC_PROF_LAYER = 2 /* tail + head launches */,
                         PDSC_PROF_NUM_KINDS = 3 };
int pdsc_profile_enable(int max_records_per_kind);   /* 0 disables and frees the events */
int pdsc_profile_reset(void);
/* bracket only every stride-th launch of `kind` (an event record costs the stream a few microseconds and separates the
 * kernels around it; bench.py samples one attention / layer launch per forward: the launches of a kind do identical work) */
int pdsc_profile_set_stride(int kind, int stride);
int pdsc_profile_read(int kind, double* total_ms, int* launches);

/* ---- the losses of libs/loss.py on the device, with their gradients ---------------------------
 * What the reference's validation and training loops (libs/trainer.py:95-107,186-194) apply to the outputs of the validation
 * forward.  Every call is asynchronous on `stream`, allocates nothing, does not synchronise and can be captured in a graph.
 * Every call is deterministic: no floating-point atomics; workgroups write fp64 partials into `ws` and a one-workgroup finishing
 * launch adds them in a fixed order.  Labels `gt` are 0 / 1 floats.  The per-element arithmetic and every sum are fp64 (computed
 * from the fp32 inputs), except where pdsc_sm_loss_features says otherwise; the gradients of the fp64 losses (dpred, dM) are
 * fp64 arrays.  All calls may share one workspace of pdsc_loss_workspace_bytes(bs, N) bytes (calls on one stream are ordered). */
size_t pdsc_loss_workspace_bytes(int bs, int N);

/* ClassificationLoss.forward (libs/loss.py:85-102).  pred, gt, weight [bs][N].
 *   num_pos = relu(sum gt - 1) + 1, num_neg = relu(sum (1 - gt) - 1) + 1 over the whole batch;
 *   weight != NULL: loss = mean(bce * weight); else balanced == 0: mean(bce); else mean(bce with pos_weight = num_neg / num_pos);
 *   bce = (1 - y) x + (1 + (pos_weight - 1) y) (log1p(exp(-|x|)) + max(-x, 0)).
 *   stats[0..7] = loss, precision, recall, F1 (pair 0 only, `pred > 0`, 0 where sklearn's zero_division applies), mean logit of the
 *   inliers, mean logit of the outliers (whole batch, denominators max(1, count)), num_pos, num_neg.
 *   dpred [bs][N] (fp64, or NULL) = d loss / d pred (the weights depend on gt only). */
int pdsc_classification_loss(const float* pred, const float* gt, const float* weight, int balanced, double* stats, double* dpred,
                             void* ws, size_t ws_bytes, int bs, int N, void* stream);

/* SpectralMatchingLoss.forward (libs/loss.py:129-138) on a given M [bs][N][ld >= N], read once.
 *   gt_M[i][j] = gt_i gt_j for i != j, 0 on the diagonal (never stored); with k = the pair's number of inliers the class sizes are
 *   P = relu(k (k - 1) - 1) + 1 and Q = relu(N^2 - k (k - 1) - 1) + 1 (the diagonal counts as negative, as in the reference).
 *   per pair l_b = balanced ? 0.5 sum_pos (M - 1)^2 / P + 0.5 sum_neg M^2 / Q : sum (M - gt_M)^2 / N^2;   loss[0] = mean_b l_b.
 *   The fp64 values l_b are left in the first bs doubles of `ws`.
 *   dM [bs][N][ld] (fp64, or NULL) = d loss / d M; only columns 0 .. N-1 of a row are written, the pad columns (ld > N) are left
 *   as they were. */
int pdsc_sm_loss_matrix(const float* M, long long ld, const float* gt, int balanced, double* loss, double* dM, void* ws,
                        size_t ws_bytes, int bs, int N, void* stream);

/* The same loss of M = clamp(1 - (1 - F F^T) / sigma^2, 0, 1) with a zero diagonal (models/PointDSC.py:160-163), taken from
 * normed = F [bs*N][128] without M ever being stored.  The Gram tiles run on v_mfma_f32_32x32x2_f32 in the k order of
 * pdsc_feature_compat and the clamp expression is the same fp32 expression, so loss[0] (and the l_b in `ws`) equal
 * pdsc_sm_loss_matrix on the matrix pdsc_feature_compat writes, bit for bit.
 *   dnormed [bs*N][128] (fp32, or NULL) = d loss / d F with g_ij = c_ij 2 (M_ij - gt_M_ij) [0 <= raw_ij <= 1] [i != j]
 *   (inclusive mask: torch.clamp's backward), c_ij the loss weight: dF_i = (2 / sigma^2) sum_j g_ij F_j, a second fp32 MFMA product.
 *   dsigma [1] (fp64, or NULL) = sum_ij g_ij 2 (1 - s_ij) / sigma^3.   Either gradient pointer may be NULL on its own. */
int pdsc_sm_loss_features(const float* normed, const float* sigma, const float* gt, int balanced, double* loss, float* dnormed,
                          double* dsigma, void* ws, size_t ws_bytes, int bs, int N, void* stream);

/* TransformationLoss.forward (libs/loss.py:34-63), forward only.  trans, gt_trans [bs][16]; src, tgt [bs][N][3]; probs [bs][N].
 *   out[0..4] = loss, recall [%], RE [deg], TE [cm], RMSE, each the mean over the bs pairs.
 *   RE = acos(clamp((trace(R^T gR) - 1) / 2, -1, 1)) in degrees, TE in cm, a pair counts for the recall if TE < te_thre && RE < re_thre.
 *   THE REFERENCE'S BROADCAST IS MIRRORED: `warp_src_keypts - tgt_keypts` subtracts pair i's warped [N][3] from the whole
 *   [bs][N][3] target, so pair i's RMSE and squared loss are means over all bs * N rows (row (j, n): R_i src[i][n] + t_i - tgt[j][n]).
 *   That is the definition for bs > 1; for bs == 1 it is the intended per-pair mean.  A pair with no probs > 0 adds 0 to the loss. */
int pdsc_transformation_loss(const float* trans, const float* gt_trans, const float* src, const float* tgt, const float* probs,
                             float re_thre, float te_thre, double* out, void* ws, size_t ws_bytes, int bs, int N, void* stream);

/* ---- backward of the spatial-consistency attention --------------------------------------------
 * The one operation of the training path that torch can only differentiate by materialising bs x N x N scores.  Exact fp32 on
 * v_mfma_f32_32x32x2_f32 like pdsc_sc_attention; no floating-point atomics: every sum has a fixed order and repeat calls are
 * bit-identical.  Asynchronous on `stream`, no allocation, no synchronisation.
 *   qkv, dqkv [bs*N][384] rows (q | k | v), q pre-scaled by log2(e)/sqrt(128) as everywhere in the library; dqkv is the gradient
 *   with respect to the rows AS PASSED (the caller scales dq back by the same factor for the gradient of an un-scaled q).
 *   compat [bs][N][ld] fp32, ld a multiple of 4 and >= N rounded up to 32; it gets no gradient (the reference builds it under
 *   no_grad).   msg, dmsg [bs*N][128];   lse [bs*N].
 * pdsc_sc_attention_lse: pdsc_sc_attention that also leaves lse[o] = m_o + log2(l_o), the log2-domain row statistic of the
 *   softmax (P_oi = exp2(compat_oi <q_o, k_i> - lse_o)); msg is bit for bit pdsc_sc_attention's at the same nsplit; scratch as
 *   pdsc_attention_scratch_bytes.
 * pdsc_sc_attention_backward: D_o = <dmsg_o, msg_o>; dV_i = sum_o P_oi dmsg_o; dZ_oi = compat_oi P_oi (<dmsg_o, v_i> - D_o);
 *   dq_o = ln2 sum_i dZ_oi k_i; dk_i = ln2 sum_o dZ_oi q_o.  Launches: the row dots, one workgroup per 128 queries and key split
 *   (dq), one per 128 keys and query split (dk, dv), both recomputing the scores from lse, and for nsplit > 1 the merge of the
 *   per-split partial sums in index order.  workspace: pdsc_attention_backward_workspace_bytes.
 * pdsc_sc_attention_backward_split: the same with the split count given (<= 0: pdsc_attention_backward_default_split, which aims
 *   at one workgroup per CU; clamped to the number of 32-row tiles); workspace: pdsc_attention_backward_split_workspace_bytes at
 *   the same nsplit.  pdsc_sc_attention_backward is nsplit = 0.  Results at different nsplit differ in summation order only.
 * Bad arguments (null pointer, bs or N <= 0, bad ld, workspace too small) return an error with nothing enqueued. */
int pdsc_sc_attention_lse(const float* qkv, const float* compat, long long ld, float* msg, float* lse, void* scratch,
                          size_t scratch_bytes, int bs, int N, int nsplit, void* stream);
size_t pdsc_attention_backward_workspace_bytes(int bs, int N);
int pdsc_sc_attention_backward(const float* qkv, const float* compat, long long ld, const float* msg, const float* lse,
                               const float* dmsg, float* dqkv, void* workspace, size_t workspace_bytes, int bs, int N,
                               void* stream);
int pdsc_attention_backward_default_split(int bs, int N);
size_t pdsc_attention_backward_split_workspace_bytes(int bs, int N, int nsplit);
int pdsc_sc_attention_backward_split(const float* qkv, const float* compat, long long ld, const float* msg, const float* lse,
                                     const float* dmsg, float* dqkv, void* workspace, size_t workspace_bytes, int bs, int N,
                                     int nsplit, void* stream);

/* ---- backward of the feature-similarity matrix -------------------------------------------------
 * What lets a loss of res['M'] (the train-mode forward's M, pdsc_feature_compat) reach the weights: for an upstream gradient
 * dM [bs][N][ld >= N] (fp32, NOT assumed symmetric; the pad columns [N, ld) are never read) and normed = F [bs*N][128]
 *   live_ij = (i != j) and 0 <= raw_ij <= 1 with raw_ij = 1 - (1 - <F_i, F_j>) / sigma^2 computed by the text pdsc_feature_compat
 *   uses (the mask is that of the M the forward wrote; inclusive, as torch.clamp's backward);   g_ij = live_ij ? dM_ij : 0
 *   dnormed [bs*N][128] (fp32, or NULL): dF_i = (1 / sigma^2) sum_j (g_ij + g_ji) F_j, both products exact fp32 on
 *   v_mfma_f32_32x32x2_f32;   dsigma [1] (fp64, or NULL) = (2 / sigma^3) sum_b sum_ij g_ij (1 - <F_i, F_j>).
 * At least one of the two must be asked for; either alone gives the bits it has in the pair.  Dead entries, the diagonal and
 * everything outside the N x N matrix are selected to 0: NaN or inf there does not reach the result.  No floating-point atomics:
 * one workgroup owns 128 rows of a pair, dsigma goes through fp64 partials in `ws` (pdsc_feature_compat_backward_workspace_bytes)
 * that a finishing launch adds in index order; repeat calls are bit-identical, and a pair's dnormed does not depend on the batch
 * it shares the launch with.  Asynchronous on `stream`, no allocation, no synchronisation.  Bad arguments (null pointer, bs or
 * N <= 0, ld < N, workspace too small) return an error with nothing enqueued. */
size_t pdsc_feature_compat_backward_workspace_bytes(int bs, int N);
int pdsc_feature_compat_backward(const float* normed, const float* sigma, const float* dM, long long ld, float* dnormed,
                                 double* dsigma, void* ws, size_t ws_bytes, int bs, int N, void* stream);

/* ---- transformation loss with a gradient: backward of the per-seed solver -----------------------
 * pdsc_seed_solve_backward: for an upstream gradient d_seed_trans [bs][S][16] of the hypotheses pdsc_seed_transforms writes (row 3
 * of every 4x4 is ignored), the gradient of the whole per-seed chain of models/PointDSC.py:248-320 -- gather, k x k feature *
 * spatial matrix, power iteration, weight normalisation, rigid_transform_3d -- with respect to the features and sigma:
 *   dnormed [bs][N][128] (fp32, or NULL; every row is written, rows no active seed names are 0) and dsigma [1] (fp64, or NULL).
 * normed, src, tgt, knn_idx, sigma, sigma_spat, num_iterations as pdsc_seed_power_iteration takes them (1 <= k <= PDSC_MAX_K,
 * 0 <= num_iterations <= PDSC_MAX_POWER_ITERS); conv_mask [bs] as pdsc_seed_transforms takes it (after pdsc_conv_mask_all_pairs
 * where the forward applied it): the iterate T the forward chose is replayed, nothing else of the forward is read.
 * One wavefront per seed rebuilds G = F F^T (accumulated in fp64) and M, keeps them in LDS, replays v_1 .. v_T, redoes the
 * Procrustes (3x3 part in fp64 registers) and walks the chain backwards.  A seed whose twelve upstream values are all zero returns
 * at once.  num_iterations == 0: v = 1, no path to the features -- both gradients are exact zeros.
 * No floating-point atomics: per-seed k x 128 blocks and fp64 dsigma terms in `ws`, then an owner pass that adds the blocks of a
 * row in (seed, neighbour) order; repeat calls are bit-identical.  An entry of knn_idx outside [0, N) is never used as an address:
 * that seed's block and dsigma term become NaN.  A seed whose M v is the zero vector gives NaN, as torch's autograd does.
 * src, tgt, sigma_spat and knn_idx get no gradient.  Asynchronous on `stream`, no allocation, no synchronisation.  Bad arguments
 * (null pointer, sizes out of range, workspace too small) return an error with nothing enqueued. */
size_t pdsc_seed_solve_backward_workspace_bytes(int bs, int N, int S, int k);
int pdsc_seed_solve_backward(const float* normed, const float* src, const float* tgt, const int* knn_idx, const float* sigma,
                             const float* sigma_spat, const unsigned int* conv_mask, const float* d_seed_trans, float* dnormed,
                             double* dsigma, void* ws, size_t ws_bytes, int bs, int N, int S, int k, int num_iterations,
                             void* stream);

/* d loss / d trans of the value pdsc_transformation_loss returns in out[0]: dtrans [bs][16] fp64, row 3 of every 4x4 zero.
 *   d / dT_i[r][c] = (2 / (bs bs N)) sum_(j,n) (R_i src[i][n] + t_i - tgt[j][n])_r (src[i][n]_c | 1): the reference's broadcast
 *   over the batch included; a pair with no probs > 0 gets exact zeros.  fp64 sums in a fixed order; workspace as the losses'. */
int pdsc_transformation_loss_grad(const float* trans, const float* src, const float* tgt, const float* probs, double* dtrans,
                                  void* ws, size_t ws_bytes, int bs, int N, void* stream);

/* ---- train-mode point-wise layer: Conv1d(k=1) -> BatchNorm1d (batch statistics) -> ReLU, forward and backward (DESIGN.md
 *      section 8 f-15; reference models/PointDSC.py:12-23,54-61 under model.train()) ------------------------------------------
 * Channel-last rows: X [M][Cin], W [Cout][Cin], b, gamma, beta, running_mean, running_var [Cout], all fp32 and contiguous.
 * Supported (Cin, Cout): (128,128) PointCN_layer_i, (128,64) fc_message.0-2, (64,64) fc_message.3-5; M >= 2, any value.
 * pdsc_pointwise_train_forward:
 *   Y = X W^T + b;   mean_c, var_c = mean and BIASED variance of Y[:, c] over the M rows;   invstd = 1 / sqrt(var + eps);
 *   Z = relu(gamma (Y - mean) invstd + beta);
 *   running_mean <- (1 - momentum) running_mean + momentum mean;
 *   running_var  <- (1 - momentum) running_var  + momentum var M / (M - 1)      (the unbiased variance, as F.batch_norm(training=True))
 *   Outputs Z [M][Cout], and for the backward Y [M][Cout], mean [Cout], invstd [Cout] -- the two statistics in FP64 (Z is computed
 *   from their fp32 roundings, in fp32); both running statistics are updated IN PLACE.
 *   The variance is mean-centred throughout (per 64-row tile in fp64, tiles merged as sum M2_t + n_t (mean_t - mean)^2 in fp64):
 *   a channel offset many times its spread costs nothing.
 * pdsc_pointwise_train_backward, given dZ [M][Cout] and Y, mean, invstd of the forward (the ReLU mask is rebuilt from Y with the
 * forward's own expression: the same bits as Z > 0; behind the mask xh and dY are evaluated in fp64 from the fp64 statistics and
 * rounded once -- with few rows dY is a small difference of O(1) terms):
 *   g = dZ [Z > 0];   dbeta = sum_rows g;   dgamma = sum_rows g xh,  xh = (Y - mean) invstd;
 *   dY = gamma invstd (g - dbeta / M - xh dgamma / M);   db = sum_rows dY (zero in exact arithmetic, computed as autograd does);
 *   dW [Cout][Cin] = dY^T X;   dX [M][Cin] = dY W.
 *   Each of dX, dW, db, dgamma, dbeta may be NULL (not wanted; at least one must be asked for); the ones asked for have the bits
 *   they have when all are.
 * The three products are exact fp32 on v_mfma_f32_32x32x2_f32.  No floating-point atomics: per-tile and per-workgroup partials in
 * `ws` (pdsc_pointwise_train_workspace_bytes; 8-byte aligned, the same size serves both calls) added in index order; repeat calls
 * are bit-identical.  X, W, Y, Z, dZ, dX must be 16-byte aligned.  Asynchronous on `stream`, no allocation, no synchronisation, no
 * memset.  Returns PDSC_ERR_ARG (null pointer, unsupported (Cin, Cout), M < 2, momentum outside [0,1], eps < 0, misaligned
 * pointer) or PDSC_ERR_WORKSPACE with nothing enqueued; pdsc_pointwise_train_workspace_bytes returns 0 for unsupported sizes. */
size_t pdsc_pointwise_train_workspace_bytes(int M, int Cin, int Cout);
int pdsc_pointwise_train_forward(const float* X, const float* W, const float* b, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, float momentum, float eps, float* Y, float* Z,
                                 double* mean, double* invstd, void* ws, size_t ws_bytes, int M, int Cin, int Cout, void* stream);
int pdsc_pointwise_train_backward(const float* X, const float* W, const float* gamma, const float* beta, const float* Y,
                                  const double* mean, const double* invstd, const float* dZ, float* dX, float* dW, float* db,
                                  float* dgamma, float* dbeta, void* ws, size_t ws_bytes, int M, int Cin, int Cout, void* stream);

/* ---- train-mode plain linears: layer0, fc_message.6 with its residual, the q|k|v projection, the classification head, forward
 *      and backward (reference models/PointDSC.py:36-45,65-77,171 under model.train()) ----------------
 * Channel-last rows, all fp32 and contiguous, any M >= 1.  Every product is exact fp32 on v_mfma_f32_32x32x2_f32 over 64-row
 * tiles.  No floating-point atomics: the backward's parameter gradients are one partial per persistent workgroup in `ws`, added in
 * index order; repeat calls are bit-identical.  Every output of a backward may be NULL (not wanted; at least one must be asked
 * for); the ones asked for have the bits they have when all are.  The forwards need no workspace; a backward's `ws` is always
 * required (pdsc_*_train_workspace_bytes; 16-byte aligned).  Matrices (X, W*, R, Y, qkv, dY, dqkv, dX) must be 16-byte aligned.
 * Asynchronous on `stream`, no allocation, no synchronisation, no memset.  Returns PDSC_ERR_ARG (null pointer, unsupported
 * (Cin, Cout), M < 1, misaligned pointer) or PDSC_ERR_WORKSPACE with nothing enqueued; the workspace queries return 0 for
 * unsupported sizes.
 *
 * pdsc_linear_train_forward:   Y [M][Cout] = X [M][Cin] W^T + b (+ R [M][Cout]; NULL: no residual).
 * pdsc_linear_train_backward:  dX [M][Cin] = dY W;  dW [Cout][Cin] = dY^T X;  db [Cout] = sum_rows dY.  (dR is dY itself.)
 *   dX and dW / db come from two independent launches: an output that is not wanted costs neither staging nor matrix instructions.
 *   Supported (Cin, Cout): (1 .. 16, 128) layer0 (Cin padded with zeros in LDS), (64, 128) fc_message.6.
 *
 * pdsc_qkv_train_forward:   qkv [M][384] = (q_scale (X Wq^T + bq) | X Wk^T + bk | X Wv^T + bv), X [M][128], W* [128][128]: the
 *   layout pdsc_sc_attention_lse takes.  The scale is applied to the PRODUCT, after the bias (one more rounding of q), not to the
 *   weights.
 * pdsc_qkv_train_backward:  with g = (q_scale dq | dk | dv) of dqkv [M][384], rounded once:  dX [M][128] = g_q Wq + g_k Wk + g_v Wv
 *   (one accumulator, parts in this order);  dW* = g_*^T X;  db* = sum_rows g_*: the gradients of the UN-scaled parameters.
 *
 * pdsc_head_train_forward:   logits [M] = relu(relu(X W0^T + b0) W1^T + b1) . w2 + b2, X [M][128], W0 [32][128], W1 [32][32],
 *   W2 [1][32], in one launch.  pre [M][64] (may be NULL: the training path passes NULL) receives the two pre-activations
 *   (X W0^T + b0 | relu(.) W1^T + b1) as the kernel holds them, for tests that need the kernel's own ReLU masks.
 * pdsc_head_train_backward:  from dlogits [M]: dX [M][128], dW0, db0, dW1, db1, dW2, db2.  Both pre-activations are recomputed per
 *   tile by the forward's own code and the two ReLU masks taken from them: the forward's bits, no mask tensor.  One launch computes
 *   all parameter gradients when any is wanted (and dX when it is), then the merge. */
size_t pdsc_linear_train_workspace_bytes(int M, int Cin, int Cout);
int pdsc_linear_train_forward(const float* X, const float* W, const float* b, const float* R, float* Y, int M, int Cin, int Cout,
                              void* stream);
int pdsc_linear_train_backward(const float* X, const float* W, const float* dY, float* dX, float* dW, float* db, void* ws,
                               size_t ws_bytes, int M, int Cin, int Cout, void* stream);
size_t pdsc_qkv_train_workspace_bytes(int M);
int pdsc_qkv_train_forward(const float* X, const float* Wq, const float* bq, const float* Wk, const float* bk, const float* Wv,
                           const float* bv, float q_scale, float* qkv, int M, void* stream);
int pdsc_qkv_train_backward(const float* X, const float* Wq, const float* Wk, const float* Wv, float q_scale, const float* dqkv,
                            float* dX, float* dWq, float* dbq, float* dWk, float* dbk, float* dWv, float* dbv, void* ws,
                            size_t ws_bytes, int M, void* stream);
size_t pdsc_head_train_workspace_bytes(int M);
int pdsc_head_train_forward(const float* X, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                            const float* b2, float* logits, float* pre, int M, void* stream);
int pdsc_head_train_backward(const float* X, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                             const float* dlogits, float* dX, float* dW0, float* db0, float* dW1, float* db1, float* dW2, float* db2,
                             void* ws, size_t ws_bytes, int M, void* stream);

/* ---- the trainer's update on the device: finite-gradient guard, Adam or SGD, skip decision (DESIGN.md section 8 f-25;
 *      reference train_3DMatch.py:48-66 and the guard of libs/trainer.py:123-130) -------------------------------------------------
 * THE RULE.  All tensor arithmetic is fp32 round-to-nearest with NO fused multiply-add: every product and every sum below is its
 * own rounding (the library is built with -ffp-contract=off); `/` and sqrt are the correctly rounded ones.  A numpy float32
 * program that says the same reproduces the kernels bit for bit (tests/optimizer_oracle.py).
 *   Adam (torch.optim.Adam with L2 weight_decay added to the gradient -- not AdamW --, no amsgrad, no maximize), for a tensor
 *   that has taken t - 1 successful steps:
 *     b1pow = b1pow beta1;  b2pow = b2pow beta2                          (fp64 running products, 1.0 when fresh)
 *     step32 = fp32(lr / (1 - b1pow));  sq32 = fp32(sqrt(1 - b2pow))     (fp64, then one rounding)
 *     B1 = fp32(beta1), OB1 = fp32(1 - beta1), B2 = fp32(beta2), OB2 = fp32(1 - beta2), E = fp32(eps), WD = fp32(weight_decay)
 *     g1 = g + WD p   (g1 = g when weight_decay == 0)
 *     m' = B1 m + OB1 g1;   v' = B2 v + (OB2 g1) g1;   d = sqrt(v') / sq32 + E;   p' = p - step32 (m' / d)
 *   SGD (torch.optim.SGD, dampening 0, no nesterov):
 *     g1 as above;  buf' = g1 on the tensor's first successful step, else fp32(momentum) buf + g1;  p' = p - fp32(lr) buf'
 *     momentum == 0: no buffer is touched, p' = p - fp32(lr) g1.
 *   Guard: when any element of any PRESENT gradient of any group of the step is NaN or +-Inf, the whole step changes nothing
 *   (parameters, moments, step counts and running products keep their bits) and the skipped counter goes up by one.  Parameters
 *   are not looked at.  A tensor whose grad is NULL is left out of the step: its values, step count and products stand still --
 *   step counts are per tensor.
 * ONE STEP is, in stream order: pdsc_optim_check of every group, pdsc_optim_update of every group, pdsc_optim_finish of every
 * group with `last` = 1 on the last one only.  check sets guard[0] when it sees a non-finite element (identical plain stores);
 * update returns at once when guard[0] is set and reads the per-tensor step state WITHOUT writing it (a tensor spans several
 * workgroups: all of them compute the new products from the old state); finish commits the step state of the present tensors
 * (unless guard[0] is set) and, with `last`, adds guard[0] to guard[1] (skipped steps), adds 1 to guard[2] (calls) and clears
 * guard[0].  Nothing clears the flag while a launch of the same step may still read or set it.  With use_guard == 0 no check is
 * needed and the flag is ignored.
 * `tensors` is a HOST table; every launch copies up to pdsc_optim_tensors_per_launch() of its rows into its kernel arguments
 * (synchronously: the caller may reuse the table at once), so a step is 3 ceil(count / that) launches whatever the tensors' sizes,
 * and parameters and gradients may live anywhere.  param and grad need 4-byte alignment only (16-byte accesses are used where
 * both allow them, the same bits either way).
 * `state` (device, 16-byte aligned, pdsc_optim_state_bytes(kind, numel[], count) bytes, opaque, zero-filled = fresh) holds the
 * step state {b1pow, b2pow (fp64), step (int64), unused} of every tensor, 32 bytes each, then per tensor m | v (Adam) or buf
 * (SGD), each padded to a multiple of 4 floats.  `guard` is 4 device uint32 {flag, skipped, calls, unused}, zero-filled by the
 * caller once.
 * All three are enqueue-only: no host synchronisation, no allocation, no memset; repeat calls are bit-identical.  PDSC_ERR_ARG
 * before any HIP call, with the text in pdsc_last_error(): null call / table / state / guard / param, a pointer that is not
 * 4-byte aligned (state: 16), count < 1, numel < 1 or >= 2^31, state_bytes too small, unknown kind, lr / beta1 / beta2 / eps /
 * weight_decay / momentum non-finite or outside what torch accepts (lr, eps, weight_decay, momentum >= 0; 0 <= beta < 1).
 * pdsc_optim_state_bytes returns 0 for bad arguments. */
enum pdsc_optim_kind { PDSC_OPTIM_ADAM = 0, PDSC_OPTIM_SGD = 1 };

typedef struct pdsc_optim_tensor {
    float* param;            /* device, numel floats */
    const float* grad;       /* device, numel floats; NULL: absent at this step */
    long long numel;
} pdsc_optim_tensor;

typedef struct pdsc_optim_call {
    int kind;                            /* enum pdsc_optim_kind */
    int count;                           /* rows of `tensors`: all tensors of one parameter group, in a fixed order */
    const pdsc_optim_tensor* tensors;    /* HOST */
    void* state;
    size_t state_bytes;
    unsigned int* guard;
    int use_guard;                       /* 0 / 1 */
    int reserved;                        /* 0 */
    double lr, beta1, beta2, eps, weight_decay, momentum;      /* Adam reads lr, betas, eps, weight_decay; SGD lr, momentum, weight_decay */
} pdsc_optim_call;

size_t pdsc_optim_state_bytes(int kind, const long long* numel, int count);
int pdsc_optim_tensors_per_launch(void);
int pdsc_optim_check(const pdsc_optim_call* call, void* stream);
int pdsc_optim_update(const pdsc_optim_call* call, void* stream);
int pdsc_optim_finish(const pdsc_optim_call* call, int last, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POINTDSC_HIP_H */
