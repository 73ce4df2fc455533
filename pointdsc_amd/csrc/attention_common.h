// Shared between the two attention kernels (attention.hip: exact fp32 MFMA; attention_split.hip: fp16x3 split).
#pragma once
#include "pdsc_common.h"

namespace pdsc {

struct AttArgs {
    const float* qkv;        // [bs*N][384]
    const float* compat;     // [bs][N][ld]
    long long ld;
    float* msg;              // [bs*N][128]
    float* part_o;           // [bs][nsplit][Npad][128]   un-normalised partial outputs
    float* part_ml;          // [bs][nsplit][Npad][2]     (running max (log2 domain), partial sum)
    int N, Npad, nsplit, num_tiles;
    const int* nvalid;       // ragged batches (r06): [bs] correspondences per pair (<= N; strides stay those of N), or NULL
    float* lse;              // f-12: [bs*N] row statistic m + log2(l) of the softmax (log2 domain) for the backward, or NULL
};

// arguments of the split-precision kernels (attention_split.hip)
struct AttSplitArgs {
    const sp16* qs;             // [bs*N][256]  (hi | lo), q pre-scaled by log2(e)/sqrt(C)
    const unsigned char* kv;     // [bs][num_tiles][32 KiB]
    const void* compat;          // [bs][N][ld] fp32, or (C16) unorm16 in the tile order of pdsc_spatial_compat_u16
    long long ld;
    float* msg;                  // [bs*N][128]
    float* part_o;               // [bs][nsplit][Npad][128]
    float* part_ml;              // [bs][nsplit][Npad][2]
    int N, Npad, nsplit, num_tiles, nq, bs;
    int prio_mode;               // A/B knob PDSC_ATT_PRIO: 1 = s_setprio 1 for the younger half of the waves, 2 = for the older half
    int compute_all_waves;       // A/B knob PDSC_ATT_ALL_WAVES (experiments builds): 1 = waves without a valid query compute anyway (r01-r03)
    int compat_nt;               // A/B knob PDSC_ATT_COMPAT_NT: stream the compat slices with the non-temporal policy
    int items;                   // persistent form: number of (pair, key split, query block) items (= the one-item form's grid)
    int part_frag;               // key-split partials in point-fragment order (split_layout.h: PF), straight from the accumulators
    const int* nvalid;           // ragged batches: [bs] correspondences per pair (<= N), or NULL: every pair has N
    long long* trace;            // diagnostics (pdsc_attention_trace): [workgroup][wave][8] cycle sums, else NULL
    // leaf form (sc_attention_split_kernel<..., MG = true>): part_o / part_ml are [bs][nleaf][Npad][..] (point-fragment order)
    int nleaf;                   // leaves per pair (a multiple of nsplit; <= the tile count of the shortest pair)
};


// Running row maximum over four more logits: mx = max(mx, a, b, c, d) as a chain of two three-operand maxima (v_max3_f32 each)
// instead of the tree fmaxf(fmaxf(mx, fmaxf(a, b)), fmaxf(c, d)), which the backend keeps as written -- with one quieting
// v_max_f32 x, x per leaf on top: 28 instructions for the 16 logits of a tile against 8.  max is exact and does not depend on the
// order of its operands, and both forms drop a quiet NaN operand (the logits come out of v_fma_f32 / v_mul_f32, which return no
// signalling one): the same value bit for bit.  Every path of the split kernel that needs
// a row maximum (the three compat modes of phase B, the first tile, a leaf boundary, the ragged last tile) goes through this one.
__device__ __forceinline__ float row_max4(float mx, float a, float b, float c, float d) {
    mx = __builtin_fmaxf(__builtin_fmaxf(mx, a), b);
    return __builtin_fmaxf(__builtin_fmaxf(mx, c), d);
}

typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// merge of the per-split partials (defined in attention.hip)
int launch_attention_combine(const AttArgs& a, int bs, hipStream_t st);
// exact-fp32 attention with an optional per-pair count array (ragged batches; pdsc_sc_attention = the same with NULL)
int launch_attention_fp32(const float* qkv, const float* compat, long long ld, float* msg, void* scratch, size_t scratch_bytes, int bs, int N,
                          int nsplit, const int* nvalid, hipStream_t st, float* lse = nullptr);

// ---- split-precision attention (attention_split.hip); nvalid: ragged batches (ragged.h), NULL = every pair has N -------------
// msg != NULL: merged output rows (key split 1, or the combine launch); msg == NULL: the key-split partials stay in `scratch`
int launch_attention_split_ex(const void* q_split, const void* kv_tiles, const void* compat, int compat_format, long long ld,
                              float* msg, void* scratch, size_t scratch_bytes, int bs, int N, int nsplit, int partial_layout,
                              const int* nvalid, hipStream_t st, int value_width = PDSC_CHANNELS);
// value_width (both launchers): channels of V in the tile images and of the partials -- PDSC_CHANNELS, or 64 for the folded value
// projection (pdsc_config.value_fold; point-fragment partials only)

// leaf form (sc_attention_split_kernel<..., MG = true>): C leaf partials per query, left in `scratch` in point-fragment order for
// the H3 layer kernel to merge
constexpr int PDSC_ATT_MAX_LEAVES = 8;       // = MERGE_MAX_SPLIT_H3 (merge_partials.h): what the layer kernel merges while it loads
int attention_leaf_count(int N);
int leaf_plan(int bs, int N, int leaves_mode, int* nw_out, int* nsplit_out, int* nleaf_out);
int launch_attention_leaves(const void* q_split, const void* kv_tiles, const void* compat, int compat_format, long long ld,
                            void* scratch, size_t scratch_bytes, int bs, int N, int leaves_mode, const int* nvalid, int n_min,
                            hipStream_t st, int value_width = PDSC_CHANNELS);

}  // namespace pdsc
