// Arguments shared by the kernels of the fused point-wise layer: layer.hip (one 4-wave workgroup per 32-point tile, activations
// in LDS, fp32), layer_wave.hip (one wavefront per tile, activations in registers: the generic form), layer_h3.hip (the pipelined
// H3 kernel of the forward), layer_coop.hip (four wavefronts per tile, launches of few tiles) and layer_split.hip (the all-split
// kernel of experiments builds).
#pragma once
#include "pdsc_common.h"
#include "merge_partials.h"

namespace pdsc {

struct LayerArgs {
    const float* msg;        // [M][128]  attention output            (tail), or NULL when the partials below are given
    const float* part_o;     // [bs][nsplit][Npad][128] un-normalised partial outputs of the attention key splits
    const float* part_ml;    // [bs][nsplit][Npad][2]   (reference exponent (log2), partial sum)
    int nsplit, Npad;        // nsplit = partials the kernel merges per row
    int part_slots;          // partials per pair in the LAYOUT of part_o / part_ml (>= nsplit).  Larger than nsplit where the attention
                             // workgroups merged their leaves themselves (attention_split.hip): ONE partial to merge, left in
                             // the pair's leaf-0 slot of the [bs][nleaf][Npad] scratch (layer_h3.hip / layer_coop.hip only)
    const float* res;        // [M][128]  featB of this layer         (tail residual)
    const float* feat_in;    // [M][128]  used when there is no tail  (first head)
    float* feat_out;         // [M][128]  tail result, written when non-null
    float* featB_out;        // [M][128]  head
    float* qkv_out;          // [M][384]  head
    const float *w1, *b1, *w2, *b2, *w3, *b3;      // fc1 [64][128], fc2 [64][64], fc3 [128][64]
    const float *wp, *bp, *wq, *bq;                // pcn [128][128], qkv [384][128]
    const sp16* wq_split;  // optional: qkv weights as fp16 hi [384][128] | lo [384][128] -> the q|k|v projection runs in
                             // split precision (three fp16 MFMAs per operand pair); its error is of the order the attention's
                             // operand split already has, and q, k, v never touch the residual stream
    sp16* qs;              // head, optional: Q split stream   [bs*N][256]          (split_layout.h)
    unsigned char* kv;       // head, optional: K/V tile stream  [bs][tiles][32 KiB]  (split_layout.h)
    int N, bs;               // rows are bs pairs of N points; a workgroup's 32-point tile never straddles two pairs
    // optional (layer_wave.hip): the weights in MFMA-fragment order, one 8 KiB chunk per WChunk in the order the kernel
    // consumes them (pdsc_wfrag_build_tail / _head); when given they replace w1..w3 / wp, wq, wq_split
    const unsigned char* wf_tail;
    const unsigned char* wf_head;
    int gemm_format;         // format the fragment streams were built in: PDSC_LAYER_GEMM_F32 (fc1..fc3, pcn as fp32 rows) or
                             // PDSC_LAYER_GEMM_H3 (fp16 hi / scaled-lo pairs: those GEMMs run on v_mfma_f32_32x32x16_f16)
    int io_flags;            // enum pdsc_layer_io: which of part_o / res / featB_out are in point-fragment order (layer_h3.hip only)
    int stagger_cycles, stagger_mode;   // layer_h3.hip: start delay of half the first round's wavefronts (A/B knobs PDSC_LAYER_STAGGER, _MODE)
    long long* trace;        // diagnostics (pdsc_layer_trace): [workgroup][wave][16] shader-clock stamps, else NULL
    unsigned int* range_flag; // fp16 range sentinel (pdsc_common.h): [bs] words, or NULL outside a forward
    int value_fold;          // 1: the folded layer (pdsc_config.value_fold; layer_h3.hip / layer_coop.hip, point-fragment forms only):
                             // wf_tail / wf_head are the PDSC_WS_FOLD_*_H3 streams, msg / part_o hold 64 channels, V^T planes are 64 wide
    const int* nvalid;       // ragged batches (ragged.h): [bs] correspondences per pair (<= N): tiles past a pair's own rows are
                             // skipped, its last tile is padded / zeroed from ITS count; NULL = every pair has N rows
};

// Which fused-layer kernel a launch takes: the workgroup-per-tile kernel of layer.hip (natural-layout weights), the
// wavefront-per-tile kernel of layer_wave.hip (natural weights or fragment streams), the pipelined H3 kernel of layer_h3.hip
// (H3 fragment streams; launch_layer_h3 hands launches of few tiles to layer_coop.hip itself) or the all-split kernel of
// layer_split.hip (experiments builds; w1, w2, w3, wp, wq then point at the hi|lo matrices of the split-weight buffer).
enum class LayerKernel { Block, Wave, H3, X3 };
// key-split partials the kernel merges while it loads (merge_partials.h); larger splits go through attention_combine_kernel
constexpr int layer_merge_limit(LayerKernel k) {
    return k == LayerKernel::Block ? MERGE_MAX_SPLIT_BLOCK : k == LayerKernel::H3 ? MERGE_MAX_SPLIT_H3 : MERGE_MAX_SPLIT;
}

// The one mapping from the public call (include/pointdsc_hip.h) to the kernels' argument.  What the struct does not expose stays
// zero: nvalid, range_flag and value_fold are the forward's own, trace is set by whoever launches (launch_layer_h3 leaves the
// few-tile kernel of layer_coop.hip when it is set, and the product build's launch_layer_wave rejects a launch with it).
// Every kernel a forward can launch reports to the fp16 range sentinel when range_flag is given: layer_h3.hip, layer_coop.hip,
// the fp32-GEMM forms of layer_wave.hip and layer.hip.  Three paths carry NO sentinel, and no product forward runs them: the generic
// H3 form of layer_wave_kernel (stage tests; experiments knob PDSC_LAYER_H3_VARIANT = 0), layer_split.hip (experiments builds), and
// the one-launch-per-conv encoder under the split attention (experiments knob PDSC_FUSED_LAYERS = 0; api.hip:run_encoder_per_conv),
// whose pdsc_pack_qkv_split converts q, k, v without a note: range_flag is zeroed and never set there.
inline LayerArgs layer_args_from_call(const pdsc_layer_call& c) {
    LayerArgs a{};
    a.msg = c.msg; a.part_o = c.part_o; a.part_ml = c.part_ml; a.nsplit = c.nsplit; a.part_slots = c.nsplit; a.Npad = c.Npad;
    a.res = c.res; a.feat_in = c.feat_in; a.feat_out = c.feat_out; a.featB_out = c.featB_out; a.qkv_out = c.qkv_out;
    a.qs = (sp16*)c.q_split; a.kv = (unsigned char*)c.kv_tiles;
    a.w1 = (const float*)c.w1; a.b1 = c.b1; a.w2 = (const float*)c.w2; a.b2 = c.b2; a.w3 = (const float*)c.w3; a.b3 = c.b3;
    a.wp = (const float*)c.wp; a.bp = c.bp; a.wq = (const float*)c.wq; a.bq = c.bq; a.wq_split = (const sp16*)c.wq_split;
    a.wf_tail = (const unsigned char*)c.wfrag_tail; a.wf_head = (const unsigned char*)c.wfrag_head;
    a.gemm_format = c.gemm_format; a.io_flags = c.io_flags;
    a.N = c.N; a.bs = c.bs;
    return a;
}

// layer.hip: every argument check of the fused-layer entry points (`who` names the caller in the error text), and the launch.
// tail = msg or partials given, head = featB_out given.
int validate_layer_args(const LayerArgs& a, LayerKernel kernel, const char* who);
int dispatch_layer(const LayerArgs& a, LayerKernel kernel, hipStream_t st);

int launch_layer_wave(const LayerArgs& a, bool tail, bool head, hipStream_t st);      // layer_wave.hip
int launch_layer_h3(const LayerArgs& a, bool tail, bool head, hipStream_t st);        // layer_h3.hip (H3 fragment streams only)
int launch_layer_h3_coop(const LayerArgs& a, bool tail, bool head, hipStream_t st);   // layer_coop.hip (same contract, few tiles)
int launch_layer_x3(const LayerArgs& a, bool tail, bool head, hipStream_t st);        // layer_split.hip (experiments builds, else an error)
bool launch_layer_h3_fits(const LayerArgs& a, bool tail, bool head);                  // ... and only this output set
// The forms layer_h3_kernel and layer_h3_coop_kernel are instantiated in: which halves run, featB in point-fragment order (PF), the
// folded layer.  layer_h3_form (layer_h3.hip) decides; Unserved = the folded layer without point-fragment featB (error text set).
enum class H3Form { TailHeadPF, HeadPF, TailHead, Tail, Head, FoldTailHeadPF, FoldHeadPF, FoldTail, Unserved };
H3Form layer_h3_form(const LayerArgs& a, bool tail, bool head);
// the folded layer's weights of one layer (layer_wave.hip): wfold = W1f Wv [64][128] | b' [64] fp32, and its H3 tail / head streams
int build_value_fold(const float* w1, const float* b1, const float* wqkv, const float* bqkv, const float* w2, const float* b2,
                     const float* w3, const float* b3, const float* wp, const float* bp, float* wfold, void* tail_out, void* head_out,
                     hipStream_t st);

}  // namespace pdsc

long long* pdsc_layer_trace_buffer(void);      // layer.hip: the buffer of pdsc_layer_trace, or NULL
