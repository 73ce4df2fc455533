// Host side of libpointdsc_hip.so: error plumbing, packed-weight layout, workspace layout (entries by WsId) and the whole-path
// orchestrator pdsc_forward: one pdsc_forward_call with an explicit mode, checked whole before the first launch, then one
// function per stage (reference PointDSC.forward, models/PointDSC.py:128-197).  Pure HIP runtime --
// no torch types cross this boundary.  Every stage is enqueued on the caller's stream with no host synchronisation, so one
// forward is hipGraph-capturable.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include "pdsc_common.h"
#include "ragged.h"
#include "attention_common.h"
#include "layer_args.h"

namespace pdsc {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return PDSC_ERR_LAUNCH;
    }
    return PDSC_OK;
}

// ---- dynamic-LDS opt-in, once per (kernel, device) ----------------------------------------------
int ensure_dynamic_lds(const void* fn, size_t bytes, const char* what) {
    // granted size per (kernel, device): a larger request on one device must not mark the others as served
    struct Entry { const void* fn; size_t granted[64]; };
    static Entry table[64];
    static int used = 0;
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return check_launch(what);
    std::lock_guard<std::mutex> lock(mu);
    Entry* e = nullptr;
    for (int i = 0; i < used; ++i)
        if (table[i].fn == fn) { e = &table[i]; break; }
    if (e && dev < 64 && e->granted[dev] >= bytes) return PDSC_OK;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return check_launch(what);
    if (!e && used < 64) { e = &table[used++]; e->fn = fn; memset(e->granted, 0, sizeof(e->granted)); }
    if (e && dev < 64) e->granted[dev] = bytes;
    return PDSC_OK;
}

__global__ void fill_u32_kernel(unsigned int* p, unsigned int value, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) p[i] = value;
}
__global__ void copy_u32_kernel(unsigned int* __restrict__ dst, const unsigned int* __restrict__ src, size_t count) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
// slot := max(slot, max_i |x[i]|) on the bit patterns (non-negative floats order like unsigned integers; NaN patterns sort above inf,
// so a NaN anywhere shows as "out of range")
__global__ void absmax_kernel(const float* __restrict__ x, size_t count, unsigned int* __restrict__ slot) {
    unsigned int m = 0u;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned int u = __float_as_uint(x[i]) & 0x7fffffffu;
        m = u > m ? u : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned int o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(slot, m);
}
static int launch_absmax(const float* x, size_t count, unsigned int* slot, hipStream_t st) {
    const size_t blocks = (count + 1023) / 1024;
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, x, count, slot);
    return check_launch("absmax");
}
int launch_copy_u32(unsigned int* dst, const unsigned int* src, size_t count, hipStream_t st) {
    if (count == 0) return PDSC_OK;
    const size_t blocks = (count + 255) / 256;
    hipLaunchKernelGGL(copy_u32_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, dst, src, count);
    return check_launch("copy");
}
int launch_fill_u32(unsigned int* p, unsigned int value, size_t count, hipStream_t st) {
    if (count == 0) return PDSC_OK;
    hipLaunchKernelGGL(fill_u32_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, p, value, count);
    return check_launch("fill");
}

// ---- opt-in event timing -----------------------------------------------------------------------
// stride: only every stride-th launch of the kind is bracketed by events (an event record costs the stream ~3.5 us and breaks
// the back-to-back issue of the kernels around it: 50 records per forward were 8 % of a 2 ms step)
struct ProfKind { hipEvent_t* start = nullptr; hipEvent_t* stop = nullptr; int cap = 0, n = 0, stride = 1; long long calls = 0; bool open = false; };
static ProfKind g_prof[PDSC_PROF_NUM_KINDS];

void profile_mark_begin(int kind, hipStream_t st) {
    ProfKind& p = g_prof[kind];
    if (p.cap == 0 || p.n >= p.cap) return;
    if ((p.calls++ % p.stride) != 0) return;
    (void)hipEventRecord(p.start[p.n], st);
    p.open = true;
}
void profile_mark_end(int kind, hipStream_t st) {
    ProfKind& p = g_prof[kind];
    if (!p.open) return;
    (void)hipEventRecord(p.stop[p.n], st);
    p.open = false;
    ++p.n;
}

static bool config_ok(const pdsc_config* c) {
    if (!c) { set_error("pdsc_config is null"); return false; }
    if (c->num_channels != PDSC_CHANNELS) { set_error("num_channels=%d (only %d supported)", c->num_channels, PDSC_CHANNELS); return false; }
    if (c->in_dim < 1 || c->in_dim > 16) { set_error("in_dim=%d must be in [1,16]", c->in_dim); return false; }
    if (c->num_layers < 0 || c->num_layers > 64) { set_error("num_layers=%d", c->num_layers); return false; }
    if (c->num_iterations < 0 || c->num_iterations > PDSC_MAX_POWER_ITERS) { set_error("num_iterations=%d", c->num_iterations); return false; }
    if (c->k < 1 || c->k > PDSC_MAX_K) { set_error("k=%d must be in [1,%d]", c->k, PDSC_MAX_K); return false; }
    if (c->refine_iters < 0) { set_error("refine_iters=%d", c->refine_iters); return false; }
    if (c->attention_precision < PDSC_ATT_FP16X3 || c->attention_precision > PDSC_ATT_FP16X3_ALL) {
        set_error("attention_precision=%d", c->attention_precision); return false;
    }
#ifndef PDSC_EXPERIMENTS
    if (c->attention_precision == PDSC_ATT_FP16X3_ALL) {
        set_error("attention_precision=PDSC_ATT_FP16X3_ALL (all-split layer GEMMs) exists in experiments builds only");
        return false;
    }
#endif
    if (c->compat_format != PDSC_COMPAT_U16 && c->compat_format != PDSC_COMPAT_F32) { set_error("compat_format=%d", c->compat_format); return false; }
    if (c->layer_gemm != PDSC_LAYER_GEMM_F32 && c->layer_gemm != PDSC_LAYER_GEMM_H3) { set_error("layer_gemm=%d", c->layer_gemm); return false; }
    if (c->att_leaves < PDSC_LEAVES_PER_LAUNCH || c->att_leaves > PDSC_ATT_MAX_LEAVES) { set_error("att_leaves=%d (enum pdsc_att_leaves, or 2..%d leaves)", c->att_leaves, PDSC_ATT_MAX_LEAVES); return false; }
    if (c->value_fold != PDSC_VALUE_FOLD_OFF && c->value_fold != PDSC_VALUE_FOLD_ON) { set_error("value_fold=%d (enum pdsc_value_fold)", c->value_fold); return false; }
    if (c->value_fold == PDSC_VALUE_FOLD_ON && (c->attention_precision != PDSC_ATT_FP16X3 || c->layer_gemm != PDSC_LAYER_GEMM_H3)) {
        set_error("value_fold=1 needs attention_precision=PDSC_ATT_FP16X3 and layer_gemm=PDSC_LAYER_GEMM_H3 (got %d, %d)",
                  c->attention_precision, c->layer_gemm);
        return false;
    }
    return true;
}

static long long section_floats(int section) {
    const long long C = PDSC_CHANNELS, H = C / 2;
    switch (section) {
        case PDSC_W_LAYER0_W: return C * 16;
        case PDSC_W_LAYER0_B: return C;
        case PDSC_W_PCN_W: return C * C;
        case PDSC_W_PCN_B: return C;
        case PDSC_W_QKV_W: return 3 * C * C;
        case PDSC_W_QKV_B: return 3 * C;
        case PDSC_W_FC1_W: return H * C;
        case PDSC_W_FC1_B: return H;
        case PDSC_W_FC2_W: return H * H;
        case PDSC_W_FC2_B: return H;
        case PDSC_W_FC3_W: return C * H;
        case PDSC_W_FC3_B: return C;
        case PDSC_W_CLS1_W: return 32 * C;
        case PDSC_W_CLS1_B: return 32;
        case PDSC_W_CLS2_W: return 32 * 32;
        case PDSC_W_CLS2_B: return 32;
        case PDSC_W_CLS3_W: return 32;
        case PDSC_W_CLS3_B: return 4;   // 1 used, padded to keep every section 16-byte aligned
        case PDSC_W_SIGMA: return 4;
        case PDSC_W_SIGMA_SPAT: return 4;
    }
    return -1;
}
static bool per_layer(int section) { return section >= PDSC_W_PCN_W && section <= PDSC_W_FC3_B; }

static long long layer_block_floats() {
    long long n = 0;
    for (int s = PDSC_W_PCN_W; s <= PDSC_W_FC3_B; ++s) n += section_floats(s);
    return n;
}

static long long wpack_offset(const pdsc_config* c, int section, int layer) {
    if (section < 0 || section >= PDSC_W_NUM_SECTIONS) return -1;
    long long off = 0;
    if (section <= PDSC_W_LAYER0_B) {
        for (int s = 0; s < section; ++s) off += section_floats(s);
        return off;
    }
    off = section_floats(PDSC_W_LAYER0_W) + section_floats(PDSC_W_LAYER0_B);
    if (per_layer(section)) {
        if (layer < 0 || layer >= c->num_layers) return -1;
        off += (long long)layer * layer_block_floats();
        for (int s = PDSC_W_PCN_W; s < section; ++s) off += section_floats(s);
        return off;
    }
    off += (long long)c->num_layers * layer_block_floats();
    for (int s = PDSC_W_CLS1_W; s < section; ++s) off += section_floats(s);
    return off;
}

// ---- workspace layout --------------------------------------------------------------------------
// One id per entry, in layout order; ws_names[id] is the name pdsc_workspace_offset serves.
enum WsId {
    WS_COMPAT, WS_FEATA, WS_FEATB, WS_FEATC, WS_QKV, WS_MSG, WS_T64A, WS_T64B, WS_ATT_SCRATCH, WS_Q_SPLIT, WS_KV_TILES, WS_NORMED,
    WS_NORMED_PF, WS_H1, WS_H2, WS_CONF, WS_KEYS, WS_NMS_WS, WS_SEEDS, WS_KNN_DIST, WS_KNN_IDX, WS_EIG_ITERS, WS_CONV_MASK,
    WS_SEED_TRANS, WS_SEED_W, WS_COUNTS, WS_BEST, WS_INITIAL_TRANS, WS_SOLVES, WS_RANGE_FLAG, WS_REFINE_TRACE,
#ifdef PDSC_EXPERIMENTS
    WS_SCORE_DBG,
#endif
    WS_NUM
};
static const char* const ws_names[] = {
    "compat", "featA", "featB", "featC", "qkv", "msg", "t64a", "t64b", "att_scratch", "q_split", "kv_tiles", "normed",
    "normed_pf", "h1", "h2", "conf", "keys", "nms_ws", "seeds", "knn_dist", "knn_idx", "eig_iters", "conv_mask",
    "seed_trans", "seed_w", "counts", "best", "initial_trans", "solves", "range_flag", "refine_trace",
#ifdef PDSC_EXPERIMENTS
    "score_dbg",
#endif
};
static_assert(sizeof(ws_names) / sizeof(ws_names[0]) == WS_NUM, "ws_names must name every WsId, in order");

struct WsLayout {
    size_t offset[WS_NUM], bytes[WS_NUM], total;
    template <class T> T* at(void* ws, WsId id) const { return (T*)((char*)ws + offset[id]); }
};

static WsLayout make_layout(const pdsc_config* c, int bs, int N, int S) {
    WsLayout L{};
    size_t* B = L.bytes;
    const size_t M = (size_t)bs * N, C = PDSC_CHANNELS, f = sizeof(float);
    const size_t ld = (size_t)pdsc_compat_ld(N);
    const int k = c->k < N - 1 ? c->k : N - 1;
    const int iters = c->num_iterations > 0 ? c->num_iterations : 1;
    const bool compat16 = c->attention_precision != PDSC_ATT_FP32 && c->compat_format == PDSC_COMPAT_U16;
    B[WS_COMPAT] = (size_t)bs * N * ld * (compat16 ? sizeof(unsigned short) : f);
    B[WS_FEATA] = M * C * f;
    const size_t Mpf = (size_t)bs * round_up(N, 32);          // featB / featC may be kept in point-fragment order: whole 32-row tiles per pair
    B[WS_FEATB] = B[WS_FEATC] = Mpf * C * f;
    B[WS_QKV] = M * 3 * C * f;
    B[WS_MSG] = M * C * f;
    B[WS_T64A] = B[WS_T64B] = M * (C / 2) * f;
    {
        const size_t a32 = pdsc_attention_scratch_bytes(bs, N, 0), a16 = pdsc_attention_split_scratch_bytes(bs, N, 0);
        const size_t amg = c->att_leaves >= PDSC_LEAVES_CANONICAL ? pdsc_attention_leaf_scratch_bytes(bs, N, c->att_leaves) : 0;
        B[WS_ATT_SCRATCH] = c->attention_precision == PDSC_ATT_FP32 ? a32 : (a16 > amg ? a16 : amg);
    }
    B[WS_Q_SPLIT] = c->attention_precision != PDSC_ATT_FP32 ? pdsc_split_q_bytes(bs, N) : 0;
    B[WS_KV_TILES] = c->attention_precision != PDSC_ATT_FP32 ? pdsc_split_kv_bytes(bs, N) : 0;
    B[WS_NORMED] = M * C * f;
    B[WS_NORMED_PF] = knn_seeds_uses_fused(bs, N, S, k) ? Mpf * C * f : 0;      // the fused kNN's B operand (point-fragment order)
    B[WS_H1] = B[WS_H2] = M * 32 * f;
    B[WS_CONF] = B[WS_KEYS] = M * f;
    B[WS_NMS_WS] = pdsc_nms_workspace_bytes(bs, N);
    B[WS_SEEDS] = (size_t)bs * S * sizeof(int);
    B[WS_KNN_DIST] = (size_t)bs * S * ld * f;
    B[WS_KNN_IDX] = (size_t)bs * S * (k > 0 ? k : 1) * sizeof(int);
    B[WS_EIG_ITERS] = (size_t)bs * S * iters * PDSC_MAX_K * f;
    B[WS_CONV_MASK] = (size_t)bs * sizeof(unsigned int);
    B[WS_SEED_TRANS] = (size_t)bs * S * 16 * f;
    B[WS_SEED_W] = (size_t)bs * S * (k > 0 ? k : 1) * f;
    B[WS_COUNTS] = (size_t)bs * S * sizeof(int);
    B[WS_BEST] = (size_t)bs * sizeof(int);
    B[WS_INITIAL_TRANS] = (size_t)bs * 16 * f;
    B[WS_SOLVES] = (size_t)bs * sizeof(int);
    B[WS_RANGE_FLAG] = (size_t)bs * sizeof(unsigned int);      // fp16 range sentinel (pdsc_common.h): != 0 = pair b left the fp16 range
    B[WS_REFINE_TRACE] = (size_t)bs * PDSC_REFINE_TRACE * sizeof(int);      // inlier count per refinement iteration, -1 padded (parity census)
#ifdef PDSC_EXPERIMENTS
    B[WS_SCORE_DBG] = (size_t)bs * S * 16 * f;        // diagnostics of the scoring kernel (score.hip, DBG)
#endif
    for (int i = 0; i < WS_NUM; ++i) {        // entries follow one another in id order, each rounded up to 256 bytes
        L.offset[i] = L.total;
        L.total += (size_t)round_up((long long)B[i], 256);
    }
    return L;
}

}  // namespace pdsc

using namespace pdsc;

extern "C" int pdsc_version(void) { return PDSC_VERSION; }

extern "C" int pdsc_experiments_enabled(void) {
#ifdef PDSC_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}
extern "C" const char* pdsc_last_error(void) { return g_err; }

extern "C" long long pdsc_wpack_floats(const pdsc_config* cfg) {
    if (!config_ok(cfg)) return -1;
    return wpack_offset(cfg, PDSC_W_SIGMA_SPAT, 0) + section_floats(PDSC_W_SIGMA_SPAT);
}
extern "C" long long pdsc_wpack_offset(const pdsc_config* cfg, int section, int layer) {
    if (!config_ok(cfg)) return -1;
    return wpack_offset(cfg, section, layer);
}

extern "C" size_t pdsc_workspace_bytes(const pdsc_config* cfg, int bs, int N, int num_seeds) {
    if (!config_ok(cfg) || bs <= 0 || N <= 1 || num_seeds <= 0) return 0;
    return make_layout(cfg, bs, N, num_seeds).total;
}
extern "C" long long pdsc_workspace_offset(const pdsc_config* cfg, int bs, int N, int num_seeds, const char* name) {
    if (!config_ok(cfg) || bs <= 0 || N <= 1 || num_seeds <= 0 || !name) return -1;
    const WsLayout L = make_layout(cfg, bs, N, num_seeds);
    for (int i = 0; i < WS_NUM; ++i)
        if (strcmp(ws_names[i], name) == 0) return (long long)L.offset[i];
    return -1;
}

extern "C" int pdsc_profile_enable(int max_records) {
    for (int k = 0; k < PDSC_PROF_NUM_KINDS; ++k) {
        ProfKind& p = g_prof[k];
        for (int i = 0; i < p.cap; ++i) { (void)hipEventDestroy(p.start[i]); (void)hipEventDestroy(p.stop[i]); }
        delete[] p.start; delete[] p.stop;
        const int keep_stride = p.stride;
        p = ProfKind();
        p.stride = keep_stride;
        if (max_records > 0) {
            p.start = new hipEvent_t[max_records];
            p.stop = new hipEvent_t[max_records];
            for (int i = 0; i < max_records; ++i) {
                if (hipEventCreate(&p.start[i]) != hipSuccess || hipEventCreate(&p.stop[i]) != hipSuccess)
                    return check_launch("pdsc_profile_enable");
            }
            p.cap = max_records;
        }
    }
    return PDSC_OK;
}
extern "C" int pdsc_profile_reset(void) {
    for (int k = 0; k < PDSC_PROF_NUM_KINDS; ++k) { g_prof[k].n = 0; g_prof[k].open = false; g_prof[k].calls = 0; }
    return PDSC_OK;
}
extern "C" int pdsc_profile_set_stride(int kind, int stride) {
    PDSC_REQUIRE(kind >= 0 && kind < PDSC_PROF_NUM_KINDS && stride >= 1, "pdsc_profile_set_stride: kind=%d stride=%d", kind, stride);
    g_prof[kind].stride = stride;
    g_prof[kind].calls = 0;
    return PDSC_OK;
}
extern "C" int pdsc_profile_read(int kind, double* total_ms, int* launches) {
    PDSC_REQUIRE(kind >= 0 && kind < PDSC_PROF_NUM_KINDS && total_ms && launches, "pdsc_profile_read: bad argument");
    ProfKind& p = g_prof[kind];
    double tot = 0.0;
    for (int i = 0; i < p.n; ++i) {
        if (hipEventSynchronize(p.stop[i]) != hipSuccess) return check_launch("pdsc_profile_read");
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.start[i], p.stop[i]) != hipSuccess) return check_launch("pdsc_profile_read");
        tot += ms;
    }
    *total_ms = tot;
    *launches = p.n;
    return PDSC_OK;
}

#define PDSC_TRY(call)                 \
    do {                               \
        const int rc__ = (call);       \
        if (rc__ != PDSC_OK) return rc__; \
    } while (0)

// Everything the encoder loop of run_forward needs to know, decided once by plan_encoder (pure host code, no launch in it).
struct EncoderPlan {
    bool fused;              // one launch per (tail of layer i, head of layer i + 1); false: one pdsc_linear launch per conv
    bool split;              // split-precision attention; every field below but `kernel` is set for the fused split path only
    LayerKernel kernel;      // the fused-layer kernel of every launch
    bool x3, frag;           // layer weights: split fp16 (PDSC_ATT_FP16X3_ALL) / fragment streams / else natural layout
    bool fuse_merge;         // the layer kernel merges the key-split partials while loading (no combine launch, no msg round trip)
    bool pf, leaves, fold;   // point-fragment hand-offs; attention in leaf form; the folded layer (64-channel value projection)
    int gemm;                // arithmetic of fc1..fc3 / PointCN (enum pdsc_layer_gemm)
    int ns, Npad;            // key split of the attention launch, padded row count of the partials
    int nleaf, value_width;  // leaves per query (leaf form); channels of V and of the partials
    int leaf_ns;             // leaf form: workgroups per query block (a divisor of nleaf); 1 = each merges its own leaves into one partial
    int ws_tail, ws_head;    // sections of the split-weight buffer that hold the fragment streams
};

static int plan_encoder(const pdsc_config* cfg, int bs, int N, const int* nvalid, int n_min, EncoderPlan* plan) {
    EncoderPlan& p = *plan = EncoderPlan{};
    p.split = cfg->attention_precision != PDSC_ATT_FP32;
    p.x3 = cfg->attention_precision == PDSC_ATT_FP16X3_ALL;
    p.fused = env_int("PDSC_FUSED_LAYERS", 1) != 0 && cfg->num_layers > 0;     // tuning/A-B knob: 0 = one pdsc_linear launch per conv
    const bool canonical = cfg->att_leaves >= PDSC_LEAVES_CANONICAL;
    const int min_tiles = (n_min + 31) / 32;         // 32-key tiles of the shortest pair (ragged batches)
    p.ns = p.split ? pdsc_attention_split_default_split(bs, N) : 0;
#define PDSC_REQUIRE_SHORTEST_PAIR(cond)                                                                                             \
    PDSC_REQUIRE(cond, "pdsc_forward(testing): the shortest pair (%d correspondences) has fewer 32-key tiles than the key split " \
                 "planned for bs=%d, N=%d (%d): batch pairs of more similar size", n_min, bs, N, p.ns)
    // Every pair must keep at least one tile per key split.  Two checks, because they do not reject the same calls.  This one
    // alone catches the un-fused path (PDSC_FUSED_LAYERS = 0, or no layers): whatever the layer kernels, a configuration without
    // canonical leaves runs the key split ...
    if (nvalid && p.split && !canonical) PDSC_REQUIRE_SHORTEST_PAIR(min_tiles >= p.ns);
    // the workgroup-per-tile / wavefront kernel over natural-layout weights, by the size rule (pdsc_layer_prefers_block);
    // (experiments builds) PDSC_LAYER_VARIANT = b / w forces one
    const char* var = env_str("PDSC_LAYER_VARIANT");
    const bool force_block = var && var[0] == 'b', force_wave = var && var[0] == 'w';
    auto by_size = [&](int pairs, int rows) {
        return force_block || (!force_wave && pdsc_layer_prefers_block(pairs, rows)) ? LayerKernel::Block : LayerKernel::Wave;
    };
    if (!p.fused || !p.split) {
        // exact fp32 sees the batch as ONE run of bs * N independent rows (see run_fused_layer)
        p.kernel = by_size(1, bs * N);
        return PDSC_OK;
    }
    // split precision: head of layer 0, then per layer attention (partials left un-merged when the keys are split)
    // + ONE launch for the merge, the tail of layer i and the head of layer i+1
    p.Npad = (int)round_up(N, 256);
    // arithmetic of fc1..fc3 / PointCN (enum pdsc_layer_gemm); A/B knob PDSC_LAYER_GEMM = 0 / 1 overrides
    p.gemm = env_int("PDSC_LAYER_GEMM", cfg->layer_gemm) == PDSC_LAYER_GEMM_H3 ? PDSC_LAYER_GEMM_H3 : PDSC_LAYER_GEMM_F32;
    const bool h3 = p.gemm == PDSC_LAYER_GEMM_H3;
    // Which layer kernel.  H3 GEMMs: layer_h3_kernel, or the bit-identical layer_h3_coop_kernel for launches of at most 2560
    // tiles (launch_layer_h3 decides) -- never the fp32 kernels: N = 1000 x 1 0.384 ms per forward against 0.557 with the
    // workgroup-per-tile fp32 kernel (profiles/r03_b_ab_*.txt, r03_k_ab_coop.txt).  fp32 GEMMs: layer_wave_kernel over the
    // fragment streams, or the workgroup-per-tile kernel of layer.hip over natural-layout weights for small problems.
    // tuning/A-B knobs: PDSC_LAYER_FRAG = 0 = natural-layout weights whatever the size; PDSC_LAYER_H3_VARIANT = 0 = layer_wave_kernel
    // with the H3 GEMMs
    const LayerKernel natural = by_size(bs, N);
    p.frag = env_int("PDSC_LAYER_FRAG", 1) && !p.x3 && !force_block && (natural == LayerKernel::Wave || h3);
    p.kernel = p.x3     ? LayerKernel::X3
               : !p.frag ? natural
                         : h3 && env_int("PDSC_LAYER_H3_VARIANT", 1) != 0 ? LayerKernel::H3 : LayerKernel::Wave;
    // the layer kernels merge the key-split partials while loading (merge_partials.h), up to the limit of the kernel chosen
    p.fuse_merge = env_int("PDSC_FUSE_MERGE", 1) && p.ns > 1 && p.ns <= layer_merge_limit(p.kernel);      // tuning/A-B knob
    // H3 kernel: the hand-offs attention -> layer kernel -> next layer kernel can go in point-fragment order (split_layout.h);
    // A/B knob PDSC_LAYER_PF = 0: plain rows
    const bool pf_ok = p.kernel == LayerKernel::H3 && env_int("PDSC_LAYER_PF", 1) != 0;
    // leaf form (r05, enum pdsc_att_leaves): the key range cut into leaves that depend on N alone; the H3 layer kernel merges the
    // leaf partials exactly as it merges key-split partials (the other layer kernels keep the per-launch key split)
    int lf_ns = 0, lf_nw = 0;
    if (canonical) PDSC_TRY(leaf_plan(bs, N, cfg->att_leaves, &lf_nw, &lf_ns, &p.nleaf));
    p.leaf_ns = lf_ns;
    p.leaves = pf_ok && canonical && (!nvalid || min_tiles >= 2 * p.nleaf);
    // ... and this one alone catches a canonical-leaves configuration whose launch ends up not using the leaves
    if (nvalid && !p.leaves) PDSC_REQUIRE_SHORTEST_PAIR(min_tiles >= p.ns);
#undef PDSC_REQUIRE_SHORTEST_PAIR
    p.pf = p.leaves || (pf_ok && p.fuse_merge);
    // value fold (enum pdsc_value_fold): fc1 inside the value projection -- 64-channel V', partials and P V' on the point-fragment
    // hand-offs (leaves and key splits of 2..8) up to N = PDSC_VALUE_FOLD_MAX_N (a function of N alone, so canonical leaves stay
    // batch invariant); the row-order hand-offs and larger N keep the 128-channel path
    p.fold = cfg->value_fold == PDSC_VALUE_FOLD_ON && p.pf && N <= PDSC_VALUE_FOLD_MAX_N;
    p.value_width = p.fold ? PDSC_CHANNELS / 2 : PDSC_CHANNELS;
    p.ws_tail = p.fold ? PDSC_WS_FOLD_TAIL_H3 : h3 ? PDSC_WS_FRAG_TAIL_H3 : PDSC_WS_FRAG_TAIL;
    p.ws_head = p.fold ? PDSC_WS_FOLD_HEAD_H3 : h3 ? PDSC_WS_FRAG_HEAD_H3 : PDSC_WS_FRAG_HEAD;
    return PDSC_OK;
}

// The call (include/pointdsc_hip.h: struct pdsc_forward_call, enum pdsc_forward_mode) plus what is derived from it once: encoder
// plan, workspace layout, the buffers more than one stage uses, a few scalars.
struct ForwardCtx {
    const pdsc_forward_call& c;
    hipStream_t main;    // the caller's stream
    EncoderPlan plan;
    WsLayout L;
    hipStream_t st;      // where the next launch goes: the caller's stream, after fork_tail the tail stream
    int M, S, k, cfmt;   // cfmt: enum pdsc_compat_format of the compat buffer
    long long ld;
    bool split;
    float *compat, *featA, *featB, *featC, *qkv, *msg, *normed, *normed_pf, *conf, *keys, *seed_trans;
    int *seeds, *knn_idx, *counts;
    unsigned int *conv_mask, *range_flag;
    unsigned int* range_report;      // device address of c.range_report (validate_call), or NULL
    void *att_scratch, *q_split, *kv_tiles;
    const float* W(int section, int layer) const { return c.wpack + wpack_offset(c.cfg, section, layer); }
    const void* WS(int section, int layer) const { return (const unsigned short*)c.wsplit + pdsc_wsplit_offset(c.cfg, section, layer); }
};

static const char* mode_name(int mode) {
    return mode == PDSC_FORWARD_TESTING ? "testing" : mode == PDSC_FORWARD_VALIDATION ? "validation" : mode == PDSC_FORWARD_PROBE ? "probe" : "?";
}
// PDSC_REQUIRE whose text names the call and its mode; `c` is the pdsc_forward_call in scope
#define PDSC_REQUIRE_CALL(cond, fmt, ...) PDSC_REQUIRE(cond, "pdsc_forward(%s): " fmt, mode_name(c.mode), ##__VA_ARGS__)

// Every argument check of the call: pure host code but for one pointer query, nothing is enqueued before it has passed.
static int validate_call(ForwardCtx& x) {
    const pdsc_forward_call& c = x.c;
    if (!config_ok(c.cfg)) return PDSC_ERR_ARG;
    PDSC_REQUIRE(c.mode == PDSC_FORWARD_TESTING || c.mode == PDSC_FORWARD_VALIDATION || c.mode == PDSC_FORWARD_PROBE,
                 "pdsc_forward: unknown mode %d (enum pdsc_forward_mode)", c.mode);
    const bool testing = c.mode == PDSC_FORWARD_TESTING;
    PDSC_REQUIRE_CALL(testing || !c.tail_stream, "a tail stream belongs to the testing forward only");
    PDSC_REQUIRE_CALL(testing || !c.range_report, "range_report belongs to the testing forward only");
    PDSC_REQUIRE_CALL(!c.tail_stream || (c.fork_event && c.join_event && c.tail_stream != x.main),
                      "a tail stream (different from the main stream) needs the fork and join events");
    const int N = c.N, n_min = c.n_min, k = c.cfg->k < N - 1 ? c.cfg->k : N - 1;
    PDSC_REQUIRE_CALL((c.num_corr == nullptr) == (c.num_seeds_per_pair == nullptr), "both per-pair count arrays (device, [bs] int32) or neither");
    if (c.num_corr) {
        PDSC_REQUIRE_CALL(testing, "a ragged batch belongs to the testing forward only");
        PDSC_REQUIRE_CALL(n_min >= 2 && n_min <= N, "n_min=%d (N=%d)", n_min, N);
        // one launch has one neighbour count k = min(cfg->k, N - 1); the reference clamps per pair, k_b = min(k, num_corr_b - 1)
        // (models/PointDSC.py:250): a pair with fewer than k + 1 correspondences must be its own call
        PDSC_REQUIRE_CALL(n_min > k, "the shortest pair (%d correspondences) has no "
                          "more than k=%d: the reference clamps k per pair (k = min(k, num_corr - 1)); run such a pair in its own call", n_min, k);
    }
    PDSC_REQUIRE_CALL(c.mode != PDSC_FORWARD_VALIDATION || (c.M && c.ldM >= N), "M matrix [bs][N][ldM >= N] required");
    PDSC_REQUIRE_CALL(c.mode != PDSC_FORWARD_PROBE || c.absmax, "absmax [PDSC_RANGE_NUM_KINDS] (device) required");
    const bool outputs = c.mode == PDSC_FORWARD_PROBE || (c.final_trans && c.final_labels);
    PDSC_REQUIRE_CALL(c.wpack && c.corr_pos && c.src_keypts && c.tgt_keypts && outputs && c.workspace, "null pointer");
    PDSC_REQUIRE_CALL(c.bs > 0 && N > 1, "bs=%d N=%d", c.bs, N);
    PDSC_REQUIRE_CALL(c.num_seeds >= 1 && c.num_seeds <= N,
                      "num_seeds=%d (int(N*ratio) must be >= 1; the reference fails on an empty seed set)", c.num_seeds);
    x.range_report = nullptr;
    if (c.range_report) {
        // must be host memory the device can write (hipHostMalloc / a registered range): anything else would fault inside the kernel
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, c.range_report) != hipSuccess || at.type != hipMemoryTypeHost || at.devicePointer == nullptr) {
            (void)hipGetLastError();
            PDSC_REQUIRE_CALL(false, "range_report %p is not pinned, device-mapped host memory", (void*)c.range_report);
        }
        x.range_report = (unsigned int*)at.devicePointer;
    }
    return PDSC_OK;
}

// layout, workspace size check, shared buffers and derived scalars (x.c and x.plan are set)
static int bind_workspace(ForwardCtx& x) {
    const pdsc_forward_call& c = x.c;
    const WsLayout& L = x.L = make_layout(c.cfg, c.bs, c.N, c.num_seeds);
    if (c.workspace_bytes < L.total) {
        set_error("pdsc_forward(%s): workspace %zu < %zu bytes", mode_name(c.mode), c.workspace_bytes, L.total);
        return PDSC_ERR_WORKSPACE;
    }
    void* ws = c.workspace;
    x.st = x.main;
    x.M = c.bs * c.N; x.S = c.num_seeds; x.k = c.cfg->k < c.N - 1 ? c.cfg->k : c.N - 1;
    x.ld = pdsc_compat_ld(c.N);
    x.compat = L.at<float>(ws, WS_COMPAT); x.featA = L.at<float>(ws, WS_FEATA); x.featB = L.at<float>(ws, WS_FEATB);
    x.featC = L.at<float>(ws, WS_FEATC); x.qkv = L.at<float>(ws, WS_QKV); x.msg = L.at<float>(ws, WS_MSG);
    x.normed = L.at<float>(ws, WS_NORMED); x.conf = L.at<float>(ws, WS_CONF); x.keys = L.at<float>(ws, WS_KEYS);
    x.seed_trans = L.at<float>(ws, WS_SEED_TRANS); x.seeds = L.at<int>(ws, WS_SEEDS); x.knn_idx = L.at<int>(ws, WS_KNN_IDX);
    x.counts = L.at<int>(ws, WS_COUNTS); x.conv_mask = L.at<unsigned int>(ws, WS_CONV_MASK); x.att_scratch = L.at<void>(ws, WS_ATT_SCRATCH);
    const bool split = x.split = x.plan.split;
    PDSC_REQUIRE_CALL(!split || c.wsplit, "the split-precision modes need the split-weight buffer (pdsc_wsplit_build)");
    x.q_split = split ? L.at<void>(ws, WS_Q_SPLIT) : nullptr;
    x.kv_tiles = split ? L.at<void>(ws, WS_KV_TILES) : nullptr;
    // fp16 range sentinel: zeroed by the layer0 launch, set by the layer kernels' conversion sites (LayerArgs.range_flag), read by
    // the refinement launch
    x.range_flag = split && c.mode != PDSC_FORWARD_PROBE ? L.at<unsigned int>(ws, WS_RANGE_FLAG) : nullptr;
    x.cfmt = split && c.cfg->compat_format == PDSC_COMPAT_U16 ? PDSC_COMPAT_U16 : PDSC_COMPAT_F32;
    // (testing forward, large batches: the seeds' kNN runs fused -- knn_fused_kernel -- and takes the normalised rows in
    // point-fragment order too; normed_pf != NULL says so)
    const bool knn_fused = c.mode == PDSC_FORWARD_TESTING && knn_seeds_uses_fused(c.bs, c.N, x.S, x.k);
    x.normed_pf = knn_fused ? L.at<float>(ws, WS_NORMED_PF) : nullptr;
    return PDSC_OK;
}

// Probe: slot[kind] := max(slot[kind], max |v|); every other mode: nothing
static int probe_absmax(const ForwardCtx& x, int kind, const float* v, size_t count) {
    return x.c.absmax ? launch_absmax(v, count, (unsigned int*)x.c.absmax + kind, x.st) : PDSC_OK;
}

// Step 1 (models/PointDSC.py:150-155): compat, then layer0 of the SCNonlocal encoder
static int run_compat_layer0(const ForwardCtx& x) {
    const pdsc_forward_call& c = x.c;
    if (x.cfmt == PDSC_COMPAT_U16)
        PDSC_TRY(pdsc_spatial_compat_u16(c.src_keypts, c.tgt_keypts, x.W(PDSC_W_SIGMA_SPAT, 0), (unsigned short*)x.compat, x.ld, c.bs, c.N, x.st));
    else
        PDSC_TRY(pdsc_spatial_compat(c.src_keypts, c.tgt_keypts, x.W(PDSC_W_SIGMA_SPAT, 0), x.compat, nullptr, x.ld, c.bs, c.N, x.st));
    PDSC_TRY(launch_layer0(c.corr_pos, c.cfg->in_dim, x.W(PDSC_W_LAYER0_W, 0), x.W(PDSC_W_LAYER0_B, 0), x.featA, x.M, x.range_flag, c.bs, x.st));
    return probe_absmax(x, PDSC_RANGE_LAYER0, x.featA, (size_t)x.M * PDSC_CHANNELS);
}

// the row-order split attention: merged rows in msg_out, or (msg_out == NULL) the key-split partials left in att_scratch
static int attention_split(const ForwardCtx& x, float* msg_out, int nsplit) {
    return launch_attention_split_ex(x.q_split, x.kv_tiles, x.compat, x.cfmt, x.ld, msg_out, x.att_scratch, x.L.bytes[WS_ATT_SCRATCH], x.c.bs,
                                     x.c.N, nsplit, PDSC_PARTIALS_ROWS, x.c.num_corr, x.st);
}

// One fused launch: the tail of layer i (i = -1: none, the input is featA) and the head of layer i+1 (last: none, the result is
// featA); cur = the residual input of the tail, nxt = where the head leaves featB.
static int run_fused_layer(const ForwardCtx& x, int i, bool last, const float* cur, float* nxt) {
    const EncoderPlan& plan = x.plan;
    const bool tail = i >= 0, head = !last, split = x.split;
    // the attention's partials (leaves or key splits), when the layer kernel merges them itself
    const bool parts = plan.pf || plan.fuse_merge;
    // slots = partials per pair in the scratch layout; nparts = partials the layer kernel merges: one where every attention
    // workgroup owned all the leaves of its query block and merged them itself (it sits in the pair's leaf-0 slot)
    const int slots = plan.leaves ? plan.nleaf : plan.ns;
    const int nparts = plan.leaves && plan.leaf_ns == 1 ? 1 : slots;
    const float* part_o = parts ? (const float*)x.att_scratch : nullptr;
    const float* part_ml = parts ? part_o + (size_t)x.c.bs * slots * plan.Npad * plan.value_width : nullptr;
    pdsc_layer_call c{};
    // exact fp32: the batch is ONE run of M independent rows (bs = 1, N = M), so the per-pair counts of a ragged batch do
    // not describe it (with them the kernel took counts[0] for the row count of the whole batch).  Padding rows are computed
    // like any row; nothing valid reads them.
    c.bs = split ? x.c.bs : 1; c.N = split ? x.c.N : x.M;
    if (tail) {
        c.msg = parts ? nullptr : x.msg;
        c.part_o = part_o; c.part_ml = part_ml; c.nsplit = nparts; c.Npad = plan.Npad;
        c.res = cur;
    } else
        c.feat_in = x.featA;
    if (last) c.feat_out = x.featA;
    if (head) {
        c.featB_out = nxt; c.qkv_out = split ? nullptr : x.qkv;
        c.q_split = x.q_split; c.kv_tiles = x.kv_tiles;
    }
    if (plan.frag) {
        if (tail) c.wfrag_tail = x.WS(plan.ws_tail, i);
        if (head) c.wfrag_head = x.WS(plan.ws_head, i + 1);
        c.gemm_format = plan.gemm;
    } else {
        // natural layout; x3 (experiments builds: layer_split.hip): the hi|lo matrices of the split-weight buffer instead
        auto mat = [&](int section, int l) { return plan.x3 ? x.WS(section, l) : (const void*)x.W(section, l); };
        if (tail) {
            c.w1 = mat(PDSC_W_FC1_W, i); c.b1 = x.W(PDSC_W_FC1_B, i); c.w2 = mat(PDSC_W_FC2_W, i); c.b2 = x.W(PDSC_W_FC2_B, i);
            c.w3 = mat(PDSC_W_FC3_W, i); c.b3 = x.W(PDSC_W_FC3_B, i);
        }
        if (head) {
            c.wp = mat(PDSC_W_PCN_W, i + 1); c.bp = x.W(PDSC_W_PCN_B, i + 1); c.wq = mat(PDSC_W_QKV_W, i + 1); c.bq = x.W(PDSC_W_QKV_B, i + 1);
            if (split) c.wq_split = x.WS(PDSC_W_QKV_W, i + 1);
        }
    }
    if (plan.pf) c.io_flags = (tail ? PDSC_IO_PARTIALS_PF | PDSC_IO_RES_PF : 0) | (head ? PDSC_IO_FEATB_PF : 0);
    // the forward's own fields: EVERY launch reports to the range sentinel (NULL in exact fp32 and in the probe: bind_workspace);
    // the point-fragment route takes no trace (layer_args.h)
    LayerArgs a = layer_args_from_call(c);
    a.nvalid = split ? x.c.num_corr : nullptr;
    a.range_flag = x.range_flag;
    if (tail) a.part_slots = slots;
    if (plan.pf)
        a.value_fold = plan.fold;
    else
        a.trace = pdsc_layer_trace_buffer();
    PDSC_TRY(validate_layer_args(a, plan.kernel, "pdsc_forward(layer)"));
    return dispatch_layer(a, plan.kernel, x.st);
}

// head of layer 0, then per layer: attention + ONE launch for the merge of the key-split partials (when they are left
// un-merged), the tail of layer i and the head of layer i+1
static int run_encoder_fused(const ForwardCtx& x) {
    const pdsc_forward_call& c = x.c;
    const EncoderPlan& plan = x.plan;
    const size_t att_bytes = x.L.bytes[WS_ATT_SCRATCH];
    PDSC_TRY(run_fused_layer(x, -1, false, nullptr, x.featB));
    float *cur = x.featB, *nxt = x.featC;
    for (int i = 0; i < c.cfg->num_layers; ++i) {
        if (!x.split)
            PDSC_TRY(launch_attention_fp32(x.qkv, x.compat, x.ld, x.msg, x.att_scratch, att_bytes, c.bs, c.N, 0, c.num_corr, x.st));      // (r06: ragged batches too)
        else if (plan.leaves)
            PDSC_TRY(launch_attention_leaves(x.q_split, x.kv_tiles, x.compat, x.cfmt, x.ld, x.att_scratch, att_bytes, c.bs, c.N,
                                             c.cfg->att_leaves, c.num_corr, c.n_min, x.st, plan.value_width));
        else if (plan.pf)
            PDSC_TRY(launch_attention_split_ex(x.q_split, x.kv_tiles, x.compat, x.cfmt, x.ld, nullptr, x.att_scratch, att_bytes, c.bs, c.N,
                                               plan.ns, PDSC_PARTIALS_PF, c.num_corr, x.st, plan.value_width));
        else
            PDSC_TRY(attention_split(x, plan.fuse_merge ? nullptr : x.msg, plan.ns));
        PDSC_TRY(run_fused_layer(x, i, i + 1 == c.cfg->num_layers, cur, nxt));
        float* tmp = cur; cur = nxt; nxt = tmp;
    }
    return PDSC_OK;
}

// One launch per conv, every intermediate in the workspace: the probe (which records |max| of each kind), num_layers == 0 and
// the tuning knob PDSC_FUSED_LAYERS = 0 (experiments builds; NO range sentinel on this path: pdsc_pack_qkv_split does not note)
static int run_encoder_per_conv(const ForwardCtx& x) {
    const int C = PDSC_CHANNELS, H = C / 2, M = x.M;
    float *t64a = x.L.at<float>(x.c.workspace, WS_T64A), *t64b = x.L.at<float>(x.c.workspace, WS_T64B);
    for (int i = 0; i < x.c.cfg->num_layers; ++i) {
        PDSC_TRY(pdsc_linear(x.featA, C, x.W(PDSC_W_PCN_W, i), x.W(PDSC_W_PCN_B, i), nullptr, 0, x.featB, C, M, C, C, 1, x.st));
        PDSC_TRY(probe_absmax(x, PDSC_RANGE_POINTCN, x.featB, (size_t)M * C));
        PDSC_TRY(pdsc_linear(x.featB, C, x.W(PDSC_W_QKV_W, i), x.W(PDSC_W_QKV_B, i), nullptr, 0, x.qkv, 3 * C, M, C, 3 * C, 0, x.st));
        PDSC_TRY(probe_absmax(x, PDSC_RANGE_QKV, x.qkv, (size_t)M * 3 * C));
        if (x.split) {
            PDSC_TRY(pdsc_pack_qkv_split(x.qkv, x.q_split, x.kv_tiles, x.c.bs, x.c.N, x.st));
            PDSC_TRY(attention_split(x, x.msg, 0));
        } else
            PDSC_TRY(pdsc_sc_attention(x.qkv, x.compat, x.ld, x.msg, x.att_scratch, x.L.bytes[WS_ATT_SCRATCH], x.c.bs, x.c.N, 0, x.st));
        PDSC_TRY(probe_absmax(x, PDSC_RANGE_MESSAGE, x.msg, (size_t)M * C));
        PDSC_TRY(pdsc_linear(x.msg, C, x.W(PDSC_W_FC1_W, i), x.W(PDSC_W_FC1_B, i), nullptr, 0, t64a, H, M, C, H, 1, x.st));
        PDSC_TRY(probe_absmax(x, PDSC_RANGE_FC1, t64a, (size_t)M * H));
        PDSC_TRY(pdsc_linear(t64a, H, x.W(PDSC_W_FC2_W, i), x.W(PDSC_W_FC2_B, i), nullptr, 0, t64b, H, M, H, H, 1, x.st));
        PDSC_TRY(probe_absmax(x, PDSC_RANGE_FC2, t64b, (size_t)M * H));
        PDSC_TRY(pdsc_linear(t64b, H, x.W(PDSC_W_FC3_W, i), x.W(PDSC_W_FC3_B, i), x.featB, C, x.featA, C, M, H, C, 0, x.st));
        PDSC_TRY(probe_absmax(x, PDSC_RANGE_FEATURE, x.featA, (size_t)M * C));
    }
    return PDSC_OK;
}

// Two streams (pdsc_forward_call.tail_stream): everything after the encoder -- a strictly sequential chain of ~15 small, latency-bound
// launches -- goes to the caller's second (high-priority) stream: with several forwards in flight its workgroups are then
// dispatched ahead of the queued workgroups of another forward's attention launch instead of behind them.
static int fork_tail(ForwardCtx& x) {
    if (!x.c.tail_stream) return PDSC_OK;
    if (hipEventRecord((hipEvent_t)x.c.fork_event, x.main) != hipSuccess ||
        hipStreamWaitEvent((hipStream_t)x.c.tail_stream, (hipEvent_t)x.c.fork_event, 0) != hipSuccess)
        return check_launch("pdsc_forward(fork)");
    x.st = (hipStream_t)x.c.tail_stream;
    return PDSC_OK;
}
// join: whatever the caller enqueues on the main stream next is ordered after the results
static int join_tail(const ForwardCtx& x) {
    if (!x.c.tail_stream) return PDSC_OK;
    if (hipEventRecord((hipEvent_t)x.c.join_event, (hipStream_t)x.c.tail_stream) != hipSuccess ||
        hipStreamWaitEvent(x.main, (hipEvent_t)x.c.join_event, 0) != hipSuccess)
        return check_launch("pdsc_forward(join)");
    return PDSC_OK;
}

// Step 2.1 (:156,:171,:174): confidence head, normalise, then the seeds: by NMS (Testing), or the top S by confidence next to the
// feature similarity matrix (Validation, :158-163 and :176)
static int run_seed_selection(const ForwardCtx& x) {
    const pdsc_forward_call& c = x.c;
    const int C = PDSC_CHANNELS, M = x.M;
    float *h1 = x.L.at<float>(c.workspace, WS_H1), *h2 = x.L.at<float>(c.workspace, WS_H2);
    if (env_int("PDSC_CLS_FUSED", 1))       // (A/B knob, experiments builds: 0 = the two pdsc_linear launches of r01-r03; same bits)
        PDSC_TRY(launch_classifier_hidden(x.featA, x.W(PDSC_W_CLS1_W, 0), x.W(PDSC_W_CLS1_B, 0), x.W(PDSC_W_CLS2_W, 0), x.W(PDSC_W_CLS2_B, 0), h2, M, x.st));
    else {
        PDSC_TRY(pdsc_linear(x.featA, C, x.W(PDSC_W_CLS1_W, 0), x.W(PDSC_W_CLS1_B, 0), nullptr, 0, h1, 32, M, C, 32, 1, x.st));
        PDSC_TRY(pdsc_linear(h1, 32, x.W(PDSC_W_CLS2_W, 0), x.W(PDSC_W_CLS2_B, 0), nullptr, 0, h2, 32, M, 32, 32, 1, x.st));
    }
    if (x.normed_pf)
        PDSC_TRY(launch_normalize_conf_pf(x.featA, h2, x.W(PDSC_W_CLS3_W, 0), x.W(PDSC_W_CLS3_B, 0), x.normed, x.normed_pf, x.conf, c.bs, c.N, x.st));
    else
        PDSC_TRY(pdsc_normalize_confidence(x.featA, h2, x.W(PDSC_W_CLS3_W, 0), x.W(PDSC_W_CLS3_B, 0), x.normed, x.conf, M, x.st));
    if (c.mode == PDSC_FORWARD_TESTING) {
        PDSC_TRY(launch_nms_keys_grid(c.src_keypts, x.conf, c.cfg->nms_radius, x.keys, x.L.at<void>(c.workspace, WS_NMS_WS),
                                      pdsc_nms_workspace_bytes(c.bs, c.N), c.bs, c.N, c.num_corr, x.st));
        return launch_rank_select(x.keys, x.seeds, c.bs, c.N, x.S, c.num_corr, c.num_seeds_per_pair, x.st, x.conv_mask);      // (+ the solver's mask := all-ones)
    }
    PDSC_TRY(pdsc_feature_compat(x.normed, x.W(PDSC_W_SIGMA, 0), c.M, c.ldM, c.bs, c.N, x.st));
    return pdsc_rank_select(x.conf, x.seeds, c.bs, c.N, x.S, x.st);
}

// Step 3 & 4 (:182 -> :234-336): per-seed hypotheses and their scores
static int run_hypotheses(const ForwardCtx& x) {
    const pdsc_forward_call& c = x.c;
    const bool testing = c.mode == PDSC_FORWARD_TESTING;
    const int iters = c.cfg->num_iterations;
    void* ws = c.workspace;
    float *knn_dist = x.L.at<float>(ws, WS_KNN_DIST), *eig = x.L.at<float>(ws, WS_EIG_ITERS), *seed_w = x.L.at<float>(ws, WS_SEED_W);
    PDSC_TRY(launch_knn_seeds_form(x.normed, x.normed_pf, x.seeds, knn_dist, x.knn_idx, c.bs, c.N, x.S, x.k, c.num_corr, x.normed_pf ? 2 : 1, x.st));
    if (!testing && c.bs > 1) {
        // validation forward: the early exit is taken over the seeds of ALL pairs of the batch (one torch.allclose over
        // [bs*S, k]) -- the per-pair masks are AND-ed before the iterate is chosen, so the two steps stay apart
        PDSC_TRY(pdsc_seed_power_iteration(x.normed, c.src_keypts, c.tgt_keypts, x.knn_idx, x.W(PDSC_W_SIGMA, 0), x.W(PDSC_W_SIGMA_SPAT, 0), eig, x.conv_mask,
                                           nullptr, c.bs, c.N, x.S, x.k, iters, x.st));
        PDSC_TRY(pdsc_conv_mask_all_pairs(x.conv_mask, c.bs, x.st));
        PDSC_TRY(pdsc_seed_transforms(c.src_keypts, c.tgt_keypts, x.knn_idx, eig, x.conv_mask, x.seed_trans, seed_w, c.bs, c.N, x.S, x.k, iters, x.st));
    } else
        PDSC_TRY(launch_seed_solve_forward(x.normed, c.src_keypts, c.tgt_keypts, x.knn_idx, x.W(PDSC_W_SIGMA, 0), x.W(PDSC_W_SIGMA_SPAT, 0), eig, x.conv_mask,
                                           /*seed_M=*/nullptr, x.seed_trans, seed_w, c.bs, c.N, x.S, x.k, iters, /*mask_ready=*/testing, x.st));
#ifdef PDSC_EXPERIMENTS
    score_debug_slot() = env_int("PDSC_SCORE_DEBUG", 0) ? x.L.at<float>(ws, WS_SCORE_DBG) : nullptr;
#endif
    PDSC_TRY(launch_score_hypotheses(x.seed_trans, c.src_keypts, c.tgt_keypts, c.cfg->inlier_threshold, x.counts, c.bs, c.N, x.S, c.num_corr, x.st));
#ifdef PDSC_EXPERIMENTS
    score_debug_slot() = nullptr;
#endif
    return PDSC_OK;
}

// best hypothesis + its labels, then post refinement (:186 -> :403-438) in the same launch; final_labels stay those of the
// pre-refinement best hypothesis
static int finish_testing(const ForwardCtx& x) {
    const pdsc_forward_call& c = x.c;
    const WsLayout& L = x.L;
    void* ws = c.workspace;
    return launch_select_and_refine(x.counts, x.seed_trans, c.src_keypts, c.tgt_keypts, c.cfg->inlier_threshold, c.cfg->refine_threshold, c.cfg->refine_iters,
                                    L.at<int>(ws, WS_BEST), L.at<float>(ws, WS_INITIAL_TRANS), c.final_labels, c.final_trans,
                                    L.at<int>(ws, WS_SOLVES), c.bs, c.N, x.S, c.num_corr, x.st, L.at<int>(ws, WS_REFINE_TRACE), x.range_flag,
                                    x.range_report);
}
// best hypothesis is the result (:186 is skipped); the labels of the call are the logits (:190-191).  pdsc_select_best does not know
// the range sentinel: a launch of its own behind it turns the pose of every flagged pair into NaN, as the refinement launch of the
// testing forward does
static int finish_validation(const ForwardCtx& x) {
    const pdsc_forward_call& c = x.c;
    PDSC_TRY(pdsc_select_best(x.counts, x.seed_trans, c.src_keypts, c.tgt_keypts, c.cfg->inlier_threshold, x.L.at<int>(c.workspace, WS_BEST), c.final_trans,
                              x.keys /* scratch */, c.bs, c.N, x.S, x.st));
    if (x.range_flag) PDSC_TRY(launch_poison_flagged(c.final_trans, x.range_flag, c.bs, x.st));
    return launch_copy_u32((unsigned int*)c.final_labels, (const unsigned int*)x.conf, (size_t)x.M, x.st);
}

// The whole path: which mode runs which stage.  Nothing is enqueued before the call has passed every check (validate_call,
// plan_encoder and bind_workspace launch nothing); every stage after them only enqueues (no host synchronisation, no allocation,
// no state).
extern "C" int pdsc_forward(const pdsc_forward_call* call, void* stream) {
    PDSC_REQUIRE(call, "pdsc_forward: null call");
    const bool probe = call->mode == PDSC_FORWARD_PROBE, testing = call->mode == PDSC_FORWARD_TESTING;
    ForwardCtx x{*call, (hipStream_t)stream};
    PDSC_TRY(validate_call(x));
    PDSC_TRY(plan_encoder(call->cfg, call->bs, call->N, call->num_corr, call->n_min, &x.plan));
    PDSC_TRY(bind_workspace(x));
    if (probe) PDSC_TRY(launch_fill_u32((unsigned int*)call->absmax, 0u, PDSC_RANGE_NUM_KINDS, x.st));
    PDSC_TRY(run_compat_layer0(x));
    PDSC_TRY(x.plan.fused && !probe ? run_encoder_fused(x) : run_encoder_per_conv(x));
    if (probe) return PDSC_OK;
    PDSC_TRY(fork_tail(x));
    PDSC_TRY(run_seed_selection(x));
    PDSC_TRY(run_hypotheses(x));
    PDSC_TRY(testing ? finish_testing(x) : finish_validation(x));
    return join_tail(x);
}
