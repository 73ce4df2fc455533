// a-3, split-precision variant, host side: the planners (key split, leaves), the one launch path of sc_attention_split_kernel and
// the entry points.  The kernel, its decomposition and its forms (template parameters): attention_split_kernel.h.
#include <stdlib.h>
#include "attention_split_kernel.h"

namespace pdsc {

// waves per workgroup and key split for (bs, N): fill the 256 CUs (one 8-wave or two 4-wave workgroups each)
// with as few rounds x tiles-per-round as possible; prefer group counts that are multiples of 8 (XCD mapping)
static void split_plan(int bs, int N, int* nw_out, int* nsplit_out) {
    const int tiles = spl_num_tiles(N);
    const int nw = (long long)bs * ceil_div(N, 256) >= 48 ? 8 : 4;
    const int nq = ceil_div(N, nw * 32);
    const int slots = nw == 8 ? 256 : 512;
    const int cap = tiles / 4 > 1 ? tiles / 4 : 1;
    int best = 1;
    double best_cost = 1e30;
    for (int ns = 1; ns <= cap && ns <= 64; ++ns) {
        const int wgs = nq * bs * ns;
        const int rounds = ceil_div(wgs, slots);
        // per workgroup: its tiles + prologue/epilogue (~3 tiles' worth, more when partials are written)
        double cost = (double)rounds * (ceil_div(tiles, ns) + (ns > 1 ? 4.0 : 3.0));
        if (((ns * bs) & 7) != 0) cost *= 1.03;
        if (cost < best_cost - 1e-9) { best_cost = cost; best = ns; }
    }
    const int force_nw = env_int("PDSC_ATT_SPLIT_NW", 0), force_ns = env_int("PDSC_ATT_SPLIT_NS", 0);   // tuning/A-B knobs
    *nw_out = (force_nw == 4 || force_nw == 8) ? force_nw : nw;
    *nsplit_out = force_ns > 0 ? (force_ns < tiles ? force_ns : tiles) : best;
}

// ---- leaf form: leaves and plan ----------------------------------------------------------------------------------------
// Canonical leaf count: a function of N ALONE (never of the batch), so that a pair's summation tree -- every leaf from a fresh
// online-softmax state, leaves merged in leaf order by the layer kernel -- and hence its bits do not depend on how many pairs share
// the launch.  At most MERGE_MAX_SPLIT_H3 = 8 (what the layer kernel merges while loading), leaves of at least 4 tiles:
//   N <= 1504 (< 48 tiles): as many leaves as the per-launch planner's finest split for one pair (N = 1000: 8);
//   larger N: 4 -- every leaf partial is 528 B per point that the attention writes and the layer launch reads back, whatever the
//   batch: at 32 pairs of N = 5000 the price of 4 leaves (two per workgroup) is measured in profiles/r05_*ab_leaves*.txt.
int attention_leaf_count(int N) {
    const int t = spl_num_tiles(N);
    return t >= 48 ? 4 : t >= 32 ? 8 : t >= 16 ? 4 : t >= 8 ? 2 : 1;
}

// leaves_mode (pdsc_config.att_leaves): PDSC_LEAVES_CANONICAL = attention_leaf_count(N) leaves, the key split a divisor of it;
// >= 2: that many leaves (tuning, at most PDSC_ATT_MAX_LEAVES).  (PDSC_LEAVES_PER_LAUNCH does not come here: it is the key-split form.)
// The key split (workgroups per query block) is a pure function of (bs, N) and decides speed only: a workgroup that owns all the
// leaves of its query block merges them itself with the layer kernel's arithmetic (the kernel's epilogue), so the bits are those
// of the leaf count whatever the split.  pdsc_attention_leaf_split_override (diagnostics) replaces the rule by a divisor of the
// leaf count; a value that does not divide it is an error here, where the leaf count is known.
static int g_leaf_split_override = 0;
int leaf_plan(int bs, int N, int leaves_mode, int* nw_out, int* nsplit_out, int* nleaf_out) {
    int nw, ns;
    split_plan(bs, N, &nw, &ns);
    const int tiles = spl_num_tiles(N);
    int C = leaves_mode == PDSC_LEAVES_CANONICAL ? attention_leaf_count(N) : leaves_mode;
    if (C > tiles / 2) C = tiles / 2;            // every leaf at least two tiles (the kernel's boundary and restart iterations are distinct)
    if (C > PDSC_ATT_MAX_LEAVES) C = PDSC_ATT_MAX_LEAVES;
    if (C < 1) C = 1;
    // the per-launch cost model over the divisors of C; a leaf that ends inside a workgroup's range costs about a third of a tile
    const int nq = ceil_div(N, nw * 32), slots = nw == 8 ? 256 : 512;
    int best = 1;
    double best_cost = 1e30;
    for (int d = 1; d <= C; ++d) {
        if (C % d) continue;
        const int wgs = nq * bs * d, rounds = ceil_div(wgs, slots);
        double cost = (double)rounds * (ceil_div(tiles, d) + 4.0 + 0.35 * (C / d));
        if (((d * bs) & 7) != 0) cost *= 1.03;
        if (cost < best_cost - 1e-9) { best_cost = cost; best = d; }
    }
    // One workgroup per query block wherever these alone give every CU an 8-wave workgroup: the model above counts whole rounds of ONE
    // launch and so pays for the ragged last round (32 pairs of N = 5000: 640 workgroups = 2.5 rounds), which the forward in
    // flight beside this one fills; the workgroup then merges its own leaves and the layer launch loads one partial per point instead
    // of nleaf.  Measured with two forwards in flight (profiles/leaf_merge_ab.txt): 32 / 16 pairs of N = 5000 +1.3 / +2.8 %, 16 KITTI
    // pairs +1.9 %, 8 pairs of N = 10000 +1.1 %; below a full round (8 pairs of N = 5000: within the spread; 4 pairs: -12 %) the
    // model's choice stands.  A single forward on its own stream pays the last round (attention launch +10 % at 32 pairs).
    if (C > 1 && nw == 8 && (long long)nq * bs >= slots) best = 1;
    int force = g_leaf_split_override;
#ifdef PDSC_EXPERIMENTS
    if (force == 0) force = env_int("PDSC_ATT_LEAF_SPLIT", 0);       // A/B knob (experiments builds): as the override
#endif
    *nw_out = nw; *nsplit_out = best; *nleaf_out = C;
    if (force != 0) {
        PDSC_REQUIRE(force > 0 && C % force == 0, "attention leaf plan: the split override %d does not divide the %d leaves of N=%d", force, C, N);
        *nsplit_out = force;
    }
    return PDSC_OK;
}

}  // namespace pdsc

using namespace pdsc;

// scratch of `slots` partials (key splits or leaves) per pair: [bs][slots][Npad][value_width] accumulators, then [bs][slots][Npad][2] (m, l)
static size_t partials_bytes(int bs, int slots, int N, int value_width) {
    return (size_t)bs * slots * round_up(N, 256) * (value_width + 2) * sizeof(float);
}
// ... and where the (m, l) block of that scratch begins
static float* partials_ml(float* part_o, int bs, int slots, int N, int value_width) {
    return part_o + partials_bytes(bs, slots, N, value_width) / ((value_width + 2) * sizeof(float)) * value_width;
}
// LDS of a workgroup's two stages: K 16 KiB + V^T 16 KiB (8 KiB at 64 channels) + the compat rows of its nw * 32 queries, 128 B (fp32)
// or 64 B (unorm16) each -- none when the compat values go straight into registers (cm: the kernel's compat mode CM)
static size_t stage_lds_bytes(int nw, int cm, int value_width) {
    const size_t tile = value_width == PDSC_CHANNELS ? SPL_TILE_BYTES : spl_tile_bytes<PDSC_CHANNELS / 2>();
    return 2 * (tile + (cm == 2 ? 0 : (size_t)nw * 32 * (cm == 1 ? 64 : 128)));
}

extern "C" int pdsc_attention_leaf_count(int N) { return N > 0 ? attention_leaf_count(N) : -1; }

extern "C" int pdsc_attention_leaf_plan(int bs, int N, int leaves_mode, int* nsplit, int* nleaf) {
    PDSC_REQUIRE(bs > 0 && N > 0 && leaves_mode >= PDSC_LEAVES_CANONICAL && leaves_mode <= PDSC_ATT_MAX_LEAVES && nsplit && nleaf,
                 "pdsc_attention_leaf_plan: bs=%d N=%d leaves_mode=%d", bs, N, leaves_mode);
    int nw;
    return leaf_plan(bs, N, leaves_mode, &nw, nsplit, nleaf);
}

extern "C" int pdsc_attention_leaf_split_override(int d) {   // diagnostics: see include/pointdsc_hip.h
    PDSC_REQUIRE(d >= 0 && d <= PDSC_ATT_MAX_LEAVES, "pdsc_attention_leaf_split_override: d=%d (0 = the planner decides, else a divisor of the leaf count)", d);
    g_leaf_split_override = d;
    return PDSC_OK;
}

extern "C" size_t pdsc_attention_leaf_scratch_bytes(int bs, int N, int leaves_mode) {
    if (bs <= 0 || N <= 0 || leaves_mode < PDSC_LEAVES_CANONICAL) return 0;
    int nw, ns, C;
    leaf_plan(bs, N, leaves_mode, &nw, &ns, &C);     // (the leaf count does not depend on the split: an override error is the launch's to report)
    return partials_bytes(bs, C, N, PDSC_CHANNELS);
}

extern "C" size_t pdsc_split_q_bytes(int bs, int N) {
    if (bs <= 0 || N <= 0) return 0;
    return (size_t)bs * N * SPL_Q_LD * sizeof(sp16);
}
extern "C" size_t pdsc_split_kv_bytes(int bs, int N) {
    if (bs <= 0 || N <= 0) return 0;
    return (size_t)bs * spl_num_tiles(N) * SPL_TILE_STRIDE;
}

extern "C" int pdsc_attention_split_default_split(int bs, int N) {
    if (bs <= 0 || N <= 0) return -1;
    int nw, ns;
    split_plan(bs, N, &nw, &ns);
    return ns;
}

extern "C" size_t pdsc_attention_split_scratch_bytes(int bs, int N, int nsplit) {
    if (bs <= 0 || N <= 0) return 0;
    int nw, ns;
    split_plan(bs, N, &nw, &ns);
    if (nsplit <= 0) nsplit = ns;
    return nsplit == 1 ? 0 : partials_bytes(bs, nsplit, N, PDSC_CHANNELS);
}

extern "C" int pdsc_pack_qkv_split(const float* qkv, void* q_split, void* kv_tiles, int bs, int N, void* stream) {
    PDSC_REQUIRE(qkv && q_split && kv_tiles, "pdsc_pack_qkv_split: null pointer");
    PDSC_REQUIRE(bs > 0 && N > 0, "pdsc_pack_qkv_split: bs=%d N=%d", bs, N);
    const int tiles = spl_num_tiles(N);
    hipLaunchKernelGGL(pack_qkv_split_kernel, dim3(tiles, bs), dim3(256), 0, (hipStream_t)stream, qkv, (sp16*)q_split,
                       (unsigned char*)kv_tiles, N, tiles);
    return check_launch("pdsc_pack_qkv_split");
}

static long long* g_att_trace = nullptr;
extern "C" int pdsc_attention_trace(long long* device_buffer) {   // diagnostics: see include/pointdsc_hip.h
    g_att_trace = device_buffer;
    return PDSC_OK;
}

// ---- the launch path --------------------------------------------------------------------------------------------------------
// One instantiation of the kernel: dynamic-LDS opt-in, the profile marks and the launch -- the only place that names the kernel.
// `what` labels a failed LDS opt-in; the callers check the launch itself.
template <int NW, int CM, bool TRACE, bool PS, bool PEEL, bool MG, int VW>
static int launch_instance(const AttSplitArgs& a, unsigned grid, unsigned block, size_t lds, hipStream_t st, const char* what) {
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&sc_attention_split_kernel<NW, CM, TRACE, PS, PEEL, MG, VW>), lds, what);
    if (rc != PDSC_OK) return rc;
    profile_mark_begin(PDSC_PROF_ATTENTION, st);
    hipLaunchKernelGGL((sc_attention_split_kernel<NW, CM, TRACE, PS, PEEL, MG, VW>), dim3(grid), dim3(block), lds, st, a);
    profile_mark_end(PDSC_PROF_ATTENTION, st);
    return PDSC_OK;
}
typedef int (*AttLaunchFn)(const AttSplitArgs&, unsigned, unsigned, size_t, hipStream_t, const char*);

// the forms that experiments builds add to the sixteen of the product (all false there)
struct AttExperiment {
    bool trace = false;       // per-phase cycle counts (pdsc_attention_trace); 8 waves
    bool persist = false;     // PDSC_ATT_PERSIST: one workgroup per CU walks several items; 8 waves, LDS-staged compat
    bool no_peel = false;     // PDSC_ATT_PEEL = 0: the straight-line tile loop; 8 waves, unorm16 compat
};                            // (and compat mode 2, PDSC_ATT_CREG: fp32 compat values straight into registers)

// (waves, compat mode, value width, leaf form) [+ an experiments-only form] -> the instantiation that runs it.  The product:
// {8, 4 waves} x {fp32, unorm16 compat} x {plain 128, 64-wide point-fragment, leaf 128, leaf 64}.
static AttLaunchFn select_instance(int nw, int cm, int value_width, bool leaf, const AttExperiment& x) {
    const bool w8 = nw == 8, c16 = cm == 1, v64 = value_width != PDSC_CHANNELS;
#ifdef PDSC_EXPERIMENTS
    if (x.persist) return c16 ? launch_instance<8, 1, false, true, true, false, 128> : launch_instance<8, 0, false, true, true, false, 128>;
    if (x.trace) return c16 ? launch_instance<8, 1, true, false, true, false, 128> : launch_instance<8, 0, true, false, true, false, 128>;
    if (x.no_peel) return launch_instance<8, 1, false, false, false, false, 128>;
    if (cm == 2) return w8 ? launch_instance<8, 2, false, false, true, false, 128> : launch_instance<4, 2, false, false, true, false, 128>;
#endif
    if (leaf && v64)
        return w8 ? (c16 ? launch_instance<8, 1, false, false, true, true, 64> : launch_instance<8, 0, false, false, true, true, 64>)
                  : (c16 ? launch_instance<4, 1, false, false, true, true, 64> : launch_instance<4, 0, false, false, true, true, 64>);
    if (leaf)
        return w8 ? (c16 ? launch_instance<8, 1, false, false, true, true, 128> : launch_instance<8, 0, false, false, true, true, 128>)
                  : (c16 ? launch_instance<4, 1, false, false, true, true, 128> : launch_instance<4, 0, false, false, true, true, 128>);
    if (v64)
        return w8 ? (c16 ? launch_instance<8, 1, false, false, true, false, 64> : launch_instance<8, 0, false, false, true, false, 64>)
                  : (c16 ? launch_instance<4, 1, false, false, true, false, 64> : launch_instance<4, 0, false, false, true, false, 64>);
    return w8 ? (c16 ? launch_instance<8, 1, false, false, true, false, 128> : launch_instance<8, 0, false, false, true, false, 128>)
              : (c16 ? launch_instance<4, 1, false, false, true, false, 128> : launch_instance<4, 0, false, false, true, false, 128>);
}

// What the two launchers share: the argument checks (error texts prefixed with `who`, as validate_layer_args), the kernel arguments
// that do not depend on the plan, and the LDS of the two stages.  The plan -- key split or leaves -- and what follows from it
// (nsplit, nleaf, part_ml, part_frag, msg, items) stay with the caller.
struct AttLaunch {
    AttSplitArgs a;
    int nw, ns;               // split_plan(bs, N): waves per workgroup (of either plan) and the per-launch planner's key split
    int cm;                   // the kernel's compat mode: 0 = fp32, 1 = unorm16
    size_t lds;               // stage_lds_bytes
};
static int prepare_attention_launch(const char* who, const void* q_split, const void* kv_tiles, const void* compat, int compat_format,
                                    long long ld, void* scratch, bool scratch_required, int bs, int N, const int* nvalid, int value_width,
                                    AttLaunch* p) {
    PDSC_REQUIRE(q_split && kv_tiles && compat && (scratch || !scratch_required), "%s: null pointer", who);
    PDSC_REQUIRE(value_width == PDSC_CHANNELS || value_width == PDSC_CHANNELS / 2, "%s: value_width=%d", who, value_width);
    PDSC_REQUIRE(bs > 0 && N > 0, "%s: bs=%d N=%d", who, bs, N);
    PDSC_REQUIRE(compat_format == PDSC_COMPAT_F32 || compat_format == PDSC_COMPAT_U16, "%s: compat_format=%d", who, compat_format);
    const bool c16 = compat_format == PDSC_COMPAT_U16;
    PDSC_REQUIRE(ld >= round_up(N, SPL_BK) && ld % (c16 ? 8 : 4) == 0, "%s: ld=%lld must be a multiple of %d and >= N rounded up to 32", who, ld, c16 ? 8 : 4);
    *p = AttLaunch{};
    p->cm = c16 ? 1 : 0;
    split_plan(bs, N, &p->nw, &p->ns);
    AttSplitArgs& a = p->a;
    a.qs = (const sp16*)q_split; a.kv = (const unsigned char*)kv_tiles; a.compat = compat; a.ld = ld;
    a.N = N; a.Npad = (int)round_up(N, 256); a.num_tiles = spl_num_tiles(N); a.bs = bs;
    a.nq = ceil_div(N, p->nw * 32);
    a.part_o = (float*)scratch;
    a.nvalid = nvalid;
    a.compat_nt = c16 ? 0 : 1;                 // (the wide variant still takes it as an argument)
    p->lds = stage_lds_bytes(p->nw, p->cm, value_width);
    return PDSC_OK;
}

// One attention launch in the leaf form: C leaf partials per query in scratch ([bs][C][Npad][128] then [bs][C][Npad][2], point-
// fragment order) for the H3 layer kernel to merge (C <= MERGE_MAX_SPLIT_H3).
int pdsc::launch_attention_leaves(const void* q_split, const void* kv_tiles, const void* compat, int compat_format, long long ld,
                                  void* scratch, size_t scratch_bytes, int bs, int N, int leaves_mode, const int* nvalid, int n_min,
                                  hipStream_t st, int value_width) {
    AttLaunch p;
    if (const int rc = prepare_attention_launch("pdsc_sc_attention_leaves", q_split, kv_tiles, compat, compat_format, ld, scratch, true, bs, N,
                                                nvalid, value_width, &p); rc != PDSC_OK) return rc;
    int nw, ns, C;                               // (nw: the per-launch planner's, p.nw)
    if (const int prc = leaf_plan(bs, N, leaves_mode, &nw, &ns, &C); prc != PDSC_OK) return prc;
    // ragged batches: every pair cuts ITS OWN tiles into C leaves -- the shortest pair needs at least C of them
    PDSC_REQUIRE(!nvalid || (n_min + 31) / 32 >= 2 * C, "pdsc_sc_attention_leaves: the shortest pair (%d correspondences) has fewer than two "
                 "32-key tiles for each of the %d leaves planned for bs=%d, N=%d", n_min, C, bs, N);
    const size_t need = partials_bytes(bs, C, N, value_width);
    if (scratch_bytes < need) {
        set_error("pdsc_sc_attention_leaves: scratch %zu < %zu bytes", scratch_bytes, need);
        return PDSC_ERR_WORKSPACE;
    }
    AttSplitArgs& a = p.a;
    a.nsplit = ns;
    a.nleaf = C;
    a.part_ml = partials_ml(a.part_o, bs, C, N, value_width);
    a.part_frag = 1;
    const unsigned grid = (unsigned)(a.nq * ns * bs);
    a.items = (int)grid;
    const AttLaunchFn launch = select_instance(p.nw, p.cm, value_width, true, AttExperiment{});
    const int rc = launch(a, grid, p.nw * 64, p.lds, st, "pdsc_sc_attention_leaves(dynamic LDS)");
    return rc != PDSC_OK ? rc : check_launch("pdsc_sc_attention_leaves");
}

// One attention launch in the key-split form; msg != NULL and a key split > 1: followed by the combine launch
static int launch_attention_split(const void* q_split, const void* kv_tiles, const void* compat, int compat_format, long long ld,
                                  float* msg, void* scratch, size_t scratch_bytes, int bs, int N, int nsplit, void* stream,
                                  int partial_layout = PDSC_PARTIALS_ROWS, const int* nvalid = nullptr, int value_width = PDSC_CHANNELS) {
    AttLaunch p;
    if (const int rc = prepare_attention_launch("pdsc_sc_attention_split", q_split, kv_tiles, compat, compat_format, ld, scratch, false, bs, N,
                                                nvalid, value_width, &p); rc != PDSC_OK) return rc;
    AttSplitArgs& a = p.a;
    const int nw = p.nw;
    const bool v64 = value_width != PDSC_CHANNELS;
    if (nsplit <= 0) nsplit = p.ns;
    if (nsplit > a.num_tiles) nsplit = a.num_tiles;
    PDSC_REQUIRE(msg || nsplit > 1, "pdsc_sc_attention_split: msg == NULL needs a key split > 1 (partials stay in scratch)");
    const size_t need = nsplit == 1 ? 0 : partials_bytes(bs, nsplit, N, value_width);
    if (need > 0 && (!scratch || scratch_bytes < need)) {
        set_error("pdsc_sc_attention_split: scratch %zu < %zu bytes", scratch_bytes, need);
        return PDSC_ERR_WORKSPACE;
    }
    PDSC_REQUIRE(partial_layout == PDSC_PARTIALS_ROWS || partial_layout == PDSC_PARTIALS_PF, "pdsc_sc_attention_split: partial_layout=%d", partial_layout);
    PDSC_REQUIRE(partial_layout == PDSC_PARTIALS_ROWS || (!msg && nsplit > 1), "pdsc_sc_attention_split: point-fragment partials are not merged here (msg must be NULL, key split > 1)");
    a.part_frag = partial_layout == PDSC_PARTIALS_PF;
    PDSC_REQUIRE(!v64 || a.part_frag, "pdsc_sc_attention_split: a 64-channel value projection leaves point-fragment partials only");
    a.msg = msg;
    a.nsplit = nsplit;
    a.part_ml = a.part_o ? partials_ml(a.part_o, bs, nsplit, N, value_width) : nullptr;
    a.trace = g_att_trace;
    a.prio_mode = env_int("PDSC_ATT_PRIO", 0);
    a.compute_all_waves = env_int("PDSC_ATT_ALL_WAVES", 0);
    unsigned grid = (unsigned)(a.nq * nsplit * bs);
    a.items = (int)grid;
    hipStream_t st = (hipStream_t)stream;
    // the folded value projection (pdsc_config.value_fold) runs the one-item, peeled form with point-fragment partials, and no other
    AttExperiment x;
    const char* launched = v64 ? "pdsc_sc_attention_split(64-channel values)" : "pdsc_sc_attention_split";
#ifdef PDSC_EXPERIMENTS
    if (!v64) {
        x.trace = nw == 8 && a.trace;
        // A/B knob PDSC_ATT_CREG = 1: fp32 compat values straight into registers (no compat LDS stage)
        if (p.cm == 0 && !x.trace && env_int("PDSC_ATT_CREG", 0) != 0) {
            p.cm = 2;
            p.lds = stage_lds_bytes(nw, p.cm, value_width);
        }
        // A/B knob PDSC_ATT_PERSIST = 1: one workgroup per CU walking its items (point-fragment partials, 8-wave plan, whole
        // multiples of 8 items, at least two per workgroup)
        x.persist = nw == 8 && p.cm != 2 && !x.trace && !nvalid && a.part_frag && (grid & 7) == 0 && grid >= 512 && env_int("PDSC_ATT_PERSIST", 0) != 0;
        if (x.persist) {
            unsigned pgrid = (unsigned)env_int("PDSC_ATT_PERSIST_GRID", 256) & ~7u;      // A/B knob: workgroups (multiple of 8)
            grid = (pgrid < 8 || pgrid > grid) ? 256 : pgrid;
            launched = "pdsc_sc_attention_split(persistent)";
        }
        x.no_peel = !x.persist && !x.trace && nw == 8 && p.cm == 1 && env_int("PDSC_ATT_PEEL", 1) == 0;
    }
#endif
    // The row-order epilogue transposes through one 32 x 132-float patch per wave, which may exceed the two stages.  Point-fragment
    // partials leave straight from the accumulators: the workgroup asks for its two stages only -- 96 KiB with the unorm16
    // matrix -- and leaves the rest of the CU's 160 KiB to other kernels.
    const size_t patch_bytes = (size_t)nw * 32 * (PDSC_CHANNELS * 4 + 16);
    const size_t lds_bytes = (a.part_frag || p.lds > patch_bytes) ? p.lds : patch_bytes;
    int rc = select_instance(nw, p.cm, value_width, false, x)(a, grid, nw * 64, lds_bytes, st, "pdsc_sc_attention_split(dynamic LDS)");
    if (rc != PDSC_OK) return rc;
    rc = check_launch(launched);
    if (rc != PDSC_OK) return rc;
    if (nsplit > 1 && msg) {
        AttArgs c{};
        c.msg = msg; c.part_o = a.part_o; c.part_ml = a.part_ml;
        c.N = N; c.Npad = a.Npad; c.nsplit = nsplit; c.num_tiles = a.num_tiles;
        rc = launch_attention_combine(c, bs, st);
    }
    return rc;
}

extern "C" int pdsc_sc_attention_split(const void* q_split, const void* kv_tiles, const float* compat, long long ld,
                                       float* msg, void* scratch, size_t scratch_bytes, int bs, int N, int nsplit,
                                       void* stream) {
    return launch_attention_split(q_split, kv_tiles, compat, PDSC_COMPAT_F32, ld, msg, scratch, scratch_bytes, bs, N, nsplit, stream);
}

int pdsc::launch_attention_split_ex(const void* q_split, const void* kv_tiles, const void* compat, int compat_format, long long ld,
                                    float* msg, void* scratch, size_t scratch_bytes, int bs, int N, int nsplit, int partial_layout,
                                    const int* nvalid, hipStream_t st, int value_width) {
    // (this entry reports a bad format before anything else; the shared checks would name a null pointer first)
    PDSC_REQUIRE(compat_format == PDSC_COMPAT_F32 || compat_format == PDSC_COMPAT_U16, "pdsc_sc_attention_split: compat_format=%d", compat_format);
    return launch_attention_split(q_split, kv_tiles, compat, compat_format, ld, msg, scratch, scratch_bytes, bs, N, nsplit, st, partial_layout,
                                  nvalid, value_width);
}

extern "C" int pdsc_sc_attention_split_partials(const void* q_split, const void* kv_tiles, const void* compat, int compat_format,
                                                long long ld, void* scratch, size_t scratch_bytes, int bs, int N, int nsplit,
                                                int partial_layout, void* stream) {
    return pdsc::launch_attention_split_ex(q_split, kv_tiles, compat, compat_format, ld, nullptr, scratch, scratch_bytes, bs, N, nsplit,
                                           partial_layout, nullptr, (hipStream_t)stream);
}

extern "C" int pdsc_sc_attention_split_u16(const void* q_split, const void* kv_tiles, const unsigned short* compat_u16,
                                           long long ld, float* msg, void* scratch, size_t scratch_bytes, int bs, int N,
                                           int nsplit, void* stream) {
    return launch_attention_split(q_split, kv_tiles, compat_u16, PDSC_COMPAT_U16, ld, msg, scratch, scratch_bytes, bs, N, nsplit, stream);
}
