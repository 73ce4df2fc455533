// f-8: o3d.registration.global_optimization as the multiway driver calls it (multiway/test_multi_ate.py:166-174, :217-224) on the
// device: Levenberg-Marquardt over the 6 F pose unknowns with the line process on the uncertain edges, edge pruning, second pass.
// The algorithm (the contract of DESIGN.md section 8 f-8 / include/pointdsc_hip.h) is in posegraph_core.h, written against a team
// of threads; here the team is one persistent 512-thread workgroup per graph, which runs both passes and both prunings of its
// graph in one launch and exits on its own.  H, the factor, b, delta, the trial poses, the residuals, the per-edge Jacobians and
// normal blocks and the per-node incidence lists live in the caller's workspace (global memory, L2-resident: 2 x 0.94 MB at
// F = 57); the Cholesky panels live in LDS.  Bound: latency of one workgroup (dependent solves); reported as time only.
#include "pdsc_common.h"
#include "posegraph_core.h"

namespace pdsc {
namespace {

constexpr int PG_NT = 512;
constexpr int PG_NW = PG_NT / PDSC_WAVE;

// fixed-order reductions: per-thread sequential (the caller's loop), wave butterfly, waves in index order
struct BlockTeam {
    int tid, nt;
    double* red;        // [PG_NW] in LDS
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ double sum(double v) const {
        v = wave_sum(v);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < PG_NW; ++w) s += red[w];
        return s;
    }
    __device__ __forceinline__ double maxv(double v) const {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        double s = red[0];
#pragma unroll
        for (int w = 1; w < PG_NW; ++w) s = fmax(s, red[w]);
        return s;
    }
    __device__ __forceinline__ bool any(bool p) const { return __syncthreads_or(p ? 1 : 0) != 0; }
    __device__ __forceinline__ long long clock() const { return (long long)wall_clock64(); }      // constant 100 MHz
};

struct PgLayout {
    size_t H, L, b, delta, poses, trial, zeta, q, Js, em, inc_start, inc, lidx, graph_bytes;
};

inline PgLayout pg_layout(int max_nodes, int max_edges) {
    const long long n = 6LL * max_nodes, E = max_edges > 0 ? max_edges : 1;
    PgLayout L;
    size_t o = 0;
    auto take = [&](long long bytes) { const size_t at = o; o += (size_t)round_up(bytes, 256); return at; };
    L.H = take(n * n * 8);
    L.L = take((n + 1) * n * 8);
    L.b = take(n * 8);
    L.delta = take(n * 8);
    L.poses = take(max_nodes * 16LL * 8);
    L.trial = take(max_nodes * 16LL * 8);
    L.zeta = take(E * 6 * 8);
    L.q = take(E * 8);
    L.Js = take(E * 36 * 8);
    L.em = take(E * pg::EM * 8);
    L.inc_start = take((max_nodes + 1) * 4LL);
    L.inc = take(E * 2 * 4);
    L.lidx = take((E + 1) * 4);
    L.graph_bytes = o;
    return L;
}

inline size_t pg_lds_bytes(int max_nodes) { return (size_t)((6 * max_nodes + 1) * pg::LD + pg::NB * pg::LD) * sizeof(double); }

__global__ __launch_bounds__(PG_NT) void posegraph_kernel(const double* __restrict__ nodes, const int* __restrict__ source,
                                                          const int* __restrict__ target, const double* __restrict__ X,
                                                          const double* __restrict__ info, const unsigned char* __restrict__ uncertain,
                                                          const unsigned char* __restrict__ live_in, const int* __restrict__ node_offset,
                                                          const int* __restrict__ edge_offset, double max_distance, double prune_threshold,
                                                          double preference, int reference, double* __restrict__ nodes_out,
                                                          double* __restrict__ confidence, unsigned char* __restrict__ live_out,
                                                          double* __restrict__ record, long long* __restrict__ ticks, unsigned char* __restrict__ workspace,
                                                          PgLayout lay,
                                                          int max_nodes, int max_edges, int total_nodes, int total_edges) {
    extern __shared__ double pg_lds[];
    __shared__ double red[PG_NW];
    const int gi = blockIdx.x;
    const BlockTeam tm{(int)threadIdx.x, PG_NT, red};
    const int n0 = node_offset[gi], n1 = node_offset[gi + 1], e0 = edge_offset[gi], e1 = edge_offset[gi + 1];
    double* rec = record + (size_t)gi * pg::REC;
    // offsets that leave the arrays: nothing of this graph can be touched but its record
    if (n0 < 0 || n1 < n0 || n1 > total_nodes || e0 < 0 || e1 < e0 || e1 > total_edges) {
        for (int k = tm.tid; k < pg::REC; k += PG_NT) rec[k] = k == 0 ? 1.0 : 0.0;
        return;
    }
    const int F = n1 - n0, E = e1 - e0;
    if (F < 1 || F > max_nodes || E > max_edges) {          // beyond the workspace: invalid, like a NaN
        for (int k = tm.tid; k < pg::REC; k += PG_NT) rec[k] = k == 0 ? 1.0 : 0.0;
        for (int i = tm.tid; i < 16 * F; i += PG_NT) nodes_out[(size_t)n0 * 16 + i] = __builtin_nan("");
        for (int e = tm.tid; e < E; e += PG_NT) {
            live_out[e0 + e] = live_in ? live_in[e0 + e] : 1;
            confidence[e0 + e] = 1.0;
        }
        return;
    }
    unsigned char* wb = workspace + (size_t)gi * lay.graph_bytes;
    pg::Graph g;
    g.F = F; g.E = E;
    g.nodes_in = nodes + (size_t)n0 * 16;
    g.src = source + e0; g.tgt = target + e0;
    g.X = X + (size_t)e0 * 16; g.info = info + (size_t)e0 * 36;
    g.uncertain = uncertain + e0;
    g.live_in = live_in ? live_in + e0 : nullptr;
    g.nodes_out = nodes_out + (size_t)n0 * 16;
    g.conf = confidence + e0; g.live = live_out + e0; g.rec = rec;
    g.ticks = ticks ? ticks + (size_t)gi * 3 : nullptr;
    g.H = reinterpret_cast<double*>(wb + lay.H); g.L = reinterpret_cast<double*>(wb + lay.L);
    g.b = reinterpret_cast<double*>(wb + lay.b); g.delta = reinterpret_cast<double*>(wb + lay.delta);
    g.poses = reinterpret_cast<double*>(wb + lay.poses); g.trial = reinterpret_cast<double*>(wb + lay.trial);
    g.zeta = reinterpret_cast<double*>(wb + lay.zeta); g.q = reinterpret_cast<double*>(wb + lay.q);
    g.Js = reinterpret_cast<double*>(wb + lay.Js); g.em = reinterpret_cast<double*>(wb + lay.em);
    g.inc_start = reinterpret_cast<int*>(wb + lay.inc_start); g.inc = reinterpret_cast<int*>(wb + lay.inc);
    g.lidx = reinterpret_cast<int*>(wb + lay.lidx);
    g.panel = pg_lds; g.dblk = pg_lds + (size_t)(6 * max_nodes + 1) * pg::LD;
    g.max_distance = max_distance; g.prune_threshold = prune_threshold; g.preference = preference; g.reference = reference;
    pg::run_graph(g, tm);
}

__global__ void posegraph_nodes_kernel(const double* __restrict__ X, const unsigned char* __restrict__ uncertain,
                                       const unsigned char* __restrict__ live, const int* __restrict__ node_offset,
                                       const int* __restrict__ edge_offset, double* __restrict__ nodes, int num_graphs, int total_nodes,
                                       int total_edges) {
    const int gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= num_graphs) return;
    const int n0 = node_offset[gi], n1 = node_offset[gi + 1], e0 = edge_offset[gi], e1 = edge_offset[gi + 1];
    if (n0 < 0 || n1 < n0 || n1 > total_nodes || e0 < 0 || e1 < e0 || e1 > total_edges) return;
    pg::node_chain(X + (size_t)e0 * 16, uncertain + e0, live ? live + e0 : nullptr, e1 - e0, n1 - n0, nodes + (size_t)n0 * 16);
}

}  // namespace

size_t posegraph_workspace_bytes(int num_graphs, int max_nodes, int max_edges) {
    if (num_graphs <= 0 || max_nodes <= 0 || max_nodes > PDSC_POSEGRAPH_MAX_NODES || max_edges < 0) return 0;
    return pg_layout(max_nodes, max_edges).graph_bytes * (size_t)num_graphs;
}

int launch_posegraph_nodes(const double* X, const unsigned char* uncertain, const unsigned char* live, const int* node_offset,
                           const int* edge_offset, double* nodes, int num_graphs, int total_nodes, int total_edges, hipStream_t st) {
    PDSC_REQUIRE(X && uncertain && node_offset && edge_offset && nodes, "pdsc_posegraph_nodes: null pointer");
    PDSC_REQUIRE(num_graphs > 0 && num_graphs <= 65535 && total_nodes > 0 && total_edges >= 0,
                 "pdsc_posegraph_nodes: num_graphs=%d total_nodes=%d total_edges=%d", num_graphs, total_nodes, total_edges);
    hipLaunchKernelGGL(posegraph_nodes_kernel, dim3(ceil_div(num_graphs, 64)), dim3(64), 0, st, X, uncertain, live, node_offset,
                       edge_offset, nodes, num_graphs, total_nodes, total_edges);
    return check_launch("pdsc_posegraph_nodes");
}

int launch_global_optimization(const double* nodes, const int* source, const int* target, const double* X, const double* info,
                               const unsigned char* uncertain, const unsigned char* live_in, const int* node_offset,
                               const int* edge_offset, double max_distance, double prune_threshold, double preference, int reference,
                               double* nodes_out, double* confidence, unsigned char* live_out, double* record, long long* ticks,
                               void* workspace, size_t workspace_bytes, int num_graphs, int max_nodes, int max_edges, int total_nodes, int total_edges,
                               hipStream_t st) {
    PDSC_REQUIRE(nodes && source && target && X && info && uncertain && node_offset && edge_offset && nodes_out && confidence &&
                     live_out && record && workspace,
                 "pdsc_global_optimization: null pointer");
    PDSC_REQUIRE(num_graphs > 0 && num_graphs <= 65535 && max_nodes > 0 && max_nodes <= PDSC_POSEGRAPH_MAX_NODES && max_edges >= 0 &&
                     max_edges <= (1 << 20) && total_nodes > 0 && total_edges >= 0,
                 "pdsc_global_optimization: num_graphs=%d max_nodes=%d (1..%d) max_edges=%d total_nodes=%d total_edges=%d", num_graphs,
                 max_nodes, PDSC_POSEGRAPH_MAX_NODES, max_edges, total_nodes, total_edges);
    PDSC_REQUIRE(nodes != nodes_out, "pdsc_global_optimization: nodes_out must not alias nodes");
    PDSC_REQUIRE(!isnan(max_distance) && !isnan(prune_threshold) && !isnan(preference),
                 "pdsc_global_optimization: NaN option");
    PDSC_REQUIRE(reference >= 0 && reference < max_nodes, "pdsc_global_optimization: reference_node=%d outside [0, %d)", reference,
                 max_nodes);
    const PgLayout lay = pg_layout(max_nodes, max_edges);
    PDSC_REQUIRE(workspace_bytes >= lay.graph_bytes * (size_t)num_graphs, "pdsc_global_optimization: workspace %zu bytes < %zu",
                 workspace_bytes, lay.graph_bytes * (size_t)num_graphs);
    const size_t lds = pg_lds_bytes(max_nodes);
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&posegraph_kernel), lds, "pdsc_global_optimization(dynamic LDS)");
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL(posegraph_kernel, dim3(num_graphs), dim3(PG_NT), lds, st, nodes, source, target, X, info, uncertain, live_in,
                       node_offset, edge_offset, max_distance, prune_threshold, preference, reference, nodes_out, confidence, live_out,
                       record, ticks, (unsigned char*)workspace, lay, max_nodes, max_edges, total_nodes, total_edges);
    return check_launch("pdsc_global_optimization");
}

}  // namespace pdsc

extern "C" size_t pdsc_posegraph_workspace_bytes(int num_graphs, int max_nodes, int max_edges) {
    return pdsc::posegraph_workspace_bytes(num_graphs, max_nodes, max_edges);
}

extern "C" int pdsc_posegraph_nodes(const double* X, const unsigned char* uncertain, const unsigned char* live, const int* node_offset,
                                    const int* edge_offset, double* nodes, int num_graphs, int total_nodes, int total_edges,
                                    void* stream) {
    return pdsc::launch_posegraph_nodes(X, uncertain, live, node_offset, edge_offset, nodes, num_graphs, total_nodes, total_edges,
                                        (hipStream_t)stream);
}

extern "C" int pdsc_global_optimization(const double* nodes, const int* source, const int* target, const double* X, const double* info,
                                        const unsigned char* uncertain, const unsigned char* live_in, const int* node_offset,
                                        const int* edge_offset, double max_correspondence_distance, double edge_prune_threshold,
                                        double preference_loop_closure, int reference_node, double* nodes_out, double* confidence,
                                        unsigned char* live_out, double* record, long long* ticks, void* workspace,
                                        size_t workspace_bytes, int num_graphs, int max_nodes, int max_edges, int total_nodes,
                                        int total_edges, void* stream) {
    return pdsc::launch_global_optimization(nodes, source, target, X, info, uncertain, live_in, node_offset, edge_offset,
                                            max_correspondence_distance, edge_prune_threshold, preference_loop_closure, reference_node,
                                            nodes_out, confidence, live_out, record, ticks, workspace, workspace_bytes, num_graphs,
                                            max_nodes, max_edges, total_nodes, total_edges, (hipStream_t)stream);
}
