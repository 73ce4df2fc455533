// f-10: the PMC baseline, i.e. the exact maximum clique of the compatibility graph of
//   reference baseline_scripts/baseline_3DMatch.py:56-77 (PMC):
//     edge (i, j), i > j  <=>  |sum((c_i[0:3] - c_j[0:3])**2) - sum((c_i[3:6] - c_j[3:6])**2)| < inlier_threshold     (c = corr[0], fp32;
//                              SQUARED distances, as the reference writes it)
//     pred_labels = 1 on a maximum clique;  pred_trans = rigid_transform_3d(src_keypts, tgt_keypts, pred_labels)
// The reference builds the edge list in a Python double loop and hands it to a libpmc.so it does not ship.  Here:
//   pmc_adjacency_kernel : N x N edge rule -> row-major bitset (one wave ballot per 64 columns); run twice, the second time with the
//                          vertices renumbered by the search order (the rule is re-evaluated, nothing is permuted bit by bit)
//   pmc_degree_kernel    : row popcounts
//   pmc_order_kernel     : position of every vertex in the order (degree descending, index ascending), by counting
//   pmc_greedy_kernel    : one wave per start vertex: repeatedly take the first (= highest-degree) common neighbour
//   pmc_bound_kernel     : lower bound = the largest greedy clique (ties: first start vertex in the order)
//   pmc_search_kernel    : one single-wave workgroup per root.  Root q owns the cliques whose LAST member in the order is q: its
//                          candidates are q's neighbours earlier in the order, renumbered 0 .. n_loc - 1; their adjacency is an
//                          n_loc x n_loc bit matrix and every candidate set of the depth-first search a bitset over n_loc (lane l
//                          holds word l).  Bound: greedy sequential colouring (Tomita / San Segundo); only vertices whose colour
//                          exceeds (incumbent - current size) are branched on.  The incumbent is PRIVATE: it starts at the bound
//                          fixed by pmc_bound_kernel and only this root's own finds raise it, so a root's result and its node
//                          count are functions of the inputs alone.  Matrix and stack live in LDS when they fit (48 KiB pool);
//   pmc_search_slab_kernel: ... the roots that did not fit are searched again from scratch by a few workgroups that own a slab of
//                          the workspace each (same code through generic pointers).
//   pmc_finish_kernel    : winner by (size, then root position in the order; the greedy clique wins a tie against any root),
//                          labels, clique_size, proven, counters
//   pdsc_rigid_transform_3d with the 0/1 labels as weights.
// Every loop has a trip count bounded by N, n_loc, the stack depth or max_nodes; no workgroup waits for another one.
#include "pdsc_common.h"

namespace pdsc {

typedef unsigned long long u64;

constexpr int PMC_MAX_N = 16384;                     // 256 words per row: 4 per lane in the greedy kernel
constexpr int PMC_KW = PMC_MAX_N / 64 / 64;
constexpr int PMC_MAX_LOCAL = 4096;                  // candidates of one root: one 64-bit word per lane
constexpr int PMC_MAX_DEPTH = 1024;                  // stack levels (= an upper bound of the clique size a root may look for, minus one)
constexpr int PMC_POOL_WORDS = 6144;                 // 48 KiB of LDS per workgroup for the local matrix and the stack
constexpr int PMC_SLAB_WGS = 64;                     // workgroups (per pair) of the slab pass
constexpr int PMC_SLAB_NODE_COST = 8;                // what a node of the slab pass is charged against max_nodes (its matrix and stack are
                                                     // behind the L2, not in LDS: every colouring step waits for a global load)
enum { PMC_ST_DONE = 0, PMC_ST_BUDGET = 1, PMC_ST_SLAB = 2, PMC_ST_UNSERVED = 3 };

// byte offsets of the workspace arrays (every array is [bs] x its per-pair size)
struct PmcLayout {
    size_t info, bits, pbits, cliq, deg, perm, gsize, lb, rsize, rstat, rnodes, slab, total;
    size_t slab_words;      // u64 words of one slab
    int W;                  // words per adjacency row
    int nl_max;             // candidates a slab can serve
};

static PmcLayout pmc_layout(int bs, int N) {
    PmcLayout L{};
    const size_t W = (size_t)(N + 63) / 64, B = (size_t)bs, n = (size_t)N;
    L.W = (int)W;
    L.nl_max = N - 1 < PMC_MAX_LOCAL ? (N > 1 ? N - 1 : 1) : PMC_MAX_LOCAL;
    const size_t wl = (size_t)(L.nl_max + 63) / 64;
    const size_t levels = (size_t)(L.nl_max < PMC_MAX_DEPTH ? L.nl_max : PMC_MAX_DEPTH) + 1;
    L.slab_words = (size_t)L.nl_max * wl + 2 * wl * levels;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
    L.info = take(B * 4 * sizeof(long long));
    L.bits = take(B * n * W * 8);
    L.pbits = take(B * n * W * 8);
    L.cliq = take(B * n * W * 8);
    L.deg = take(B * n * 4);
    L.perm = take(B * n * 4);
    L.gsize = take(B * n * 4);
    L.lb = take(B * 2 * 4);
    L.rsize = take(B * n * 4);
    L.rstat = take(B * n * 4);
    L.rnodes = take(B * n * 4);
    L.slab = take(B * PMC_SLAB_WGS * L.slab_words * 8);
    L.total = o;
    return L;
}

__device__ __forceinline__ u64 pmc_shfl64(u64 v, int src) {
    const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ int pmc_wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
// first / last member of a bitset held one word per lane (-1: empty); wave-uniform
__device__ __forceinline__ int pmc_first(u64 w) {
    const u64 m = __builtin_amdgcn_ballot_w64(w != 0ull);
    if (m == 0ull) return -1;
    const int l = __builtin_ctzll(m);
    return l * 64 + __builtin_ctzll(pmc_shfl64(w, l));
}
__device__ __forceinline__ int pmc_last(u64 w) {
    const u64 m = __builtin_amdgcn_ballot_w64(w != 0ull);
    if (m == 0ull) return -1;
    const int l = 63 - __builtin_clzll(m);
    return l * 64 + 63 - __builtin_clzll(pmc_shfl64(w, l));
}

// bits[b][i][w] bit l = edge(v(i), v(64 w + l)), v = perm (or the identity).  grid (ld_words, ceil(N / 64), bs), 256 threads:
// a wave owns one word of 16 rows.
__global__ __launch_bounds__(256) void pmc_adjacency_kernel(const float* __restrict__ corr, const int* __restrict__ perm, float thr,
                                                            u64* __restrict__ bits, long long ld_words, int N) {
    const int b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* c = corr + (size_t)b * N * 6;
    const int* pm = perm ? perm + (size_t)b * N : nullptr;
    u64* out = bits + (size_t)b * N * ld_words;
    const int w = blockIdx.x;
    const int j = w * 64 + lane;
    float cj[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (j < N) {
        const int vj = pm ? pm[j] : j;
#pragma unroll
        for (int d = 0; d < 6; ++d) cj[d] = c[(size_t)vj * 6 + d];
    }
    const int i0 = (blockIdx.y * 4 + wave) * 16;
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + r;
        if (i >= N) break;                                                   // wave-uniform
        const int vi = pm ? pm[i] : i;
        float ci[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) ci[d] = c[(size_t)vi * 6 + d];
        const float ax = ci[0] - cj[0], ay = ci[1] - cj[1], az = ci[2] - cj[2];
        const float bx = ci[3] - cj[3], by = ci[4] - cj[4], bz = ci[5] - cj[5];
        const float s1 = (ax * ax + ay * ay) + az * az;                      // np.sum of three fp32 terms, left to right
        const float s2 = (bx * bx + by * by) + bz * bz;
        const bool edge = j < N && j != i && fabsf(s1 - s2) < thr;
        const u64 word = __builtin_amdgcn_ballot_w64(edge);
        if (lane == 0) out[(size_t)i * ld_words + w] = word;
    }
}

// one wave per row
__global__ __launch_bounds__(256) void pmc_degree_kernel(const u64* __restrict__ bits, int* __restrict__ deg, int W, int N) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const u64* row = bits + ((size_t)b * N + i) * W;
    int s = 0;
    for (int w = lane; w < W; w += 64) s += __popcll(row[w]);
    s = wave_sum(s);
    if (lane == 0) deg[(size_t)b * N + i] = s;
}

// perm[position of i] = i, position = #{j : deg_j > deg_i or (deg_j == deg_i and j < i)}; one wave per vertex
__global__ __launch_bounds__(256) void pmc_order_kernel(const int* __restrict__ deg, int* __restrict__ perm, int N) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const int* dg = deg + (size_t)b * N;
    const int di = dg[i];
    int cnt = 0;
    for (int j = lane; j < N; j += 64) {
        const int dj = dg[j];
        cnt += (dj > di) || (dj == di && j < i);
    }
    cnt = wave_sum(cnt);
    if (lane == 0) perm[(size_t)b * N + cnt] = i;
}

// Greedy clique from start vertex q (ids = positions in the order): P = N(q); take the first member u of P, P &= N(u), until P is
// empty.  One wave; returns the size (wave-uniform).  `mark` (optional, W words, cleared by the caller, any address space) receives
// the clique's members.
__device__ int pmc_greedy(const u64* __restrict__ rows, int W, int N, int q, u64* mark) {
    const int lane = threadIdx.x & 63;
    u64 P[PMC_KW];
#pragma unroll
    for (int k = 0; k < PMC_KW; ++k) {
        const int w = lane + 64 * k;
        P[k] = w < W ? rows[(size_t)q * W + w] : 0ull;
    }
    if (mark && lane == 0) mark[q >> 6] |= 1ull << (q & 63);
    int size = 1;
    for (int step = 0; step < N; ++step) {
        int myw = 0x7fffffff;
#pragma unroll
        for (int k = PMC_KW - 1; k >= 0; --k)
            if (P[k] != 0ull) myw = lane + 64 * k;
        const int wmin = pmc_wave_min(myw);
        if (wmin == 0x7fffffff) break;
        u64 word = 0ull;
#pragma unroll
        for (int k = 0; k < PMC_KW; ++k)
            if (lane + 64 * k == wmin) word = P[k];
        word = pmc_shfl64(word, wmin & 63);
        const int u = wmin * 64 + __builtin_ctzll(word);
        ++size;
        if (mark && lane == 0) mark[u >> 6] |= 1ull << (u & 63);
#pragma unroll
        for (int k = 0; k < PMC_KW; ++k) {
            const int w = lane + 64 * k;
            if (w < W) P[k] &= rows[(size_t)u * W + w];
        }
    }
    return size;
}

__global__ __launch_bounds__(256) void pmc_greedy_kernel(const u64* __restrict__ pbits, int* __restrict__ gsize, int W, int N) {
    const int b = blockIdx.y;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= N) return;
    const int s = pmc_greedy(pbits + (size_t)b * N * W, W, N, q, nullptr);
    if ((threadIdx.x & 63) == 0) gsize[(size_t)b * N + q] = s;
}

// lb[b] = {largest greedy size, the first start vertex that reaches it}; one workgroup per pair
__global__ __launch_bounds__(256) void pmc_bound_kernel(const int* __restrict__ gsize, int* __restrict__ lb, int N) {
    __shared__ int ss[256], sq[256];
    const int b = blockIdx.x, t = threadIdx.x;
    int bs = 0, bq = 0x7fffffff;
    for (int q = t; q < N; q += 256) {
        const int s = gsize[(size_t)b * N + q];
        if (s > bs) { bs = s; bq = q; }                                      // ascending q per thread: the first one stays
    }
    ss[t] = bs; sq[t] = bq;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
            const int s2 = ss[t + off], q2 = sq[t + off];
            if (s2 > ss[t] || (s2 == ss[t] && q2 < sq[t])) { ss[t] = s2; sq[t] = q2; }
        }
        __syncthreads();
    }
    if (t == 0) { lb[b * 2] = ss[0]; lb[b * 2 + 1] = sq[0]; }
}

struct PmcLds {
    u64 pool[PMC_POOL_WORDS];
    unsigned short l2g[PMC_MAX_LOCAL];
    unsigned short cur[PMC_MAX_DEPTH + 1];
    unsigned short bestp[PMC_MAX_DEPTH + 1];
};

// Branch and bound below root q by the calling wave (a whole 64-thread workgroup).  slab == nullptr: matrix and stack in the LDS pool,
// a root that does not fit gets status PMC_ST_SLAB; otherwise they live in the slab and a root that does not fit is PMC_ST_UNSERVED.
// One NODE = one branching step: a vertex joins the current clique and the child's candidate set is formed.
// pool_words: the part of the LDS pool that may be used (tests shrink it to send every root through the slab pass).  Returns the nodes expanded.
__device__ int pmc_search_root(const PmcLayout& L, char* ws, PmcLds& S, u64* slab, int b, int q, int N, int max_nodes, int pool_words) {
    const int lane = threadIdx.x & 63, W = L.W;
    const u64* rows = reinterpret_cast<const u64*>(ws + L.pbits) + (size_t)b * N * W;
    int* rsize = reinterpret_cast<int*>(ws + L.rsize) + (size_t)b * N;
    int* rstat = reinterpret_cast<int*>(ws + L.rstat) + (size_t)b * N;
    int* rnodes = reinterpret_cast<int*>(ws + L.rnodes) + (size_t)b * N;
    const int lb = reinterpret_cast<const int*>(ws + L.lb)[b * 2];

    // candidates: q's neighbours at positions < q
    u64 F[PMC_KW];
    int cntk[PMC_KW];
    int n_loc = 0;
#pragma unroll
    for (int k = 0; k < PMC_KW; ++k) {
        const int w = lane + 64 * k;
        u64 x = w < W ? rows[(size_t)q * W + w] : 0ull;
        if (w * 64 + 63 >= q) x = (w * 64 < q) ? (x & ((1ull << (q & 63)) - 1ull)) : 0ull;      // (w*64 < q <= w*64+63: q & 63 == q - 64 w; == 0 gives 0)
        F[k] = x;
        cntk[k] = wave_sum((int)__popcll(x));
        n_loc += cntk[k];
    }
    int status = PMC_ST_BUDGET, nodes = 0, best = lb, bestd = 0;
    bool run = true;
    if (n_loc + 1 <= lb) { status = PMC_ST_DONE; run = false; }              // cannot hold a clique larger than the bound
    const int Wl = (n_loc + 63) / 64;
    u64* mat = slab ? slab : S.pool;
    int levels = 0;
    if (run) {
        const int nl_cap = slab ? L.nl_max : PMC_MAX_LOCAL;
        const size_t words = slab ? L.slab_words : (size_t)pool_words;
        if (n_loc > nl_cap || n_loc > PMC_MAX_LOCAL) { status = PMC_ST_UNSERVED; run = false; }
        else if ((size_t)n_loc * Wl + 4 * (size_t)Wl > words) { status = slab ? PMC_ST_UNSERVED : PMC_ST_SLAB; run = false; }
        else {
            const size_t lv = (words - (size_t)n_loc * Wl) / (2 * (size_t)Wl);
            levels = lv > (size_t)PMC_MAX_DEPTH ? PMC_MAX_DEPTH : (int)lv;    // >= 2
        }
    }
    if (run) {
        // local index -> position: the set bits of F in ascending order
        __syncthreads();                                                     // (the previous root of this workgroup is done with the LDS)
        int base = 0;
#pragma unroll
        for (int k = 0; k < PMC_KW; ++k) {
            const int mine = (int)__popcll(F[k]);
            int incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            int pos = base + incl - mine;
            u64 x = F[k];
            const int w = lane + 64 * k;
            for (int e = 0; e < 64; ++e) {
                if (x == 0ull) break;
                const int bit = __builtin_ctzll(x);
                x &= x - 1ull;
                if (pos < PMC_MAX_LOCAL) S.l2g[pos] = (unsigned short)(w * 64 + bit);
                ++pos;
            }
            base += cntk[k];
        }
        __syncthreads();
        // local adjacency matrix: row a, word wl
        for (int wl = 0; wl < Wl; ++wl) {
            const int bi = wl * 64 + lane;
            const int gb = bi < n_loc ? (int)S.l2g[bi] : -1;
            for (int a = 0; a < n_loc; ++a) {
                const int ga = S.l2g[a];
                bool bit = false;
                if (gb >= 0) bit = (rows[(size_t)ga * W + (gb >> 6)] >> (gb & 63)) & 1ull;
                const u64 word = __builtin_amdgcn_ballot_w64(bit);
                if (lane == 0) mat[(size_t)a * Wl + wl] = word;
            }
        }
        __syncthreads();
        u64* stk = mat + (size_t)n_loc * Wl;                                 // level d: P at (2 d) Wl, B at (2 d + 1) Wl; lane l owns word l of both
        u64 Pw = 0ull;
        if (lane < Wl) Pw = (lane * 64 + 64 <= n_loc) ? ~0ull : ((1ull << (n_loc - lane * 64)) - 1ull);
        int d = 0, s = 1, mode = 0;
        const long long cap = 4ll * max_nodes + 8;
        for (long long it = 0; it < cap; ++it) {
            if (mode == 0) {                                                 // ---- expand the node (clique of s, candidates Pw) at level d
                if (s > best) {
                    best = s; bestd = d;
                    __syncthreads();
                    for (int i = lane; i < d; i += 64) S.bestp[i] = S.cur[i];
                    __syncthreads();
                }
                const int cnt = wave_sum((int)__popcll(Pw));
                if (cnt == 0 || s + cnt <= best) { mode = 2; continue; }
                const int k = best - s;                                      // colours 1 .. k cannot lift a clique above the incumbent
                u64 U = Pw, Bw = 0ull;
                int c = 0;
                for (int ci = 0; ci < n_loc; ++ci) {
                    if (__builtin_amdgcn_ballot_w64(U != 0ull) == 0ull) break;
                    ++c;
                    u64 Q = U;
                    for (int vi = 0; vi < n_loc; ++vi) {
                        const int v = pmc_first(Q);
                        if (v < 0) break;
                        const u64 r = lane < Wl ? mat[(size_t)v * Wl + lane] : 0ull;
                        Q &= ~r;
                        if (lane == (v >> 6)) {
                            const u64 m = 1ull << (v & 63);
                            Q &= ~m; U &= ~m;
                            if (c > k) Bw |= m;
                        }
                    }
                }
                if (d == 0 && min(n_loc, c) + 1 > levels) {                  // a clique of c candidates would need c + 1 levels
                    status = slab ? PMC_ST_UNSERVED : PMC_ST_SLAB;
                    run = false;
                    break;
                }
                if (__builtin_amdgcn_ballot_w64(Bw != 0ull) == 0ull) { mode = 2; continue; }
                if (lane < Wl) {
                    stk[(size_t)(2 * d) * Wl + lane] = Pw;
                    stk[(size_t)(2 * d + 1) * Wl + lane] = Bw;
                }
                mode = 1;
                continue;
            }
            if (mode == 1) {                                                 // ---- next branching vertex of level d
                u64 Bw = 0ull;
                Pw = 0ull;
                if (lane < Wl) {
                    Pw = stk[(size_t)(2 * d) * Wl + lane];
                    Bw = stk[(size_t)(2 * d + 1) * Wl + lane];
                }
                const int cnt = wave_sum((int)__popcll(Pw));
                const int v = pmc_last(Bw);
                if (v < 0 || s + cnt <= best) { mode = 2; continue; }
                if (nodes >= max_nodes) break;                               // status stays PMC_ST_BUDGET
                if (d + 2 > levels) {                                        // never taken after the check at the root; guards the stack
                    status = slab ? PMC_ST_UNSERVED : PMC_ST_SLAB;
                    run = false;
                    break;
                }
                ++nodes;
                if (lane == (v >> 6)) {
                    const u64 m = 1ull << (v & 63);
                    Pw &= ~m; Bw &= ~m;
                    stk[(size_t)(2 * d) * Wl + lane] = Pw;
                    stk[(size_t)(2 * d + 1) * Wl + lane] = Bw;
                }
                if (lane == 0) S.cur[d] = (unsigned short)v;
                Pw &= lane < Wl ? mat[(size_t)v * Wl + lane] : 0ull;
                ++d; ++s;
                mode = 0;
                continue;
            }
            if (d == 0) { status = PMC_ST_DONE; break; }                     // ---- back to the parent
            --d; --s;
            mode = 1;
        }
    }
    const bool found = run && best > lb;
    if (found) {                                                             // the clique: q and the recorded path, as positions
        u64* out = reinterpret_cast<u64*>(ws + L.cliq) + ((size_t)b * N + q) * W;
        for (int w = lane; w < W; w += 64) out[w] = 0ull;
        __syncthreads();
        if (lane == 0) atomicOr(out + (q >> 6), 1ull << (q & 63));
        for (int i = lane; i < bestd; i += 64) {
            const int g = S.l2g[S.bestp[i]];
            atomicOr(out + (g >> 6), 1ull << (g & 63));
        }
    }
    if (lane == 0) {
        rsize[q] = found ? best : 0;
        rstat[q] = status;
        rnodes[q] = run ? nodes : 0;
    }
    return nodes;
}

__global__ __launch_bounds__(64) void pmc_search_kernel(char* ws, PmcLayout L, int N, int max_nodes, int pool_words) {
    __shared__ PmcLds S;
    pmc_search_root(L, ws, S, nullptr, blockIdx.y, blockIdx.x, N, max_nodes, pool_words);
}

// Workgroup g of a pair serves the roots q = g, g + 64, ... that the first pass left with PMC_ST_SLAB, in ascending order, and all of
// them share ONE budget of max_nodes, a node being charged PMC_SLAB_NODE_COST: the assignment is static, so this is as deterministic
// as the first pass, and the pass ends after max_nodes / 8 of its slow nodes however many such roots there are.  Roots the budget
// does not reach stay "not exhausted".
__global__ __launch_bounds__(64) void pmc_search_slab_kernel(char* ws, PmcLayout L, int N, int max_nodes) {
    __shared__ PmcLds S;
    const int b = blockIdx.y;
    u64* slab = reinterpret_cast<u64*>(ws + L.slab) + ((size_t)b * PMC_SLAB_WGS + blockIdx.x) * L.slab_words;
    int* rstat = reinterpret_cast<int*>(ws + L.rstat) + (size_t)b * N;
    int left = max_nodes / PMC_SLAB_NODE_COST;
    for (int q = blockIdx.x; q < N; q += PMC_SLAB_WGS) {
        if (rstat[q] != PMC_ST_SLAB) continue;                               // (workgroup-uniform; only this workgroup writes rstat[q])
        if (left <= 0) {
            if (threadIdx.x == 0) rstat[q] = PMC_ST_BUDGET;                  // (size 0 and nodes 0 were written by the first pass)
            continue;
        }
        left -= pmc_search_root(L, ws, S, slab, b, q, N, left, 0);
    }
}

// winner, labels, clique_size, proven, counters; one workgroup per pair
__global__ __launch_bounds__(256) void pmc_finish_kernel(char* ws, PmcLayout L, float* __restrict__ labels, int* __restrict__ clique_size,
                                                         int* __restrict__ proven, int N) {
    __shared__ int ss[256], sq[256], sbad[256];
    __shared__ long long sn[256], sc[256];
    __shared__ u64 sel[PMC_MAX_N / 64];
    const int b = blockIdx.x, t = threadIdx.x, W = L.W;
    const int* rsize = reinterpret_cast<const int*>(ws + L.rsize) + (size_t)b * N;
    const int* rstat = reinterpret_cast<const int*>(ws + L.rstat) + (size_t)b * N;
    const int* rnodes = reinterpret_cast<const int*>(ws + L.rnodes) + (size_t)b * N;
    const int* perm = reinterpret_cast<const int*>(ws + L.perm) + (size_t)b * N;
    const int* lb = reinterpret_cast<const int*>(ws + L.lb) + b * 2;
    const u64* rows = reinterpret_cast<const u64*>(ws + L.pbits) + (size_t)b * N * W;
    int bs = 0, bq = 0x7fffffff, bad = 0;
    long long nn = 0, searched = 0;
    for (int q = t; q < N; q += 256) {
        const int s = rsize[q];
        if (s > bs) { bs = s; bq = q; }
        bad += rstat[q] != PMC_ST_DONE;
        nn += rnodes[q];
        searched += rnodes[q] > 0;
    }
    ss[t] = bs; sq[t] = bq; sbad[t] = bad; sn[t] = nn; sc[t] = searched;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
            const int s2 = ss[t + off], q2 = sq[t + off];
            if (s2 > ss[t] || (s2 == ss[t] && q2 < sq[t])) { ss[t] = s2; sq[t] = q2; }
            sbad[t] += sbad[t + off]; sn[t] += sn[t + off]; sc[t] += sc[t + off];
        }
        __syncthreads();
    }
    const int win = ss[0], winq = sq[0];                                      // win > lb[0] or 0
    for (int w = t; w < W; w += 256) sel[w] = win > 0 ? (reinterpret_cast<const u64*>(ws + L.cliq) + ((size_t)b * N + winq) * W)[w] : 0ull;
    __syncthreads();
    if (win == 0 && t < 64) pmc_greedy(rows, W, N, lb[1], sel);               // (first wave; the greedy clique again, members marked)
    __syncthreads();
    for (int q = t; q < N; q += 256) labels[(size_t)b * N + perm[q]] = (sel[q >> 6] >> (q & 63)) & 1ull ? 1.0f : 0.0f;
    if (t == 0) {
        clique_size[b] = win > 0 ? win : lb[0];
        proven[b] = sbad[0] == 0;
        long long* info = reinterpret_cast<long long*>(ws + L.info) + (size_t)b * 4;
        info[0] = sn[0]; info[1] = sc[0]; info[2] = sbad[0]; info[3] = lb[0];
    }
}

}  // namespace pdsc

using namespace pdsc;

extern "C" int pdsc_pmc_adjacency(const float* corr_pos, float inlier_threshold, unsigned long long* bits, long long ld_words, int bs, int N,
                                  void* stream) {
    PDSC_REQUIRE(corr_pos && bits, "pdsc_pmc_adjacency: null pointer");
    PDSC_REQUIRE(bs > 0 && bs <= 65535 && N > 0 && N <= PMC_MAX_N && ld_words >= (N + 63) / 64 && ld_words <= 65535,
                 "pdsc_pmc_adjacency: bs=%d N=%d ld_words=%lld (1 <= N <= %d, ld_words >= ceil(N / 64))", bs, N, ld_words, PMC_MAX_N);
    hipLaunchKernelGGL(pmc_adjacency_kernel, dim3((unsigned)ld_words, ceil_div(N, 64), bs), dim3(256), 0, (hipStream_t)stream, corr_pos,
                       (const int*)nullptr, inlier_threshold, bits, ld_words, N);
    return check_launch("pdsc_pmc_adjacency");
}

extern "C" size_t pdsc_pmc_workspace_bytes(int bs, int N) {
    if (bs <= 0 || bs > 65535 || N <= 0 || N > PMC_MAX_N) return 0;
    return pmc_layout(bs, N).total;
}

// stage_ms (host, optional): milliseconds of {adjacency, ordering and bound, search, labels and Procrustes} between events on the
// stream; asking for them synchronises the host at the end (tools/pmc_bench.py)
static int pmc_baseline_impl(const float* corr_pos, const float* src_keypts, const float* tgt_keypts, float inlier_threshold,
                             int max_nodes, float* pred_trans, float* pred_labels, int* clique_size, int* proven, void* workspace,
                             size_t workspace_bytes, int bs, int N, void* stream, int lds_words, float* stage_ms) {
    PDSC_REQUIRE(corr_pos && src_keypts && tgt_keypts && pred_trans && pred_labels && clique_size && proven && workspace,
                 "pdsc_pmc_baseline: null pointer");
    PDSC_REQUIRE(bs > 0 && bs <= 65535 && N > 0 && N <= PMC_MAX_N, "pdsc_pmc_baseline: bs=%d N=%d (1 <= N <= %d)", bs, N, PMC_MAX_N);
    PDSC_REQUIRE(max_nodes >= 1 && max_nodes <= (1 << 30), "pdsc_pmc_baseline: max_nodes=%d (1 .. 2^30: the budget is mandatory and finite)",
                 max_nodes);
    const PmcLayout L = pmc_layout(bs, N);
    if (workspace_bytes < L.total) {
        set_error("pdsc_pmc_baseline: workspace %zu < %zu bytes", workspace_bytes, L.total);
        return PDSC_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int W = L.W;
    u64* bits = (u64*)(ws + L.bits);
    u64* pbits = (u64*)(ws + L.pbits);
    int* deg = (int*)(ws + L.deg);
    int* perm = (int*)(ws + L.perm);
    int* gsize = (int*)(ws + L.gsize);
    int* lb = (int*)(ws + L.lb);
    const dim3 rows4(ceil_div(N, 4), bs);
    int rc;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    auto mark = [&](int i) -> int {
        if (!stage_ms) return PDSC_OK;
        if (hipEventCreate(&ev[i]) != hipSuccess || hipEventRecord(ev[i], st) != hipSuccess) {
            (void)hipGetLastError();
            set_error("pdsc_pmc_baseline_ex: event %d failed", i);
            return PDSC_ERR_LAUNCH;
        }
        return PDSC_OK;
    };
    auto drop = [&]() {
        for (int i = 0; i < 5; ++i)
            if (ev[i]) (void)hipEventDestroy(ev[i]);
    };
    auto run = [&]() -> int {
        if ((rc = mark(0)) != PDSC_OK) return rc;
        hipLaunchKernelGGL(pmc_adjacency_kernel, dim3(W, ceil_div(N, 64), bs), dim3(256), 0, st, corr_pos, (const int*)nullptr, inlier_threshold,
                           bits, (long long)W, N);
        if ((rc = check_launch("pdsc_pmc_baseline(adjacency)")) != PDSC_OK) return rc;
        if ((rc = mark(1)) != PDSC_OK) return rc;
        hipLaunchKernelGGL(pmc_degree_kernel, rows4, dim3(256), 0, st, bits, deg, W, N);
        if ((rc = check_launch("pdsc_pmc_baseline(degree)")) != PDSC_OK) return rc;
        hipLaunchKernelGGL(pmc_order_kernel, rows4, dim3(256), 0, st, deg, perm, N);
        if ((rc = check_launch("pdsc_pmc_baseline(order)")) != PDSC_OK) return rc;
        hipLaunchKernelGGL(pmc_adjacency_kernel, dim3(W, ceil_div(N, 64), bs), dim3(256), 0, st, corr_pos, (const int*)perm, inlier_threshold,
                           pbits, (long long)W, N);
        if ((rc = check_launch("pdsc_pmc_baseline(ordered adjacency)")) != PDSC_OK) return rc;
        hipLaunchKernelGGL(pmc_greedy_kernel, rows4, dim3(256), 0, st, pbits, gsize, W, N);
        if ((rc = check_launch("pdsc_pmc_baseline(greedy)")) != PDSC_OK) return rc;
        hipLaunchKernelGGL(pmc_bound_kernel, dim3(bs), dim3(256), 0, st, gsize, lb, N);
        if ((rc = check_launch("pdsc_pmc_baseline(bound)")) != PDSC_OK) return rc;
        if ((rc = mark(2)) != PDSC_OK) return rc;
        hipLaunchKernelGGL(pmc_search_kernel, dim3(N, bs), dim3(64), 0, st, ws, L, N, max_nodes, lds_words);
        if ((rc = check_launch("pdsc_pmc_baseline(search)")) != PDSC_OK) return rc;
        hipLaunchKernelGGL(pmc_search_slab_kernel, dim3(PMC_SLAB_WGS, bs), dim3(64), 0, st, ws, L, N, max_nodes);
        if ((rc = check_launch("pdsc_pmc_baseline(slab search)")) != PDSC_OK) return rc;
        if ((rc = mark(3)) != PDSC_OK) return rc;
        hipLaunchKernelGGL(pmc_finish_kernel, dim3(bs), dim3(256), 0, st, ws, L, pred_labels, clique_size, proven, N);
        if ((rc = check_launch("pdsc_pmc_baseline(finish)")) != PDSC_OK) return rc;
        if ((rc = pdsc_rigid_transform_3d(src_keypts, tgt_keypts, pred_labels, 0.0f, pred_trans, bs, N, stream)) != PDSC_OK) return rc;
        return mark(4);
    };
    rc = run();
    if (rc == PDSC_OK && stage_ms) {
        if (hipEventSynchronize(ev[4]) != hipSuccess) {
            (void)hipGetLastError();
            set_error("pdsc_pmc_baseline_ex: hipEventSynchronize failed");
            rc = PDSC_ERR_LAUNCH;
        }
        for (int i = 0; i < 4 && rc == PDSC_OK; ++i)
            if (hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]) != hipSuccess) {
                (void)hipGetLastError();
                set_error("pdsc_pmc_baseline_ex: hipEventElapsedTime failed");
                rc = PDSC_ERR_LAUNCH;
            }
    }
    drop();
    return rc;
}

extern "C" int pdsc_pmc_baseline(const float* corr_pos, const float* src_keypts, const float* tgt_keypts, float inlier_threshold,
                                 int max_nodes, float* pred_trans, float* pred_labels, int* clique_size, int* proven, void* workspace,
                                 size_t workspace_bytes, int bs, int N, void* stream) {
    return pmc_baseline_impl(corr_pos, src_keypts, tgt_keypts, inlier_threshold, max_nodes, pred_trans, pred_labels, clique_size, proven,
                             workspace, workspace_bytes, bs, N, stream, PMC_POOL_WORDS, nullptr);
}

extern "C" int pdsc_pmc_baseline_ex(const float* corr_pos, const float* src_keypts, const float* tgt_keypts, float inlier_threshold,
                                    int max_nodes, float* pred_trans, float* pred_labels, int* clique_size, int* proven, void* workspace,
                                    size_t workspace_bytes, int bs, int N, int lds_words, float* stage_ms, void* stream) {
    PDSC_REQUIRE(lds_words >= 0 && lds_words <= PMC_POOL_WORDS, "pdsc_pmc_baseline_ex: lds_words=%d (0 = all %d, else 1 .. %d)", lds_words,
                 PMC_POOL_WORDS, PMC_POOL_WORDS);
    return pmc_baseline_impl(corr_pos, src_keypts, tgt_keypts, inlier_threshold, max_nodes, pred_trans, pred_labels, clique_size, proven,
                             workspace, workspace_bytes, bs, N, stream, lds_words ? lds_words : PMC_POOL_WORDS, stage_ms);
}
