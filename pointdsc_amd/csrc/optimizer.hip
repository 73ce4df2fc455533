// The trainer's update on the device: finite-gradient guard, Adam or SGD, and the skip decision, all on
// the stream -- nothing is read back.  THE RULE is the contract of include/pointdsc_hip.h ("the trainer's update on the device"):
// fp32 round-to-nearest, every product and every sum its own rounding (-ffp-contract=off: no fmaf is written below), correctly
// rounded `/` and sqrtf; the bias corrections are fp64 running products rounded once.  tests/optimizer_oracle.py says the same in
// numpy float32 and the kernels match it bit for bit.
//
// Decomposition.  A step walks a table of up to OPT_MAX_TENSORS {param, grad, numel} rows that travels in the KERNEL ARGUMENTS (the
// launch copies them synchronously: no staging buffer a host that runs ahead could overwrite, no launch per tensor, parameters and
// gradients wherever autograd put them).  A tensor is cut into chunks of OPT_CHUNK elements, one workgroup each; block0[] holds the
// first workgroup of every row (an absent gradient gets none) and a workgroup finds its row by a binary search on blockIdx.x, all
// in scalar registers.  Three launches per table, in stream order:
//   check   every present gradient is scanned; a thread that sees NaN / +-Inf stores 1 to guard[0] (identical plain stores)
//   update  returns when guard[0] is set; otherwise applies the rule, READING the per-tensor step state only
//   finish  commits the step state of the present tensors (unless guard[0]); the step's last one settles the guard block
// Hazards.  A tensor spans several workgroups, so no workgroup of `update` may store b1pow / b2pow / step: each recomputes the new
// products from the old state, and `finish`, a later launch, stores the same expression's value.  The flag is cleared by the
// step's LAST finish only, after every launch that may read or set it.
// The arithmetic is written on scalars (a broadcast multiplied into a float4 is what makes packed fp32 with operand selects:
// build.py); 16-byte loads and stores are used when param and grad allow them and move the same bits.
#include "pdsc_common.h"

namespace pdsc {

constexpr int OPT_MAX_TENSORS = 128;
constexpr int OPT_THREADS = 256;
constexpr int OPT_PER_THREAD = 4;
constexpr int OPT_CHUNK = OPT_THREADS * OPT_PER_THREAD;
constexpr size_t OPT_STEP_BYTES = 32;

struct OptStep {                 // per-tensor step state at the head of the state buffer; all zero = fresh
    double b1pow, b2pow;
    long long step;
    long long unused;
};
static_assert(sizeof(OptStep) == OPT_STEP_BYTES, "OptStep");

struct OptTable {                // 3596 bytes, 3600 with its padding; with the other arguments 3608 / 3688 / 3692 bytes per kernel
    float* p[OPT_MAX_TENSORS];
    const float* g[OPT_MAX_TENSORS];            // nullptr: absent
    unsigned int soff[OPT_MAX_TENSORS];         // the tensor's m (buf) in the state buffer, in units of 16 bytes
    int numel[OPT_MAX_TENSORS];
    int block0[OPT_MAX_TENSORS + 1];            // first workgroup of row i; block0[n] = the grid
    int n;                                      // rows in use
    int base;                                   // index of row 0 in the group (its OptStep)
};

struct OptHyper {
    double lr, beta1, beta2;
    float B1, OB1, B2, OB2, E, WD, MOM, LR;
    int kind, use_guard, has_wd, has_mom;
};
static_assert(sizeof(OptTable) + sizeof(OptHyper) + 2 * sizeof(void*) + 256 <= 4096, "kernel arguments over 4 KB");

// row of workgroup b: the largest i with block0[i] <= b (rows without workgroups share their successor's block0 and lose)
__device__ __forceinline__ int opt_row(const OptTable& t, int b) {
    int lo = 0, hi = t.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.block0[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool opt_non_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(OPT_THREADS) void optim_check_kernel(const OptTable t, unsigned int* __restrict__ guard) {
    const int row = opt_row(t, blockIdx.x);
    const float* __restrict__ g = t.g[row];
    const int numel = t.numel[row];
    const int base = ((int)blockIdx.x - t.block0[row]) * OPT_CHUNK;
    bool bad = false;
    if ((((uintptr_t)g) & 15) == 0) {
        const int e = base + (int)threadIdx.x * OPT_PER_THREAD;
        if (e + OPT_PER_THREAD <= numel) {
            const float4 x = *reinterpret_cast<const float4*>(g + e);
            bad = opt_non_finite(x.x) || opt_non_finite(x.y) || opt_non_finite(x.z) || opt_non_finite(x.w);
        } else {
            for (int i = e; i < numel; ++i) bad = bad || opt_non_finite(g[i]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < OPT_PER_THREAD; ++j) {
            const int e = base + j * OPT_THREADS + (int)threadIdx.x;
            if (e < numel) bad = bad || opt_non_finite(g[e]);
        }
    }
    if (bad) guard[0] = 1u;
}

struct OptScalars {              // what one workgroup derives from the table, the hyper-parameters and the OLD step state
    float step32, sq32;          // Adam
    bool first;                  // SGD: the tensor's first successful step
};

__device__ __forceinline__ void opt_adam(const OptHyper& h, const OptScalars& s, float& p, float g, float& m, float& v) {
    float g1 = g;
    if (h.has_wd) g1 = g + h.WD * p;
    const float m2 = h.B1 * m + h.OB1 * g1;
    const float v2 = h.B2 * v + (h.OB2 * g1) * g1;
    const float d = sqrtf(v2) / s.sq32 + h.E;
    p = p - s.step32 * (m2 / d);
    m = m2;
    v = v2;
}

__device__ __forceinline__ void opt_sgd(const OptHyper& h, const OptScalars& s, float& p, float g, float& buf) {
    float g1 = g;
    if (h.has_wd) g1 = g + h.WD * p;
    float b = g1;
    if (h.has_mom) {
        if (!s.first) b = h.MOM * buf + g1;
        buf = b;
    }
    p = p - h.LR * b;
}

// correctly rounded fp64 sqrt of x in (0, 1]: the library's result (at most one ulp off) and its two neighbours, judged by the exact
// residuals x - s s' of fmas -- the test pdsc::sqrt_rn makes in fp32
__device__ __forceinline__ double opt_sqrt_rn(double x) {
    double s = sqrt(x);
    const double sd = __longlong_as_double(__double_as_longlong(s) - 1);
    const double su = __longlong_as_double(__double_as_longlong(s) + 1);
    const double rd = fma(-sd, s, x);
    const double ru = fma(-su, s, x);
    s = rd <= 0.0 ? sd : s;
    s = ru > 0.0 ? su : s;
    return s;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(const OptTable t, const OptHyper h, char* __restrict__ state,
                                                                    const unsigned int* __restrict__ guard) {
    if (h.use_guard && guard[0] != 0u) return;
    const int row = opt_row(t, blockIdx.x);
    float* __restrict__ p = t.p[row];
    const float* __restrict__ g = t.g[row];
    const int numel = t.numel[row];
    const int npad = (numel + 3) & ~3;
    float* __restrict__ m = reinterpret_cast<float*>(state + (size_t)t.soff[row] * 16);      // Adam's m, SGD's buf
    float* __restrict__ v = m + npad;
    const OptStep st = reinterpret_cast<const OptStep*>(state)[t.base + row];                // read only: see "Hazards"
    OptScalars s;
    s.first = st.step == 0;
    {
        const double b1 = (s.first ? 1.0 : st.b1pow) * h.beta1;
        const double b2 = (s.first ? 1.0 : st.b2pow) * h.beta2;
        s.step32 = (float)(h.lr / (1.0 - b1));
        s.sq32 = (float)opt_sqrt_rn(1.0 - b2);
    }
    const int base = ((int)blockIdx.x - t.block0[row]) * OPT_CHUNK;
    const bool adam = h.kind == PDSC_OPTIM_ADAM;
    const int e4 = base + (int)threadIdx.x * OPT_PER_THREAD;
    if (((((uintptr_t)p) | ((uintptr_t)g)) & 15) == 0 && e4 + OPT_PER_THREAD <= numel) {
        float4 pv = *reinterpret_cast<const float4*>(p + e4);
        const float4 gv = *reinterpret_cast<const float4*>(g + e4);
        if (adam) {
            float4 mv = *reinterpret_cast<const float4*>(m + e4);
            float4 vv = *reinterpret_cast<const float4*>(v + e4);
            opt_adam(h, s, pv.x, gv.x, mv.x, vv.x);
            opt_adam(h, s, pv.y, gv.y, mv.y, vv.y);
            opt_adam(h, s, pv.z, gv.z, mv.z, vv.z);
            opt_adam(h, s, pv.w, gv.w, mv.w, vv.w);
            *reinterpret_cast<float4*>(m + e4) = mv;
            *reinterpret_cast<float4*>(v + e4) = vv;
        } else if (h.has_mom) {
            float4 mv = *reinterpret_cast<const float4*>(m + e4);
            opt_sgd(h, s, pv.x, gv.x, mv.x);
            opt_sgd(h, s, pv.y, gv.y, mv.y);
            opt_sgd(h, s, pv.z, gv.z, mv.z);
            opt_sgd(h, s, pv.w, gv.w, mv.w);
            *reinterpret_cast<float4*>(m + e4) = mv;
        } else {
            float unused = 0.f;
            opt_sgd(h, s, pv.x, gv.x, unused);
            opt_sgd(h, s, pv.y, gv.y, unused);
            opt_sgd(h, s, pv.z, gv.z, unused);
            opt_sgd(h, s, pv.w, gv.w, unused);
        }
        *reinterpret_cast<float4*>(p + e4) = pv;
        return;
    }
    const bool vec = ((((uintptr_t)p) | ((uintptr_t)g)) & 15) == 0;      // the ragged end of an aligned tensor: this thread's own 4
#pragma unroll
    for (int j = 0; j < OPT_PER_THREAD; ++j) {
        const int e = vec ? e4 + j : base + j * OPT_THREADS + (int)threadIdx.x;
        if (e >= numel) continue;
        float pe = p[e];
        const float ge = g[e];
        if (adam) {
            float me = m[e], ve = v[e];
            opt_adam(h, s, pe, ge, me, ve);
            m[e] = me;
            v[e] = ve;
        } else if (h.has_mom) {
            float be = m[e];
            opt_sgd(h, s, pe, ge, be);
            m[e] = be;
        } else {
            float unused = 0.f;
            opt_sgd(h, s, pe, ge, unused);
        }
        p[e] = pe;
    }
}

// one workgroup of OPT_MAX_TENSORS threads, thread i = row i
__global__ __launch_bounds__(OPT_MAX_TENSORS) void optim_finish_kernel(const OptTable t, const OptHyper h, char* __restrict__ state,
                                                                        unsigned int* __restrict__ guard, int last) {
    const unsigned int flag = h.use_guard ? guard[0] : 0u;
    const int i = (int)threadIdx.x;
    if (i < t.n && t.g[i] != nullptr && flag == 0u) {
        OptStep* sp = reinterpret_cast<OptStep*>(state) + (t.base + i);
        OptStep st = *sp;
        const bool first = st.step == 0;
        st.b1pow = (first ? 1.0 : st.b1pow) * h.beta1;       // the update kernel's expressions
        st.b2pow = (first ? 1.0 : st.b2pow) * h.beta2;
        st.step += 1;
        *sp = st;
    }
    __syncthreads();             // every thread has read the flag before it is cleared
    if (last && i == 0) {
        guard[1] += flag != 0u ? 1u : 0u;
        guard[2] += 1u;
        guard[0] = 0u;
    }
}

static size_t opt_tensor_floats(int kind, long long numel) {
    const size_t npad = ((size_t)numel + 3) & ~(size_t)3;
    return kind == PDSC_OPTIM_ADAM ? 2 * npad : npad;
}

static size_t opt_header_bytes(int count) { return (size_t)count * OPT_STEP_BYTES; }

static bool opt_finite_in(double x, double lo, double hi_exclusive) { return x == x && x >= lo && x < hi_exclusive; }

// every argument rule of the three entry points; nothing below touches the HIP runtime
static int opt_validate(const pdsc_optim_call* c, const char* what) {
    PDSC_REQUIRE(c != nullptr, "%s: null pointer (call)", what);
    PDSC_REQUIRE(c->kind == PDSC_OPTIM_ADAM || c->kind == PDSC_OPTIM_SGD, "%s: unknown kind %d", what, c->kind);
    PDSC_REQUIRE(c->count >= 1, "%s: count=%d", what, c->count);
    PDSC_REQUIRE(c->tensors && c->state && c->guard, "%s: null pointer (tensors, state or guard)", what);
    PDSC_REQUIRE(((uintptr_t)c->state & 15) == 0 && ((uintptr_t)c->guard & 3) == 0,
                 "%s: state must be 16-byte aligned and guard 4-byte aligned", what);
    PDSC_REQUIRE(c->use_guard == 0 || c->use_guard == 1, "%s: use_guard=%d", what, c->use_guard);
    const double inf = HUGE_VAL;
    PDSC_REQUIRE(opt_finite_in(c->lr, 0.0, inf), "%s: lr=%g (finite and >= 0)", what, c->lr);
    PDSC_REQUIRE(opt_finite_in(c->weight_decay, 0.0, inf), "%s: weight_decay=%g (finite and >= 0)", what, c->weight_decay);
    if (c->kind == PDSC_OPTIM_ADAM) {
        PDSC_REQUIRE(opt_finite_in(c->beta1, 0.0, 1.0), "%s: beta1=%g (0 <= beta1 < 1)", what, c->beta1);
        PDSC_REQUIRE(opt_finite_in(c->beta2, 0.0, 1.0), "%s: beta2=%g (0 <= beta2 < 1)", what, c->beta2);
        PDSC_REQUIRE(opt_finite_in(c->eps, 0.0, inf), "%s: eps=%g (finite and >= 0)", what, c->eps);
    } else {
        PDSC_REQUIRE(opt_finite_in(c->momentum, 0.0, inf), "%s: momentum=%g (finite and >= 0)", what, c->momentum);
    }
    size_t floats = 0;
    for (int i = 0; i < c->count; ++i) {
        const pdsc_optim_tensor& t = c->tensors[i];
        PDSC_REQUIRE(t.param != nullptr, "%s: null pointer (param of tensor %d)", what, i);
        PDSC_REQUIRE(t.numel >= 1 && t.numel < (1ll << 31), "%s: numel=%lld (tensor %d)", what, t.numel, i);
        PDSC_REQUIRE((((uintptr_t)t.param | (uintptr_t)t.grad) & 3) == 0, "%s: param and grad must be 4-byte aligned (tensor %d)", what, i);
        floats += opt_tensor_floats(c->kind, t.numel);
    }
    const size_t need = opt_header_bytes(c->count) + floats * sizeof(float);
    PDSC_REQUIRE(c->state_bytes >= need, "%s: state of %zu bytes, needs %zu", what, c->state_bytes, need);
    PDSC_REQUIRE(need / 16 <= 0xffffffffull, "%s: state of %zu bytes is beyond the table's 32-bit offsets", what, need);
    return PDSC_OK;
}

static OptHyper opt_hyper(const pdsc_optim_call* c) {
    OptHyper h{};
    h.lr = c->lr; h.beta1 = c->beta1; h.beta2 = c->beta2;
    h.B1 = (float)c->beta1; h.OB1 = (float)(1.0 - c->beta1); h.B2 = (float)c->beta2; h.OB2 = (float)(1.0 - c->beta2);
    h.E = (float)c->eps; h.WD = (float)c->weight_decay; h.MOM = (float)c->momentum; h.LR = (float)c->lr;
    h.kind = c->kind; h.use_guard = c->use_guard; h.has_wd = c->weight_decay != 0.0; h.has_mom = c->momentum != 0.0;
    return h;
}

enum OptPhase { OPT_CHECK, OPT_UPDATE, OPT_FINISH };

// the table in chunks of OPT_MAX_TENSORS rows, one launch of `phase` each (none for a chunk without a present gradient)
static int opt_run(const pdsc_optim_call* c, OptPhase phase, int last, hipStream_t st, const char* what) {
    const OptHyper h = opt_hyper(c);
    char* state = (char*)c->state;
    size_t off16 = (opt_header_bytes(c->count) + 15) / 16;
    int last_chunk = -1;         // the step's last finish must run even when its chunk has no gradient: it settles the guard block
    if (phase == OPT_FINISH && last) last_chunk = (c->count - 1) / OPT_MAX_TENSORS;
    for (int base = 0, chunk = 0; base < c->count; base += OPT_MAX_TENSORS, ++chunk) {
        OptTable t{};
        t.n = c->count - base < OPT_MAX_TENSORS ? c->count - base : OPT_MAX_TENSORS;
        t.base = base;
        long long blocks = 0;
        for (int i = 0; i < t.n; ++i) {
            const pdsc_optim_tensor& r = c->tensors[base + i];
            t.p[i] = r.param; t.g[i] = r.grad; t.numel[i] = (int)r.numel; t.soff[i] = (unsigned int)off16;
            t.block0[i] = (int)blocks;
            if (r.grad) blocks += (r.numel + OPT_CHUNK - 1) / OPT_CHUNK;
            off16 += opt_tensor_floats(c->kind, r.numel) / 4;
        }
        for (int i = t.n; i <= OPT_MAX_TENSORS; ++i) t.block0[i] = (int)blocks;
        if (blocks >= (1ll << 31)) {
            set_error("%s: %lld workgroups in one launch", what, blocks);
            return PDSC_ERR_ARG;
        }
        if (phase == OPT_FINISH) {
            if (blocks == 0 && chunk != last_chunk) continue;
            hipLaunchKernelGGL(optim_finish_kernel, dim3(1), dim3(OPT_MAX_TENSORS), 0, st, t, h, state, c->guard,
                               chunk == last_chunk ? 1 : 0);
        } else if (blocks > 0) {
            if (phase == OPT_CHECK)
                hipLaunchKernelGGL(optim_check_kernel, dim3((unsigned)blocks), dim3(OPT_THREADS), 0, st, t, c->guard);
            else
                hipLaunchKernelGGL(optim_update_kernel, dim3((unsigned)blocks), dim3(OPT_THREADS), 0, st, t, h, state, c->guard);
        }
    }
    return check_launch(what);
}

}  // namespace pdsc

extern "C" size_t pdsc_optim_state_bytes(int kind, const long long* numel, int count) {
    if ((kind != PDSC_OPTIM_ADAM && kind != PDSC_OPTIM_SGD) || !numel || count < 1) return 0;
    size_t floats = 0;
    for (int i = 0; i < count; ++i) {
        if (numel[i] < 1 || numel[i] >= (1ll << 31)) return 0;
        floats += pdsc::opt_tensor_floats(kind, numel[i]);
    }
    return pdsc::opt_header_bytes(count) + floats * sizeof(float);
}

extern "C" int pdsc_optim_tensors_per_launch(void) { return pdsc::OPT_MAX_TENSORS; }

extern "C" int pdsc_optim_check(const pdsc_optim_call* call, void* stream) {
    const int rc = pdsc::opt_validate(call, "pdsc_optim_check");
    if (rc != PDSC_OK) return rc;
    return pdsc::opt_run(call, pdsc::OPT_CHECK, 0, (hipStream_t)stream, "pdsc_optim_check");
}

extern "C" int pdsc_optim_update(const pdsc_optim_call* call, void* stream) {
    const int rc = pdsc::opt_validate(call, "pdsc_optim_update");
    if (rc != PDSC_OK) return rc;
    return pdsc::opt_run(call, pdsc::OPT_UPDATE, 0, (hipStream_t)stream, "pdsc_optim_update");
}

extern "C" int pdsc_optim_finish(const pdsc_optim_call* call, int last, void* stream) {
    const int rc = pdsc::opt_validate(call, "pdsc_optim_finish");
    if (rc != PDSC_OK) return rc;
    PDSC_REQUIRE(last == 0 || last == 1, "pdsc_optim_finish: last=%d", last);
    return pdsc::opt_run(call, pdsc::OPT_FINISH, last, (hipStream_t)stream, "pdsc_optim_finish");
}
