// Fused Adam / AdamW step (torch.optim's _single_tensor_adam, amsgrad = maximize = False) for gfx950: one
// elementwise pass over a table of (param, grad, exp_avg, exp_avg_sq) quadruples, the step count and the
// schedule count kept on the device.  See include/ffc_amd.h for the formulas and the roundings.
//
//   prologue : one thread.  t <- t + 1, then lr_eff, lr_eff / (1 - beta1^t), sqrt(1 - beta2^t) and
//              1 - lr_eff wd in fp64 from t and s, each rounded to fp32 once into the state block.
//   update   : a workgroup owns one 8192-element chunk of one tensor: 28 bytes of traffic per element (p, g, m, v
//              read, p, m, v written), float4 accesses when all four tensors of the entry are 16-byte aligned.
//   tick     : s <- s + 1 in each state block (scheduler.step()).
// Elementwise and in place: no atomics, no workspace, nothing depends on the launch split, the alignment or the
// device's CU count.  Up to 64 entries ride in one launch's arguments.
#include "ffc_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_EC = 8192;      // elements of a chunk: 8 float4 per thread and tensor
constexpr int OPT_MAX_JOBS = 64;  // entries per launch (the table rides in the kernel arguments: 48 bytes each)

struct OptState {   // the layout include/ffc_amd.h documents; ffc_optim_state_bytes() = sizeof
    long long t;
    long long s;
    float lr_eff;
    float step_size;
    float sqrt_bc2;
    float decay;
};
static_assert(sizeof(OptState) == 32, "ffc_optim_state_bytes");

struct OptDev {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long numel;
    int off;    // first workgroup of the entry in this launch
    int evec;   // float4 accesses: every tensor of the entry is 16-byte aligned
};

struct OptTable {
    OptDev j[OPT_MAX_JOBS];
    int n;
};

struct OptCoef {
    float w1;     // (float)(1 - beta1): the lerp weight
    float omw1;   // 1.0f - w1
    float b2;     // (float)beta2
    float w2;     // (float)(1 - beta2)
    float eps;
    float wd;     // Adam mode: g + wd p
    int adamw;
};

__global__ void optim_prologue_kernel(OptState* st, double lr, double beta1, double beta2, double wd, long long T) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long t = st->t + 1;
    st->t = t;
    double lr_eff = lr;
    if (T > 0) {
        const double f = 1.0 - (double)st->s / (double)T;
        lr_eff = lr * (f > 0.0 ? f : 0.0);
    }
    const double bc1 = 1.0 - pow(beta1, (double)t);
    const double bc2 = 1.0 - pow(beta2, (double)t);
    st->lr_eff = (float)lr_eff;
    st->step_size = (float)(lr_eff / bc1);
    st->sqrt_bc2 = (float)sqrt(bc2);
    st->decay = (float)(1.0 - lr_eff * wd);
}

__global__ void optim_tick_kernel(OptState* st, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st[i].s += 1;
}

// one element; every operation as written (no contraction beyond the explicit fmaf), so the float4 and the
// 4-byte paths are bit-identical
__device__ __forceinline__ void optim_update(float& p, float g, float& m, float& v, const OptCoef& c, float step_size,
                                             float sqrt_bc2, float decay) {
#pragma clang fp contract(off)
    float pp = p;
    if (c.adamw)
        pp = pp * decay;
    else
        g = fmaf(c.wd, pp, g);
    const float d = g - m;
    const float mm = c.w1 < 0.5f ? fmaf(c.w1, d, m) : g - d * c.omw1;   // torch's lerp(m, g, 1 - beta1)
    const float vv = fmaf(c.w2 * g, g, c.b2 * v);
    const float denom = sqrtf(vv) / sqrt_bc2 + c.eps;
    p = fmaf(-step_size, mm / denom, pp);
    m = mm;
    v = vv;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(OptTable t, OptCoef c, const OptState* st) {
    // the entry of this workgroup: the last one whose first workgroup is <= blockIdx.x
    int lo = 0, hi = t.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int)blockIdx.x >= t.j[mid].off)
            lo = mid;
        else
            hi = mid - 1;
    }
    const OptDev& j = t.j[lo];
    const int chunk = blockIdx.x - j.off;
    const int tid = threadIdx.x;
    const float step_size = st->step_size, sqrt_bc2 = st->sqrt_bc2, decay = st->decay;
    const long long e0 = (long long)chunk * OPT_EC;
    const int n = (int)min((long long)OPT_EC, j.numel - e0);
    float* p = j.p + e0;
    const float* g = j.g + e0;
    float* m = j.m + e0;
    float* v = j.v + e0;
    int done = 0;
    if (j.evec) {   // e0 is a multiple of 8192: the chunk keeps the tensors' alignment
        const int n4 = n >> 2;
#pragma unroll 2
        for (int i = tid; i < n4; i += OPT_THREADS) {
            float4 P = reinterpret_cast<float4*>(p)[i];
            const float4 G = reinterpret_cast<const float4*>(g)[i];
            float4 M = reinterpret_cast<float4*>(m)[i];
            float4 V = reinterpret_cast<float4*>(v)[i];
            optim_update(P.x, G.x, M.x, V.x, c, step_size, sqrt_bc2, decay);
            optim_update(P.y, G.y, M.y, V.y, c, step_size, sqrt_bc2, decay);
            optim_update(P.z, G.z, M.z, V.z, c, step_size, sqrt_bc2, decay);
            optim_update(P.w, G.w, M.w, V.w, c, step_size, sqrt_bc2, decay);
            reinterpret_cast<float4*>(p)[i] = P;
            reinterpret_cast<float4*>(m)[i] = M;
            reinterpret_cast<float4*>(v)[i] = V;
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < n; i += OPT_THREADS) {
        float P = p[i], M = m[i], V = v[i];
        optim_update(P, g[i], M, V, c, step_size, sqrt_bc2, decay);
        p[i] = P;
        m[i] = M;
        v[i] = V;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool overlaps(const float* a, const float* b, long long n) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    const uintptr_t bytes = 4 * (uintptr_t)n;
    return x < y + bytes && y < x + bytes;
}

long long opt_chunks(long long numel) { return (numel + OPT_EC - 1) / OPT_EC; }

// validate the list and collect its non-empty entries; nullptr: ok
const char* opt_collect(float* const* p, const float* const* g, float* const* m, float* const* v,
                        const long long* numel, int n, std::vector<OptDev>& jobs) {
    jobs.clear();
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0) return "negative numel";
        if (numel[i] == 0) continue;
        if (!p[i] || !g[i] || !m[i] || !v[i]) return "null tensor pointer in the list";
        const float* q[4] = {p[i], g[i], m[i], v[i]};
        for (int a = 0; a < 4; ++a)
            for (int b = a + 1; b < 4; ++b)
                if (overlaps(q[a], q[b], numel[i])) return "param, grad, exp_avg and exp_avg_sq must not alias";
        if (opt_chunks(numel[i]) >= (1LL << 31)) return "too many chunks";
        OptDev d{};
        d.p = p[i];
        d.g = g[i];
        d.m = m[i];
        d.v = v[i];
        d.numel = numel[i];
        d.evec = aligned16(d.p) && aligned16(d.g) && aligned16(d.m) && aligned16(d.v);
        jobs.push_back(d);
    }
    return nullptr;
}

int opt_per_launch(int jobs_per_launch) {
    return jobs_per_launch >= 1 && jobs_per_launch <= OPT_MAX_JOBS ? jobs_per_launch : OPT_MAX_JOBS;
}

bool unit(double b) { return b >= 0.0 && b < 1.0; }   // false for NaN

}  // namespace

extern "C" size_t ffc_optim_state_bytes(void) { return sizeof(OptState); }
extern "C" int ffc_optim_max_jobs(void) { return OPT_MAX_JOBS; }
extern "C" int ffc_optim_chunk(void) { return OPT_EC; }

extern "C" int ffc_optim_step(float* const* param, const float* const* grad, float* const* exp_avg,
                              float* const* exp_avg_sq, const long long* numel, int n, void* state, double lr,
                              double beta1, double beta2, double eps, double weight_decay, long long decay_steps,
                              int mode, int jobs_per_launch, void* stream) {
    FFC_CHECK_ARG(n >= 0, "ffc_optim_step: n >= 0");
    FFC_CHECK_ARG(n == 0 || (param && grad && exp_avg && exp_avg_sq && numel),
                  "ffc_optim_step: null list of params, grads, exp_avgs, exp_avg_sqs or numel");
    FFC_CHECK_ARG(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0,
                  "ffc_optim_step: null or misaligned state block (8-byte aligned, ffc_optim_state_bytes)");
    FFC_CHECK_ARG(unit(beta1) && unit(beta2), "ffc_optim_step: beta1 and beta2 in [0, 1)");
    FFC_CHECK_ARG(eps >= 0.0 && std::isfinite(eps), "ffc_optim_step: eps >= 0");
    FFC_CHECK_ARG(lr >= 0.0 && std::isfinite(lr), "ffc_optim_step: lr >= 0");
    FFC_CHECK_ARG(weight_decay >= 0.0 && std::isfinite(weight_decay), "ffc_optim_step: weight_decay >= 0");
    FFC_CHECK_ARG(decay_steps >= 0, "ffc_optim_step: decay_steps >= 0 (0: no schedule)");
    FFC_CHECK_ARG(mode == FFC_OPTIM_ADAMW || mode == FFC_OPTIM_ADAM,
                  "ffc_optim_step: bad mode (FFC_OPTIM_ADAMW or FFC_OPTIM_ADAM)");
    std::vector<OptDev> jobs;
    const char* err = opt_collect(param, grad, exp_avg, exp_avg_sq, numel, n, jobs);
    if (err) {
        ffc::set_error(std::string("ffc_optim_step: ") + err);
        return FFC_E_INVALID;
    }
    const int per = opt_per_launch(jobs_per_launch);
    for (size_t i0 = 0; i0 < jobs.size(); i0 += per) {   // every launch's grid, before the first launch
        long long b = 0;
        for (size_t k = i0; k < std::min(jobs.size(), i0 + per); ++k) b += opt_chunks(jobs[k].numel);
        FFC_CHECK_ARG(b < (1LL << 31), "ffc_optim_step: too many chunks in one launch");
    }
    hipStream_t st = (hipStream_t)stream;
    OptState* dst = static_cast<OptState*>(state);
    hipLaunchKernelGGL(optim_prologue_kernel, dim3(1), dim3(64), 0, st, dst, lr, beta1, beta2,
                       mode == FFC_OPTIM_ADAMW ? weight_decay : 0.0, decay_steps);
    OptCoef c{};
    c.w1 = (float)(1.0 - beta1);
    c.omw1 = 1.0f - c.w1;
    c.b2 = (float)beta2;
    c.w2 = (float)(1.0 - beta2);
    c.eps = (float)eps;
    c.wd = (float)weight_decay;
    c.adamw = mode == FFC_OPTIM_ADAMW;
    for (size_t i0 = 0; i0 < jobs.size(); i0 += per) {
        OptTable t;
        t.n = (int)std::min<size_t>(per, jobs.size() - i0);
        long long b = 0;
        for (int k = 0; k < t.n; ++k) {
            t.j[k] = jobs[i0 + k];
            t.j[k].off = (int)b;
            b += opt_chunks(t.j[k].numel);
        }
        hipLaunchKernelGGL(optim_update_kernel, dim3((unsigned)b), dim3(OPT_THREADS), 0, st, t, c,
                           (const OptState*)dst);
    }
    return ffc::launch_status("ffc_optim_step");
}

extern "C" int ffc_optim_tick(void* state, int n_states, void* stream) {
    FFC_CHECK_ARG(state && (reinterpret_cast<uintptr_t>(state) & 7) == 0,
                  "ffc_optim_tick: null or misaligned state block (8-byte aligned, ffc_optim_state_bytes)");
    FFC_CHECK_ARG(n_states >= 1, "ffc_optim_tick: n_states >= 1");
    hipLaunchKernelGGL(optim_tick_kernel, dim3((n_states + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                       static_cast<OptState*>(state), n_states);
    return ffc::launch_status("ffc_optim_tick");
}
