// Adaptive-weight critic loss (layers/aw_loss.py:13-107, aw_method.aw_loss) for gfx950: the three dot
// products of the critic's two gradient lists, the weights of Algorithm 1 / 2 and the combined
// gradient, in three launches over a table of gradient pairs.  See include/ffc_amd.h for the formulas.
//
//   A  dots    : a workgroup owns one 16384-element chunk of one tensor and writes three fp64 partials,
//                sum g_r^2, sum g_f^2, sum g_r g_f (products of fp32 values: exact in fp64).
//   B  weights : one workgroup.  Thread t adds the partials t, t + 256, ... of the global (tensor, chunk)
//                order, then the workgroup's fixed tree; rs / fs = mean sigmoid of the logits in fp64;
//                thread 0 selects the case and writes stats = [rr, ff, rf, rs, fs, w_r, w_f, case].
//   C  combine : out = w_r g_r + w_f g_f per chunk, the weights rounded to fp32 once.
// Every sum has a fixed place in a fixed tree (lanes by xor shuffles, waves in order, partials by their
// global chunk index): no atomics, results are bitwise reproducible and independent of the device's CU
// count and of how the list is split over launches (A and C take 16 jobs per launch; B is single).
#include "ffc_internal.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int AW_THREADS = 256;
constexpr int AW_EC = 16384;      // elements of a chunk
constexpr int AW_MAX_JOBS = 16;   // jobs per launch (the table rides in the kernel arguments)

struct AwDev {
    const float* gr;
    const float* gf;
    float* out;
    long long numel;
    int nchunk;
    int off;     // first workgroup of the job in this launch
    int base;    // global index of the job's first chunk (over all launches)
    int evec;    // float4 accesses: every tensor of the job is 16-byte aligned
};

struct AwTable {
    AwDev j[AW_MAX_JOBS];
    int n;
};

struct AwParams {
    double alpha1, alpha2, delta, epsilon;
    int normalized;
};

__device__ __forceinline__ const AwDev& aw_find(const AwTable& t, int& chunk) {
    int k = 0;
    while (k + 1 < t.n && (int)blockIdx.x >= t.j[k + 1].off) ++k;
    chunk = blockIdx.x - t.j[k].off;
    return t.j[k];
}

using ffc::block_sum_f64;   // sum over the workgroup, in every thread (ffc_internal.h)

// ------------------------------------------------------------------ A: partials of the three dots
__global__ __launch_bounds__(AW_THREADS) void aw_dots_kernel(AwTable t, double* part) {
    int chunk;
    const AwDev& j = aw_find(t, chunk);
    const int tid = threadIdx.x;
    const long long e0 = (long long)chunk * AW_EC;
    const int n = (int)min((long long)AW_EC, j.numel - e0);
    const float* a = j.gr + e0;
    const float* b = j.gf + e0;
    __shared__ double red[4];
    double rr = 0.0, ff = 0.0, rf = 0.0;
    int done = 0;
    if (j.evec) {   // e0 is a multiple of 16384: the chunk keeps the tensors' alignment
        const int n4 = n >> 2;
#pragma unroll 4
        for (int i = tid; i < n4; i += AW_THREADS) {
            const float4 x = reinterpret_cast<const float4*>(a)[i];
            const float4 y = reinterpret_cast<const float4*>(b)[i];
            const double x0 = x.x, x1 = x.y, x2 = x.z, x3 = x.w, y0 = y.x, y1 = y.y, y2 = y.z, y3 = y.w;
            rr += (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
            ff += (y0 * y0 + y1 * y1) + (y2 * y2 + y3 * y3);
            rf += (x0 * y0 + x1 * y1) + (x2 * y2 + x3 * y3);
        }
        done = n4 << 2;
    } else {        // the same tree from 4-byte loads: the sums do not depend on the alignment
        const int n4 = n >> 2;
#pragma unroll 4
        for (int i = tid; i < n4; i += AW_THREADS) {
            const double x0 = a[4 * i], x1 = a[4 * i + 1], x2 = a[4 * i + 2], x3 = a[4 * i + 3];
            const double y0 = b[4 * i], y1 = b[4 * i + 1], y2 = b[4 * i + 2], y3 = b[4 * i + 3];
            rr += (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
            ff += (y0 * y0 + y1 * y1) + (y2 * y2 + y3 * y3);
            rf += (x0 * y0 + x1 * y1) + (x2 * y2 + x3 * y3);
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < n; i += AW_THREADS) {
        const double x = a[i], y = b[i];
        rr += x * x;
        ff += y * y;
        rf += x * y;
    }
    rr = block_sum_f64(rr, red);
    ff = block_sum_f64(ff, red);
    rf = block_sum_f64(rf, red);
    if (tid == 0) {
        double* p = part + 3 * (size_t)(j.base + chunk);
        p[0] = rr;
        p[1] = ff;
        p[2] = rf;
    }
}

// ------------------------------------------------------------------ B: the weights
__device__ __forceinline__ double aw_sigmoid_sum(const float* x, long long n, int tid) {
    double s = 0.0;
    for (long long i = tid; i < n; i += AW_THREADS) s += 1.0 / (1.0 + exp(-(double)x[i]));
    return s;
}

__global__ __launch_bounds__(AW_THREADS) void aw_weights_kernel(const double* part, int nchunks, const float* real_v,
                                                                long long n_real, const float* fake_v,
                                                                long long n_fake, AwParams p, double* stats) {
    const int tid = threadIdx.x;
    __shared__ double red[4];
    double rr = 0.0, ff = 0.0, rf = 0.0;
    for (int c = tid; c < nchunks; c += AW_THREADS) {
        rr += part[3 * (size_t)c];
        ff += part[3 * (size_t)c + 1];
        rf += part[3 * (size_t)c + 2];
    }
    rr = block_sum_f64(rr, red);
    ff = block_sum_f64(ff, red);
    rf = block_sum_f64(rf, red);
    const double rs = block_sum_f64(aw_sigmoid_sum(real_v, n_real, tid), red) / (double)n_real;
    const double fs = block_sum_f64(aw_sigmoid_sum(fake_v, n_fake, tid), red) / (double)n_fake;
    if (tid != 0) return;
    rr += 1e-4;   // aw_loss.py:23, :35: added to avoid division by zero
    ff += 1e-4;
    const double r_norm = sqrt(rr), f_norm = sqrt(ff);
    const double one_r = p.normalized ? 1.0 / r_norm : 1.0;
    const double one_f = p.normalized ? 1.0 / f_norm : 1.0;
    const double eps = p.epsilon;
    double w_r, w_f;
    int which;
    if (rs < p.alpha1 || rs < fs - p.delta) {
        w_r = one_r + eps;
        if (rf <= 0.0) {
            which = 1;
            w_f = (p.normalized ? -rf / (ff * r_norm) : -rf / ff) + eps;
        } else {
            which = 2;
            w_f = eps;
        }
    } else if (rs > p.alpha2 && rs > fs - p.delta) {
        w_f = one_f + eps;
        if (rf <= 0.0) {
            which = 3;
            w_r = (p.normalized ? -rf / (rr * f_norm) : -rf / rr) + eps;
        } else {
            which = 4;
            w_r = eps;
        }
    } else {
        which = 5;
        w_r = one_r + eps;
        w_f = one_f + eps;
    }
    stats[0] = rr;
    stats[1] = ff;
    stats[2] = rf;
    stats[3] = rs;
    stats[4] = fs;
    stats[5] = w_r;
    stats[6] = w_f;
    stats[7] = (double)which;
}

// ------------------------------------------------------------------ C: out = w_r g_r + w_f g_f
__global__ __launch_bounds__(AW_THREADS) void aw_combine_kernel(AwTable t, const double* stats) {
    int chunk;
    const AwDev& j = aw_find(t, chunk);
    const int tid = threadIdx.x;
    const float wr = (float)stats[5], wf = (float)stats[6];
    const long long e0 = (long long)chunk * AW_EC;
    const int n = (int)min((long long)AW_EC, j.numel - e0);
    const float* a = j.gr + e0;
    const float* b = j.gf + e0;
    float* out = j.out + e0;
    int done = 0;
    if (j.evec) {
        const int n4 = n >> 2;
#pragma unroll 4
        for (int i = tid; i < n4; i += AW_THREADS) {
            const float4 x = reinterpret_cast<const float4*>(a)[i];
            const float4 y = reinterpret_cast<const float4*>(b)[i];
            reinterpret_cast<float4*>(out)[i] = make_float4(fmaf(wf, y.x, wr * x.x), fmaf(wf, y.y, wr * x.y),
                                                            fmaf(wf, y.z, wr * x.z), fmaf(wf, y.w, wr * x.w));
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < n; i += AW_THREADS) out[i] = fmaf(wf, b[i], wr * a[i]);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool overlaps(const float* a, const float* b, long long n) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    const uintptr_t bytes = 4 * (uintptr_t)n;
    return x < y + bytes && y < x + bytes;
}

long long aw_chunks(long long numel) { return (numel + AW_EC - 1) / AW_EC; }

// validate the list and collect its non-empty jobs with their global chunk bases; nullptr: ok
const char* aw_collect(const float* const* g_real, const float* const* g_fake, float* const* out,
                       const long long* numel, int n, std::vector<AwDev>& jobs, long long& total) {
    total = 0;
    jobs.clear();
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0) return "negative numel";
        if (numel[i] == 0) continue;   // an empty tensor has no chunk and no partial
        if (!g_real[i] || !g_fake[i] || (out && !out[i])) return "null tensor pointer in the list";
        if (out && (overlaps(out[i], g_real[i], numel[i]) || overlaps(out[i], g_fake[i], numel[i])))
            return "out must not alias g_real or g_fake";
        AwDev d{};
        d.gr = g_real[i];
        d.gf = g_fake[i];
        d.out = out ? out[i] : nullptr;
        d.numel = numel[i];
        const long long nc = aw_chunks(numel[i]);
        if (total + nc >= (1LL << 31)) return "too many chunks";
        d.nchunk = (int)nc;
        d.base = (int)total;
        d.evec = aligned16(d.gr) && aligned16(d.gf) && (!out || aligned16(d.out));
        total += nc;
        jobs.push_back(d);
    }
    return nullptr;
}

// table of jobs[i0, i0 + m) for one launch; returns its workgroups
unsigned aw_table(const std::vector<AwDev>& jobs, size_t i0, int m, AwTable& t) {
    long long b = 0;
    t.n = m;
    for (int k = 0; k < m; ++k) {
        t.j[k] = jobs[i0 + k];
        t.j[k].off = (int)b;
        b += t.j[k].nchunk;
    }
    return (unsigned)b;
}

int aw_per_launch(int jobs_per_launch) {
    return jobs_per_launch >= 1 && jobs_per_launch <= AW_MAX_JOBS ? jobs_per_launch : AW_MAX_JOBS;
}

}  // namespace

extern "C" int ffc_aw_chunk(void) { return AW_EC; }

extern "C" size_t ffc_aw_ws_doubles(const long long* numel, int n) {
    if (!numel || n < 0) return 0;
    size_t chunks = 0;
    for (int i = 0; i < n; ++i)
        if (numel[i] > 0) chunks += (size_t)aw_chunks(numel[i]);
    return 3 * chunks + 1;   // never 0: a list of empty tensors still has a workspace
}

extern "C" int ffc_aw_weights(const float* const* g_real, const float* const* g_fake, const long long* numel, int n,
                              const float* real_validity, long long n_real, const float* fake_validity,
                              long long n_fake, double alpha1, double alpha2, double delta, double epsilon,
                              int normalized, int jobs_per_launch, double* ws, size_t ws_doubles, double* stats,
                              void* stream) {
    FFC_CHECK_ARG(g_real && g_fake && numel && n >= 1, "ffc_aw_weights: a list of n >= 1 gradient pairs");
    FFC_CHECK_ARG(real_validity && fake_validity && n_real >= 1 && n_fake >= 1,
                  "ffc_aw_weights: real_validity and fake_validity need at least one element each");
    FFC_CHECK_ARG(alpha1 < alpha2, "ffc_aw_weights: alpha1 < alpha2");
    FFC_CHECK_ARG(ws && stats, "ffc_aw_weights: null workspace or stats");
    std::vector<AwDev> jobs;
    long long total;
    const char* err = aw_collect(g_real, g_fake, nullptr, numel, n, jobs, total);
    if (err) {
        ffc::set_error(std::string("ffc_aw_weights: ") + err);
        return FFC_E_INVALID;
    }
    FFC_CHECK_ARG(ws_doubles >= 3 * (size_t)total, "ffc_aw_weights: workspace too small (ffc_aw_ws_doubles)");
    hipStream_t st = (hipStream_t)stream;
    const int per = aw_per_launch(jobs_per_launch);
    for (size_t i0 = 0; i0 < jobs.size(); i0 += per) {
        AwTable t;
        const unsigned blocks = aw_table(jobs, i0, (int)std::min<size_t>(per, jobs.size() - i0), t);
        hipLaunchKernelGGL(aw_dots_kernel, dim3(blocks), dim3(AW_THREADS), 0, st, t, ws);
    }
    const AwParams p{alpha1, alpha2, delta, epsilon, normalized ? 1 : 0};
    hipLaunchKernelGGL(aw_weights_kernel, dim3(1), dim3(AW_THREADS), 0, st, (const double*)ws, (int)total,
                       real_validity, n_real, fake_validity, n_fake, p, stats);
    return ffc::launch_status("ffc_aw_weights");
}

extern "C" int ffc_aw_combine(const float* const* g_real, const float* const* g_fake, float* const* out,
                              const long long* numel, int n, const double* stats, int jobs_per_launch,
                              void* stream) {
    FFC_CHECK_ARG(g_real && g_fake && out && numel && n >= 1, "ffc_aw_combine: a list of n >= 1 gradient pairs");
    FFC_CHECK_ARG(stats, "ffc_aw_combine: null stats");
    std::vector<AwDev> jobs;
    long long total;
    const char* err = aw_collect(g_real, g_fake, out, numel, n, jobs, total);
    if (err) {
        ffc::set_error(std::string("ffc_aw_combine: ") + err);
        return FFC_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    const int per = aw_per_launch(jobs_per_launch);
    for (size_t i0 = 0; i0 < jobs.size(); i0 += per) {
        AwTable t;
        const unsigned blocks = aw_table(jobs, i0, (int)std::min<size_t>(per, jobs.size() - i0), t);
        hipLaunchKernelGGL(aw_combine_kernel, dim3(blocks), dim3(AW_THREADS), 0, st, t, stats);
    }
    return ffc::launch_status("ffc_aw_combine");
}
