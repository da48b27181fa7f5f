// Spectral norm (torch.nn.utils.spectral_norm's pre-hook, SpectralNorm.compute_weight with one power
// iteration) for gfx950: the power iteration, sigma and W = W_orig / sigma of a table of layers in
// three launches (two in eval mode), and the backward in two.  See include/ffc_amd.h for the formulas
// and the matrix view (R, stride_m, stride_i).
//
// Forward, per layer, Wm (M x K):
//   A  colsum : pa[rc][k] = sum over the 64 rows of row chunk rc of Wm[m][k] * u[m].  A workgroup owns
//               64 rows x 256 columns (64 x 64 in the 4-byte form); its four waves take every fourth
//               row, their column sums are added in wave order.               (training mode only)
//   B  matvec : p[k] = sum_rc pa[rc][k] (fp64, rc in order; eval mode: p = the stored v), staged in LDS
//               for a chunk of 2048 columns; pb[cc][m] = sum_k Wm[m][k] p[k] over the chunk, one wave
//               per row; the row-block-0 workgroups also write psq[cc] = sum p[k]^2 (fp64).
//   C  scale  : every workgroup rebuilds nv = max(||p||, eps) from psq, t[m] = (sum_cc pb[cc][m]) / nv,
//               nt = max(||t||, eps), sigma = sum_m (t[m] / nt) * t[m] (a job with flags bit 0: nv =
//               ||p|| + eps, nt = ||t|| + eps, the l2normalize of the SAGAN wrapper); together the layer's
//               workgroups write u = t / nt, v = p / nv (and the saved copies), workgroup 0 writes
//               sigma, and each scales its 16384-element chunk: W = W_orig / sigma.
//               v = normalize(p) and t = Wm v = (Wm p) / nv: the division commutes with the product, so
//               B needs no norm and no launch sits between A and B.
// Backward: D  pdot[chunk] = <dw, w_orig> over the chunk (fp64); E  dw_orig = dw / sigma - c u[m] v[k],
//               c = (sum_chunk pdot) / sigma^2.
// Every sum has a fixed place in a fixed tree (lanes by xor shuffles, waves in order, partials in
// order in fp64): no atomics, results are bitwise reproducible and independent of the table a layer
// is launched in and of the device's CU count.
#include "ffc_internal.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int SN_THREADS = 256;
constexpr int SN_RA = 64;        // rows of a colsum tile
constexpr int SN_RB = 16;        // rows of a matvec tile
constexpr int SN_CB = 2048;      // columns of a matvec tile (staged in LDS)
constexpr int SN_EC = 16384;     // elements of an elementwise chunk
constexpr int SN_MAX_JOBS = 16;  // jobs per launch (the table rides in the kernel arguments)
constexpr float SN_EPS = 1e-12f;

struct SnDev {
    const float* w_orig;
    float* u;
    float* v;
    float* w;
    float* sigma;
    float* u_save;
    float* v_save;
    const float* dw;
    float* dw_orig;
    double* psq;    // [ncb]
    double* pdot;   // [nchunk]
    float* pa;      // [nra][K]
    float* pb;      // [ncb][M]
    int M, K, R, stride_i;
    int flags;      // ffc_sn_job.flags
    int vec;        // rows read by float4: R % 4 == 0, w_orig 16-byte aligned
    int evec;       // elementwise passes by float4: the tensors are 16-byte aligned
    int nra, nca, nrb, ncb, nchunk;
    int offA, offB, offE;   // first workgroup of the job in launches A, B and C / D / E
};

struct SnTable {
    SnDev j[SN_MAX_JOBS];
    int n;
};

struct SnSizes {
    int nra, ncb, nchunk;
    size_t psq, pdot, pa, pb, total;   // byte offsets inside the job's workspace, and its size
};

inline bool sn_sizes(int M, int K, SnSizes& s) {
    if (M <= 0 || K <= 0 || (long long)M * K >= (1LL << 31)) return false;
    s.nra = (M + SN_RA - 1) / SN_RA;
    s.ncb = (K + SN_CB - 1) / SN_CB;
    s.nchunk = (int)(((long long)M * K + SN_EC - 1) / SN_EC);
    s.psq = 0;
    s.pdot = s.psq + 8 * (size_t)s.ncb;
    s.pa = s.pdot + 8 * (size_t)s.nchunk;
    s.pb = s.pa + 4 * (size_t)s.nra * K;
    s.total = (s.pb + 4 * (size_t)s.ncb * M + 15) & ~(size_t)15;
    return true;
}

__device__ __forceinline__ const SnDev& sn_find(const SnTable& t, int SnDev::*off, int& bid) {
    int k = 0;
    while (k + 1 < t.n && (int)blockIdx.x >= t.j[k + 1].*off) ++k;
    bid = blockIdx.x - t.j[k].*off;
    return t.j[k];
}

// element offset of Wm[0][k] (the row m adds m * rs, rs = K for dim 0, R for dim 1)
__device__ __forceinline__ int sn_col(const SnDev& j, int k) {
    if (j.R == j.K) return k;
    const int i = k / j.R;
    return i * j.stride_i + (k - i * j.R);
}

using ffc::block_sum_f64;   // sum over the workgroup, in every thread (ffc_internal.h)

// the divisor of normalize(x) from ||x||^2: max(||x||, eps), or ||x|| + eps with FFC_SN_EPS_ADD.  The same
// fp32 value in every workgroup of a layer: sq is merged in one fixed order
__device__ __forceinline__ float sn_norm(double sq, int flags) {
    const float n = (float)sqrt(sq);
    return (flags & FFC_SN_EPS_ADD) ? n + SN_EPS : fmaxf(n, SN_EPS);
}

// ------------------------------------------------------------------ A: partial columns of Wm^T u
__global__ __launch_bounds__(SN_THREADS) void sn_colsum_kernel(SnTable t) {
    int bid;
    const SnDev& j = sn_find(t, &SnDev::offA, bid);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = j.vec ? 4 : 1;
    const int rc = bid / j.nca, cc = bid - rc * j.nca;
    const int k0 = (cc * 64 + lane) * V;
    const int m0 = rc * SN_RA, m1 = min(j.M, m0 + SN_RA);
    const int rs = j.R == j.K ? j.K : j.R;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    if (k0 < j.K) {   // float4 form: K % 4 == 0, so k0 + 3 < K and the four columns share a run of R
        const float* col = j.w_orig + sn_col(j, k0);
        if (j.vec) {
#pragma unroll 4
            for (int m = m0 + wave; m < m1; m += 4) {
                const float um = j.u[m];
                const float4 x = *reinterpret_cast<const float4*>(col + (size_t)m * rs);
                a0 = fmaf(um, x.x, a0);
                a1 = fmaf(um, x.y, a1);
                a2 = fmaf(um, x.z, a2);
                a3 = fmaf(um, x.w, a3);
            }
        } else {
#pragma unroll 4
            for (int m = m0 + wave; m < m1; m += 4) a0 = fmaf(j.u[m], col[(size_t)m * rs], a0);
        }
    }
    __shared__ float red[4][4][64];   // [wave][component][lane]
    red[wave][0][lane] = a0;
    red[wave][1][lane] = a1;
    red[wave][2][lane] = a2;
    red[wave][3][lane] = a3;
    __syncthreads();
    if (wave == 0 && k0 < j.K) {
        float* out = j.pa + (size_t)rc * j.K + k0;
        for (int c = 0; c < V; ++c) out[c] = (red[0][c][lane] + red[1][c][lane]) + (red[2][c][lane] + red[3][c][lane]);
    }
}

// ------------------------------------------------------------------ B: partial rows of Wm p
__global__ __launch_bounds__(SN_THREADS) void sn_matvec_kernel(SnTable t, int training) {
    int bid;
    const SnDev& j = sn_find(t, &SnDev::offB, bid);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rb = bid / j.ncb, cc = bid - rb * j.ncb;
    const int kc0 = cc * SN_CB, kn = min(SN_CB, j.K - kc0);
    __shared__ __align__(16) float p[SN_CB];
    __shared__ double red[4];
    double sq = 0.0;
    for (int q = tid; q < kn; q += SN_THREADS) {
        float pv;
        if (training) {
            double s = 0.0;
            for (int r = 0; r < j.nra; ++r) s += (double)j.pa[(size_t)r * j.K + kc0 + q];
            pv = (float)s;
            sq += (double)pv * (double)pv;
        } else {
            pv = j.v[kc0 + q];
        }
        p[q] = pv;
    }
    __syncthreads();
    if (training && rb == 0) {   // block-uniform
        sq = block_sum_f64(sq, red);
        if (tid == 0) j.psq[cc] = sq;
    }
    const int rs = j.R == j.K ? j.K : j.R;
    const int m1 = min(j.M, (rb + 1) * SN_RB);
    for (int m = rb * SN_RB + wave; m < m1; m += 4) {   // wave-uniform
        const float* row = j.w_orig + (size_t)m * rs;
        float acc = 0.0f;
        if (j.vec) {
#pragma unroll 4
            for (int q = lane * 4; q < kn; q += 256) {   // kn % 4 == 0: K % 4 == 0
                const float4 x = *reinterpret_cast<const float4*>(row + sn_col(j, kc0 + q));
                const float4 pv = *reinterpret_cast<const float4*>(p + q);
                acc = fmaf(x.x, pv.x, acc);
                acc = fmaf(x.y, pv.y, acc);
                acc = fmaf(x.z, pv.z, acc);
                acc = fmaf(x.w, pv.w, acc);
            }
        } else if (j.R % 4 == 0) {   // w_orig off 16-byte alignment: the float4 form's order from 4-byte loads
            for (int q = lane * 4; q < kn; q += 256) {
                const float* x = row + sn_col(j, kc0 + q);
                acc = fmaf(x[0], p[q], acc);
                acc = fmaf(x[1], p[q + 1], acc);
                acc = fmaf(x[2], p[q + 2], acc);
                acc = fmaf(x[3], p[q + 3], acc);
            }
        } else {
            for (int q = lane; q < kn; q += 64) acc = fmaf(row[sn_col(j, kc0 + q)], p[q], acc);
        }
        acc = ffc::wave_sum(acc);
        if (lane == 0) j.pb[(size_t)cc * j.M + m] = acc;
    }
}

// ------------------------------------------------------------------ C: u, v, sigma, W = W_orig / sigma
__global__ __launch_bounds__(SN_THREADS) void sn_scale_kernel(SnTable t, int training) {
    int chunk;
    const SnDev& j = sn_find(t, &SnDev::offE, chunk);
    const int tid = threadIdx.x;
    const int M = j.M, K = j.K;
    __shared__ double red[4];
    float nv = 1.0f, nt = 1.0f;
    if (training) {
        double s = 0.0;
        for (int c = 0; c < j.ncb; ++c) s += j.psq[c];
        nv = sn_norm(s, j.flags);
    }
    auto t_of = [&](int m) {
        double s = 0.0;
        for (int c = 0; c < j.ncb; ++c) s += (double)j.pb[(size_t)c * M + m];
        return training ? (float)s / nv : (float)s;
    };
    if (training) {
        double st = 0.0;
        for (int m = tid; m < M; m += SN_THREADS) {
            const float tm = t_of(m);
            st += (double)tm * (double)tm;
        }
        nt = sn_norm(block_sum_f64(st, red), j.flags);
    }
    double sd = 0.0;
    for (int m = tid; m < M; m += SN_THREADS) {
        const float tm = t_of(m);
        const float um = training ? tm / nt : j.u[m];
        sd += (double)um * (double)tm;
    }
    const float sigma = (float)block_sum_f64(sd, red);
    if (chunk == 0 && tid == 0) *j.sigma = sigma;
    // this call's u and v, spread over the job's workgroups
    const int step = j.nchunk * SN_THREADS;
    if (training || j.u_save) {
        for (int m = chunk * SN_THREADS + tid; m < M; m += step) {
            const float um = training ? t_of(m) / nt : j.u[m];
            if (training) j.u[m] = um;
            if (j.u_save) j.u_save[m] = um;
        }
        for (int k = chunk * SN_THREADS + tid; k < K; k += step) {
            float vk;
            if (training) {
                double s = 0.0;
                for (int r = 0; r < j.nra; ++r) s += (double)j.pa[(size_t)r * K + k];
                vk = (float)s / nv;
                j.v[k] = vk;
            } else {
                vk = j.v[k];
            }
            if (j.v_save) j.v_save[k] = vk;
        }
    }
    const int total = M * K;
    const int e0 = chunk * SN_EC, n = min(SN_EC, total - e0);
    const float* src = j.w_orig + e0;
    float* dst = j.w + e0;
    int done = 0;
    if (j.evec) {   // e0 is a multiple of 16384: the chunk keeps the tensors' alignment
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += SN_THREADS) {
            const float4 x = reinterpret_cast<const float4*>(src)[i];
            reinterpret_cast<float4*>(dst)[i] = make_float4(x.x / sigma, x.y / sigma, x.z / sigma, x.w / sigma);
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < n; i += SN_THREADS) dst[i] = src[i] / sigma;
}

// ------------------------------------------------------------------ D: partials of <dw, w_orig>
__global__ __launch_bounds__(SN_THREADS) void sn_dot_kernel(SnTable t) {
    int chunk;
    const SnDev& j = sn_find(t, &SnDev::offE, chunk);
    const int tid = threadIdx.x;
    const int e0 = chunk * SN_EC, n = min(SN_EC, j.M * j.K - e0);
    const float* a = j.dw + e0;
    const float* b = j.w_orig + e0;
    __shared__ double red[4];
    double s = 0.0;
    int done = 0;
    if (j.evec) {
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += SN_THREADS) {
            const float4 x = reinterpret_cast<const float4*>(a)[i];
            const float4 y = reinterpret_cast<const float4*>(b)[i];
            s += ((double)x.x * (double)y.x + (double)x.y * (double)y.y) +
                 ((double)x.z * (double)y.z + (double)x.w * (double)y.w);
        }
        done = n4 << 2;
    } else {        // the same tree from 4-byte loads: pdot does not depend on the alignment
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += SN_THREADS) {
            const float* x = a + 4 * i;
            const float* y = b + 4 * i;
            s += ((double)x[0] * (double)y[0] + (double)x[1] * (double)y[1]) +
                 ((double)x[2] * (double)y[2] + (double)x[3] * (double)y[3]);
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < n; i += SN_THREADS) s += (double)a[i] * (double)b[i];
    s = block_sum_f64(s, red);
    if (tid == 0) j.pdot[chunk] = s;
}

// ------------------------------------------------------------------ E: dw_orig
__device__ __forceinline__ void sn_mk(const SnDev& j, int e, int& m, int& k) {
    if (j.R == j.K) {
        m = e / j.K;
        k = e - m * j.K;
    } else {
        const int i = e / j.stride_i, rem = e - i * j.stride_i;
        m = rem / j.R;
        k = i * j.R + (rem - m * j.R);
    }
}

__global__ __launch_bounds__(SN_THREADS) void sn_bwd_apply_kernel(SnTable t) {
    int chunk;
    const SnDev& j = sn_find(t, &SnDev::offE, chunk);
    const int tid = threadIdx.x;
    double dot = 0.0;
    for (int c = 0; c < j.nchunk; ++c) dot += j.pdot[c];
    const float sigma = *j.sigma;
    const float inv = 1.0f / sigma;
    const float coef = (float)(dot / ((double)sigma * (double)sigma));
    const int e0 = chunk * SN_EC, n = min(SN_EC, j.M * j.K - e0);
    const float* dw = j.dw + e0;
    float* out = j.dw_orig + e0;
    int done = 0;
    if (j.evec) {
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += SN_THREADS) {
            const float4 g = reinterpret_cast<const float4*>(dw)[i];
            float4 r;
            int m, k;
            if (j.vec) {   // R % 4 == 0: the four elements share a row and are consecutive in k
                sn_mk(j, e0 + 4 * i, m, k);
                const float cu = coef * j.u[m];
                r.x = fmaf(-cu, j.v[k], g.x * inv);
                r.y = fmaf(-cu, j.v[k + 1], g.y * inv);
                r.z = fmaf(-cu, j.v[k + 2], g.z * inv);
                r.w = fmaf(-cu, j.v[k + 3], g.w * inv);
            } else {
                sn_mk(j, e0 + 4 * i, m, k);
                r.x = fmaf(-coef * j.u[m], j.v[k], g.x * inv);
                sn_mk(j, e0 + 4 * i + 1, m, k);
                r.y = fmaf(-coef * j.u[m], j.v[k], g.y * inv);
                sn_mk(j, e0 + 4 * i + 2, m, k);
                r.z = fmaf(-coef * j.u[m], j.v[k], g.z * inv);
                sn_mk(j, e0 + 4 * i + 3, m, k);
                r.w = fmaf(-coef * j.u[m], j.v[k], g.w * inv);
            }
            reinterpret_cast<float4*>(out)[i] = r;
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < n; i += SN_THREADS) {
        int m, k;
        sn_mk(j, e0 + i, m, k);
        out[i] = fmaf(-coef * j.u[m], j.v[k], dw[i] * inv);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// validate jobs[0..n) (n <= SN_MAX_JOBS) and build their device table; nullptr: ok, else the message
const char* sn_build(const ffc_sn_job* jobs, int n, bool backward, void* ws, size_t ws_bytes, SnTable& t) {
    long long bA = 0, bB = 0, bE = 0;
    t.n = n;
    for (int i = 0; i < n; ++i) {
        const ffc_sn_job& a = jobs[i];
        SnSizes s;
        if (!sn_sizes(a.M, a.K, s)) return "M, K must be positive with M * K < 2^31";
        if (!a.w_orig || !a.u || !a.v || !a.sigma) return "null tensor pointer in a job";
        if (backward ? (!a.dw || !a.dw_orig) : !a.w) return "null tensor pointer in a job";
        if (!backward && a.w == a.w_orig) return "w must not be w_orig";
        if (!backward && (a.u_save == nullptr) != (a.v_save == nullptr)) return "u_save and v_save go together";
        const bool dim0 = a.R == a.K && a.stride_m == a.K;
        const bool dim1 = a.R >= 1 && a.R < a.K && a.K % a.R == 0 && a.stride_m == a.R &&
                          a.stride_i == (long long)a.M * a.R;
        if (a.flags & ~FFC_SN_EPS_ADD) return "unknown bit in flags";
        if (!dim0 && !dim1) return "unsupported matrix view (dim 0 or dim 1 of a dense weight)";
        if (a.ws_off < 0 || (a.ws_off & 15) || (size_t)a.ws_off > ws_bytes || ws_bytes - (size_t)a.ws_off < s.total)
            return "workspace too small (ffc_sn_ws_bytes per job, at ws_off)";
        char* base = static_cast<char*>(ws) + a.ws_off;
        SnDev& d = t.j[i];
        d = SnDev{};
        d.w_orig = a.w_orig;
        d.u = backward && a.u_save ? a.u_save : a.u;
        d.v = backward && a.v_save ? a.v_save : a.v;
        d.w = a.w;
        d.sigma = a.sigma;
        d.u_save = backward ? nullptr : a.u_save;
        d.v_save = backward ? nullptr : a.v_save;
        d.dw = a.dw;
        d.dw_orig = a.dw_orig;
        d.psq = reinterpret_cast<double*>(base + s.psq);
        d.pdot = reinterpret_cast<double*>(base + s.pdot);
        d.pa = reinterpret_cast<float*>(base + s.pa);
        d.pb = reinterpret_cast<float*>(base + s.pb);
        d.M = a.M;
        d.K = a.K;
        d.R = a.R;
        d.flags = a.flags;
        d.stride_i = dim0 ? a.M * a.K : (int)a.stride_i;
        d.vec = a.R % 4 == 0 && aligned16(a.w_orig);
        d.evec = backward ? aligned16(a.w_orig) && aligned16(a.dw) && aligned16(a.dw_orig)
                          : aligned16(a.w_orig) && aligned16(a.w);
        d.nra = s.nra;
        d.nca = (a.K + (d.vec ? 256 : 64) - 1) / (d.vec ? 256 : 64);
        d.nrb = (a.M + SN_RB - 1) / SN_RB;
        d.ncb = s.ncb;
        d.nchunk = s.nchunk;
        d.offA = (int)bA;
        d.offB = (int)bB;
        d.offE = (int)bE;
        bA += (long long)d.nra * d.nca;
        bB += (long long)d.nrb * d.ncb;
        bE += d.nchunk;
        if (bA >= (1LL << 31) || bB >= (1LL << 31)) return "grid too large";
    }
    return nullptr;
}

unsigned sn_blocks(const SnTable& t, int which) {
    const SnDev& l = t.j[t.n - 1];
    if (which == 0) return (unsigned)(l.offA + l.nra * l.nca);
    if (which == 1) return (unsigned)(l.offB + l.nrb * l.ncb);
    return (unsigned)(l.offE + l.nchunk);
}

}  // namespace

extern "C" size_t ffc_sn_ws_bytes(int M, int K) {
    SnSizes s;
    return sn_sizes(M, K, s) ? s.total : 0;
}

extern "C" int ffc_sn_forward(const ffc_sn_job* jobs, int n, int training, void* ws, size_t ws_bytes, void* stream) {
    FFC_CHECK_ARG(jobs && n >= 1, "ffc_sn_forward: a table of n >= 1 jobs");
    FFC_CHECK_ARG(ws, "ffc_sn_forward: null workspace");
    FFC_CHECK_ARG(aligned16(ws), "ffc_sn_forward: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    for (int i0 = 0; i0 < n; i0 += SN_MAX_JOBS) {   // validate the whole table before the first launch
        SnTable t;
        const char* err = sn_build(jobs + i0, std::min(SN_MAX_JOBS, n - i0), false, ws, ws_bytes, t);
        if (err) {
            ffc::set_error(std::string("ffc_sn_forward: ") + err);
            return FFC_E_INVALID;
        }
    }
    for (int i0 = 0; i0 < n; i0 += SN_MAX_JOBS) {
        SnTable t;
        sn_build(jobs + i0, std::min(SN_MAX_JOBS, n - i0), false, ws, ws_bytes, t);
        if (training)
            hipLaunchKernelGGL(sn_colsum_kernel, dim3(sn_blocks(t, 0)), dim3(SN_THREADS), 0, st, t);
        hipLaunchKernelGGL(sn_matvec_kernel, dim3(sn_blocks(t, 1)), dim3(SN_THREADS), 0, st, t, training ? 1 : 0);
        hipLaunchKernelGGL(sn_scale_kernel, dim3(sn_blocks(t, 2)), dim3(SN_THREADS), 0, st, t, training ? 1 : 0);
    }
    return ffc::launch_status("ffc_sn_forward");
}

extern "C" int ffc_sn_backward(const ffc_sn_job* jobs, int n, void* ws, size_t ws_bytes, void* stream) {
    FFC_CHECK_ARG(jobs && n >= 1, "ffc_sn_backward: a table of n >= 1 jobs");
    FFC_CHECK_ARG(ws, "ffc_sn_backward: null workspace");
    FFC_CHECK_ARG(aligned16(ws), "ffc_sn_backward: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    for (int i0 = 0; i0 < n; i0 += SN_MAX_JOBS) {
        SnTable t;
        const char* err = sn_build(jobs + i0, std::min(SN_MAX_JOBS, n - i0), true, ws, ws_bytes, t);
        if (err) {
            ffc::set_error(std::string("ffc_sn_backward: ") + err);
            return FFC_E_INVALID;
        }
    }
    for (int i0 = 0; i0 < n; i0 += SN_MAX_JOBS) {
        SnTable t;
        sn_build(jobs + i0, std::min(SN_MAX_JOBS, n - i0), true, ws, ws_bytes, t);
        hipLaunchKernelGGL(sn_dot_kernel, dim3(sn_blocks(t, 2)), dim3(SN_THREADS), 0, st, t);
        hipLaunchKernelGGL(sn_bwd_apply_kernel, dim3(sn_blocks(t, 2)), dim3(SN_THREADS), 0, st, t);
    }
    return ffc::launch_status("ffc_sn_backward");
}
