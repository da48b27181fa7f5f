// Self_Attn (layers/attention_layer.py:8-40) on gfx950: fused flash-style attention, its attention
// matrix on request, and its deterministic backward.  DESIGN.md §7g has the formulas and budgets.
//
//   S[i, j] = sum_r q[r, i] k[r, j]   P = softmax_j S   o[c, i] = sum_j v[c, j] P[i, j]   y = gamma o + x
//
// q, k (d = C / 8 rows) and v (C rows) are rows of the stacked projection (B, 2d + C, N), N = H W.
// Every product is exact fp32 on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain).  One wave owns a
// 32-wide tile of queries (forward, dq) or of keys (dk, dv) and walks the other index in tiles of
// 32; nothing N x N is written unless ffc_attn_matrix is called.  No LDS, no barriers, no atomics: a
// wave's results are its own, so every gradient is bit-reproducible.
//
// The accumulator of a 32x32x2 MFMA has its column on the lane and row rowkey(t, h) = (t & 3) +
// 8 (t >> 2) + 4 h in register t of lane half h.  A score tile computed with the summed index (keys
// in the forward) on the rows is therefore the next product's B operand as it stands: k-step t of that
// product pairs rows rowkey(t, 0) and rowkey(t, 1), and the A operand is loaded in the same order
// (load_keys16).  A sum does not care in which order its terms are paired.
#include <cmath>

#include "ffc_internal.h"

namespace {

constexpr int ATT_WAVES = 4;          // waves (32-wide tiles) per workgroup
constexpr int ATT_THREADS = 64 * ATT_WAVES;
constexpr int ATT_MAX_N = 1 << 16;
constexpr int PREP_THREADS = 256;

__device__ __forceinline__ int rowkey(int t, int h) { return (t & 3) + 8 * (t >> 2) + 4 * h; }

__device__ __forceinline__ floatx16 mfma2(float a, float b, floatx16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// o[t] = p[min(j0 + rowkey(t, h), N - 1)], t = 0..15.  vec: p + j0 is 16-byte aligned and the tile
// j0 .. j0 + 31 lies inside the row (wave-uniform).
__device__ __forceinline__ void load_keys16(const float* __restrict__ p, int j0, int h, int N, bool vec,
                                            float (&o)[16]) {
    if (vec) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const floatx4 f = *reinterpret_cast<const floatx4*>(p + j0 + 8 * g + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[4 * g + e] = f[e];
        }
    } else {
#pragma unroll
        for (int t = 0; t < 16; ++t) o[t] = p[min(j0 + rowkey(t, h), N - 1)];
    }
}

// ------------------------------------------------------------------------------------ forward
// grid (ceil(N / 128), B); wave w of a workgroup owns queries i0 = (4 blockIdx.x + w) 32 ...
template <int CB>
__global__ __launch_bounds__(ATT_THREADS) void attn_fwd_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, long long bs,
    const float* __restrict__ x, const float* __restrict__ gamma, float* __restrict__ y, float* __restrict__ Lout,
    float* __restrict__ osave, int C, int d, int N, int vec) {
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int i0 = (blockIdx.x * ATT_WAVES + (threadIdx.x >> 6)) * 32;
    if (i0 >= N) return;
    const size_t b = blockIdx.y;
    const float* qb = q + b * bs;
    const float* kb = k + b * bs;
    const float* vb = v + b * bs;
    const int il = min(i0 + c, N - 1);
    float qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int r = 2 * s + h;
        qf[s] = r < d ? qb[(size_t)min(r, d - 1) * N + il] : 0.0f;
    }
    floatx16 o[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int t = 0; t < 16; ++t) o[cb][t] = 0.0f;
    float m = -INFINITY, l = 0.0f;

    for (int j0 = 0; j0 < N; j0 += 32) {
        const int jl = min(j0 + c, N - 1);
        const bool vt = vec && j0 + 32 <= N;
        floatx16 s;
#pragma unroll
        for (int t = 0; t < 16; ++t) s[t] = 0.0f;
#pragma unroll
        for (int st = 0; st < 4; ++st) {   // S^T[j][i]: A = k (rows j), B = q (columns i)
            if (2 * st < d) {
                const int r = 2 * st + h;
                const float a = r < d ? kb[(size_t)min(r, d - 1) * N + jl] : 0.0f;
                s = mfma2(a, qf[st], s);
            }
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int t = 0; t < 16; ++t) {   // padded keys never enter the maximum or the sum
            if (j0 + rowkey(t, h) >= N) s[t] = -INFINITY;
            tmax = fmaxf(tmax, s[t]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);   // finite: key j0 is real
        const float alpha = __expf(m - mn);
        m = mn;
        float psum = 0.0f;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            s[t] = __expf(s[t] - mn);
            psum += s[t];
        }
        l = fmaf(l, alpha, psum);   // this half's 16 keys of every tile; the halves meet at the end
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
            for (int t = 0; t < 16; ++t) o[cb][t] *= alpha;
            const int row = cb * 32 + c;
            float vv[16];
            load_keys16(vb + (size_t)min(row, C - 1) * N, j0, h, N, vt, vv);
#pragma unroll
            for (int t = 0; t < 16; ++t) o[cb] = mfma2(row < C ? vv[t] : 0.0f, s[t], o[cb]);
        }
    }
    l += __shfl_xor(l, 32, 64);
    if (i0 + c >= N) return;   // padded queries are not stored
    const float inv = 1.0f / l, g = gamma[0];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int row = cb * 32 + rowkey(t, h);
            if (row < C) {
                const size_t idx = (b * C + row) * N + i0 + c;
                const float ov = o[cb][t] * inv;
                y[idx] = fmaf(g, ov, x[idx]);
                if (osave) osave[idx] = ov;
            }
        }
    if (h == 0) Lout[b * N + i0 + c] = m + logf(l);
}

// ------------------------------------------------------------------------------------ attention matrix
// P[b, i, j] = exp(S[i, j] - L[b, i]); same grid as the forward, keys on the lanes so rows of P are
// written in 128-byte runs
__global__ __launch_bounds__(ATT_THREADS) void attn_matrix_kernel(const float* __restrict__ q,
                                                                  const float* __restrict__ k, long long bs,
                                                                  const float* __restrict__ L, float* __restrict__ P,
                                                                  int d, int N) {
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int i0 = (blockIdx.x * ATT_WAVES + (threadIdx.x >> 6)) * 32;
    if (i0 >= N) return;
    const size_t b = blockIdx.y;
    const float* qb = q + b * bs;
    const float* kb = k + b * bs;
    const int il = min(i0 + c, N - 1);
    float qf[4], Lr[16];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int r = 2 * s + h;
        qf[s] = r < d ? qb[(size_t)min(r, d - 1) * N + il] : 0.0f;
    }
    load_keys16(L + b * N, i0, h, N, false, Lr);
    for (int j0 = 0; j0 < N; j0 += 32) {
        const int jl = min(j0 + c, N - 1);
        floatx16 s;
#pragma unroll
        for (int t = 0; t < 16; ++t) s[t] = 0.0f;
#pragma unroll
        for (int st = 0; st < 4; ++st) {   // S[i][j]: A = q (rows i), B = k (columns j)
            if (2 * st < d) {
                const int r = 2 * st + h;
                const float kv = r < d ? kb[(size_t)min(r, d - 1) * N + jl] : 0.0f;
                s = mfma2(qf[st], kv, s);
            }
        }
        if (j0 + c < N) {
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int i = i0 + rowkey(t, h);
                if (i < N) P[(b * N + i) * N + j0 + c] = __expf(s[t] - Lr[t]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------ backward
// Dn[b, i] = sum_c dy[c, i] o[c, i] and this workgroup's share of dgamma = sum dy o; grid (ceil(N / 256), B)
__global__ __launch_bounds__(PREP_THREADS) void attn_bwd_prep_kernel(const float* __restrict__ dy,
                                                                     const float* __restrict__ o,
                                                                     float* __restrict__ Dn, float* __restrict__ part,
                                                                     int C, int N) {
    __shared__ float red[PREP_THREADS];
    const int i = blockIdx.x * PREP_THREADS + threadIdx.x;
    const size_t b = blockIdx.y;
    float acc = 0.0f;
    if (i < N) {
        for (int c = 0; c < C; ++c) {
            const size_t idx = (b * C + c) * N + i;
            acc = fmaf(dy[idx], o[idx], acc);
        }
        Dn[b * N + i] = acc;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = PREP_THREADS / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[b * gridDim.x + blockIdx.x] = red[0];
}

// dgamma = the n partials summed in one fixed order (fp64), one workgroup
__global__ __launch_bounds__(PREP_THREADS) void attn_dgamma_kernel(const float* __restrict__ part, int n,
                                                                   float* __restrict__ dgamma) {
    __shared__ double red[PREP_THREADS];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += PREP_THREADS) acc += (double)part[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = PREP_THREADS / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) dgamma[0] = (float)red[0];
}

// key-tile-major: the wave owns dk, dv of keys j0 .. j0 + 31 and walks every query tile.  Queries on
// the rows (registers), keys on the lanes.  With dy in place of do = gamma dy throughout, gamma
// multiplies the results once at the end.
template <int CB>
__global__ __launch_bounds__(ATT_THREADS) void attn_bwd_kv_kernel(
    const float* __restrict__ dy, const float* __restrict__ q, const float* __restrict__ k,
    const float* __restrict__ v, long long bs, const float* __restrict__ L, const float* __restrict__ Dn,
    const float* __restrict__ gamma, float* __restrict__ dk, float* __restrict__ dv, long long gbs, int C, int d,
    int N, int vec) {
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int j0 = (blockIdx.x * ATT_WAVES + (threadIdx.x >> 6)) * 32;
    if (j0 >= N) return;
    const size_t b = blockIdx.y;
    const float* qb = q + b * bs;
    const float* kb = k + b * bs;
    const float* vb = v + b * bs;
    const float* dyb = dy + b * C * N;
    const int jl = min(j0 + c, N - 1);
    const bool jok = j0 + c < N;
    float kf[4], vf[16 * CB];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int r = 2 * s + h;
        kf[s] = r < d ? kb[(size_t)min(r, d - 1) * N + jl] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 16 * CB; ++s) {
        const int cc = 2 * s + h;
        vf[s] = cc < C ? vb[(size_t)min(cc, C - 1) * N + jl] : 0.0f;
    }
    floatx16 adv[CB], adk;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        adk[t] = 0.0f;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) adv[cb][t] = 0.0f;
    }

    for (int i0 = 0; i0 < N; i0 += 32) {
        const int il = min(i0 + c, N - 1);
        const bool vt = vec && i0 + 32 <= N;
        floatx16 s, dp;
#pragma unroll
        for (int t = 0; t < 16; ++t) s[t] = dp[t] = 0.0f;
#pragma unroll
        for (int st = 0; st < 4; ++st) {   // S[i][j]: A = q (rows i), B = k (columns j)
            if (2 * st < d) {
                const int r = 2 * st + h;
                const float a = r < d ? qb[(size_t)min(r, d - 1) * N + il] : 0.0f;
                s = mfma2(a, kf[st], s);
            }
        }
#pragma unroll
        for (int st = 0; st < 16 * CB; ++st) {   // dP[i][j] = sum_c dy[c, i] v[c, j]
            if (2 * st < C) {
                const int cc = 2 * st + h;
                const float a = cc < C ? dyb[(size_t)min(cc, C - 1) * N + il] : 0.0f;
                dp = mfma2(a, vf[st], dp);
            }
        }
        float Lr[16], Dr[16];
        load_keys16(L + b * N, i0, h, N, vt, Lr);
        load_keys16(Dn + b * N, i0, h, N, vt, Dr);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const float p = (jok && i0 + rowkey(t, h) < N) ? __expf(s[t] - Lr[t]) : 0.0f;
            s[t] = p;
            dp[t] = p * (dp[t] - Dr[t]);   // dS / gamma
        }
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {   // dv[c, j] += sum_i dy[c, i] P[i, j]
            const int row = cb * 32 + c;
            float a[16];
            load_keys16(dyb + (size_t)min(row, C - 1) * N, i0, h, N, vt, a);
#pragma unroll
            for (int t = 0; t < 16; ++t) adv[cb] = mfma2(row < C ? a[t] : 0.0f, s[t], adv[cb]);
        }
        {   // dk[r, j] += sum_i q[r, i] dS[i, j]: rows r >= d of the tile are zero
            float a[16];
            load_keys16(qb + (size_t)min(c, d - 1) * N, i0, h, N, vt, a);
#pragma unroll
            for (int t = 0; t < 16; ++t) adk = mfma2(c < d ? a[t] : 0.0f, dp[t], adk);
        }
    }
    if (!jok) return;
    const float g = gamma[0];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int row = cb * 32 + rowkey(t, h);
            if (row < C) dv[b * gbs + (size_t)row * N + j0 + c] = g * adv[cb][t];
        }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int r = t + 4 * h;
        if (r < d) dk[b * gbs + (size_t)r * N + j0 + c] = g * adk[t];
    }
}

// query-tile-major: the wave owns dq of queries i0 .. i0 + 31 and walks every key tile.  Keys on the
// rows (registers), queries on the lanes, as in the forward.
template <int CB>
__global__ __launch_bounds__(ATT_THREADS) void attn_bwd_q_kernel(
    const float* __restrict__ dy, const float* __restrict__ q, const float* __restrict__ k,
    const float* __restrict__ v, long long bs, const float* __restrict__ L, const float* __restrict__ Dn,
    const float* __restrict__ gamma, float* __restrict__ dq, long long gbs, int C, int d, int N, int vec) {
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int i0 = (blockIdx.x * ATT_WAVES + (threadIdx.x >> 6)) * 32;
    if (i0 >= N) return;
    const size_t b = blockIdx.y;
    const float* qb = q + b * bs;
    const float* kb = k + b * bs;
    const float* vb = v + b * bs;
    const float* dyb = dy + b * C * N;
    const int il = min(i0 + c, N - 1);
    float qf[4], dyf[16 * CB];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int r = 2 * s + h;
        qf[s] = r < d ? qb[(size_t)min(r, d - 1) * N + il] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 16 * CB; ++s) {
        const int cc = 2 * s + h;
        dyf[s] = cc < C ? dyb[(size_t)min(cc, C - 1) * N + il] : 0.0f;
    }
    const float Li = L[b * N + il], Di = Dn[b * N + il];
    floatx16 adq;
#pragma unroll
    for (int t = 0; t < 16; ++t) adq[t] = 0.0f;

    for (int j0 = 0; j0 < N; j0 += 32) {
        const int jl = min(j0 + c, N - 1);
        const bool vt = vec && j0 + 32 <= N;
        floatx16 s, dp;
#pragma unroll
        for (int t = 0; t < 16; ++t) s[t] = dp[t] = 0.0f;
#pragma unroll
        for (int st = 0; st < 4; ++st) {   // S^T[j][i]
            if (2 * st < d) {
                const int r = 2 * st + h;
                const float a = r < d ? kb[(size_t)min(r, d - 1) * N + jl] : 0.0f;
                s = mfma2(a, qf[st], s);
            }
        }
#pragma unroll
        for (int st = 0; st < 16 * CB; ++st) {   // dP^T[j][i] = sum_c v[c, j] dy[c, i]
            if (2 * st < C) {
                const int cc = 2 * st + h;
                const float a = cc < C ? vb[(size_t)min(cc, C - 1) * N + jl] : 0.0f;
                dp = mfma2(a, dyf[st], dp);
            }
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const float p = j0 + rowkey(t, h) < N ? __expf(s[t] - Li) : 0.0f;
            dp[t] = p * (dp[t] - Di);   // dS / gamma
        }
        float a[16];   // dq[r, i] += sum_j k[r, j] dS[i, j]
        load_keys16(kb + (size_t)min(c, d - 1) * N, j0, h, N, vt, a);
#pragma unroll
        for (int t = 0; t < 16; ++t) adq = mfma2(c < d ? a[t] : 0.0f, dp[t], adq);
    }
    if (i0 + c >= N) return;
    const float g = gamma[0];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int r = t + 4 * h;
        if (r < d) dq[b * gbs + (size_t)r * N + i0 + c] = g * adq[t];
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the supported shapes; nullptr when (B, C, H, W) is one of them
const char* attn_refuse(int B, int C, int H, int W, std::string& msg) {
    const bool ok = C % 8 == 0 && C >= 8 && C <= 64 && H >= 1 && W >= 1 && (long long)H * W <= ATT_MAX_N &&
                    B >= 1 && B <= 65535;
    if (ok) return nullptr;
    msg = "unsupported Self_Attn shape (B, C, H, W) = (" + std::to_string(B) + ", " + std::to_string(C) + ", " +
          std::to_string(H) + ", " + std::to_string(W) + "): C % 8 == 0, 8 <= C <= 64, 1 <= H * W <= " +
          std::to_string(ATT_MAX_N) + ", 1 <= B <= 65535";
    return msg.c_str();
}

#define ATT_CHECK_SHAPE(name)                                         \
    do {                                                              \
        std::string m_;                                               \
        if (attn_refuse(B, C, H, W, m_)) {                            \
            ::ffc::set_error(std::string(name ": ") + m_);            \
            return FFC_E_INVALID;                                     \
        }                                                             \
    } while (0)

}  // namespace

extern "C" int ffc_attn_supported(int C, int H, int W) {
    std::string m;
    return attn_refuse(1, C, H, W, m) ? 0 : 1;
}

extern "C" size_t ffc_attn_ws_floats(int B, int C, int H, int W) {
    std::string m;
    if (attn_refuse(B, C, H, W, m)) return 0;
    const size_t N = (size_t)H * W;
    return (size_t)B * N + (size_t)B * ((N + PREP_THREADS - 1) / PREP_THREADS);
}

extern "C" int ffc_attn_forward(const float* q, const float* k, const float* v, long long bstride, const float* x,
                                const float* gamma, float* y, float* L, float* o, int B, int C, int H, int W,
                                void* stream) {
    ATT_CHECK_SHAPE("ffc_attn_forward");
    FFC_CHECK_ARG(q && k && v && x && gamma && y && L, "ffc_attn_forward: null pointer");
    const int N = H * W, d = C / 8;
    FFC_CHECK_ARG(bstride >= (long long)(2 * d + C) * N, "ffc_attn_forward: batch stride below (2d + C) N");
    const int vec = N % 4 == 0 && bstride % 4 == 0 && aligned16(v);
    const dim3 grid((N + 32 * ATT_WAVES - 1) / (32 * ATT_WAVES), B);
    hipStream_t st = (hipStream_t)stream;
    if (C <= 32)
        hipLaunchKernelGGL(attn_fwd_kernel<1>, grid, dim3(ATT_THREADS), 0, st, q, k, v, bstride, x, gamma, y, L, o, C, d,
                           N, vec);
    else
        hipLaunchKernelGGL(attn_fwd_kernel<2>, grid, dim3(ATT_THREADS), 0, st, q, k, v, bstride, x, gamma, y, L, o, C, d,
                           N, vec);
    return ffc::launch_status("ffc_attn_forward");
}

extern "C" int ffc_attn_matrix(const float* q, const float* k, long long bstride, const float* L, float* P, int B,
                               int C, int H, int W, void* stream) {
    ATT_CHECK_SHAPE("ffc_attn_matrix");
    FFC_CHECK_ARG(q && k && L && P, "ffc_attn_matrix: null pointer");
    const int N = H * W, d = C / 8;
    FFC_CHECK_ARG(bstride >= (long long)d * N, "ffc_attn_matrix: batch stride below d N");
    const dim3 grid((N + 32 * ATT_WAVES - 1) / (32 * ATT_WAVES), B);
    hipLaunchKernelGGL(attn_matrix_kernel, grid, dim3(ATT_THREADS), 0, (hipStream_t)stream, q, k, bstride, L, P, d, N);
    return ffc::launch_status("ffc_attn_matrix");
}

extern "C" int ffc_attn_backward(const float* dy, const float* q, const float* k, const float* v, long long bstride,
                                 const float* o, const float* L, const float* gamma, float* dq, float* dk, float* dv,
                                 long long gbstride, float* dgamma, float* ws, int B, int C, int H, int W,
                                 void* stream) {
    ATT_CHECK_SHAPE("ffc_attn_backward");
    FFC_CHECK_ARG(dy && q && k && v && o && L && gamma && dq && dk && dv && dgamma && ws,
                  "ffc_attn_backward: null pointer");
    const int N = H * W, d = C / 8;
    FFC_CHECK_ARG(bstride >= (long long)(2 * d + C) * N && gbstride >= (long long)(2 * d + C) * N,
                  "ffc_attn_backward: batch stride below (2d + C) N");
    const int vec = N % 4 == 0 && bstride % 4 == 0 && aligned16(q) && aligned16(k) && aligned16(dy) && aligned16(L) &&
                    aligned16(ws);
    const int chunks = (N + PREP_THREADS - 1) / PREP_THREADS;
    float* Dn = ws;
    float* part = ws + (size_t)B * N;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(attn_bwd_prep_kernel, dim3(chunks, B), dim3(PREP_THREADS), 0, st, dy, o, Dn, part, C, N);
    hipLaunchKernelGGL(attn_dgamma_kernel, dim3(1), dim3(PREP_THREADS), 0, st, part, B * chunks, dgamma);
    const dim3 grid((N + 32 * ATT_WAVES - 1) / (32 * ATT_WAVES), B);
    if (C <= 32) {
        hipLaunchKernelGGL(attn_bwd_kv_kernel<1>, grid, dim3(ATT_THREADS), 0, st, dy, q, k, v, bstride, L, Dn, gamma, dk,
                           dv, gbstride, C, d, N, vec);
        hipLaunchKernelGGL(attn_bwd_q_kernel<1>, grid, dim3(ATT_THREADS), 0, st, dy, q, k, v, bstride, L, Dn, gamma, dq,
                           gbstride, C, d, N, vec);
    } else {
        hipLaunchKernelGGL(attn_bwd_kv_kernel<2>, grid, dim3(ATT_THREADS), 0, st, dy, q, k, v, bstride, L, Dn, gamma, dk,
                           dv, gbstride, C, d, N, vec);
        hipLaunchKernelGGL(attn_bwd_q_kernel<2>, grid, dim3(ATT_THREADS), 0, st, dy, q, k, v, bstride, L, Dn, gamma, dq,
                           gbstride, C, d, N, vec);
    }
    return ffc::launch_status("ffc_attn_backward");
}

// ==================================================================================== wide channels
// 72 <= C <= 256 (9 <= d <= 32): the same formulas, tiles and operand orders as above; DESIGN.md §7l.
// What changes is where the channels go.  S takes up to 16 k-steps (q or k of the wave's own tile in 16
// registers).  o and dv need P alone, so they are split over channel groups of 64 on a grid axis, each
// group recomputing S (16 MFMAs against its 32): two accumulator tiles per wave, as at C <= 64.  dq and dk
// need dS = P (dP - D) and dP sums over every channel, so one wave runs the whole sum (C / 2 k-steps, both
// operands streamed from memory: 128 registers of its own tile's v or dy spill) and owns a full 32-row dq /
// dk tile; dv has its own kernel.
// Nothing is reduced across workgroups except dgamma (attn_dgamma_kernel's fixed order).
namespace {

constexpr int ATTW_DS = 16;   // k-steps of S: d <= 32
constexpr int ATTW_GC = 64;   // channels of one group of the forward and of dv
constexpr int ATTW_MAX_C = 256;

// rows r = 2 s + h of a (d, N) matrix at column n, the B (or A) operand of S's k-step s
__device__ __forceinline__ void load_rows(const float* __restrict__ p, int d, int N, int n, int h,
                                          float (&o)[ATTW_DS]) {
#pragma unroll
    for (int s = 0; s < ATTW_DS; ++s) {
        const int r = 2 * s + h;
        o[s] = r < d ? p[(size_t)min(r, d - 1) * N + n] : 0.0f;
    }
}

// the score tile: rows from a (loaded here, column n of a), columns from bf (load_rows of the other side)
__device__ __forceinline__ floatx16 scores(const float* __restrict__ a, const float (&bf)[ATTW_DS], int d, int N,
                                           int n, int h) {
    floatx16 s;
#pragma unroll
    for (int t = 0; t < 16; ++t) s[t] = 0.0f;
#pragma unroll
    for (int st = 0; st < ATTW_DS; ++st) {
        if (2 * st < d) {
            const int r = 2 * st + h;
            const float av = r < d ? a[(size_t)min(r, d - 1) * N + n] : 0.0f;
            s = mfma2(av, bf[st], s);
        }
    }
    return s;
}

// grid (ceil(N / 128), ceil(C / 64), B); blockIdx.y is the channel group, group 0 writes L
__global__ __launch_bounds__(ATT_THREADS) void attnw_fwd_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, long long bs,
    const float* __restrict__ x, const float* __restrict__ gamma, float* __restrict__ y, float* __restrict__ Lout,
    float* __restrict__ osave, int C, int d, int N, int vec) {
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int i0 = (blockIdx.x * ATT_WAVES + (threadIdx.x >> 6)) * 32;
    if (i0 >= N) return;
    const int c0 = blockIdx.y * ATTW_GC;
    const size_t b = blockIdx.z;
    const float* kb = k + b * bs;
    const float* vb = v + b * bs;
    float qf[ATTW_DS];
    load_rows(q + b * bs, d, N, min(i0 + c, N - 1), h, qf);
    floatx16 o[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int t = 0; t < 16; ++t) o[cb][t] = 0.0f;
    float m = -INFINITY, l = 0.0f;

    for (int j0 = 0; j0 < N; j0 += 32) {
        const bool vt = vec && j0 + 32 <= N;
        floatx16 s = scores(kb, qf, d, N, min(j0 + c, N - 1), h);   // S^T[j][i]
        float tmax = -INFINITY;
#pragma unroll
        for (int t = 0; t < 16; ++t) {   // padded keys never enter the maximum or the sum
            if (j0 + rowkey(t, h) >= N) s[t] = -INFINITY;
            tmax = fmaxf(tmax, s[t]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);   // finite: key j0 is real
        const float alpha = __expf(m - mn);
        m = mn;
        float psum = 0.0f;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            s[t] = __expf(s[t] - mn);
            psum += s[t];
        }
        l = fmaf(l, alpha, psum);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            if (c0 + cb * 32 < C) {   // the last group may hold one block only
#pragma unroll
                for (int t = 0; t < 16; ++t) o[cb][t] *= alpha;
                const int row = c0 + cb * 32 + c;
                float vv[16];
                load_keys16(vb + (size_t)min(row, C - 1) * N, j0, h, N, vt, vv);
#pragma unroll
                for (int t = 0; t < 16; ++t) o[cb] = mfma2(row < C ? vv[t] : 0.0f, s[t], o[cb]);
            }
        }
    }
    l += __shfl_xor(l, 32, 64);
    if (i0 + c >= N) return;   // padded queries are not stored
    const float inv = 1.0f / l, g = gamma[0];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int row = c0 + cb * 32 + rowkey(t, h);
            if (row < C) {
                const size_t idx = (b * C + row) * N + i0 + c;
                const float ov = o[cb][t] * inv;
                y[idx] = fmaf(g, ov, x[idx]);
                if (osave) osave[idx] = ov;
            }
        }
    if (h == 0 && blockIdx.y == 0) Lout[b * N + i0 + c] = m + logf(l);
}

// grid (ceil(N / 128), B), as attn_matrix_kernel
__global__ __launch_bounds__(ATT_THREADS) void attnw_matrix_kernel(const float* __restrict__ q,
                                                                   const float* __restrict__ k, long long bs,
                                                                   const float* __restrict__ L, float* __restrict__ P,
                                                                   int d, int N) {
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int i0 = (blockIdx.x * ATT_WAVES + (threadIdx.x >> 6)) * 32;
    if (i0 >= N) return;
    const size_t b = blockIdx.y;
    const float* qb = q + b * bs;
    float kf[ATTW_DS], Lr[16];
    load_keys16(L + b * N, i0, h, N, false, Lr);
    for (int j0 = 0; j0 < N; j0 += 32) {
        load_rows(k + b * bs, d, N, min(j0 + c, N - 1), h, kf);
        const floatx16 s = scores(qb, kf, d, N, min(i0 + c, N - 1), h);   // S[i][j]
        if (j0 + c < N) {
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int i = i0 + rowkey(t, h);
                if (i < N) P[(b * N + i) * N + j0 + c] = __expf(s[t] - Lr[t]);
            }
        }
    }
}

// dv[c, j] = gamma sum_i dy[c, i] P[i, j]: key-tile-major, grid (ceil(N / 128), ceil(C / 64), B)
__global__ __launch_bounds__(ATT_THREADS) void attnw_bwd_v_kernel(
    const float* __restrict__ dy, const float* __restrict__ q, const float* __restrict__ k, long long bs,
    const float* __restrict__ L, const float* __restrict__ gamma, float* __restrict__ dv, long long gbs, int C, int d,
    int N, int vec) {
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int j0 = (blockIdx.x * ATT_WAVES + (threadIdx.x >> 6)) * 32;
    if (j0 >= N) return;
    const int c0 = blockIdx.y * ATTW_GC;
    const size_t b = blockIdx.z;
    const float* qb = q + b * bs;
    const float* dyb = dy + b * C * N;
    const bool jok = j0 + c < N;
    float kf[ATTW_DS];
    load_rows(k + b * bs, d, N, min(j0 + c, N - 1), h, kf);
    floatx16 adv[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int t = 0; t < 16; ++t) adv[cb][t] = 0.0f;

    for (int i0 = 0; i0 < N; i0 += 32) {
        const bool vt = vec && i0 + 32 <= N;
        floatx16 s = scores(qb, kf, d, N, min(i0 + c, N - 1), h);   // S[i][j]
        float Lr[16];
        load_keys16(L + b * N, i0, h, N, vt, Lr);
#pragma unroll
        for (int t = 0; t < 16; ++t) s[t] = (jok && i0 + rowkey(t, h) < N) ? __expf(s[t] - Lr[t]) : 0.0f;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            if (c0 + cb * 32 < C) {
                const int row = c0 + cb * 32 + c;
                float a[16];
                load_keys16(dyb + (size_t)min(row, C - 1) * N, i0, h, N, vt, a);
#pragma unroll
                for (int t = 0; t < 16; ++t) adv[cb] = mfma2(row < C ? a[t] : 0.0f, s[t], adv[cb]);
            }
        }
    }
    if (!jok) return;
    const float g = gamma[0];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int row = c0 + cb * 32 + rowkey(t, h);
            if (row < C) dv[b * gbs + (size_t)row * N + j0 + c] = g * adv[cb][t];
        }
}

// dq (KEYS = false: the wave owns queries n0 .. n0 + 31, walks key tiles, rows of the score tiles are keys)
// or dk (KEYS = true: owns keys, walks query tiles, rows are queries); grid (ceil(N / 128), B).  own is the
// matrix of the owned index (q | k), oth the walked one; cown / coth likewise of the channel sum dP (dy | v).
// With dy in place of do = gamma dy, gamma multiplies the result at the end.
template <bool KEYS>
__global__ __launch_bounds__(ATT_THREADS) void attnw_bwd_qk_kernel(
    const float* __restrict__ own, const float* __restrict__ oth, const float* __restrict__ cown,
    const float* __restrict__ coth, long long bs, long long cown_bs, long long coth_bs, const float* __restrict__ L,
    const float* __restrict__ Dn, const float* __restrict__ gamma, float* __restrict__ dout, long long gbs, int C,
    int d, int N, int vec) {
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int n0 = (blockIdx.x * ATT_WAVES + (threadIdx.x >> 6)) * 32;
    if (n0 >= N) return;
    const size_t b = blockIdx.y;
    const float* ob = oth + b * bs;
    const float* cob = coth + b * coth_bs;
    const float* cwb = cown + b * cown_bs;
    const int nl = min(n0 + c, N - 1);
    const bool nok = n0 + c < N;
    float of[ATTW_DS];
    load_rows(own + b * bs, d, N, nl, h, of);
    const float Ln = L[b * N + nl], Dnn = Dn[b * N + nl];   // KEYS = false: the lane's own query
    floatx16 acc;
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0.0f;

    for (int m0 = 0; m0 < N; m0 += 32) {
        const int ml = min(m0 + c, N - 1);
        const bool vt = vec && m0 + 32 <= N;
        floatx16 s = scores(ob, of, d, N, ml, h);
        floatx16 dp;
#pragma unroll
        for (int t = 0; t < 16; ++t) dp[t] = 0.0f;
#pragma unroll 8
        for (int st = 0; st < C / 2; ++st) {   // dP over every channel (C is even: 2 st + h < C)
            const size_t cc = 2 * st + h;
            dp = mfma2(cob[cc * N + ml], cwb[cc * N + nl], dp);
        }
        if (KEYS) {
            float Lr[16], Dr[16];
            load_keys16(L + b * N, m0, h, N, vt, Lr);
            load_keys16(Dn + b * N, m0, h, N, vt, Dr);
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const float p = (nok && m0 + rowkey(t, h) < N) ? __expf(s[t] - Lr[t]) : 0.0f;
                dp[t] = p * (dp[t] - Dr[t]);   // dS / gamma
            }
        } else {
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const float p = m0 + rowkey(t, h) < N ? __expf(s[t] - Ln) : 0.0f;
                dp[t] = p * (dp[t] - Dnn);
            }
        }
        float a[16];   // d(own)[r, n] += sum_m oth[r, m] dS: rows r >= d of the tile are zero
        load_keys16(ob + (size_t)min(c, d - 1) * N, m0, h, N, vt, a);
#pragma unroll
        for (int t = 0; t < 16; ++t) acc = mfma2(c < d ? a[t] : 0.0f, dp[t], acc);
    }
    if (!nok) return;
    const float g = gamma[0];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int r = rowkey(t, h);
        if (r < d) dout[b * gbs + (size_t)r * N + n0 + c] = g * acc[t];
    }
}

const char* attnw_refuse(int B, int C, int H, int W, std::string& msg) {
    const bool ok = C % 8 == 0 && C >= 72 && C <= ATTW_MAX_C && H >= 1 && W >= 1 &&
                    (long long)H * W <= ATT_MAX_N && B >= 1 && B <= 65535;
    if (ok) return nullptr;
    msg = "unsupported wide Self_Attn shape (B, C, H, W) = (" + std::to_string(B) + ", " + std::to_string(C) + ", " +
          std::to_string(H) + ", " + std::to_string(W) + "): C % 8 == 0, 72 <= C <= " + std::to_string(ATTW_MAX_C) +
          ", 1 <= H * W <= " + std::to_string(ATT_MAX_N) + ", 1 <= B <= 65535";
    return msg.c_str();
}

#define ATTW_CHECK_SHAPE(name)                                        \
    do {                                                              \
        std::string m_;                                               \
        if (attnw_refuse(B, C, H, W, m_)) {                           \
            ::ffc::set_error(std::string(name ": ") + m_);            \
            return FFC_E_INVALID;                                     \
        }                                                             \
    } while (0)

void launch_bwd_qk(dim3 grid, hipStream_t st, const float* dy, const float* q, const float* k, const float* v,
                   long long bs, const float* L, const float* Dn, const float* gamma, float* dq, float* dk,
                   long long gbs, int C, int d, int N, int vec) {
    const long long dys = (long long)C * N;
    hipLaunchKernelGGL((attnw_bwd_qk_kernel<true>), grid, dim3(ATT_THREADS), 0, st, k, q, v, dy, bs, bs, dys, L, Dn,
                       gamma, dk, gbs, C, d, N, vec);
    hipLaunchKernelGGL((attnw_bwd_qk_kernel<false>), grid, dim3(ATT_THREADS), 0, st, q, k, dy, v, bs, dys, bs, L, Dn,
                       gamma, dq, gbs, C, d, N, vec);
}

}  // namespace

extern "C" int ffc_attnw_supported(int C, int H, int W) {
    std::string m;
    return attnw_refuse(1, C, H, W, m) ? 0 : 1;
}

extern "C" size_t ffc_attnw_ws_floats(int B, int C, int H, int W) {
    std::string m;
    if (attnw_refuse(B, C, H, W, m)) return 0;
    const size_t N = (size_t)H * W;
    return (size_t)B * N + (size_t)B * ((N + PREP_THREADS - 1) / PREP_THREADS);
}

extern "C" int ffc_attnw_forward(const float* q, const float* k, const float* v, long long bstride, const float* x,
                                 const float* gamma, float* y, float* L, float* o, int B, int C, int H, int W,
                                 void* stream) {
    ATTW_CHECK_SHAPE("ffc_attnw_forward");
    FFC_CHECK_ARG(q && k && v && x && gamma && y && L, "ffc_attnw_forward: null pointer");
    const int N = H * W, d = C / 8;
    FFC_CHECK_ARG(bstride >= (long long)(2 * d + C) * N, "ffc_attnw_forward: batch stride below (2d + C) N");
    const int vec = N % 4 == 0 && bstride % 4 == 0 && aligned16(v);
    const dim3 grid((N + 32 * ATT_WAVES - 1) / (32 * ATT_WAVES), (C + ATTW_GC - 1) / ATTW_GC, B);
    hipLaunchKernelGGL(attnw_fwd_kernel, grid, dim3(ATT_THREADS), 0, (hipStream_t)stream, q, k, v, bstride, x, gamma, y,
                       L, o, C, d, N, vec);
    return ffc::launch_status("ffc_attnw_forward");
}

extern "C" int ffc_attnw_matrix(const float* q, const float* k, long long bstride, const float* L, float* P, int B,
                                int C, int H, int W, void* stream) {
    ATTW_CHECK_SHAPE("ffc_attnw_matrix");
    FFC_CHECK_ARG(q && k && L && P, "ffc_attnw_matrix: null pointer");
    const int N = H * W, d = C / 8;
    FFC_CHECK_ARG(bstride >= (long long)d * N, "ffc_attnw_matrix: batch stride below d N");
    const dim3 grid((N + 32 * ATT_WAVES - 1) / (32 * ATT_WAVES), B);
    hipLaunchKernelGGL(attnw_matrix_kernel, grid, dim3(ATT_THREADS), 0, (hipStream_t)stream, q, k, bstride, L, P, d, N);
    return ffc::launch_status("ffc_attnw_matrix");
}

extern "C" int ffc_attnw_backward(const float* dy, const float* q, const float* k, const float* v, long long bstride,
                                  const float* o, const float* L, const float* gamma, float* dq, float* dk, float* dv,
                                  long long gbstride, float* dgamma, float* ws, int B, int C, int H, int W,
                                  void* stream) {
    ATTW_CHECK_SHAPE("ffc_attnw_backward");
    FFC_CHECK_ARG(dy && q && k && v && o && L && gamma && dq && dk && dv && dgamma && ws,
                  "ffc_attnw_backward: null pointer");
    const int N = H * W, d = C / 8;
    FFC_CHECK_ARG(bstride >= (long long)(2 * d + C) * N && gbstride >= (long long)(2 * d + C) * N,
                  "ffc_attnw_backward: batch stride below (2d + C) N");
    const int vec = N % 4 == 0 && bstride % 4 == 0 && aligned16(q) && aligned16(k) && aligned16(dy) && aligned16(L) &&
                    aligned16(ws);
    const int chunks = (N + PREP_THREADS - 1) / PREP_THREADS;
    float* Dn = ws;
    float* part = ws + (size_t)B * N;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(attn_bwd_prep_kernel, dim3(chunks, B), dim3(PREP_THREADS), 0, st, dy, o, Dn, part, C, N);
    hipLaunchKernelGGL(attn_dgamma_kernel, dim3(1), dim3(PREP_THREADS), 0, st, part, B * chunks, dgamma);
    const int tiles = (N + 32 * ATT_WAVES - 1) / (32 * ATT_WAVES);
    hipLaunchKernelGGL(attnw_bwd_v_kernel, dim3(tiles, (C + ATTW_GC - 1) / ATTW_GC, B), dim3(ATT_THREADS), 0, st, dy, q,
                       k, bstride, L, gamma, dv, gbstride, C, d, N, vec);
    launch_bwd_qk(dim3(tiles, B), st, dy, q, k, v, bstride, L, Dn, gamma, dq, dk, gbstride, C, d, N, vec);
    return ffc::launch_status("ffc_attnw_backward");
}
