// Metric arithmetic of torch_fidelity (metric_fid.py, metric_kid.py, metric_isc.py) from feature batches on
// gfx950: fp32 features / logits in, every accumulation fp64.  See include/ffc_amd.h for the formulas.
//
//   moments  A  pivot / s1 : 32 columns x 8 row groups per workgroup; the first call on an empty state forms the
//                            batch's column mean (the pivot), every call adds sum (x - pivot) to s1
//            B  S2         : one workgroup owns one 64 x 64 tile of the upper triangle, walks the whole batch in
//                            chunks of 32 rows staged pivoted and converted in LDS, four waves of 2 x 2
//                            v_mfma_f64_16x16x4_f64 tiles, then adds its tile to S2 in place and mirrors it
//   KID      A  tiles      : one workgroup per (subset, pair, 64 x 64 tile): rows gathered through the index table
//                            while staging, the Gram tile on the fp64 MFMA, (gamma g + c0)^degree and the two sums
//                            in the epilogue; XX and YY run their upper triangle only
//            B  finish     : one workgroup per subset adds the tile partials in tile order
//   ISC      A  rows       : a wave per row (16 columns per lane in registers), 128 rows per workgroup
//            B  finish     : one workgroup per chunk
// Every sum has a fixed place in a fixed order (k ascending inside a tile, lanes by xor shuffles, waves in order,
// partials by index): no atomics, results are bitwise reproducible and independent of the device's CU count.
//
// The fp64 MFMA tile loop (mma_chunk, zero_acc) and its fragment maps are in mfma_f64_tile.h.
#include "ffc_internal.h"
#include "mfma_f64_tile.h"

#include <cmath>

namespace {

using ffc::block_sum_f64;
using ffc::mma_chunk;
using ffc::MT_KC;
using ffc::wave_sum_f64;
using ffc::zero_acc;

constexpr int MT_THREADS = 256;
constexpr int MT_TILE = 64;      // output tile side of a workgroup (moments S2, KID Gram)
constexpr int FM_LD = MT_TILE + 8;   // moments LDS image [k][column]: 72 doubles per k row
constexpr int KID_LD = MT_KC + 4;    // KID LDS image [row][k]: 36 doubles per row
constexpr int FM_COLS = 32, FM_GROUPS = 8;   // kernel A of the moments
constexpr int ISC_CPL = 16;      // logits columns per lane: C <= 1024
constexpr int ISC_ROWS = 128;    // rows per workgroup
constexpr int ISC_MAX_C = 64 * ISC_CPL;
constexpr int FM_MAX_D = 2048;

// ------------------------------------------------------------------ moments A: pivot and s1
// state = [n, pivot[D], s1[D], S2[D][D]]
__global__ __launch_bounds__(MT_THREADS) void fm_pivot_kernel(const float* X, int B, int D, double* state) {
    const int tid = threadIdx.x, c = tid & (FM_COLS - 1), g = tid / FM_COLS;
    const int col = blockIdx.x * FM_COLS + c;
    const bool live = col < D;
    const bool first = state[0] == 0.0;
    double* pivot = state + 1;
    double* s1 = pivot + D;
    __shared__ double red[FM_GROUPS][FM_COLS];
    double piv = 0.0;
    if (first) {
        double s = 0.0;
        if (live)
            for (int r = g; r < B; r += FM_GROUPS) s += (double)X[(long long)r * D + col];
        red[g][c] = s;
        __syncthreads();
        s = 0.0;
#pragma unroll
        for (int q = 0; q < FM_GROUPS; ++q) s += red[q][c];
        piv = s / (double)B;
        __syncthreads();
    } else if (live) {
        piv = pivot[col];
    }
    double s = 0.0;
    if (live)
        for (int r = g; r < B; r += FM_GROUPS) s += (double)X[(long long)r * D + col] - piv;
    red[g][c] = s;
    __syncthreads();
    if (g == 0 && live) {
        s = 0.0;
#pragma unroll
        for (int q = 0; q < FM_GROUPS; ++q) s += red[q][c];
        if (first) pivot[col] = piv;
        s1[col] += s;
    }
}

// ------------------------------------------------------------------ moments B: S2 += (X - p)^T (X - p)
__global__ __launch_bounds__(MT_THREADS) void fm_s2_kernel(const float* X, int B, int D, double* state, int T) {
    int bi = 0, rem = blockIdx.x;
    while (rem >= T - bi) {
        rem -= T - bi;
        ++bi;
    }
    const int bj = bi + rem;
    const bool diag = bi == bj;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* pivot = state + 1;
    double* S2 = state + 1 + 2 * (size_t)D;
    __shared__ double As[MT_KC * FM_LD];
    __shared__ double Bs[MT_KC * FM_LD];
    const int c = tid & 63, r0 = tid >> 6;
    const int ci = bi * MT_TILE + c, cj = bj * MT_TILE + c;
    const double pi = ci < D ? pivot[ci] : 0.0, pj = cj < D ? pivot[cj] : 0.0;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    doublex4 acc[2][2];
    zero_acc(acc);
    for (int k0 = 0; k0 < B; k0 += MT_KC) {
        __syncthreads();   // the previous chunk's reads
#pragma unroll
        for (int q = 0; q < MT_KC / 4; ++q) {
            const int r = r0 + 4 * q;
            const bool row = k0 + r < B;
            const float* x = X + (long long)(k0 + r) * D;
            As[r * FM_LD + c] = row && ci < D ? (double)x[ci] - pi : 0.0;
            if (!diag) Bs[r * FM_LD + c] = row && cj < D ? (double)x[cj] - pj : 0.0;
        }
        __syncthreads();
        mma_chunk<1, FM_LD>(As, diag ? As : Bs, wi, wj, acc);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = bi * MT_TILE + wi + 16 * a + (lane >> 4) + 4 * r;
                const int gj = bj * MT_TILE + wj + 16 * b + (lane & 15);
                if (gi < D && gj < D && gi <= gj) {   // the upper triangle owns the value; the mirror copies it
                    const double v = S2[(size_t)gi * D + gj] + acc[a][b][r];
                    S2[(size_t)gi * D + gj] = v;
                    if (gi != gj) S2[(size_t)gj * D + gi] = v;
                }
            }
    // the pivot kernel of this call has read n; the next call's reads it after this kernel
    if (blockIdx.x == 0 && tid == 0) state[0] += (double)B;
}

// ------------------------------------------------------------------ KID A: Gram tiles
struct KidArgs {
    const float* F1;
    const float* F2;
    const long long* idx1;
    const long long* idx2;
    long long N1, N2;
    int m, D, degree, T;
    double gamma, coef0;
};

__global__ __launch_bounds__(MT_THREADS) void kid_tiles_kernel(KidArgs p, double* part) {
    const int s = blockIdx.z, pair = blockIdx.y, ti = blockIdx.x / p.T, tj = blockIdx.x % p.T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* out = part + 2 * (((size_t)s * 3 + pair) * p.T * p.T + blockIdx.x);
    if (pair < 2 && ti > tj) {   // symmetric pairs: the finish kernel counts the upper tiles twice
        if (tid == 0) out[0] = out[1] = 0.0;
        return;
    }
    const float* FA = pair == 1 ? p.F2 : p.F1;
    const float* FB = pair == 0 ? p.F1 : p.F2;
    const long long NA = pair == 1 ? p.N2 : p.N1, NB = pair == 0 ? p.N1 : p.N2;
    const long long* IA = (pair == 1 ? p.idx2 : p.idx1) + (size_t)s * p.m;
    const long long* IB = (pair == 0 ? p.idx1 : p.idx2) + (size_t)s * p.m;
    __shared__ double As[MT_TILE * KID_LD];
    __shared__ double Bs[MT_TILE * KID_LD];
    __shared__ double red[4];
    const int k = tid & 31, r0 = tid >> 5;
    // row of the feature matrix per staged row: -1 a tile row behind m (zeros), -2 an index out of range (NaN)
    long long ra[8], rb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int ia = ti * MT_TILE + r0 + 8 * q, ib = tj * MT_TILE + r0 + 8 * q;
        ra[q] = rb[q] = -1;
        if (ia < p.m) {
            const long long v = IA[ia];
            ra[q] = v >= 0 && v < NA ? v : -2;
        }
        if (ib < p.m) {
            const long long v = IB[ib];
            rb[q] = v >= 0 && v < NB ? v : -2;
        }
    }
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    const double qnan = __builtin_nan("");
    doublex4 acc[2][2];
    zero_acc(acc);
    for (int k0 = 0; k0 < p.D; k0 += MT_KC) {
        const bool kin = k0 + k < p.D;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = r0 + 8 * q;
            double a = 0.0, b = 0.0;
            if (ra[q] == -2) a = qnan;
            else if (ra[q] >= 0 && kin) a = (double)FA[ra[q] * p.D + k0 + k];
            if (rb[q] == -2) b = qnan;
            else if (rb[q] >= 0 && kin) b = (double)FB[rb[q] * p.D + k0 + k];
            As[r * KID_LD + k] = a;
            Bs[r * KID_LD + k] = b;
        }
        __syncthreads();
        mma_chunk<KID_LD, 1>(As, Bs, wi, wj, acc);
    }
    double sum = 0.0, dg = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = ti * MT_TILE + wi + 16 * a + (lane >> 4) + 4 * r;
                const int gj = tj * MT_TILE + wj + 16 * b + (lane & 15);
                if (gi < p.m && gj < p.m) {
                    const double v = p.gamma * acc[a][b][r] + p.coef0;
                    double kv = v;
                    for (int d = 1; d < p.degree; ++d) kv *= v;
                    sum += kv;
                    if (gi == gj) dg += kv;
                }
            }
    sum = block_sum_f64(sum, red);
    dg = block_sum_f64(dg, red);
    if (tid == 0) {
        out[0] = sum;
        out[1] = dg;
    }
}

// ------------------------------------------------------------------ KID B: six sums per subset
__global__ __launch_bounds__(MT_THREADS) void kid_finish_kernel(KidArgs p, const double* part, double* sums) {
    const int s = blockIdx.x, tid = threadIdx.x;
    __shared__ double red[4];
    double bad = 0.0;
    for (int i = tid; i < p.m; i += MT_THREADS) {
        const long long a = p.idx1[(size_t)s * p.m + i], b = p.idx2[(size_t)s * p.m + i];
        if (a < 0 || a >= p.N1 || b < 0 || b >= p.N2) bad += 1.0;
    }
    bad = block_sum_f64(bad, red);
    const int TT = p.T * p.T;
    double res[6];
    for (int pair = 0; pair < 3; ++pair) {
        const double* q = part + 2 * ((size_t)s * 3 + pair) * TT;
        double sum = 0.0, dg = 0.0;
        for (int x = tid; x < TT; x += MT_THREADS) {
            const double w = pair < 2 && x / p.T < x % p.T ? 2.0 : 1.0;
            sum += w * q[2 * x];
            dg += q[2 * x + 1];
        }
        res[2 * pair] = block_sum_f64(sum, red);
        res[2 * pair + 1] = block_sum_f64(dg, red);
    }
    if (tid == 0)
        for (int i = 0; i < 6; ++i) sums[6 * (size_t)s + i] = bad != 0.0 ? __builtin_nan("") : res[i];
}

// ------------------------------------------------------------------ ISC A: rows
__device__ __forceinline__ long long isc_chunk_begin(long long N, int splits, int i) { return (long long)i * N / splits; }

// partial of workgroup b of chunk i: [sum p log p, colsum[C], complement[C]], complement = sum (1 - p)
__global__ __launch_bounds__(MT_THREADS) void isc_rows_kernel(const float* logits, const long long* perm, long long N,
                                                              int C, int splits, int nb, double* part) {
    const int chunk = blockIdx.y, b = blockIdx.x;
    const long long r_begin = isc_chunk_begin(N, splits, chunk), r_end = isc_chunk_begin(N, splits, chunk + 1);
    const long long first = r_begin + (long long)b * ISC_ROWS;
    if (first >= r_end) return;   // the finish kernel reads the first ceil(n_i / ISC_ROWS) partials only
    const int rows = (int)min((long long)ISC_ROWS, r_end - first);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ double cs_l[ISC_MAX_C];
    __shared__ double ct_l[ISC_MAX_C];
    __shared__ double pl_l[4];
    double cs[ISC_CPL], ct[ISC_CPL], pl = 0.0;
#pragma unroll
    for (int q = 0; q < ISC_CPL; ++q) cs[q] = ct[q] = 0.0;
    const float qnan = __builtin_nanf("");
    for (int r = wave; r < rows; r += 4) {
        const long long src = perm[first + r];
        const bool ok = src >= 0 && src < N;   // an index out of range forms no address: the row is NaN
        const float* x = logits + (ok ? src : 0) * C;
        float v[ISC_CPL];
        float mx = -INFINITY;
        int imx = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < ISC_CPL; ++q) {
            const int c = lane + 64 * q;
            v[q] = c < C ? (ok ? x[c] : qnan) : -INFINITY;
            if (c < C && v[q] > mx) {
                mx = v[q];
                imx = c;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float om = __shfl_xor(mx, off, 64);
            const int oi = __shfl_xor(imx, off, 64);
            if (om > mx || (om == mx && oi < imx)) {
                mx = om;
                imx = oi;
            }
        }
        // log-sum-exp around the first maximum, its own term left out of the sum: L = log1p(rest) keeps
        // log p of a peaked row to its relative accuracy
        double e[ISC_CPL], rest = 0.0;
#pragma unroll
        for (int q = 0; q < ISC_CPL; ++q) {
            const int c = lane + 64 * q;
            e[q] = c < C && c != imx ? exp((double)v[q] - (double)mx) : 0.0;
            rest += e[q];
        }
        rest = wave_sum_f64(rest);
        const double L = log1p(rest), inv = 1.0 / (1.0 + rest);
#pragma unroll
        for (int q = 0; q < ISC_CPL; ++q) {
            const int c = lane + 64 * q;
            if (c < C) {
                const bool top = c == imx;
                const double prob = top ? inv : e[q] * inv;
                const double logp = top ? -L : ((double)v[q] - (double)mx) - L;
                pl += prob * logp;
                cs[q] += prob;
                ct[q] += top ? rest * inv : 1.0 - prob;
            }
        }
    }
    pl = wave_sum_f64(pl);
    if (lane == 0) pl_l[wave] = pl;
    for (int w = 0; w < 4; ++w) {   // the four waves in order
        if (wave == w) {
#pragma unroll
            for (int q = 0; q < ISC_CPL; ++q) {
                const int c = lane + 64 * q;
                if (c < C) {
                    cs_l[c] = w ? cs_l[c] + cs[q] : cs[q];
                    ct_l[c] = w ? ct_l[c] + ct[q] : ct[q];
                }
            }
        }
        __syncthreads();
    }
    double* out = part + ((size_t)chunk * nb + b) * (1 + 2 * (size_t)C);
    if (tid == 0) out[0] = (pl_l[0] + pl_l[1]) + (pl_l[2] + pl_l[3]);
    for (int c = tid; c < C; c += MT_THREADS) {
        out[1 + c] = cs_l[c];
        out[1 + C + c] = ct_l[c];
    }
}

// ------------------------------------------------------------------ ISC B: per chunk [n_i, sum p log p, exponent,
// score, colsum[C]]
__global__ __launch_bounds__(MT_THREADS) void isc_finish_kernel(const double* part, long long N, int C, int splits, int nb,
                                                                double* out) {
    const int chunk = blockIdx.x, tid = threadIdx.x;
    const long long cnt = isc_chunk_begin(N, splits, chunk + 1) - isc_chunk_begin(N, splits, chunk);
    const int nbi = (int)((cnt + ISC_ROWS - 1) / ISC_ROWS);
    const size_t stride = 1 + 2 * (size_t)C;
    const double* p = part + (size_t)chunk * nb * stride;
    double* o = out + (size_t)chunk * (4 + (size_t)C);
    const double n = (double)cnt;
    __shared__ double red[4];
    double cross = 0.0;   // sum_c colsum_c log(colsum_c / n)
    for (int c = tid; c < C; c += MT_THREADS) {
        double s = 0.0, t = 0.0;
        for (int b = 0; b < nbi; ++b) {
            s += p[b * stride + 1 + c];
            t += p[b * stride + 1 + C + c];
        }
        o[4 + c] = s;
        // log q from the complement where q is near 1: log(1 - t / n) keeps what the rounding of colsum drops
        const double frac = t / n;
        const double lq = frac < 0.5 ? log1p(-frac) : log(s / n);
        cross += s > 0.0 ? s * lq : s;   // 0 log 0 = 0; NaN stays NaN
    }
    cross = block_sum_f64(cross, red);
    double pl = 0.0;
    for (int b = tid; b < nbi; b += MT_THREADS) pl += p[b * stride];
    pl = block_sum_f64(pl, red);
    if (tid == 0) {
        const double ex = (pl - cross) / n;
        o[0] = n;
        o[1] = pl;
        o[2] = ex;
        o[3] = exp(ex);
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int isc_blocks(long long N, int splits) { return (int)((N / splits + 1 + ISC_ROWS - 1) / ISC_ROWS); }

int kid_tiles(int m) { return (m + MT_TILE - 1) / MT_TILE; }

}  // namespace

extern "C" size_t ffc_feat_moments_state_doubles(int D) {
    if (D < 1 || D > FM_MAX_D) return 0;
    return 1 + 2 * (size_t)D + (size_t)D * D;
}

extern "C" int ffc_feat_moments_update(const float* X, int B, int D, double* state, void* stream) {
    FFC_CHECK_ARG(X && aligned(X, 4), "ffc_feat_moments_update: X null or not aligned to 4 bytes");
    FFC_CHECK_ARG(state && aligned(state, 8), "ffc_feat_moments_update: state null or not aligned to 8 bytes");
    FFC_CHECK_ARG(B >= 1, "ffc_feat_moments_update: B >= 1");
    FFC_CHECK_ARG(D >= 1 && D <= FM_MAX_D, "ffc_feat_moments_update: D out of range (1 .. 2048)");
    hipStream_t st = (hipStream_t)stream;
    const int T = (D + MT_TILE - 1) / MT_TILE;
    hipLaunchKernelGGL(fm_pivot_kernel, dim3((D + FM_COLS - 1) / FM_COLS), dim3(MT_THREADS), 0, st, X, B, D, state);
    hipLaunchKernelGGL(fm_s2_kernel, dim3(T * (T + 1) / 2), dim3(MT_THREADS), 0, st, X, B, D, state, T);
    return ffc::launch_status("ffc_feat_moments_update");
}

extern "C" size_t ffc_kid_ws_doubles(int subsets, int m) {
    if (subsets < 1 || m < 2) return 0;
    const size_t T = (size_t)kid_tiles(m);
    return 6 * (size_t)subsets * T * T;
}

extern "C" int ffc_kid_sums(const float* F1, long long N1, const float* F2, long long N2, int D, const long long* idx1,
                            const long long* idx2, int subsets, int m, int degree, double gamma, double coef0,
                            double* ws, size_t ws_doubles, double* sums, void* stream) {
    FFC_CHECK_ARG(F1 && F2 && aligned(F1, 4) && aligned(F2, 4), "ffc_kid_sums: F1 or F2 null or not aligned to 4 bytes");
    FFC_CHECK_ARG(idx1 && idx2 && aligned(idx1, 8) && aligned(idx2, 8),
                  "ffc_kid_sums: idx1 or idx2 null or not aligned to 8 bytes");
    FFC_CHECK_ARG(ws && sums && aligned(ws, 8) && aligned(sums, 8), "ffc_kid_sums: ws or sums null or not aligned to 8 bytes");
    FFC_CHECK_ARG(N1 >= 1 && N2 >= 1, "ffc_kid_sums: N1, N2 >= 1");
    FFC_CHECK_ARG(D >= 1 && D <= FM_MAX_D, "ffc_kid_sums: D out of range (1 .. 2048)");
    FFC_CHECK_ARG(m >= 2, "ffc_kid_sums: m < 2");
    FFC_CHECK_ARG(subsets >= 1 && subsets <= 65535, "ffc_kid_sums: subsets out of range (1 .. 65535)");
    FFC_CHECK_ARG(degree >= 1, "ffc_kid_sums: degree >= 1");
    FFC_CHECK_ARG(std::isfinite(gamma) && std::isfinite(coef0), "ffc_kid_sums: gamma and coef0 must be finite");
    const int T = kid_tiles(m);
    FFC_CHECK_ARG((long long)T * T <= 0x7fffffffLL, "ffc_kid_sums: m too large");
    FFC_CHECK_ARG(ws_doubles >= ffc_kid_ws_doubles(subsets, m), "ffc_kid_sums: workspace too small (ffc_kid_ws_doubles)");
    hipStream_t st = (hipStream_t)stream;
    const KidArgs p{F1, F2, idx1, idx2, N1, N2, m, D, degree, T, gamma, coef0};
    hipLaunchKernelGGL(kid_tiles_kernel, dim3(T * T, 3, subsets), dim3(MT_THREADS), 0, st, p, ws);
    hipLaunchKernelGGL(kid_finish_kernel, dim3(subsets), dim3(MT_THREADS), 0, st, p, (const double*)ws, sums);
    return ffc::launch_status("ffc_kid_sums");
}

extern "C" size_t ffc_isc_ws_doubles(long long N, int C, int splits) {
    if (N < 1 || C < 1 || C > ISC_MAX_C || splits < 1 || N < splits) return 0;
    return (size_t)splits * isc_blocks(N, splits) * (1 + 2 * (size_t)C);
}

extern "C" int ffc_isc_sums(const float* logits, long long N, int C, const long long* perm, int splits, double* ws,
                            size_t ws_doubles, double* out, void* stream) {
    FFC_CHECK_ARG(logits && aligned(logits, 4), "ffc_isc_sums: logits null or not aligned to 4 bytes");
    FFC_CHECK_ARG(perm && aligned(perm, 8), "ffc_isc_sums: perm null or not aligned to 8 bytes");
    FFC_CHECK_ARG(ws && out && aligned(ws, 8) && aligned(out, 8), "ffc_isc_sums: ws or out null or not aligned to 8 bytes");
    FFC_CHECK_ARG(C >= 1 && C <= ISC_MAX_C, "ffc_isc_sums: C out of range (1 .. 1024)");
    FFC_CHECK_ARG(splits >= 1 && splits <= 65535, "ffc_isc_sums: splits out of range (1 .. 65535)");
    FFC_CHECK_ARG(N >= splits, "ffc_isc_sums: N < splits (an empty chunk)");
    FFC_CHECK_ARG(N <= 0x7fffffffLL, "ffc_isc_sums: N too large");
    FFC_CHECK_ARG(ws_doubles >= ffc_isc_ws_doubles(N, C, splits), "ffc_isc_sums: workspace too small (ffc_isc_ws_doubles)");
    hipStream_t st = (hipStream_t)stream;
    const int nb = isc_blocks(N, splits);
    hipLaunchKernelGGL(isc_rows_kernel, dim3(nb, splits), dim3(MT_THREADS), 0, st, logits, perm, N, C, splits, nb, ws);
    hipLaunchKernelGGL(isc_finish_kernel, dim3(splits), dim3(MT_THREADS), 0, st, (const double*)ws, N, C, splits, nb, out);
    return ffc::launch_status("ffc_isc_sums");
}
