// Improved precision and recall (torch_fidelity metric_prc.py:57-66) from two feature matrices on gfx950: fp32
// features in, everything else fp64, squared distances throughout.  See include/ffc_amd.h for the formulas.
//
//   norms     a wave per row of F1 and F2: n[i] = sum_k x_ik^2 (lane l adds k = l, l + 64, ..., then the xor tree);
//             lane 0 also zeroes the row's hit flag, so the call needs no memset
//   radii     grid (row tiles of 64) x (column strips of PRC_STRIP_TILES tiles): a workgroup walks the column tiles
//             of its strip, forms each 64 x 64 tile d2 = max(0, n_i + n_j - 2 g_ij) with g on the fp64 MFMA (the KID
//             tile loop), lays it over the operand images in LDS and lets thread (row, quarter) fold 16 columns
//             into its sorted list of the 8 smallest; at the end the four lists of a row are merged and the
//             k + 1 smallest go to the workspace
//   finish    a thread per row merges the strips' candidates; r2 is the (k + 1)-th smallest
//   coverage  a workgroup per 64 x 64 tile of (F2 rows) x (F1 columns): the OR of d2 <= r1[j] per row and of
//             d2 <= r2[i] per column is formed in LDS, then the constant 1 is stored to hit_2 / hit_1
//   counts    one workgroup sums the flags as doubles
// The smallest k + 1 of a multiset and an OR of constants do not depend on the order of visits, and a tile's d2
// does not depend on which strip or workgroup forms it: no atomics, results are bitwise reproducible and
// independent of the strip length and the device's CU count.
#include "ffc_internal.h"
#include "mfma_f64_tile.h"

#include <cmath>

namespace {

constexpr int PRC_THREADS = 256;
constexpr int PRC_TILE = 64;
constexpr int PRC_LD = ffc::MT_KC + 4;        // operand images [row][k]: 36 doubles per row
constexpr int PRC_IMG_LD = PRC_TILE + 1;      // the d2 tile laid over both operand images: 65 doubles per row
constexpr int PRC_SM = 2 * PRC_TILE * PRC_LD; // doubles of LDS: 36.9 KB
constexpr int PRC_STRIP_TILES = 16;           // column tiles per strip (1024 columns)
constexpr int PRC_KEEP = 8;                   // minima tracked per row: neighborhood + 1 <= 8
constexpr int PRC_MAX_D = 4096;
constexpr int PRC_MAX_TILES = 65535;          // gridDim.y
static_assert(PRC_TILE * PRC_IMG_LD <= PRC_SM && PRC_TILE * 4 * PRC_KEEP <= PRC_SM, "the overlays fit the images");

using ffc::block_sum_f64;
using ffc::mma_chunk;
using ffc::MT_KC;
using ffc::wave_sum_f64;
using ffc::zero_acc;

// best: ascending, the PRC_KEEP smallest values seen (with multiplicity)
__device__ __forceinline__ void keep_smallest(double (&best)[PRC_KEEP], double v) {
    if (v < best[PRC_KEEP - 1]) {
        best[PRC_KEEP - 1] = v;
#pragma unroll
        for (int i = PRC_KEEP - 1; i > 0; --i) {
            const double lo = fmin(best[i - 1], best[i]), hi = fmax(best[i - 1], best[i]);
            best[i - 1] = lo;
            best[i] = hi;
        }
    }
}

// rows of the feature matrix that thread tid stages for tile t: tile row (tid >> 5) + 8 q, -1 behind N (zeros)
__device__ __forceinline__ void tile_rows(int t, long long N, long long (&rows)[8]) {
    const int r0 = threadIdx.x >> 5;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const long long i = (long long)t * PRC_TILE + r0 + 8 * q;
        rows[q] = i < N ? i : -1;
    }
}

// acc <- FA[ra] FB[rb]^T over all of D, k ascending in chunks of MT_KC; As, Bs: PRC_TILE * PRC_LD doubles each.
// Starts with a barrier, so whatever read the images before is done; ends without one.
__device__ __forceinline__ void gram_tile(const float* FA, const long long (&ra)[8], const float* FB,
                                          const long long (&rb)[8], int D, double* As, double* Bs, int wi, int wj,
                                          doublex4 (&acc)[2][2]) {
    const int k = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    zero_acc(acc);
    for (int k0 = 0; k0 < D; k0 += MT_KC) {
        const bool kin = k0 + k < D;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = r0 + 8 * q;
            As[r * PRC_LD + k] = ra[q] >= 0 && kin ? (double)FA[ra[q] * D + k0 + k] : 0.0;
            Bs[r * PRC_LD + k] = rb[q] >= 0 && kin ? (double)FB[rb[q] * D + k0 + k] : 0.0;
        }
        __syncthreads();
        mma_chunk<PRC_LD, 1>(As, Bs, wi, wj, acc);
    }
}

// ------------------------------------------------------------------ norms (and the zeroed flags)
__global__ __launch_bounds__(PRC_THREADS) void prc_norms_kernel(const float* F1, long long N1, const float* F2,
                                                                long long N2, int D, double* norms, int* hit_1,
                                                                int* hit_2) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (PRC_THREADS / 64) + (threadIdx.x >> 6);
    if (row >= N1 + N2) return;
    const bool first = row < N1;
    const float* x = first ? F1 + row * D : F2 + (row - N1) * D;
    double s = 0.0;
    for (int k = lane; k < D; k += 64) {
        const double v = (double)x[k];
        s += v * v;
    }
    s = wave_sum_f64(s);
    if (lane == 0) {
        norms[row] = s;
        if (first) hit_1[row] = 0;
        else hit_2[row - N1] = 0;
    }
}

// ------------------------------------------------------------------ radii: the k + 1 smallest of a strip per row
__global__ __launch_bounds__(PRC_THREADS) void prc_radii_kernel(const float* F, long long N, int D, const double* norms,
                                                                int T, int K1, double* cand) {
    const int ti = blockIdx.x, strip = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ double sm[PRC_SM];
    double* As = sm;
    double* Bs = sm + PRC_TILE * PRC_LD;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    long long ra[8], rb[8];
    tile_rows(ti, N, ra);
    double nrow[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long gi = (long long)ti * PRC_TILE + wi + 16 * a + (lane >> 4) + 4 * r;
            nrow[a][r] = gi < N ? norms[gi] : 0.0;
        }
    double best[PRC_KEEP];
#pragma unroll
    for (int c = 0; c < PRC_KEEP; ++c) best[c] = INFINITY;
    const int srow = tid & 63, sq = tid >> 6;   // the selection's map: a row and a quarter of its columns
    const int t_end = min(T, (strip + 1) * PRC_STRIP_TILES);
    doublex4 acc[2][2];
    for (int tj = strip * PRC_STRIP_TILES; tj < t_end; ++tj) {
        tile_rows(tj, N, rb);
        gram_tile(F, ra, F, rb, D, As, Bs, wi, wj, acc);
        __syncthreads();   // every wave has read its fragments: the d2 tile overlays the images
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int lj = wj + 16 * b + (lane & 15);
            const long long gj = (long long)tj * PRC_TILE + lj;
            const bool col = gj < N;
            const double ncol = col ? norms[gj] : 0.0;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int li = wi + 16 * a + (lane >> 4) + 4 * r;
                    // a column behind N never enters a list
                    sm[li * PRC_IMG_LD + lj] = col ? fmax(0.0, nrow[a][r] + ncol - 2.0 * acc[a][b][r]) : INFINITY;
                }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 16; ++c) keep_smallest(best, sm[srow * PRC_IMG_LD + sq * 16 + c]);
    }
    __syncthreads();   // the last tile's reads; the four lists of each row overlay the tile
#pragma unroll
    for (int c = 0; c < PRC_KEEP; ++c) sm[(srow * 4 + sq) * PRC_KEEP + c] = best[c];
    __syncthreads();
    const long long gi = (long long)ti * PRC_TILE + tid;
    if (tid < PRC_TILE && gi < N) {
        double m[PRC_KEEP];
#pragma unroll
        for (int c = 0; c < PRC_KEEP; ++c) m[c] = INFINITY;
        for (int x = 0; x < 4 * PRC_KEEP; ++x) keep_smallest(m, sm[tid * 4 * PRC_KEEP + x]);
        double* out = cand + ((size_t)strip * N + gi) * K1;
#pragma unroll
        for (int c = 0; c < PRC_KEEP; ++c)
            if (c < K1) out[c] = m[c];
    }
}

// ------------------------------------------------------------------ radii finish: the (k + 1)-th smallest of a row
__global__ __launch_bounds__(PRC_THREADS) void prc_radii_finish_kernel(const double* cand, long long N, int S, int K1,
                                                                       double* radii2) {
    const long long row = (long long)blockIdx.x * PRC_THREADS + threadIdx.x;
    if (row >= N) return;
    double m[PRC_KEEP];
#pragma unroll
    for (int c = 0; c < PRC_KEEP; ++c) m[c] = INFINITY;
    for (int s = 0; s < S; ++s) {
        const double* p = cand + ((size_t)s * N + row) * K1;
        for (int c = 0; c < K1; ++c) keep_smallest(m, p[c]);
    }
    double r = m[0];
#pragma unroll
    for (int c = 1; c < PRC_KEEP; ++c)
        if (c == K1 - 1) r = m[c];
    radii2[row] = r;
}

// ------------------------------------------------------------------ coverage: rows from F2, columns from F1
struct PrcCoverArgs {
    const float* F1;
    const float* F2;
    long long N1, N2;
    int D;
    const double* norms1;
    const double* norms2;
    const double* radii2_1;
    const double* radii2_2;
    int* hit_2;
    int* hit_1;
};

__global__ __launch_bounds__(PRC_THREADS) void prc_cover_kernel(PrcCoverArgs p) {
    const int tj = blockIdx.x, ti = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ double sm[PRC_SM];
    __shared__ int row_hit[PRC_TILE];
    __shared__ int col_hit[PRC_TILE];
    // the tile loop's barriers (D >= 1: at least two) stand between these stores and the epilogue's
    if (tid < PRC_TILE) row_hit[tid] = 0;
    else if (tid < 2 * PRC_TILE) col_hit[tid - PRC_TILE] = 0;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    long long ra[8], rb[8];
    tile_rows(ti, p.N2, ra);
    tile_rows(tj, p.N1, rb);
    doublex4 acc[2][2];
    gram_tile(p.F2, ra, p.F1, rb, p.D, sm, sm + PRC_TILE * PRC_LD, wi, wj, acc);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int lj = wj + 16 * b + (lane & 15);
        const long long gj = (long long)tj * PRC_TILE + lj;
        if (gj >= p.N1) continue;
        const double ncol = p.norms1[gj], rcol = p.radii2_1[gj];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int li = wi + 16 * a + (lane >> 4) + 4 * r;
                const long long gi = (long long)ti * PRC_TILE + li;
                if (gi < p.N2) {
                    const double d2 = fmax(0.0, p.norms2[gi] + ncol - 2.0 * acc[a][b][r]);
                    if (d2 <= rcol) row_hit[li] = 1;             // F2[gi] lies in the ball of F1[gj]
                    if (d2 <= p.radii2_2[gi]) col_hit[lj] = 1;   // F1[gj] lies in the ball of F2[gi]
                }
            }
    }
    __syncthreads();
    // an OR of constants: any number of workgroups may store the same 1
    if (tid < PRC_TILE) {
        if (row_hit[tid]) p.hit_2[(long long)ti * PRC_TILE + tid] = 1;
    } else if (tid < 2 * PRC_TILE) {
        if (col_hit[tid - PRC_TILE]) p.hit_1[(long long)tj * PRC_TILE + tid - PRC_TILE] = 1;
    }
}

// ------------------------------------------------------------------ counts = [sum hit_2, sum hit_1]
__global__ __launch_bounds__(PRC_THREADS) void prc_counts_kernel(const int* hit_2, long long N2, const int* hit_1,
                                                                 long long N1, double* counts) {
    const int tid = threadIdx.x;
    __shared__ double red[4];
    double s2 = 0.0, s1 = 0.0;
    for (long long i = tid; i < N2; i += PRC_THREADS) s2 += (double)hit_2[i];
    for (long long i = tid; i < N1; i += PRC_THREADS) s1 += (double)hit_1[i];
    s2 = block_sum_f64(s2, red);
    s1 = block_sum_f64(s1, red);
    if (tid == 0) {
        counts[0] = s2;
        counts[1] = s1;
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

long long prc_tiles(long long N) { return (N + PRC_TILE - 1) / PRC_TILE; }

long long prc_strips(long long N) { return (prc_tiles(N) + PRC_STRIP_TILES - 1) / PRC_STRIP_TILES; }

bool prc_sizes_ok(long long N1, long long N2, int neighborhood) {
    return neighborhood >= 1 && neighborhood + 1 <= PRC_KEEP && N1 >= neighborhood + 1 && N2 >= neighborhood + 1 &&
           prc_tiles(N1) <= PRC_MAX_TILES && prc_tiles(N2) <= PRC_MAX_TILES;
}

}  // namespace

// ws = [norms of F1 (N1), norms of F2 (N2), the strips' candidates of one set at a time]
extern "C" size_t ffc_prc_ws_bytes(long long N1, long long N2, int neighborhood) {
    if (!prc_sizes_ok(N1, N2, neighborhood)) return 0;
    const size_t c1 = (size_t)prc_strips(N1) * (size_t)N1, c2 = (size_t)prc_strips(N2) * (size_t)N2;
    return sizeof(double) * ((size_t)N1 + (size_t)N2 + (c1 > c2 ? c1 : c2) * (size_t)(neighborhood + 1));
}

extern "C" int ffc_prc(const float* F1, long long N1, const float* F2, long long N2, int D, int neighborhood,
                       double* radii2_1, double* radii2_2, int* hit_2, int* hit_1, double* counts, void* ws,
                       size_t ws_bytes, void* stream) {
    FFC_CHECK_ARG(F1 && F2 && aligned(F1, 4) && aligned(F2, 4), "ffc_prc: F1 or F2 null or not aligned to 4 bytes");
    FFC_CHECK_ARG(radii2_1 && radii2_2 && aligned(radii2_1, 8) && aligned(radii2_2, 8),
                  "ffc_prc: radii2_1 or radii2_2 null or not aligned to 8 bytes");
    FFC_CHECK_ARG(hit_2 && hit_1 && aligned(hit_2, 4) && aligned(hit_1, 4),
                  "ffc_prc: hit_2 or hit_1 null or not aligned to 4 bytes");
    FFC_CHECK_ARG(counts && ws && aligned(counts, 8) && aligned(ws, 8), "ffc_prc: counts or ws null or not aligned to 8 bytes");
    FFC_CHECK_ARG(D >= 1 && D <= PRC_MAX_D, "ffc_prc: D out of range (1 .. 4096)");
    FFC_CHECK_ARG(neighborhood >= 1 && neighborhood + 1 <= PRC_KEEP, "ffc_prc: neighborhood out of range (1 .. 7)");
    FFC_CHECK_ARG(N1 >= neighborhood + 1 && N2 >= neighborhood + 1, "ffc_prc: N1, N2 >= neighborhood + 1");
    FFC_CHECK_ARG(prc_sizes_ok(N1, N2, neighborhood), "ffc_prc: N1 or N2 too large (64 * 65535 rows)");
    FFC_CHECK_ARG(ws_bytes >= ffc_prc_ws_bytes(N1, N2, neighborhood), "ffc_prc: workspace too small (ffc_prc_ws_bytes)");
    hipStream_t st = (hipStream_t)stream;
    const int K1 = neighborhood + 1;
    double* norms1 = (double*)ws;
    double* norms2 = norms1 + N1;
    double* cand = norms2 + N2;
    const long long rows = N1 + N2;
    hipLaunchKernelGGL(prc_norms_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(PRC_THREADS), 0, st, F1, N1, F2, N2, D,
                       norms1, hit_1, hit_2);
    const float* F[2] = {F1, F2};
    const long long N[2] = {N1, N2};
    const double* norms[2] = {norms1, norms2};
    double* radii[2] = {radii2_1, radii2_2};
    for (int s = 0; s < 2; ++s) {   // the candidates of F1 are merged before those of F2 take their place
        const int T = (int)prc_tiles(N[s]), S = (int)prc_strips(N[s]);
        hipLaunchKernelGGL(prc_radii_kernel, dim3(T, S), dim3(PRC_THREADS), 0, st, F[s], N[s], D, norms[s], T, K1, cand);
        hipLaunchKernelGGL(prc_radii_finish_kernel, dim3((unsigned)((N[s] + PRC_THREADS - 1) / PRC_THREADS)),
                           dim3(PRC_THREADS), 0, st, (const double*)cand, N[s], S, K1, radii[s]);
    }
    const PrcCoverArgs p{F1, F2, N1, N2, D, norms1, norms2, radii2_1, radii2_2, hit_2, hit_1};
    hipLaunchKernelGGL(prc_cover_kernel, dim3((unsigned)prc_tiles(N1), (unsigned)prc_tiles(N2)), dim3(PRC_THREADS), 0, st, p);
    hipLaunchKernelGGL(prc_counts_kernel, dim3(1), dim3(PRC_THREADS), 0, st, (const int*)hit_2, N2, (const int*)hit_1, N1,
                       counts);
    return ffc::launch_status("ffc_prc");
}
