// Class-conditional fgan128 (fgan128_cond_complete.py:33-180) for gfx950: the generator's label /
// noise stem and the label-embedding row gather / scatter both conditional models use.
//
// Labels are an int64 DEVICE tensor read by the kernels (no host read, no sync): a captured step is
// replayed with new labels written into the same buffer.  A label outside [0, num_classes) never
// forms an address: its gathered row reads as NaN (so that sample's outputs -- and, through train-mode
// BatchNorm statistics, its batch -- are NaN, loudly), and it contributes nothing to any scatter.
//
// Stem forward (:91-101, up to the BatchNorm apply).  ConvTranspose2d(K, 256, 4, 1, 0) on a 1x1 input
// is the product x (B, K) . W (K, 256*4*4) with the weight in its native layout, so
//   pre[b][0:4096]    = z[b] . W_in + bias_in[c]                    (input_conv.0)
//   pre[b][4096:8192] = label_embed[labels[b]] . W_label + bias_label[c]   (label_conv.0)
// land in the two channel halves of one (B, 512, 4, 4) buffer: torch.cat([input, embedding], 1) is
// never materialised separately.  Products on v_mfma_f32_32x32x2_f32 (exact fp32 inputs, fp32
// accumulate): K is at most a few hundred, the kernel is bound by the launch and the W read, and
// the split-bf16 scheme would only add the splitting VALU work.  Workgroup: 32 samples x 128
// columns (8 channels), one 32 x 32 MFMA tile per wave; the epilogue writes the per-channel
// {n, mean, M2} partial row of each tile (bn_common.h slab format, one row per 32-sample tile) for
// the existing reduce / finalize kernels.
//
// Stem backward: deterministic, no float atomics.  dW = A^T . g summed over the samples in order
// by one thread per (k, column); dbias by one wave per channel; dz / d(embedding row) by a
// wave-reduced dot product per (sample, k); d label_embed.weight by the row scatter below.
//
// Row scatter: one workgroup column per class sums the gradient rows of its samples in sample order
// (fixed order: bitwise reproducible); classes absent from the batch get exact zeros.
#include "ffc_internal.h"

#include <cmath>

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_BM = 32;           // samples per workgroup
constexpr int CS_BN = 128;          // columns per workgroup: 4 waves x 32 columns = 8 channels
constexpr int CS_KC = 64;           // k per staged chunk
constexpr int CS_N = 4096;          // 256 channels x 4 x 4: columns per branch
constexpr int CS_CH = 256;          // channels per branch
constexpr int CS_KS = CS_KC + 1;    // LDS row stride (odd: conflict-free column reads)

struct StemArgs {
    const float* z;
    const long long* labels;
    const float* embed;
    const float* w_in;
    const float* b_in;
    const float* w_label;
    const float* b_label;
    float* out;
    float* slab;   // null: no statistics (eval)
    int B, Kz, NC;
};

__device__ __forceinline__ float xor_sum_channel(float v) {
    // the 32 lanes holding one channel of a 32 x 32 tile: 16 columns (lane bits 0..3) x 2 row halves (bit 5)
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

__global__ __launch_bounds__(CS_THREADS) void cond_stem_kernel(StemArgs a) {
    __shared__ float As[CS_BM * CS_KS];
    __shared__ long long lab[CS_BM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, col = lane & 31;
    constexpr int NT = 2 * CS_N / CS_BN;   // column tiles over both branches
    const int bt = blockIdx.x / NT, nt = blockIdx.x - bt * NT;
    const int branch = nt >= NT / 2;
    const int n = (nt - branch * (NT / 2)) * CS_BN + wave * 32 + col;   // column inside the branch
    const int b0 = bt * CS_BM;
    const int K = branch ? a.NC : a.Kz;
    const float* W = branch ? a.w_label : a.w_in;
    const auto rW = ffc::buf_rsrc(W, (unsigned long long)K * CS_N * 4);
    if (tid < CS_BM) lab[tid] = (branch && b0 + tid < a.B) ? a.labels[b0 + tid] : 0;
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += CS_KC) {
        // this lane's W column for the chunk, every load in flight before the A tile is staged
        float wv[CS_KC / 2];
#pragma unroll
        for (int u = 0; u < CS_KC / 2; ++u) {
            const int k = k0 + 2 * u + hh;
            wv[u] = ffc::buf_ld(rW, k < K ? (unsigned)(((size_t)k * CS_N + n) * 4) : ffc::OOB);
        }
        __syncthreads();   // labels staged (first chunk); the previous chunk's A tile consumed
#pragma unroll
        for (int j = 0; j < CS_BM * CS_KC / CS_THREADS; ++j) {
            const int i = j * CS_THREADS + tid, r = i / CS_KC, kk = i - r * CS_KC;
            const int k = k0 + kk, b = b0 + r;
            float v = 0.0f;
            if (k < K && b < a.B) {
                if (branch) {
                    const long long l = lab[r];
                    v = (l >= 0 && l < a.NC) ? a.embed[(size_t)l * a.NC + k] : NAN;
                } else {
                    v = a.z[(size_t)b * a.Kz + k];
                }
            }
            As[r * CS_KS + kk] = v;
        }
        __syncthreads();
        const float* ar = As + col * CS_KS;
#pragma unroll
        for (int u = 0; u < CS_KC / 2; ++u)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[2 * u + hh], wv[u], acc, 0, 0, 0);
    }
    // accumulator: register r of lane l -> sample row (r&3) + 8(r>>2) + 4(l>>5), column l&31
    const int c = n >> 4;   // channel inside the branch
    const float bv = (branch ? a.b_label : a.b_in)[c];
    float* out = a.out + (size_t)branch * CS_N + n;
    const int Bn = a.B;
    float* slab = a.slab;
    const int nv = min(CS_BM, Bn - b0);   // valid sample rows of this tile
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
        acc[r] += bv;
        if (row < nv) {
            out[(size_t)(b0 + row) * (2 * CS_N)] = acc[r];
            s += acc[r];
        }
    }
    if (slab == nullptr) return;
    const float cnt = (float)(nv * 16);
    const float mean = xor_sum_channel(s) / cnt;
    float q = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
        const float d = acc[r] - mean;
        if (row < nv) q = fmaf(d, d, q);
    }
    q = xor_sum_channel(q);
    if ((lane & 47) == 0) {   // column 0 of the channel, first row half
        const int nbt = (Bn + CS_BM - 1) / CS_BM;
        float4* row = reinterpret_cast<float4*>(slab) + ((size_t)branch * nbt + bt) * CS_CH + c;
        *row = make_float4(cnt, mean, q, 0.0f);
    }
}

// dW[k][n] = sum_b A[b][k] * g[b][n] over the samples in order (A row: z[b], or embed[labels[b]])
__global__ __launch_bounds__(CS_THREADS) void cond_stem_wgrad_kernel(const float* __restrict__ A,
                                                                     const long long* __restrict__ labels, int NC,
                                                                     const float* __restrict__ g, int B, int K,
                                                                     float* __restrict__ dW) {
    const int tid = threadIdx.x;
    const int n = blockIdx.x * 64 + (tid & 63);
    const int k = blockIdx.y * 16 + (tid >> 6) * 4;   // wave-uniform
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (int b = 0; b < B; ++b) {
        const float* row;
        if (labels) {
            const long long l = labels[b];
            if (l < 0 || l >= NC) continue;
            row = A + (size_t)l * K;
        } else {
            row = A + (size_t)b * K;
        }
        const float gv = g[(size_t)b * (2 * CS_N) + n];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (k + i < K) acc[i] = fmaf(row[k + i], gv, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (k + i < K) dW[(size_t)(k + i) * CS_N + n] = acc[i];
}

// dbias[c] = sum over samples and the 16 positions of channel c (512 channels: both branches); one wave each
__global__ __launch_bounds__(64) void cond_stem_dbias_kernel(const float* __restrict__ g, int B,
                                                             float* __restrict__ db_in, float* __restrict__ db_label) {
    const int c = blockIdx.x, lane = threadIdx.x;
    float s = 0.0f;
    for (int b = lane >> 4; b < B; b += 4) s += g[(size_t)b * (2 * CS_N) + c * 16 + (lane & 15)];
    s = ffc::wave_sum(s);
    if (lane == 0) {
        if (c < CS_CH) {
            if (db_in) db_in[c] = s;
        } else if (db_label) {
            db_label[c - CS_CH] = s;
        }
    }
}

// dA[b][k] = sum_n g[b][n] * W[k][n]: 4 samples per workgroup, each thread 16 columns, wave-reduced per k
constexpr int CS_DB = 4;
__global__ __launch_bounds__(CS_THREADS) void cond_stem_dinput_kernel(const float* __restrict__ g,
                                                                      const float* __restrict__ W, int B, int K,
                                                                      float* __restrict__ dA) {
    extern __shared__ float red[];   // [4 waves][CS_DB][K]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * CS_DB;
    float4 gv[CS_DB][4];
#pragma unroll
    for (int s = 0; s < CS_DB; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            gv[s][j] = b0 + s < B ? *reinterpret_cast<const float4*>(g + (size_t)(b0 + s) * (2 * CS_N) + 4 * tid + 1024 * j)
                                  : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int k = 0; k < K; ++k) {
        float4 w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = *reinterpret_cast<const float4*>(W + (size_t)k * CS_N + 4 * tid + 1024 * j);
#pragma unroll
        for (int s = 0; s < CS_DB; ++s) {
            float p = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                p = fmaf(gv[s][j].x, w[j].x, p);
                p = fmaf(gv[s][j].y, w[j].y, p);
                p = fmaf(gv[s][j].z, w[j].z, p);
                p = fmaf(gv[s][j].w, w[j].w, p);
            }
            p = ffc::wave_sum(p);
            if (lane == 0) red[(wave * CS_DB + s) * K + k] = p;
        }
    }
    __syncthreads();
    for (int i = tid; i < CS_DB * K; i += CS_THREADS) {
        const int s = i / K, k = i - s * K;
        if (b0 + s < B)
            dA[(size_t)(b0 + s) * K + k] = (red[(0 * CS_DB + s) * K + k] + red[(1 * CS_DB + s) * K + k]) +
                                           (red[(2 * CS_DB + s) * K + k] + red[(3 * CS_DB + s) * K + k]);
    }
}

// out[b][:] = table[labels[b]][:] (NaN row for a label outside the table)
template <bool VEC>
__global__ __launch_bounds__(CS_THREADS) void embed_gather_kernel(const float* __restrict__ table,
                                                                  const long long* __restrict__ labels, int NC,
                                                                  int D, float* __restrict__ out) {
    const int b = blockIdx.y;
    const long long l = labels[b];
    const bool ok = l >= 0 && l < NC;
    const int i = blockIdx.x * CS_THREADS + threadIdx.x;
    if constexpr (VEC) {
        if (4 * i >= D) return;
        float4 v = make_float4(NAN, NAN, NAN, NAN);
        if (ok) v = reinterpret_cast<const float4*>(table + (size_t)l * D)[i];
        reinterpret_cast<float4*>(out + (size_t)b * D)[i] = v;
    } else {
        if (i >= D) return;
        out[(size_t)b * D + i] = ok ? table[(size_t)l * D + i] : NAN;
    }
}

// dtable[c][:] = sum of g[b][:] over the samples with labels[b] == c, in sample order (zeros when none)
template <bool VEC>
__global__ __launch_bounds__(CS_THREADS) void embed_scatter_kernel(const float* __restrict__ g,
                                                                   const long long* __restrict__ labels, int B,
                                                                   int D, float* __restrict__ dtable) {
    const int c = blockIdx.y;
    const int i = blockIdx.x * CS_THREADS + threadIdx.x;
    if constexpr (VEC) {
        if (4 * i >= D) return;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int b = 0; b < B; ++b) {
            if (labels[b] != c) continue;   // block-uniform
            const float4 v = reinterpret_cast<const float4*>(g + (size_t)b * D)[i];
            acc.x += v.x;
            acc.y += v.y;
            acc.z += v.z;
            acc.w += v.w;
        }
        reinterpret_cast<float4*>(dtable + (size_t)c * D)[i] = acc;
    } else {
        if (i >= D) return;
        float acc = 0.0f;
        for (int b = 0; b < B; ++b)
            if (labels[b] == c) acc += g[(size_t)b * D + i];
        dtable[(size_t)c * D + i] = acc;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int ffc_cond_stem_slab_rows(int B) { return B > 0 ? (B + CS_BM - 1) / CS_BM : 0; }

extern "C" int ffc_cond_stem_forward(const float* z, const int64_t* labels, const float* label_embed,
                                     const float* w_in, const float* bias_in, const float* w_label,
                                     const float* bias_label, int B, int z_size, int num_classes, float* out,
                                     float* slab, void* stream) {
    FFC_CHECK_ARG(z && labels && label_embed && w_in && bias_in && w_label && bias_label && out,
                  "ffc_cond_stem_forward: null argument");
    FFC_CHECK_ARG(B > 0 && z_size > 0 && num_classes > 0, "ffc_cond_stem_forward: bad sizes");
    FFC_CHECK_ARG(z_size <= 65536 && num_classes <= 65536 && B <= (1 << 20), "ffc_cond_stem_forward: size too large");
    FFC_CHECK_ARG(!slab || aligned16(slab), "ffc_cond_stem_forward: slab must be 16-byte aligned");
    StemArgs a{z, reinterpret_cast<const long long*>(labels), label_embed, w_in, bias_in, w_label, bias_label,
               out, slab, B, z_size, num_classes};
    const int grid = ffc_cond_stem_slab_rows(B) * (2 * CS_N / CS_BN);
    hipLaunchKernelGGL(cond_stem_kernel, dim3(grid), dim3(CS_THREADS), 0, (hipStream_t)stream, a);
    return ffc::launch_status("ffc_cond_stem_forward");
}

extern "C" int ffc_cond_stem_backward(const float* dpre, const float* z, const int64_t* labels,
                                      const float* label_embed, const float* w_in, const float* w_label, int B,
                                      int z_size, int num_classes, float* dw_in, float* dbias_in, float* dw_label,
                                      float* dbias_label, float* dz, float* dlabel_embed, float* ws, void* stream) {
    FFC_CHECK_ARG(dpre && z && labels && label_embed && w_in && w_label, "ffc_cond_stem_backward: null argument");
    FFC_CHECK_ARG(B > 0 && z_size > 0 && num_classes > 0, "ffc_cond_stem_backward: bad sizes");
    FFC_CHECK_ARG(z_size <= 1024 && num_classes <= 1024 && B <= (1 << 20), "ffc_cond_stem_backward: size too large");
    FFC_CHECK_ARG(!dlabel_embed || ws, "ffc_cond_stem_backward: d label_embed needs B * num_classes floats of ws");
    FFC_CHECK_ARG(aligned16(dpre) && aligned16(w_in) && aligned16(w_label),
                  "ffc_cond_stem_backward: 16-byte aligned dpre / weights required");
    const long long* lab = reinterpret_cast<const long long*>(labels);
    hipStream_t st = (hipStream_t)stream;
    if (dw_in)
        hipLaunchKernelGGL(cond_stem_wgrad_kernel, dim3(CS_N / 64, (z_size + 15) / 16), dim3(CS_THREADS), 0, st, z,
                           (const long long*)nullptr, 0, dpre, B, z_size, dw_in);
    if (dw_label)
        hipLaunchKernelGGL(cond_stem_wgrad_kernel, dim3(CS_N / 64, (num_classes + 15) / 16), dim3(CS_THREADS), 0, st,
                           label_embed, lab, num_classes, dpre + CS_N, B, num_classes, dw_label);
    if (dbias_in || dbias_label)
        hipLaunchKernelGGL(cond_stem_dbias_kernel, dim3(2 * CS_CH), dim3(64), 0, st, dpre, B, dbias_in, dbias_label);
    const int gb = (B + CS_DB - 1) / CS_DB;
    if (dz)
        hipLaunchKernelGGL(cond_stem_dinput_kernel, dim3(gb), dim3(CS_THREADS), sizeof(float) * 4 * CS_DB * z_size, st,
                           dpre, w_in, B, z_size, dz);
    if (dlabel_embed) {
        hipLaunchKernelGGL(cond_stem_dinput_kernel, dim3(gb), dim3(CS_THREADS), sizeof(float) * 4 * CS_DB * num_classes,
                           st, dpre + CS_N, w_label, B, num_classes, ws);
        hipLaunchKernelGGL(embed_scatter_kernel<false>, dim3((num_classes + CS_THREADS - 1) / CS_THREADS, num_classes),
                           dim3(CS_THREADS), 0, st, ws, lab, B, num_classes, dlabel_embed);
    }
    return ffc::launch_status("ffc_cond_stem_backward");
}

extern "C" int ffc_embed_gather_rows(const float* table, const int64_t* labels, int B, int num_classes, int D,
                                     float* out, void* stream) {
    FFC_CHECK_ARG(table && labels && out && B > 0 && num_classes > 0 && D > 0, "ffc_embed_gather_rows: bad args");
    FFC_CHECK_ARG(B <= 65535, "ffc_embed_gather_rows: B > 65535");
    const long long* lab = reinterpret_cast<const long long*>(labels);
    if (D % 4 == 0 && aligned16(table) && aligned16(out))
        hipLaunchKernelGGL(embed_gather_kernel<true>, dim3((D / 4 + CS_THREADS - 1) / CS_THREADS, B), dim3(CS_THREADS),
                           0, (hipStream_t)stream, table, lab, num_classes, D, out);
    else
        hipLaunchKernelGGL(embed_gather_kernel<false>, dim3((D + CS_THREADS - 1) / CS_THREADS, B), dim3(CS_THREADS), 0,
                           (hipStream_t)stream, table, lab, num_classes, D, out);
    return ffc::launch_status("ffc_embed_gather_rows");
}

extern "C" int ffc_embed_scatter_rows(const float* grad, const int64_t* labels, int B, int num_classes, int D,
                                      float* dtable, void* stream) {
    FFC_CHECK_ARG(grad && labels && dtable && B > 0 && num_classes > 0 && D > 0, "ffc_embed_scatter_rows: bad args");
    FFC_CHECK_ARG(num_classes <= 65535, "ffc_embed_scatter_rows: num_classes > 65535");
    const long long* lab = reinterpret_cast<const long long*>(labels);
    if (D % 4 == 0 && aligned16(grad) && aligned16(dtable))
        hipLaunchKernelGGL(embed_scatter_kernel<true>, dim3((D / 4 + CS_THREADS - 1) / CS_THREADS, num_classes),
                           dim3(CS_THREADS), 0, (hipStream_t)stream, grad, lab, B, D, dtable);
    else
        hipLaunchKernelGGL(embed_scatter_kernel<false>, dim3((D + CS_THREADS - 1) / CS_THREADS, num_classes),
                           dim3(CS_THREADS), 0, (hipStream_t)stream, grad, lab, B, D, dtable);
    return ffc::launch_status("ffc_embed_scatter_rows");
}
