// Conditional batch norm (layers/cond/cond_bn.py:6-24; FFC_BN_ACT with norm_layer=ConditionalBatchNorm2d,
// ffc_bn_act.py:70-83) for gfx950: an affine-less BatchNorm2d whose per-sample scale and shift are
// the two halves of row labels[b] of an nn.Embedding(K, 2C) table E.
//
// Labels are an int64 DEVICE tensor read by the kernels (no host read, no sync), as in
// cond_kernels.hip.  A label outside [0, K) never forms an address: that sample's gamma / beta read
// as NaN (its forward outputs are NaN) and ffc_embed_scatter_rows gives it no row.
//
// Forward.  The statistics come from the existing machinery (ffc_channel_moments or a conv epilogue's
// slab, finalized with gamma = beta = NULL): scale0[c] = 1/sigma_c, shift0[c] = -mu_c/sigma_c.  Then
//   y[b,c,:] = act((x*scale0[c] + shift0[c]) * E[l_b][c] + E[l_b][C+c]) + noise_w[c]*noise[b,:]
// in one pass, up to FFC_MAX_BN_BATCH tensors per launch (bn_l and bn_g of one layer).  Three forms,
// chosen per item on the host, block-uniform in the kernel:
//   plane : HW % 4 == 0, HW >= 256, aligned: a workgroup owns a 1024-float4 chunk of one plane; the
//           plane index is block-uniform, so the label, gamma, beta, scale0, shift0 are scalar loads
//   vec   : HW % 4 == 0, aligned, small planes: one float4 per thread over the flat tensor (a float4
//           never straddles planes); gamma / beta once per float4
//   scalar: everything else (HW = 1 included): one element per thread
//
// Backward (train).  g = dy*act'(z), xh = x*scale0 + shift0, z = xh*gamma_b + beta_b:
//   sums : per plane s1 = sum g, s2 = sum g*xh in fp64, fixed order -> (B, 2C) fp32 [s2 | s1], which
//          is the per-sample gradient of the embedding row: d E = ffc_embed_scatter_rows(sums)
//   coeff: m1[c] = sum_b gamma_bc*s1[b][c] / N, m2[c] = sum_b gamma_bc*s2[b][c] / N, N = B*HW, fp64,
//          samples in order
//   apply: dx = scale0[c]*(gamma_bc*g - m1[c] - xh*m2[c]);  eval (coef NULL): dx = scale0[c]*gamma_bc*g
// Two reads of x and dy, one write of dx: the traffic of ffc_bn_bwd.
#include "ffc_internal.h"

#include <cmath>

namespace {

constexpr int CBN_THREADS = 256;
constexpr int CBN_CHUNK4 = 4 * CBN_THREADS;   // float4 groups per workgroup, plane form
enum { CBN_PLANE = 0, CBN_VEC = 1, CBN_SCALAR = 2 };

// derivative of the activation at pre-activation z (ffc_act_bwd's convention: through the output for
// ReLU / LeakyReLU / Tanh / Sigmoid, through the input for GELU; here both come from z).  Kept apart from
// ffc::act_grad on purpose: ffc::act_grad(ffc::apply_act(z), z) is not the same expression (its ReLU /
// LeakyReLU arms test act(z), these test z itself), and these kernels' arithmetic is pinned as it stands
__device__ __forceinline__ float cbn_act_grad(float z, int act, float p) {
    switch (act) {
        case FFC_ACT_RELU: return z > 0.0f ? 1.0f : 0.0f;
        case FFC_ACT_LEAKY_RELU: return z > 0.0f ? 1.0f : p;
        case FFC_ACT_TANH: {
            const float y = tanhf(z);
            return 1.0f - y * y;
        }
        case FFC_ACT_SIGMOID: {
            const float y = 1.0f / (1.0f + expf(-z));
            return y * (1.0f - y);
        }
        case FFC_ACT_GELU: {
            const float cdf = 0.5f * (1.0f + erff(z * 0.70710678118654752f));
            const float pdf = 0.39894228040143268f * expf(-0.5f * z * z);
            return cdf + z * pdf;
        }
        default: return 1.0f;
    }
}

// gamma / beta of (sample b, channel c); NaN for a label outside the table (row 0 stands in for the
// address, which is never out of bounds: K >= 1)
__device__ __forceinline__ void cbn_affine(const long long* __restrict__ labels, const float* __restrict__ embed,
                                           int K, int C, int b, int c, float& ga, float& be) {
    const long long l = labels[b];
    const bool ok = l >= 0 && l < K;
    const float* row = embed + (size_t)(ok ? l : 0) * (2 * (size_t)C);
    const float g = row[c], s = row[C + c];
    ga = ok ? g : NAN;
    be = ok ? s : NAN;
}

struct CbnDev {
    const float* x;
    float* y;
    const float* scale;
    const float* shift;
    const float* embed;
    const long long* labels;
    const float* noise_w;   // null: no noise
    const float* noise;
    int B, C, HW, K;
    int act, mode, chunks;
    float p;
};

struct CbnBatch {
    CbnDev it[FFC_MAX_BN_BATCH];
    int off[FFC_MAX_BN_BATCH + 1];
    int n;
};

__device__ __forceinline__ float cbn_fwd1(float v, float sc, float sh, float ga, float be, int act, float p) {
    return ffc::apply_act(fmaf(fmaf(v, sc, sh), ga, be), act, p);
}

__device__ __forceinline__ float4 cbn_fwd4(float4 v, float sc, float sh, float ga, float be, int act, float p) {
    return make_float4(cbn_fwd1(v.x, sc, sh, ga, be, act, p), cbn_fwd1(v.y, sc, sh, ga, be, act, p),
                       cbn_fwd1(v.z, sc, sh, ga, be, act, p), cbn_fwd1(v.w, sc, sh, ga, be, act, p));
}

__global__ __launch_bounds__(CBN_THREADS) void cbn_apply_kernel(CbnBatch a) {
    int k = 0;
    while (k + 1 < a.n && (int)blockIdx.x >= a.off[k + 1]) ++k;
    const CbnDev& t = a.it[k];
    const int bid = blockIdx.x - a.off[k];
    const int C = t.C, HW = t.HW, act = t.act;
    const float p = t.p;
    if (t.mode == CBN_PLANE) {
        const int HW4 = HW >> 2;
        const int plane = bid / t.chunks, chunk = bid - plane * t.chunks;   // block-uniform
        const int b = plane / C, c = plane - b * C;
        float ga, be;
        cbn_affine(t.labels, t.embed, t.K, C, b, c, ga, be);
        const float sc = t.scale[c], sh = t.shift[c];
        const float nw = t.noise_w ? t.noise_w[c] : 0.0f;
        const float4* x = reinterpret_cast<const float4*>(t.x) + (size_t)plane * HW4;
        float4* y = reinterpret_cast<float4*>(t.y) + (size_t)plane * HW4;
        const float4* nz = t.noise_w ? reinterpret_cast<const float4*>(t.noise) + (size_t)b * HW4 : nullptr;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = chunk * CBN_CHUNK4 + u * CBN_THREADS + threadIdx.x;
            if (i < HW4) {
                float4 r = cbn_fwd4(x[i], sc, sh, ga, be, act, p);
                if (nz) {
                    const float4 n = nz[i];
                    r.x = fmaf(nw, n.x, r.x);
                    r.y = fmaf(nw, n.y, r.y);
                    r.z = fmaf(nw, n.z, r.z);
                    r.w = fmaf(nw, n.w, r.w);
                }
                y[i] = r;
            }
        }
        return;
    }
    const long long e = (long long)bid * CBN_THREADS + threadIdx.x;   // float4 group (vec) or element (scalar)
    if (t.mode == CBN_VEC) {
        const int HW4 = HW >> 2;
        if (e >= (long long)t.B * C * HW4) return;
        const int plane = (int)(e / HW4), i = (int)(e - (long long)plane * HW4);
        const int b = plane / C, c = plane - b * C;
        float ga, be;
        cbn_affine(t.labels, t.embed, t.K, C, b, c, ga, be);
        float4 r = cbn_fwd4(reinterpret_cast<const float4*>(t.x)[e], t.scale[c], t.shift[c], ga, be, act, p);
        if (t.noise_w) {
            const float nw = t.noise_w[c];
            const float4 n = reinterpret_cast<const float4*>(t.noise)[(size_t)b * HW4 + i];
            r.x = fmaf(nw, n.x, r.x);
            r.y = fmaf(nw, n.y, r.y);
            r.z = fmaf(nw, n.z, r.z);
            r.w = fmaf(nw, n.w, r.w);
        }
        reinterpret_cast<float4*>(t.y)[e] = r;
        return;
    }
    if (e >= (long long)t.B * C * HW) return;
    const int plane = (int)(e / HW), i = (int)(e - (long long)plane * HW);
    const int b = plane / C, c = plane - b * C;
    float ga, be;
    cbn_affine(t.labels, t.embed, t.K, C, b, c, ga, be);
    float r = cbn_fwd1(t.x[e], t.scale[c], t.shift[c], ga, be, act, p);
    if (t.noise_w) r = fmaf(t.noise_w[c], t.noise[(size_t)b * HW + i], r);
    t.y[e] = r;
}

// ------------------------------------------------------------------ backward
struct CbnBwd {
    const float* x;
    const float* dy;
    const long long* labels;
    const float* embed;
    const float* scale;
    const float* shift;
    int B, C, HW, K;
    int act;
    float p;
};

using ffc::wave_sum_f64;   // the __shfl_xor tree (ffc_internal.h)

// s1 = sum g, s2 = sum g*xh of each plane; G threads per plane (64: one wave, four planes per
// workgroup; 256: the workgroup).  Every partial sum has a fixed place in a fixed tree: bitwise
// reproducible.
template <int G>
__global__ __launch_bounds__(CBN_THREADS) void cbn_bwd_sums_kernel(CbnBwd a, float* __restrict__ sums) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, HW = a.HW;
    const long long planes = (long long)a.B * C;
    const long long plane = G == 64 ? (long long)blockIdx.x * 4 + wave : (long long)blockIdx.x;   // wave-uniform
    const bool live = plane < planes;
    double s1 = 0.0, s2 = 0.0;
    int b = 0, c = 0;
    if (live) {
        b = (int)(plane / C);
        c = (int)(plane - (long long)b * C);
        float ga, be;
        cbn_affine(a.labels, a.embed, a.K, C, b, c, ga, be);
        const float sc = a.scale[c], sh = a.shift[c];
        const float* x = a.x + (size_t)plane * HW;
        const float* dy = a.dy + (size_t)plane * HW;
        for (int q = (G == 64 ? lane : tid); q < HW; q += G) {
            const float xh = fmaf(x[q], sc, sh);
            const float g = dy[q] * cbn_act_grad(fmaf(xh, ga, be), a.act, a.p);
            s1 += g;
            s2 += (double)g * xh;
        }
    }
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    if constexpr (G == 64) {
        if (live && lane == 0) {
            sums[(size_t)b * 2 * C + c] = (float)s2;
            sums[(size_t)b * 2 * C + C + c] = (float)s1;
        }
    } else {
        __shared__ double r[4][2];
        if (lane == 0) {
            r[wave][0] = s1;
            r[wave][1] = s2;
        }
        __syncthreads();
        if (tid == 0) {   // live: one plane per workgroup, grid = planes
            sums[(size_t)b * 2 * C + c] = (float)((r[0][1] + r[1][1]) + (r[2][1] + r[3][1]));
            sums[(size_t)b * 2 * C + C + c] = (float)((r[0][0] + r[1][0]) + (r[2][0] + r[3][0]));
        }
    }
}

// coef[c] = {m1, m2}: one thread per channel, the samples in order (fp64)
__global__ __launch_bounds__(CBN_THREADS) void cbn_bwd_coeff_kernel(const float* __restrict__ sums,
                                                                   const long long* __restrict__ labels,
                                                                   const float* __restrict__ embed, int B, int C,
                                                                   int K, double inv_n, float* __restrict__ coef) {
    const int c = blockIdx.x * CBN_THREADS + threadIdx.x;
    if (c >= C) return;
    double m1 = 0.0, m2 = 0.0;
    for (int b = 0; b < B; ++b) {
        const long long l = labels[b];
        const bool ok = l >= 0 && l < K;
        const float gv = embed[(size_t)(ok ? l : 0) * (2 * (size_t)C) + c];
        const double ga = ok ? (double)gv : (double)NAN;
        m2 += ga * (double)sums[(size_t)b * 2 * C + c];
        m1 += ga * (double)sums[(size_t)b * 2 * C + C + c];
    }
    coef[2 * c] = (float)(m1 * inv_n);
    coef[2 * c + 1] = (float)(m2 * inv_n);
}

__device__ __forceinline__ float cbn_dx1(float xv, float dyv, float sc, float sh, float ga, float be, float m1,
                                         float m2, int act, float p) {
    const float xh = fmaf(xv, sc, sh);
    const float g = dyv * cbn_act_grad(fmaf(xh, ga, be), act, p);
    return sc * (fmaf(ga, g, -m1) - xh * m2);
}

template <bool VEC>
__global__ __launch_bounds__(CBN_THREADS) void cbn_bwd_apply_kernel(CbnBwd a, const float* __restrict__ coef,
                                                                   float* __restrict__ dx) {
    const int C = a.C;
    const int per = VEC ? a.HW >> 2 : a.HW;   // float4 groups / elements per plane
    const long long e = (long long)blockIdx.x * CBN_THREADS + threadIdx.x;
    if (e >= (long long)a.B * C * per) return;
    const int plane = (int)(e / per);
    const int b = plane / C, c = plane - b * C;
    float ga, be;
    cbn_affine(a.labels, a.embed, a.K, C, b, c, ga, be);
    const float sc = a.scale[c], sh = a.shift[c];
    const float m1 = coef ? coef[2 * c] : 0.0f, m2 = coef ? coef[2 * c + 1] : 0.0f;
    if constexpr (VEC) {
        const float4 xv = reinterpret_cast<const float4*>(a.x)[e];
        const float4 dv = reinterpret_cast<const float4*>(a.dy)[e];
        reinterpret_cast<float4*>(dx)[e] =
            make_float4(cbn_dx1(xv.x, dv.x, sc, sh, ga, be, m1, m2, a.act, a.p),
                        cbn_dx1(xv.y, dv.y, sc, sh, ga, be, m1, m2, a.act, a.p),
                        cbn_dx1(xv.z, dv.z, sc, sh, ga, be, m1, m2, a.act, a.p),
                        cbn_dx1(xv.w, dv.w, sc, sh, ga, be, m1, m2, a.act, a.p));
    } else {
        dx[e] = cbn_dx1(a.x[e], a.dy[e], sc, sh, ga, be, m1, m2, a.act, a.p);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool bwd_args_ok(const float* x, const float* dy, const int64_t* labels, const float* embed, int B, int C, int HW,
                 int K, const float* scale0, const float* shift0, int act) {
    return x && dy && labels && embed && scale0 && shift0 && B > 0 && C > 0 && HW > 0 && K > 0 && act >= 0 &&
           act <= FFC_ACT_GELU && (long long)B * C * HW < (1LL << 31);
}

CbnBwd bwd_args(const float* x, const float* dy, const int64_t* labels, const float* embed, int B, int C, int HW,
                int K, const float* scale0, const float* shift0, int act, float p) {
    return CbnBwd{x, dy, reinterpret_cast<const long long*>(labels), embed, scale0, shift0, B, C, HW, K, act, p};
}

}  // namespace

extern "C" int ffc_cbn_act_apply_batch(const ffc_cbn_apply_item* items, int n, void* stream) {
    FFC_CHECK_ARG(items && n >= 1 && n <= FFC_MAX_BN_BATCH, "ffc_cbn_act_apply_batch: 1 <= n <= 4 items");
    CbnBatch a = {};
    long long blocks = 0;
    for (int i = 0; i < n; ++i) {
        const ffc_cbn_apply_item& t = items[i];
        FFC_CHECK_ARG(t.x && t.y && t.scale0 && t.shift0 && t.embed && t.labels && t.B > 0 && t.C > 0 && t.HW > 0 &&
                          t.num_classes > 0,
                      "ffc_cbn_act_apply_batch: bad item");
        FFC_CHECK_ARG(t.act >= 0 && t.act <= FFC_ACT_GELU, "ffc_cbn_act_apply_batch: bad activation code");
        FFC_CHECK_ARG((t.noise == nullptr) == (t.noise_w == nullptr),
                      "ffc_cbn_act_apply_batch: noise and noise_w go together");
        const long long total = (long long)t.B * t.C * t.HW;
        FFC_CHECK_ARG(total < (1LL << 31), "ffc_cbn_act_apply_batch: tensor too large");
        const bool vec = t.HW % 4 == 0 && aligned16(t.x) && aligned16(t.y) && aligned16(t.noise);
        CbnDev& d = a.it[i];
        d = CbnDev{t.x, t.y, t.scale0, t.shift0, t.embed, reinterpret_cast<const long long*>(t.labels), t.noise_w,
                   t.noise, t.B, t.C, t.HW, t.num_classes, t.act, 0, 1, t.act_param};
        a.off[i] = (int)blocks;
        if (vec && t.HW >= 256) {
            d.mode = CBN_PLANE;
            d.chunks = (t.HW / 4 + CBN_CHUNK4 - 1) / CBN_CHUNK4;
            blocks += (long long)t.B * t.C * d.chunks;
        } else if (vec) {
            d.mode = CBN_VEC;
            blocks += (total / 4 + CBN_THREADS - 1) / CBN_THREADS;
        } else {
            d.mode = CBN_SCALAR;
            blocks += (total + CBN_THREADS - 1) / CBN_THREADS;
        }
        FFC_CHECK_ARG(blocks < (1LL << 31), "ffc_cbn_act_apply_batch: grid too large");
    }
    a.n = n;
    a.off[n] = (int)blocks;
    hipLaunchKernelGGL(cbn_apply_kernel, dim3((unsigned)blocks), dim3(CBN_THREADS), 0, (hipStream_t)stream, a);
    return ffc::launch_status("ffc_cbn_act_apply_batch");
}

extern "C" int ffc_cbn_bwd_sums(const float* x, const float* dy, const int64_t* labels, const float* embed, int B,
                                int C, int HW, int num_classes, const float* scale0, const float* shift0, int act,
                                float act_param, float* sums, void* stream) {
    FFC_CHECK_ARG(bwd_args_ok(x, dy, labels, embed, B, C, HW, num_classes, scale0, shift0, act) && sums,
                  "ffc_cbn_bwd_sums: bad args");
    const CbnBwd a = bwd_args(x, dy, labels, embed, B, C, HW, num_classes, scale0, shift0, act, act_param);
    const long long planes = (long long)B * C;
    if (HW <= 1024)
        hipLaunchKernelGGL(cbn_bwd_sums_kernel<64>, dim3((unsigned)((planes + 3) / 4)), dim3(CBN_THREADS), 0,
                           (hipStream_t)stream, a, sums);
    else
        hipLaunchKernelGGL(cbn_bwd_sums_kernel<256>, dim3((unsigned)planes), dim3(CBN_THREADS), 0,
                           (hipStream_t)stream, a, sums);
    return ffc::launch_status("ffc_cbn_bwd_sums");
}

extern "C" int ffc_cbn_bwd_coeff(const float* sums, const int64_t* labels, const float* embed, int B, int C, int HW,
                                 int num_classes, float* coef, void* stream) {
    FFC_CHECK_ARG(sums && labels && embed && coef && B > 0 && C > 0 && HW > 0 && num_classes > 0,
                  "ffc_cbn_bwd_coeff: bad args");
    hipLaunchKernelGGL(cbn_bwd_coeff_kernel, dim3((C + CBN_THREADS - 1) / CBN_THREADS), dim3(CBN_THREADS), 0,
                       (hipStream_t)stream, sums, reinterpret_cast<const long long*>(labels), embed, B, C, num_classes,
                       1.0 / ((double)B * HW), coef);
    return ffc::launch_status("ffc_cbn_bwd_coeff");
}

extern "C" int ffc_cbn_bwd_apply(const float* x, const float* dy, const int64_t* labels, const float* embed, int B,
                                 int C, int HW, int num_classes, const float* scale0, const float* shift0, int act,
                                 float act_param, const float* coef, float* dx, void* stream) {
    FFC_CHECK_ARG(bwd_args_ok(x, dy, labels, embed, B, C, HW, num_classes, scale0, shift0, act) && dx,
                  "ffc_cbn_bwd_apply: bad args");
    const CbnBwd a = bwd_args(x, dy, labels, embed, B, C, HW, num_classes, scale0, shift0, act, act_param);
    const long long total = (long long)B * C * HW;
    if (HW % 4 == 0 && aligned16(x) && aligned16(dy) && aligned16(dx))
        hipLaunchKernelGGL(cbn_bwd_apply_kernel<true>, dim3((unsigned)((total / 4 + CBN_THREADS - 1) / CBN_THREADS)),
                           dim3(CBN_THREADS), 0, (hipStream_t)stream, a, coef, dx);
    else
        hipLaunchKernelGGL(cbn_bwd_apply_kernel<false>, dim3((unsigned)((total + CBN_THREADS - 1) / CBN_THREADS)),
                           dim3(CBN_THREADS), 0, (hipStream_t)stream, a, coef, dx);
    return ffc::launch_status("ffc_cbn_bwd_apply");
}
