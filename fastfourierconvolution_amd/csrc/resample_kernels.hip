// Resampling kernels of the ResNet SNGAN blocks (GBlock / DBlock, fgan128_complete.py:75-332), gfx950, fp32,
// dense NCHW planes.  No atomics, every sum in one fixed order: bitwise reproducible.
//
//   ffc_act_up2b           Y = up2_bilinear(act(scale x + shift)): F.interpolate(scale_factor=2, 'bilinear',
//                          align_corners=False) of the activated (conditional) BatchNorm output, which is never
//                          written at the low resolution
//   ffc_up2b_adjoint       dX = up2_bilinear^T dY, a gather over at most 4 x 4 of dY
//   ffc_pool2_act (+ _bwd) y = act(0.25 * 2x2 sum): AvgPool2d(2) with the next block's in-place ReLU
//   ffc_relu_sum_pool (+ _bwd)  out[b][c] = sum_hw relu(x): the critic's global sum pooling
//
// Along one axis of length n (indices clamped to [0, n-1]) the x2 bilinear weights are exact in fp32:
//   Y[2i] = 0.25 X[i-1] + 0.75 X[i]        Y[2i+1] = 0.75 X[i] + 0.25 X[i+1]
// so X[i] collects (0.25, 0.75, 0.75, 0.25) from Y[2i-1 .. 2i+2] with THOSE indices clamped to [0, 2n-1]: the
// edge pixels pick up the weight the clamped taps of the forward gave them (n = 1: Y[0] + Y[1]).
#include <algorithm>
#include <climits>
#include <cstdint>

#include "ffc_internal.h"

namespace {

// NJ input columns per thread: 2 (one 16-byte store per output row; w even, y 16-byte aligned) or 1
template <int NJ>
__global__ void act_up2b_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                const float* __restrict__ shift, int per_sample, int C, int h, int w, long long P,
                                int act, float ap, float* __restrict__ y) {
    const int wq = w / NJ;
    const long long per = (long long)h * wq, n = P * per;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long pl = i / per;
        const int r = (int)(i - pl * per), ii = r / wq, j0 = (r - ii * wq) * NJ;
        float sc = 1.0f, sh = 0.0f;
        if (scale) {
            const long long k = per_sample ? pl : pl % C;
            sc = scale[k];
            sh = shift[k];
        }
        const float* xp = x + (size_t)pl * h * w;
        const int rows[3] = {max(ii - 1, 0), ii, min(ii + 1, h - 1)};
        float hr[3][2 * NJ];   // the three input rows, interpolated along x
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
            const float* xr = xp + (size_t)rows[rr] * w;
            float a[NJ + 2];
#pragma unroll
            for (int c = 0; c < NJ + 2; ++c) {
                float v = xr[min(max(j0 - 1 + c, 0), w - 1)];
                if (scale) v = fmaf(v, sc, sh);
                a[c] = ffc::apply_act(v, act, ap);
            }
#pragma unroll
            for (int c = 0; c < NJ; ++c) {
                hr[rr][2 * c] = 0.25f * a[c] + 0.75f * a[c + 1];
                hr[rr][2 * c + 1] = 0.75f * a[c + 1] + 0.25f * a[c + 2];
            }
        }
        float top[2 * NJ], bot[2 * NJ];
#pragma unroll
        for (int c = 0; c < 2 * NJ; ++c) {
            top[c] = 0.25f * hr[0][c] + 0.75f * hr[1][c];
            bot[c] = 0.75f * hr[1][c] + 0.25f * hr[2][c];
        }
        float* yp = y + (size_t)pl * 4 * h * w + (size_t)(2 * ii) * (2 * w) + 2 * j0;
        if (NJ == 2) {
            *reinterpret_cast<floatx4*>(yp) = floatx4{top[0], top[1], top[2], top[3]};
            *reinterpret_cast<floatx4*>(yp + 2 * w) = floatx4{bot[0], bot[1], bot[2], bot[3]};
        } else {
            yp[0] = top[0];
            yp[1] = top[1];
            yp[2 * w] = bot[0];
            yp[2 * w + 1] = bot[1];
        }
    }
}

__global__ void up2b_adjoint_kernel(const float* __restrict__ dy, long long P, int h, int w, float* __restrict__ dx) {
    const int H = 2 * h, W = 2 * w;
    const long long per = (long long)h * w, n = P * per;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long pl = i / per;
        const int r = (int)(i - pl * per), ii = r / w, jj = r - ii * w;
        const float* g = dy + (size_t)pl * H * W;
        const int c0 = max(2 * jj - 1, 0), c1 = 2 * jj, c2 = 2 * jj + 1, c3 = min(2 * jj + 2, W - 1);
        float rs[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float* row = g + (size_t)min(max(2 * ii - 1 + a, 0), H - 1) * W;
            rs[a] = (0.25f * row[c0] + 0.75f * row[c1]) + (0.75f * row[c2] + 0.25f * row[c3]);
        }
        dx[i] = (0.25f * rs[0] + 0.75f * rs[1]) + (0.75f * rs[2] + 0.25f * rs[3]);
    }
}

// V2: the two floats of each input row pair as one 8-byte load (W even: every row pair is 8-byte aligned when x is)
template <int V2>
__global__ void pool2_act_kernel(const float* __restrict__ x, long long P, int H, int W, int act, float ap,
                                 float* __restrict__ y) {
    const int h = H / 2, w = W / 2;
    const long long per = (long long)h * w, n = P * per;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long pl = i / per;
        const int r = (int)(i - pl * per), yy = r / w, xx = r - yy * w;
        const float* s = x + (size_t)pl * H * W + (size_t)(2 * yy) * W + 2 * xx;
        float a, b, c, d;
        if (V2) {
            const f32x2 t = *reinterpret_cast<const f32x2*>(s), u = *reinterpret_cast<const f32x2*>(s + W);
            a = t[0], b = t[1], c = u[0], d = u[1];
        } else {
            a = s[0], b = s[1], c = s[W], d = s[W + 1];
        }
        y[i] = ffc::apply_act(((a + b) + (c + d)) * 0.25f, act, ap);
    }
}

__global__ void pool2_act_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, long long P, int h,
                                     int w, int act, float ap, float* __restrict__ dx) {
    const int W = 2 * w;
    const long long per = (long long)h * w, n = P * per;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long pl = i / per;
        const int r = (int)(i - pl * per), yy = r / w, xx = r - yy * w;
        const float g = 0.25f * dy[i] * ffc::act_grad<false>(y[i], y[i], act, ap);
        float* d = dx + (size_t)pl * 4 * per + (size_t)(2 * yy) * W + 2 * xx;
        d[0] = g;
        d[1] = g;
        d[W] = g;
        d[W + 1] = g;
    }
}

// planes of up to RSP_SMALL elements: one thread per plane, elements in index order
constexpr int RSP_SMALL = 32;
__global__ void relu_sum_small_kernel(const float* __restrict__ x, long long P, int HW, float* __restrict__ out) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
        const float* s = x + (size_t)p * HW;
        float acc = 0.0f;
        for (int q = 0; q < HW; ++q) acc += fmaxf(s[q], 0.0f);
        out[p] = acc;
    }
}

// larger planes: one wave per plane; lane l sums elements l, l + 64, ... in order, then the xor butterfly
__global__ void relu_sum_wave_kernel(const float* __restrict__ x, long long P, int HW, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long p = wave; p < P; p += nwaves) {
        const float* s = x + (size_t)p * HW;
        float acc = 0.0f;
        for (int q = lane; q < HW; q += 64) acc += fmaxf(s[q], 0.0f);
        acc = ffc::wave_sum(acc);
        if (lane == 0) out[p] = acc;
    }
}

__global__ void relu_sum_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dout, long long n, int HW,
                                    float* __restrict__ dx) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dx[i] = x[i] > 0.0f ? dout[i / HW] : 0.0f;
}

int grid_of(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8192)); }

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the element count of the larger tensor fits 32-bit indexing
bool fits(long long P, long long per) { return P <= INT_MAX && per <= INT_MAX && P * per <= INT_MAX; }

}  // namespace

extern "C" int ffc_act_up2b(const float* x, const float* scale, const float* shift, int per_sample, int B, int C,
                            int h, int w, int act, float act_param, float* y, void* stream) {
    FFC_CHECK_ARG(x && y, "ffc_act_up2b: null pointer");
    FFC_CHECK_ARG((scale == nullptr) == (shift == nullptr), "ffc_act_up2b: scale and shift go together");
    FFC_CHECK_ARG(B > 0 && C > 0 && h > 0 && w > 0, "ffc_act_up2b: bad shape");
    FFC_CHECK_ARG(act >= 0 && act <= FFC_ACT_GELU, "ffc_act_up2b: bad activation");
    FFC_CHECK_ARG(h <= INT_MAX / 2 && w <= INT_MAX / 2 && fits((long long)B * C, 4LL * h * w),
                  "ffc_act_up2b: size beyond 32-bit indexing");
    const long long P = (long long)B * C;
    hipStream_t s = (hipStream_t)stream;
    if (w % 2 == 0 && aligned(y, 16))
        hipLaunchKernelGGL(act_up2b_kernel<2>, dim3(grid_of(P * h * (w / 2))), dim3(256), 0, s, x, scale, shift,
                           per_sample, C, h, w, P, act, act_param, y);
    else
        hipLaunchKernelGGL(act_up2b_kernel<1>, dim3(grid_of(P * h * w)), dim3(256), 0, s, x, scale, shift, per_sample,
                           C, h, w, P, act, act_param, y);
    return ffc::launch_status("ffc_act_up2b");
}

extern "C" int ffc_up2b_adjoint(const float* dy, long long P, int h, int w, float* dx, void* stream) {
    FFC_CHECK_ARG(dy && dx, "ffc_up2b_adjoint: null pointer");
    FFC_CHECK_ARG(P > 0 && h > 0 && w > 0, "ffc_up2b_adjoint: bad shape");
    FFC_CHECK_ARG(h <= INT_MAX / 2 && w <= INT_MAX / 2 && fits(P, 4LL * h * w),
                  "ffc_up2b_adjoint: size beyond 32-bit indexing");
    hipLaunchKernelGGL(up2b_adjoint_kernel, dim3(grid_of(P * h * w)), dim3(256), 0, (hipStream_t)stream, dy, P, h, w,
                       dx);
    return ffc::launch_status("ffc_up2b_adjoint");
}

extern "C" int ffc_pool2_act(const float* x, long long P, int H, int W, int act, float act_param, float* y,
                             void* stream) {
    FFC_CHECK_ARG(x && y, "ffc_pool2_act: null pointer");
    FFC_CHECK_ARG(P > 0 && H > 0 && W > 0, "ffc_pool2_act: bad shape");
    FFC_CHECK_ARG(H % 2 == 0 && W % 2 == 0, "ffc_pool2_act: odd plane");
    FFC_CHECK_ARG(act >= 0 && act < FFC_ACT_GELU, "ffc_pool2_act: bad activation (GELU keeps no pre-activation)");
    FFC_CHECK_ARG(fits(P, (long long)H * W), "ffc_pool2_act: size beyond 32-bit indexing");
    const int grid = grid_of(P * (H / 2) * (W / 2));
    if (aligned(x, 8))
        hipLaunchKernelGGL(pool2_act_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, P, H, W, act,
                           act_param, y);
    else
        hipLaunchKernelGGL(pool2_act_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, P, H, W, act,
                           act_param, y);
    return ffc::launch_status("ffc_pool2_act");
}

extern "C" int ffc_pool2_act_bwd(const float* y, const float* dy, long long P, int h, int w, int act,
                                 float act_param, float* dx, void* stream) {
    FFC_CHECK_ARG(y && dy && dx, "ffc_pool2_act_bwd: null pointer");
    FFC_CHECK_ARG(P > 0 && h > 0 && w > 0, "ffc_pool2_act_bwd: bad shape");
    FFC_CHECK_ARG(act >= 0 && act < FFC_ACT_GELU, "ffc_pool2_act_bwd: bad activation");
    FFC_CHECK_ARG(h <= INT_MAX / 2 && w <= INT_MAX / 2 && fits(P, 4LL * h * w),
                  "ffc_pool2_act_bwd: size beyond 32-bit indexing");
    hipLaunchKernelGGL(pool2_act_bwd_kernel, dim3(grid_of(P * h * w)), dim3(256), 0, (hipStream_t)stream, y, dy, P, h,
                       w, act, act_param, dx);
    return ffc::launch_status("ffc_pool2_act_bwd");
}

extern "C" int ffc_relu_sum_pool(const float* x, long long P, int HW, float* out, void* stream) {
    FFC_CHECK_ARG(x && out, "ffc_relu_sum_pool: null pointer");
    FFC_CHECK_ARG(P > 0 && HW > 0, "ffc_relu_sum_pool: bad shape");
    FFC_CHECK_ARG(fits(P, HW), "ffc_relu_sum_pool: size beyond 32-bit indexing");
    if (HW <= RSP_SMALL)
        hipLaunchKernelGGL(relu_sum_small_kernel, dim3(grid_of(P)), dim3(256), 0, (hipStream_t)stream, x, P, HW, out);
    else
        hipLaunchKernelGGL(relu_sum_wave_kernel, dim3(grid_of(P * 64)), dim3(256), 0, (hipStream_t)stream, x, P, HW,
                           out);
    return ffc::launch_status("ffc_relu_sum_pool");
}

extern "C" int ffc_relu_sum_pool_bwd(const float* x, const float* dout, long long P, int HW, float* dx, void* stream) {
    FFC_CHECK_ARG(x && dout && dx, "ffc_relu_sum_pool_bwd: null pointer");
    FFC_CHECK_ARG(P > 0 && HW > 0, "ffc_relu_sum_pool_bwd: bad shape");
    FFC_CHECK_ARG(fits(P, HW), "ffc_relu_sum_pool_bwd: size beyond 32-bit indexing");
    hipLaunchKernelGGL(relu_sum_bwd_kernel, dim3(grid_of(P * HW)), dim3(256), 0, (hipStream_t)stream, x, dout,
                       P * HW, HW, dx);
    return ffc::launch_status("ffc_relu_sum_pool_bwd");
}
