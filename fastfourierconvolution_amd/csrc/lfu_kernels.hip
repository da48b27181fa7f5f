// Local Fourier unit (LFU) of SpectralTransform for gfx950: the data movement on either side of the
// Fourier unit that runs on the quadrant stack (the sketch in layers/ffc/spectral_transform.py:94-108,
// which the reference never executes).  With s = relu(bn1(conv1(.))) of shape (B, c, H, W):
//
//   xs = cat(split(cat(split(s[:, :c/4], H/2, dim=-2), dim=1), W/2, dim=-1), dim=1)   (B, c, H/2, W/2)
//        channel block q = k / (c/4) of xs is quadrant q of source channel k % (c/4):
//        q = 0 top-left, 1 bottom-left, 2 top-right, 3 bottom-right
//   ys = lfu(xs)                                     the Fourier-unit entry points (fu / fu2d kernels)
//   v  = s + fu(s) + ys.repeat(1, 1, 2, 2)           what conv2 reads
//
//   ffc_lfu_gather      xs from the pre-BN t (bn1 affine + ReLU + the x2 nearest upsample applied on load)
//   ffc_lfu_tile_add    out = v + tile(ys); out == v runs in place
//   ffc_lfu_gather_bwd  adjoint of the gather at up = 1, identity transform: ds OVERWRITTEN -- the
//                       quadrants back in channels [0, c/4), exact zeros in [c/4, c)
//   ffc_lfu_tile_bwd    adjoint of the tiling: dys = sum of the four quadrant entries of dv, in the fixed
//                       order (top-left + top-right) + (bottom-left + bottom-right)
//
// All four are pure bandwidth: one thread per four consecutive floats of an H/2 x W/2 row when
// W/2 % 4 == 0 and the tensors are 16-byte aligned (16-byte loads / stores; every quadrant row then
// starts on a 16-byte boundary of its full row, and with up = 2 the two source floats of a group on an
// 8-byte one), one thread per float otherwise.  Consecutive lanes cover consecutive addresses of a
// row and then of the next row, so a wave's accesses are runs of W/2 floats.  Grid-stride loops over
// at most LFU_MAX_BLOCKS workgroups of 256 threads (four waves of 64); no LDS, no atomics.
#include "ffc_internal.h"

namespace {

constexpr int LFU_THREADS = 256;
constexpr int LFU_MAX_BLOCKS = 2048;

struct Quad {   // position (b, k, i, j..) of a flat index over (B, c, H2, W2 / V)
    size_t b;
    int k, i, j;
};

template <int V>
__device__ __forceinline__ Quad unflatten(size_t idx, int c, int Hn, int Wn) {
    const int wv = Wn / V;
    Quad p;
    p.j = (int)(idx % wv) * V;
    idx /= wv;
    p.i = (int)(idx % Hn);
    idx /= Hn;
    p.k = (int)(idx % c);
    p.b = idx / c;
    return p;
}

__device__ __forceinline__ float in_tf(float v, bool affine, float sc, float sh, int relu) {
    if (affine) v = fmaf(v, sc, sh);
    return relu ? fmaxf(v, 0.0f) : v;
}

// xs (B, c, H2, W2) from t (B, c, h, w): H = h * up = 2 * H2, W = w * up = 2 * W2
template <int V>
__global__ __launch_bounds__(LFU_THREADS) void lfu_gather_kernel(const float* __restrict__ t, int c, int h, int w,
                                                                 int up, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, int relu,
                                                                 float* __restrict__ xs, size_t total) {
    const int H2 = h * up / 2, W2 = w * up / 2, c4 = c / 4;
    const bool affine = scale != nullptr || shift != nullptr;
    for (size_t idx = blockIdx.x * (size_t)LFU_THREADS + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * LFU_THREADS) {
        const Quad p = unflatten<V>(idx, c, H2, W2);
        const int q = p.k / c4, ch = p.k - q * c4;
        const int y = p.i + (q & 1) * H2, x = p.j + (q >> 1) * W2;   // position in the H x W plane
        const float sc = scale ? scale[ch] : 1.0f, sh = shift ? shift[ch] : 0.0f;
        const float* src = t + ((p.b * c + ch) * h + (up == 2 ? y >> 1 : y)) * (size_t)w;
        if (V == 4) {
            float4 o;
            if (up == 2) {
                const float2 a = *reinterpret_cast<const float2*>(src + (x >> 1));
                o.x = o.y = in_tf(a.x, affine, sc, sh, relu);
                o.z = o.w = in_tf(a.y, affine, sc, sh, relu);
            } else {
                const float4 a = *reinterpret_cast<const float4*>(src + x);
                o.x = in_tf(a.x, affine, sc, sh, relu);
                o.y = in_tf(a.y, affine, sc, sh, relu);
                o.z = in_tf(a.z, affine, sc, sh, relu);
                o.w = in_tf(a.w, affine, sc, sh, relu);
            }
            reinterpret_cast<float4*>(xs)[idx] = o;
        } else {
            xs[idx] = in_tf(src[up == 2 ? x >> 1 : x], affine, sc, sh, relu);
        }
    }
}

// out (B, c, H, W) = v + ys (B, c, H2, W2) tiled 2 x 2; flat index over v
template <int V>
__global__ __launch_bounds__(LFU_THREADS) void lfu_tile_add_kernel(const float* v, const float* __restrict__ ys,
                                                                   int c, int H2, int W2, float* out, size_t total) {
    for (size_t idx = blockIdx.x * (size_t)LFU_THREADS + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * LFU_THREADS) {
        const Quad p = unflatten<V>(idx, c, 2 * H2, 2 * W2);
        const int i = p.i >= H2 ? p.i - H2 : p.i, j = p.j >= W2 ? p.j - W2 : p.j;
        const float* src = ys + ((p.b * c + p.k) * H2 + i) * (size_t)W2 + j;
        if (V == 4) {
            float4 a = reinterpret_cast<const float4*>(v)[idx];
            const float4 y = *reinterpret_cast<const float4*>(src);
            a.x += y.x;
            a.y += y.y;
            a.z += y.z;
            a.w += y.w;
            reinterpret_cast<float4*>(out)[idx] = a;
        } else {
            out[idx] = v[idx] + *src;
        }
    }
}

// ds (B, c, H, W) from dxs (B, c, H2, W2); flat index over ds
template <int V>
__global__ __launch_bounds__(LFU_THREADS) void lfu_gather_bwd_kernel(const float* __restrict__ dxs, int c, int H2,
                                                                     int W2, float* __restrict__ ds, size_t total) {
    const int c4 = c / 4;
    for (size_t idx = blockIdx.x * (size_t)LFU_THREADS + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * LFU_THREADS) {
        const Quad p = unflatten<V>(idx, c, 2 * H2, 2 * W2);
        const bool live = p.k < c4;   // uniform over a plane: a wave diverges at plane boundaries only
        const int q = (p.i >= H2 ? 1 : 0) + (p.j >= W2 ? 2 : 0);
        const int i = p.i >= H2 ? p.i - H2 : p.i, j = p.j >= W2 ? p.j - W2 : p.j;
        const float* src = dxs + ((p.b * c + q * c4 + p.k) * H2 + i) * (size_t)W2 + j;
        if (V == 4)
            reinterpret_cast<float4*>(ds)[idx] = live ? *reinterpret_cast<const float4*>(src)
                                                      : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        else
            ds[idx] = live ? *src : 0.0f;
    }
}

// dys (B, c, H2, W2) = the four quadrants of dv (B, c, H, W) summed; flat index over dys
template <int V>
__global__ __launch_bounds__(LFU_THREADS) void lfu_tile_bwd_kernel(const float* __restrict__ dv, int c, int H2,
                                                                   int W2, float* __restrict__ dys, size_t total) {
    const int W = 2 * W2;
    for (size_t idx = blockIdx.x * (size_t)LFU_THREADS + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * LFU_THREADS) {
        const Quad p = unflatten<V>(idx, c, H2, W2);
        const float* top = dv + ((p.b * c + p.k) * (2 * (size_t)H2) + p.i) * W + p.j;
        const float* bot = top + (size_t)H2 * W;
        if (V == 4) {
            const float4 tl = *reinterpret_cast<const float4*>(top), tr = *reinterpret_cast<const float4*>(top + W2);
            const float4 bl = *reinterpret_cast<const float4*>(bot), br = *reinterpret_cast<const float4*>(bot + W2);
            float4 o;
            o.x = (tl.x + tr.x) + (bl.x + br.x);
            o.y = (tl.y + tr.y) + (bl.y + br.y);
            o.z = (tl.z + tr.z) + (bl.z + br.z);
            o.w = (tl.w + tr.w) + (bl.w + br.w);
            reinterpret_cast<float4*>(dys)[idx] = o;
        } else {
            dys[idx] = (top[0] + top[W2]) + (bot[0] + bot[W2]);
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int lfu_grid(size_t work) {
    const size_t blocks = (work + LFU_THREADS - 1) / LFU_THREADS;
    return (int)(blocks < (size_t)LFU_MAX_BLOCKS ? blocks : (size_t)LFU_MAX_BLOCKS);
}

// the (B, c, H, W) plane every entry point is given: c % 4 == 0, H and W even, sizes that index in int
bool lfu_shape_ok(int B, int c, int H, int W) {
    return B > 0 && c > 0 && c % 4 == 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && B <= (1 << 20) &&
           c <= 65536 && H <= 16384 && W <= 16384;
}

}  // namespace

extern "C" int ffc_lfu_gather(const float* t, int B, int c, int h, int w, int up, const float* in_scale,
                              const float* in_shift, int in_relu, float* xs, void* stream) {
    FFC_CHECK_ARG(t && xs, "ffc_lfu_gather: null argument");
    FFC_CHECK_ARG(up == 1 || up == 2, "ffc_lfu_gather: up must be 1 or 2");
    FFC_CHECK_ARG(h > 0 && w > 0 && lfu_shape_ok(B, c, h * up, w * up),
                  "ffc_lfu_gather: needs c % 4 == 0 and even H = h * up, W = w * up");
    const int W2 = w * up / 2;
    const size_t n = (size_t)B * c * (h * up / 2) * W2;
    if (W2 % 4 == 0 && aligned16(t) && aligned16(xs))
        hipLaunchKernelGGL(lfu_gather_kernel<4>, dim3(lfu_grid(n / 4)), dim3(LFU_THREADS), 0, (hipStream_t)stream, t,
                           c, h, w, up, in_scale, in_shift, in_relu, xs, n / 4);
    else
        hipLaunchKernelGGL(lfu_gather_kernel<1>, dim3(lfu_grid(n)), dim3(LFU_THREADS), 0, (hipStream_t)stream, t, c,
                           h, w, up, in_scale, in_shift, in_relu, xs, n);
    return ffc::launch_status("ffc_lfu_gather");
}

extern "C" int ffc_lfu_tile_add(const float* v, const float* ys, int B, int c, int H, int W, float* out,
                                void* stream) {
    FFC_CHECK_ARG(v && ys && out, "ffc_lfu_tile_add: null argument");
    FFC_CHECK_ARG(lfu_shape_ok(B, c, H, W), "ffc_lfu_tile_add: needs c % 4 == 0 and even H, W");
    FFC_CHECK_ARG(ys != v && ys != out, "ffc_lfu_tile_add: ys may not alias v / out");
    const size_t n = (size_t)B * c * H * W;
    if ((W / 2) % 4 == 0 && aligned16(v) && aligned16(ys) && aligned16(out))
        hipLaunchKernelGGL(lfu_tile_add_kernel<4>, dim3(lfu_grid(n / 4)), dim3(LFU_THREADS), 0, (hipStream_t)stream, v,
                           ys, c, H / 2, W / 2, out, n / 4);
    else
        hipLaunchKernelGGL(lfu_tile_add_kernel<1>, dim3(lfu_grid(n)), dim3(LFU_THREADS), 0, (hipStream_t)stream, v, ys,
                           c, H / 2, W / 2, out, n);
    return ffc::launch_status("ffc_lfu_tile_add");
}

extern "C" int ffc_lfu_gather_bwd(const float* dxs, int B, int c, int H, int W, float* ds, void* stream) {
    FFC_CHECK_ARG(dxs && ds && dxs != ds, "ffc_lfu_gather_bwd: null or aliased argument");
    FFC_CHECK_ARG(lfu_shape_ok(B, c, H, W), "ffc_lfu_gather_bwd: needs c % 4 == 0 and even H, W");
    const size_t n = (size_t)B * c * H * W;
    if ((W / 2) % 4 == 0 && aligned16(dxs) && aligned16(ds))
        hipLaunchKernelGGL(lfu_gather_bwd_kernel<4>, dim3(lfu_grid(n / 4)), dim3(LFU_THREADS), 0, (hipStream_t)stream,
                           dxs, c, H / 2, W / 2, ds, n / 4);
    else
        hipLaunchKernelGGL(lfu_gather_bwd_kernel<1>, dim3(lfu_grid(n)), dim3(LFU_THREADS), 0, (hipStream_t)stream, dxs,
                           c, H / 2, W / 2, ds, n);
    return ffc::launch_status("ffc_lfu_gather_bwd");
}

extern "C" int ffc_lfu_tile_bwd(const float* dv, int B, int c, int H, int W, float* dys, void* stream) {
    FFC_CHECK_ARG(dv && dys && dv != dys, "ffc_lfu_tile_bwd: null or aliased argument");
    FFC_CHECK_ARG(lfu_shape_ok(B, c, H, W), "ffc_lfu_tile_bwd: needs c % 4 == 0 and even H, W");
    const size_t n = (size_t)B * c * (H / 2) * (W / 2);
    if ((W / 2) % 4 == 0 && aligned16(dv) && aligned16(dys))
        hipLaunchKernelGGL(lfu_tile_bwd_kernel<4>, dim3(lfu_grid(n / 4)), dim3(LFU_THREADS), 0, (hipStream_t)stream, dv,
                           c, H / 2, W / 2, dys, n / 4);
    else
        hipLaunchKernelGGL(lfu_tile_bwd_kernel<1>, dim3(lfu_grid(n)), dim3(LFU_THREADS), 0, (hipStream_t)stream, dv, c,
                           H / 2, W / 2, dys, n);
    return ffc::launch_status("ffc_lfu_tile_bwd");
}
