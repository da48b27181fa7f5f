// Direct (VALU) ConvTranspose2d k3 s1 p1 for very few output channels (M <= 4) on gfx950, and its data
// gradient: the head of the baseline generators (torch.nn.ConvTranspose2d(64, 3, 3, stride=1,
// padding=(1,1)) + Tanh, fgan_complete.py:58-61, fgan64_complete.py:61-64, sngan_complete.py:103-104), which
// runs on the largest plane of the model and, unlike the fgan128 head (conv3x3_smallm_kernel in
// convt_smallm.hip), is trained.
//
//   forward   out[b, m, oy, ox] = act(bias[m] + sum_{c, ky, kx} x[b, c, oy + 1 - ky, ox + 1 - kx] w[c, m, ky, kx])
//   dgrad     dx[b, c, iy, ix]  =           sum_{m, ky, kx} dpre[b, m, iy - 1 + ky, ix - 1 + kx] w[c, m, ky, kx]
//
// w is the raw ConvTranspose2d weight (C, M, 3, 3): the 9 M weights of an input channel are contiguous, so
// both kernels read them per channel with scalar loads as they stand (no packed or flipped copy).
//
// Both kernels tile the plane in 32 x 16 pixels per workgroup of four waves; a lane owns 2 rows x 4 columns.
// Forward: wave q takes the channels c = q (mod 4); it stages its channel's 18 x 40 patch (halo 1, rows
// from the 16-byte aligned column x0 - 4) through registers into its own LDS double buffer -- the loads of
// channel k + 1 are in flight under channel k's FMAs -- and reads the 4 x 6 neighbourhood of its pixels as
// b32 + b128 + b32 per row (12 LDS reads feed 72 M FMAs).  The four waves' partial sums are added in wave
// order through LDS at the end (deterministic).
// Data gradient (a Conv2d 3x3 from M <= 4 to C channels, K = 9 M <= 36: too thin for an MFMA tile): the
// workgroup stages the tile of all M dpre planes once, each lane keeps its 4 x 6 x M neighbourhood in
// registers, and wave q walks the channels c = q (mod 4): 9 M scalar weights, 72 M FMAs, two float4 stores
// per channel.  Every dx element is written by one lane: no atomics.
// Rows of any width: whole aligned float4 groups when W % 4 == 0 and the tensors are 16-byte aligned,
// bounds-checked scalar loads and stores otherwise (the VEC template flag, as convt_smallm_kernel's).
#include "ffc_internal.h"

namespace {

constexpr int CT3_CMAX = 256;               // input channels (RouteCaps.CONVT3_SMALLM_CMAX)
constexpr int CT3_TW = 32, CT3_TH = 16;     // tile columns / rows
constexpr int CT3_NQ = 4;                   // waves per workgroup (forward: channel groups)
constexpr int CT3_PS = CT3_TW + 8;          // patch row: ix = x0-4 .. x0+35 (10 aligned float4 groups)
constexpr int CT3_PR = CT3_TH + 2;          // patch rows: iy = y0-1 .. y0+16
constexpr int CT3_PB = CT3_PR * CT3_PS;     // floats per channel patch
constexpr int CT3_G = CT3_PB / 4;           // float4 groups per channel patch
constexpr int CT3_GT = (CT3_G + 63) / 64;   // groups per lane (forward: one wave stages a patch)
constexpr int CT3_THREADS = 64 * CT3_NQ;
// LDS floats: the forward's [2 buffers][NQ][PB] patches, reused for the (NQ - 1) x (8 M) x 64 partial sums;
// the data gradient's [M][PB] patch
constexpr int CT3_LDS = 2 * CT3_NQ * CT3_PB > (CT3_NQ - 1) * 32 * 64 ? 2 * CT3_NQ * CT3_PB : (CT3_NQ - 1) * 32 * 64;
static_assert(CT3_TW == 32 && CT3_TH == 16, "a wave covers the tile as 8 x 8 lanes of 2 x 4 pixels");
static_assert(4 * CT3_PB <= CT3_LDS, "the data gradient's patch fits");

struct Ct3Args {
    const float* x;      // forward: input (B, C, H, W); dgrad: dpre (B, M, H, W)
    const float* w;      // (C, M, 3, 3)
    const float* bias;   // forward: (M) or null
    float* out;          // forward: (B, M, H, W); dgrad: dx (B, C, H, W)
    int B, C, H, W, M;
    int nty, ntx;
    int act;
    float act_param;
};

// one aligned 4-float group of row `row` (null: outside the image) at columns ix .. ix + 3
template <bool VEC>
__device__ __forceinline__ float4 load_group(const float* row, int ix, int W) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!row) return v;
    if (VEC) {   // W % 4 == 0 and ix % 4 == 0: the group is wholly inside or outside the row
        if ((unsigned)ix < (unsigned)W) v = *reinterpret_cast<const float4*>(row + ix);
    } else {
        if ((unsigned)ix < (unsigned)W) v.x = row[ix];
        if ((unsigned)(ix + 1) < (unsigned)W) v.y = row[ix + 1];
        if ((unsigned)(ix + 2) < (unsigned)W) v.z = row[ix + 2];
        if ((unsigned)(ix + 3) < (unsigned)W) v.w = row[ix + 3];
    }
    return v;
}

// columns ox0 .. ox0 + 3 of an output row
template <bool VEC>
__device__ __forceinline__ void store_group(float* row, int ox0, int W, float a, float b, float c, float d) {
    if (VEC) {
        if (ox0 < W) *reinterpret_cast<float4*>(row + ox0) = make_float4(a, b, c, d);
    } else {
        if (ox0 < W) row[ox0] = a;
        if (ox0 + 1 < W) row[ox0 + 1] = b;
        if (ox0 + 2 < W) row[ox0 + 2] = c;
        if (ox0 + 3 < W) row[ox0 + 3] = d;
    }
}

// the 4 x 6 neighbourhood (rows qy-1 .. qy+2, columns qx-1 .. qx+4 in tile coordinates) of a lane's pixels
__device__ __forceinline__ void read_patch(const float* patch, int qy, int qx, float (&v)[4][6]) {
    const float* p = patch + qy * CT3_PS + qx + 3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 m4 = *reinterpret_cast<const float4*>(p + i * CT3_PS + 1);
        v[i][0] = p[i * CT3_PS];
        v[i][1] = m4.x; v[i][2] = m4.y; v[i][3] = m4.z; v[i][4] = m4.w;
        v[i][5] = p[i * CT3_PS + 5];
    }
}

template <int MM, bool VEC>
__global__ __launch_bounds__(CT3_THREADS) void convt3_smallm_kernel(Ct3Args a) {
    __shared__ __attribute__((aligned(16))) float lds[CT3_LDS];
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    int bid = blockIdx.x;
    const int tx = bid % a.ntx;
    bid /= a.ntx;
    const int ty = bid % a.nty;
    const int b = bid / a.nty;
    const int y0 = ty * CT3_TH, x0 = tx * CT3_TW;
    const int qy = 2 * (lane >> 3), qx = 4 * (lane & 7);
    const int C = a.C, H = a.H, W = a.W;
    const size_t hw = (size_t)H * W;

    auto load = [&](int ci, float4 (&r)[CT3_GT]) {
        const float* xc = a.x + ((size_t)b * C + ci) * hw;
#pragma unroll
        for (int j = 0; j < CT3_GT; ++j) {
            const int n = j * 64 + lane;
            const int pr = n / (CT3_PS / 4), g = n - pr * (CT3_PS / 4);
            const int iy = y0 - 1 + pr;
            const bool rok = n < CT3_G && (unsigned)iy < (unsigned)H;
            r[j] = load_group<VEC>(rok ? xc + (size_t)iy * W : nullptr, x0 - 4 + 4 * g, W);
        }
    };
    auto buf = [&](int k) { return lds + ((k & 1) * CT3_NQ + q) * CT3_PB; };
    auto put = [&](float* dst, const float4 (&r)[CT3_GT]) {
#pragma unroll
        for (int j = 0; j < CT3_GT; ++j) {
            const int n = j * 64 + lane;
            if (n < CT3_G) reinterpret_cast<float4*>(dst)[n] = r[j];
        }
    };

    float acc[MM][2][4];
#pragma unroll
    for (int m = 0; m < MM; ++m)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[m][i][j] = 0.0f;

    // out(oy, ox) takes x(oy + 1 - ky, ox + 1 - kx): neighbourhood row i + 2 - ky, column j + 2 - kx
    auto compute = [&](int k) {
        const int ci = k * CT3_NQ + q;
        if (ci >= C) return;
        float v[4][6];
        read_patch(buf(k), qy, qx, v);
        const float* wc = a.w + (size_t)ci * (MM * 9);   // wave-uniform: scalar loads
#pragma unroll
        for (int m = 0; m < MM; ++m) {
            float k9[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) k9[t] = wc[m * 9 + t];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[m][i][j] = fmaf(v[i + 2 - ky][j + 2 - kx], k9[ky * 3 + kx], acc[m][i][j]);
        }
    };

    float4 r[CT3_GT];
    const int nsteps = (C + CT3_NQ - 1) / CT3_NQ;
    if (q < C) {
        load(q, r);
        put(buf(0), r);
    }
    __syncthreads();
    for (int k = 0; k < nsteps; ++k) {
        const int cn = (k + 1) * CT3_NQ + q;
        if (cn < C) load(cn, r);
        compute(k);
        if (cn < C) put(buf(k + 1), r);
        __syncthreads();
    }
    // fixed-order combine ((q0 + q1) + q2) + q3: waves 1 .. 3 store their sums over the patch buffers
    // (free after the loop's last barrier), wave 0 adds them in wave order
    float* part = lds;
    if (q != 0) {
#pragma unroll
        for (int m = 0; m < MM; ++m)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) part[(((q - 1) * MM + m) * 8 + i * 4 + j) * 64 + lane] = acc[m][i][j];
    }
    __syncthreads();
    if (q != 0) return;
    for (int rq = 1; rq < CT3_NQ; ++rq) {
#pragma unroll
        for (int m = 0; m < MM; ++m)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[m][i][j] += part[(((rq - 1) * MM + m) * 8 + i * 4 + j) * 64 + lane];
    }
    const int oy0 = y0 + qy, ox0 = x0 + qx;
    float* const out = a.out;
    const float ap = a.act_param;
    float bvs[MM];
#pragma unroll
    for (int m = 0; m < MM; ++m) bvs[m] = a.bias ? a.bias[m] : 0.0f;
    auto store = [&](auto actf) {
#pragma unroll
        for (int m = 0; m < MM; ++m)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int oy = oy0 + i;
                if (oy >= H) continue;
                float* row = out + (((size_t)b * MM + m) * H + oy) * W;
                store_group<VEC>(row, ox0, W, actf(acc[m][i][0] + bvs[m]), actf(acc[m][i][1] + bvs[m]),
                                 actf(acc[m][i][2] + bvs[m]), actf(acc[m][i][3] + bvs[m]));
            }
    };
    switch (a.act) {
        case FFC_ACT_RELU: store([](float v) { return fmaxf(v, 0.0f); }); break;
        case FFC_ACT_LEAKY_RELU: store([ap](float v) { return v > 0.0f ? v : v * ap; }); break;
        case FFC_ACT_TANH: store([](float v) { return tanhf(v); }); break;
        case FFC_ACT_SIGMOID: store([](float v) { return 1.0f / (1.0f + expf(-v)); }); break;
        case FFC_ACT_GELU: store([](float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }); break;
        default: store([](float v) { return v; }); break;
    }
}

template <int MM, bool VEC>
__global__ __launch_bounds__(CT3_THREADS) void convt3_smallm_dgrad_kernel(Ct3Args a) {
    __shared__ __attribute__((aligned(16))) float lds[MM * CT3_PB];
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    int bid = blockIdx.x;
    const int tx = bid % a.ntx;
    bid /= a.ntx;
    const int ty = bid % a.nty;
    const int b = bid / a.nty;
    const int y0 = ty * CT3_TH, x0 = tx * CT3_TW;
    const int qy = 2 * (lane >> 3), qx = 4 * (lane & 7);
    const int C = a.C, H = a.H, W = a.W;
    const size_t hw = (size_t)H * W;
    // the M dpre planes of the tile (+ halo), staged once by the whole workgroup
    for (int n = threadIdx.x; n < MM * CT3_G; n += CT3_THREADS) {
        const int m = n / CT3_G, nn = n - m * CT3_G;
        const int pr = nn / (CT3_PS / 4), g = nn - pr * (CT3_PS / 4);
        const int iy = y0 - 1 + pr;
        const float* gm = a.x + ((size_t)b * MM + m) * hw;
        reinterpret_cast<float4*>(lds)[n] =
            load_group<VEC>((unsigned)iy < (unsigned)H ? gm + (size_t)iy * W : nullptr, x0 - 4 + 4 * g, W);
    }
    __syncthreads();
    float v[MM][4][6];
#pragma unroll
    for (int m = 0; m < MM; ++m) read_patch(lds + m * CT3_PB, qy, qx, v[m]);
    const int iy0 = y0 + qy, ix0 = x0 + qx;
    float* const dx = a.out;
    // dx(iy, ix) takes dpre(iy - 1 + ky, ix - 1 + kx): neighbourhood row i + ky, column j + kx
    for (int c = q; c < C; c += CT3_NQ) {
        const float* wc = a.w + (size_t)c * (MM * 9);   // wave-uniform: scalar loads
        float acc[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
#pragma unroll
        for (int m = 0; m < MM; ++m) {
            float k9[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) k9[t] = wc[m * 9 + t];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[i][j] = fmaf(v[m][i + ky][j + kx], k9[ky * 3 + kx], acc[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int iy = iy0 + i;
            if (iy >= H) continue;
            float* row = dx + (((size_t)b * C + c) * H + iy) * W;
            store_group<VEC>(row, ix0, W, acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        }
    }
}

// common argument checks and tiling of the two entry points; FFC_OK or FFC_E_INVALID with the error set
int ct3_setup(const char* what, const float* in, const float* w, float* out, int B, int C, int H, int W, int M,
              Ct3Args& a, unsigned& grid, bool& vec) {
    const std::string name(what);
    FFC_CHECK_ARG(in && w && out, name + ": null pointer");
    FFC_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, name + ": B, C, H, W must be positive");
    FFC_CHECK_ARG(M >= 1 && M <= 4, name + ": 1 <= M <= 4");
    FFC_CHECK_ARG(C <= CT3_CMAX, name + ": at most 256 input channels");
    a.x = in;
    a.w = w;
    a.bias = nullptr;
    a.out = out;
    a.B = B;
    a.C = C;
    a.H = H;
    a.W = W;
    a.M = M;
    a.nty = (H + CT3_TH - 1) / CT3_TH;
    a.ntx = (W + CT3_TW - 1) / CT3_TW;
    a.act = FFC_ACT_IDENTITY;
    a.act_param = 0.0f;
    const long long tiles = (long long)B * a.nty * a.ntx;
    FFC_CHECK_ARG(tiles <= 0x7FFFFFFFll, name + ": too many tiles for one launch");
    grid = (unsigned)tiles;
    vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    return FFC_OK;
}

}  // namespace

extern "C" int ffc_convt3x3_smallm(const float* x, int C, const float* w, const float* bias, int B, int H, int W,
                                   int M, float* out, int act, float act_param, void* stream) {
    Ct3Args a;
    unsigned grid;
    bool vec;
    if (int rc = ct3_setup("ffc_convt3x3_smallm", x, w, out, B, C, H, W, M, a, grid, vec)) return rc;
    a.bias = bias;
    a.act = act;
    a.act_param = act_param;
    typedef void (*Kernel)(Ct3Args);
    static const Kernel kernels[2][4] = {
        {convt3_smallm_kernel<1, false>, convt3_smallm_kernel<2, false>, convt3_smallm_kernel<3, false>,
         convt3_smallm_kernel<4, false>},
        {convt3_smallm_kernel<1, true>, convt3_smallm_kernel<2, true>, convt3_smallm_kernel<3, true>,
         convt3_smallm_kernel<4, true>}};
    hipLaunchKernelGGL(kernels[vec][M - 1], dim3(grid), dim3(CT3_THREADS), 0, (hipStream_t)stream, a);
    return ffc::launch_status("ffc_convt3x3_smallm");
}

extern "C" int ffc_convt3x3_smallm_dgrad(const float* dpre, const float* w, int B, int C, int H, int W, int M,
                                         float* dx, void* stream) {
    Ct3Args a;
    unsigned grid;
    bool vec;
    if (int rc = ct3_setup("ffc_convt3x3_smallm_dgrad", dpre, w, dx, B, C, H, W, M, a, grid, vec)) return rc;
    typedef void (*Kernel)(Ct3Args);
    static const Kernel kernels[2][4] = {
        {convt3_smallm_dgrad_kernel<1, false>, convt3_smallm_dgrad_kernel<2, false>,
         convt3_smallm_dgrad_kernel<3, false>, convt3_smallm_dgrad_kernel<4, false>},
        {convt3_smallm_dgrad_kernel<1, true>, convt3_smallm_dgrad_kernel<2, true>,
         convt3_smallm_dgrad_kernel<3, true>, convt3_smallm_dgrad_kernel<4, true>}};
    hipLaunchKernelGGL(kernels[vec][M - 1], dim3(grid), dim3(CT3_THREADS), 0, (hipStream_t)stream, a);
    return ffc::launch_status("ffc_convt3x3_smallm_dgrad");
}
