// Register-resident FFTs of the Fourier-unit kernels: radix-2 for N = 2^k (2 .. 128) and one radix-3
// stage under radix-2 stages for N = 3 * 2^k (3 .. 48), the real-input / real-output forms on a
// half-size complex transform, and their twiddle tables.  Included by fft_common.h inside its
// namespace; plain C++ apart from the __device__ / __forceinline__ / __constant__ qualifiers, so a
// host program that defines those three away can include it too (tests/native/fft_mixed_host.cpp).
#pragma once

#include "twiddles.inc"

constexpr int ilog2c(int n) { return n <= 1 ? 0 : 1 + ilog2c(n >> 1); }
constexpr int brevc(int i, int bits) {
    int r = 0;
    for (int b = 0; b < bits; ++b) r |= ((i >> b) & 1) << (bits - 1 - b);
    return r;
}

constexpr bool is_pow2c(int n) { return n > 0 && (n & (n - 1)) == 0; }
// N = 3 * 2^k, 3 .. 48: the sizes of the mixed-radix transforms (twiddles from the 96-entry table)
constexpr bool is_3pow2c(int n) { return n % 3 == 0 && is_pow2c(n / 3) && n <= 48; }

// In-register DIT FFT of N = 3 * 2^k points, fully unrolled: radix-2 decimation down to 2^k
// sub-sequences of 3 points (x[o + 2^k m], m = 0 .. 2, sub-sequence o at block bitrev(o)), one stage of
// 3-point DFTs on them (no twiddles: one constant, sin(2 pi / 3)), then the radix-2 stages of
// fft_reg with half = 3, 6, .. N/2 and the same multiply-free W = 1 and W = -+i cases.
template <int N, bool INV>
__device__ __forceinline__ void fft3_reg(float (&re)[N], float (&im)[N]) {
    static_assert(is_3pow2c(N), "N = 3 * 2^k, 3 .. 48");
    constexpr int M = N / 3, L = ilog2c(M);
    constexpr float S3 = 0.8660253882408142f;   // sin(2 pi / 3), rounded once from double
    float xr[N], xi[N];
#pragma unroll
    for (int p = 0; p < N; ++p) {
        const int src = brevc(p / 3, L) + M * (p % 3);
        xr[p] = re[src];
        xi[p] = im[src];
    }
#pragma unroll
    for (int q = 0; q < M; ++q) {
        // X0 = a + b + c, X1 = a + w b + w^2 c, X2 = a + w^2 b + w c, w = exp(-+2 pi i / 3) = -1/2 -+ i S3:
        // X1, X2 = (a - (b + c) / 2) -+ i S3 (b - c) forward, +- inverse
        const float ar = xr[3 * q], ai = xi[3 * q];
        const float sr = xr[3 * q + 1] + xr[3 * q + 2], si = xi[3 * q + 1] + xi[3 * q + 2];
        const float dr = S3 * (xr[3 * q + 1] - xr[3 * q + 2]), di = S3 * (xi[3 * q + 1] - xi[3 * q + 2]);
        const float tr = ar - 0.5f * sr, ti = ai - 0.5f * si;
        re[3 * q] = ar + sr;
        im[3 * q] = ai + si;
        re[3 * q + 1] = INV ? tr - di : tr + di;
        im[3 * q + 1] = INV ? ti + dr : ti - dr;
        re[3 * q + 2] = INV ? tr + di : tr - di;
        im[3 * q + 2] = INV ? ti - dr : ti + dr;
    }
#pragma unroll
    for (int half = 3; half < N; half <<= 1) {
        const int step = 96 / (2 * half);
#pragma unroll
        for (int j = 0; j < half; ++j) {
            const bool quarter = j * step == 24;   // W_{2 half}^j = -+i
            float wr = 1.0f, wi = 0.0f;
            if (j != 0) {
                wr = c_tw3c[j * step];
                wi = INV ? c_tw3s[j * step] : -c_tw3s[j * step];
            }
#pragma unroll
            for (int i = j; i < N; i += 2 * half) {
                float yr, yi;
                if (j == 0) {
                    yr = re[i + half];
                    yi = im[i + half];
                } else if (quarter) {
                    yr = INV ? -im[i + half] : im[i + half];
                    yi = INV ? re[i + half] : -re[i + half];
                } else {
                    yr = re[i + half] * wr - im[i + half] * wi;
                    yi = re[i + half] * wi + im[i + half] * wr;
                }
                re[i + half] = re[i] - yr;
                im[i + half] = im[i] - yi;
                re[i] += yr;
                im[i] += yi;
            }
        }
    }
}

// In-register radix-2 DIT FFT, fully unrolled.  INV=false: exp(-2 pi i kn/N); INV=true: exp(+..).
// N = 2^k <= 128 (twiddles from the 128-entry table); N = 3 * 2^k <= 48 is fft3_reg above.
template <int N, bool INV>
__device__ __forceinline__ void fft_reg(float (&re)[N], float (&im)[N]) {
    if constexpr (is_3pow2c(N)) {
        fft3_reg<N, INV>(re, im);
    } else {
    static_assert(is_pow2c(N) && N <= 128, "N = 2^k, 1 .. 128, or 3 * 2^k, 3 .. 48");
    constexpr int L = ilog2c(N);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int j = brevc(i, L);
        if (j > i) {
            float t = re[i]; re[i] = re[j]; re[j] = t;
            t = im[i]; im[i] = im[j]; im[j] = t;
        }
    }
#pragma unroll
    for (int half = 1; half < N; half <<= 1) {
        const int step = 128 / (2 * half);
#pragma unroll
        for (int j = 0; j < half; ++j) {
            // twiddle W_{2 half}^j: 1 at j = 0, -i (forward) / +i (inverse) at the quarter turn -- both
            // multiply-free (the table's cos(pi/2) is 6e-17, not 0); the rest from the table
            const bool quarter = j * step == 32;
            float wr = 1.0f, wi = 0.0f;
            if (j != 0) {
                wr = c_twc[j * step];
                wi = INV ? c_tws[j * step] : -c_tws[j * step];
            }
#pragma unroll
            for (int i = j; i < N; i += 2 * half) {
                float xr, xi;
                if (j == 0) {
                    xr = re[i + half];
                    xi = im[i + half];
                } else if (quarter) {
                    xr = INV ? -im[i + half] : im[i + half];
                    xi = INV ? re[i + half] : -re[i + half];
                } else {
                    xr = re[i + half] * wr - im[i + half] * wi;
                    xi = re[i + half] * wi + im[i + half] * wr;
                }
                re[i + half] = re[i] - xr;
                im[i + half] = im[i] - xi;
                re[i] += xr;
                im[i] += xi;
            }
        }
    }
    }   // radix-2
}

// Real-input N-point DFT X[k] = sum_n x[n] exp(-2 pi i k n / N), k = 0 .. N/2, through ONE
// N/2-point complex FFT of z[n] = x[2n] + i x[2n+1] (half the butterflies and registers of
// fft_reg<N> on (x, 0)):  X[k] = E[k] + W^k O[k],  E = (Z[k] + conj Z[M-k]) / 2,
// O = (Z[k] - conj Z[M-k]) / 2i,  W = exp(-2 pi i / N),  M = N/2 (Z[M] = Z[0]).
template <int N>
__device__ __forceinline__ void rfft_reg(const float (&x)[N], float (&Xr)[N / 2 + 1], float (&Xi)[N / 2 + 1]) {
    constexpr int M = N / 2;
    float zr[M], zi[M];
#pragma unroll
    for (int n = 0; n < M; ++n) {
        zr[n] = x[2 * n];
        zi[n] = x[2 * n + 1];
    }
    fft_reg<M, false>(zr, zi);
    Xr[0] = zr[0] + zi[0];
    Xi[0] = 0.0f;
    Xr[M] = zr[0] - zi[0];
    Xi[M] = 0.0f;
#pragma unroll
    for (int k = 1; k < M; ++k) {
        const float ar = zr[k], ai = zi[k], br = zr[M - k], bi = zi[M - k];
        const float er = 0.5f * (ar + br), ei = 0.5f * (ai - bi);
        const float orr = 0.5f * (ai + bi), oi = 0.5f * (br - ar);
        if (4 * k == N) {   // W^k = -i
            Xr[k] = er + oi;
            Xi[k] = ei - orr;
        } else {
            float c, s;   // W^k = c - i s
            if constexpr (is_3pow2c(N)) {
                c = c_tw3c[k * (96 / N)];
                s = c_tw3s[k * (96 / N)];
            } else {
                c = c_twc[k * (128 / N)];
                s = c_tws[k * (128 / N)];
            }
            Xr[k] = er + (orr * c + oi * s);
            Xi[k] = ei + (oi * c - orr * s);
        }
    }
}

// Its inverse without normalisation, the C2R of irfftn: x[n] = sum_{k<N} F[k] exp(+2 pi i k n / N)
// with F[k] = X[k] (k <= N/2, Im of X[0] and X[N/2] ignored) and F[N-k] = conj X[k], through ONE
// N/2-point inverse FFT of Z[k] = (F[k] + F[k+M]) + i W^-k (F[k] - F[k+M]) (F[k+M] = conj X[M-k]):
// z[n] = x[2n] + i x[2n+1].
template <int N>
__device__ __forceinline__ void irfft_reg(const float (&Xr)[N / 2 + 1], const float (&Xi)[N / 2 + 1], float (&x)[N]) {
    constexpr int M = N / 2;
    float zr[M], zi[M];
    zr[0] = Xr[0] + Xr[M];
    zi[0] = Xr[0] - Xr[M];
#pragma unroll
    for (int k = 1; k < M; ++k) {
        const float ar = Xr[k], ai = Xi[k], br = Xr[M - k], bi = Xi[M - k];
        const float sr = ar + br, si = ai - bi;   // F[k] + conj X[M-k]
        const float dr = ar - br, di = ai + bi;   // F[k] - conj X[M-k]
        float tr, ti;                             // T = W^-k D, W^-k = c + i s
        if (4 * k == N) {
            tr = -di;
            ti = dr;
        } else {
            float c, s;
            if constexpr (is_3pow2c(N)) {
                c = c_tw3c[k * (96 / N)];
                s = c_tw3s[k * (96 / N)];
            } else {
                c = c_twc[k * (128 / N)];
                s = c_tws[k * (128 / N)];
            }
            tr = dr * c - di * s;
            ti = dr * s + di * c;
        }
        zr[k] = sr - ti;   // Z = S + i T
        zi[k] = si + tr;
    }
    fft_reg<M, true>(zr, zi);
#pragma unroll
    for (int n = 0; n < M; ++n) {
        x[2 * n] = zr[n];
        x[2 * n + 1] = zi[n];
    }
}
