// Host driver of the register FFTs (fastfourierconvolution_amd/csrc/fft_reg.h) for
// tests/test_fft_mixed_cpu.py: the kernels' own fft_reg / rfft_reg / irfft_reg templates, compiled
// for the CPU with the device qualifiers defined away.
//
// stdin: records "kind N count" followed by count vectors of floats
//   kind 0 / 1: fft_reg<N, false / true>   2N in (re[N] im[N])          -> 2N out
//   kind 2:     rfft_reg<N>                N in                          -> 2 (N/2+1) out (re.. im..)
//   kind 3:     irfft_reg<N>               2 (N/2+1) in (re.. im..)      -> N out
// stdout: one line per vector, %.9g.
#include <cstdio>
#include <cstdlib>

#define __device__
#define __forceinline__ inline
#define __constant__ static const
#include "fft_reg.h"

template <int N>
static bool run(int kind, int count) {
    constexpr int P = N / 2 + 1;
    for (int v = 0; v < count; ++v) {
        if (kind == 0 || kind == 1) {
            float re[N], im[N];
            for (int i = 0; i < N; ++i)
                if (scanf("%f", &re[i]) != 1) return false;
            for (int i = 0; i < N; ++i)
                if (scanf("%f", &im[i]) != 1) return false;
            if (kind == 0) fft_reg<N, false>(re, im);
            else fft_reg<N, true>(re, im);
            for (int i = 0; i < N; ++i) printf("%.9g ", re[i]);
            for (int i = 0; i < N; ++i) printf("%.9g ", im[i]);
        } else if constexpr (N % 2 == 0) {
            if (kind == 2) {
                float x[N], xr[P], xi[P];
                for (int i = 0; i < N; ++i)
                    if (scanf("%f", &x[i]) != 1) return false;
                rfft_reg<N>(x, xr, xi);
                for (int i = 0; i < P; ++i) printf("%.9g ", xr[i]);
                for (int i = 0; i < P; ++i) printf("%.9g ", xi[i]);
            } else {
                float x[N], xr[P], xi[P];
                for (int i = 0; i < P; ++i)
                    if (scanf("%f", &xr[i]) != 1) return false;
                for (int i = 0; i < P; ++i)
                    if (scanf("%f", &xi[i]) != 1) return false;
                irfft_reg<N>(xr, xi, x);
                for (int i = 0; i < N; ++i) printf("%.9g ", x[i]);
            }
        } else {
            return false;
        }
        printf("\n");
    }
    return true;
}

int main() {
    int kind, n, count;
    while (scanf("%d %d %d", &kind, &n, &count) == 3) {
        bool ok = false;
        if (kind < 0 || kind > 3 || count < 0) return 2;
        switch (n) {
            case 3: ok = run<3>(kind, count); break;
            case 6: ok = run<6>(kind, count); break;
            case 12: ok = run<12>(kind, count); break;
            case 24: ok = run<24>(kind, count); break;
            case 48: ok = run<48>(kind, count); break;
            case 8: ok = run<8>(kind, count); break;
            case 32: ok = run<32>(kind, count); break;
        }
        if (!ok) return 3;
    }
    return 0;
}
