// The ordered reduce of per-block partial sums that dwln_train.hip and lncf_train.hip share: part [R][N] -> out, two jobs in one launch.
#pragma once
#include "common.h"

// out[n] = sum over the R rows of part [R][N], rows in ascending order inside each of the four waves, then the waves in ascending order; double sums
struct DwlnRJob {
    const void* part;
    void *out1, *out2;                          // column n -> out1[n] for n < n1, else out2[n - n1]
    int R, N, n1, blocks;
};
template <typename T>
__global__ __launch_bounds__(256) void dwln_reduce_kernel(DwlnRJob j0, DwlnRJob j1) {
    __shared__ double sm[4][64];
    const bool first = (int)blockIdx.x < j0.blocks;
    const int b = first ? blockIdx.x : blockIdx.x - j0.blocks;
    const T* part = reinterpret_cast<const T*>(first ? j0.part : j1.part);
    T* out1 = reinterpret_cast<T*>(first ? j0.out1 : j1.out1);
    T* out2 = reinterpret_cast<T*>(first ? j0.out2 : j1.out2);
    const int R = first ? j0.R : j1.R, N = first ? j0.N : j1.N, n1 = first ? j0.n1 : j1.n1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = b * 64 + lane;
    double a = 0;
    if (n < N)
        for (int r = wave; r < R; r += 4) a += (double)part[(size_t)r * N + n];
    sm[wave][lane] = a;
    __syncthreads();
    if (wave == 0 && n < N) {
        a = ((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane];
        if (n < n1) out1[n] = (T)a;
        else out2[n - n1] = (T)a;
    }
}
