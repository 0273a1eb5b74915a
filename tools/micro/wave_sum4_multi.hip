// wave_sum4_multi<2> and <3> (csrc/device_utils.h) against wave_sum4, bit for bit: tree t of the interleaved form must leave in every
// lane exactly what wave_sum4 leaves for the same four inputs -- same operations, same order -- on inputs whose sums DO depend on the
// order (products of unit-scale values of mixed sign), in one call and in the head / tail halves a caller may put work between.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../semtools_amd/csrc/device_utils.h"
constexpr int TREES = 5, ROUNDS = 64;
__global__ void k(const float *in, float *lone, float *multi)
{
    const int lane = threadIdx.x & 63;
    for (int r = 0; r < ROUNDS; ++r) {
        float v[TREES][4];
        for (int t = 0; t < TREES; ++t)
            for (int j = 0; j < 4; ++j) v[t][j] = in[((r * TREES + t) * 4 + j) * 64 + lane];
        for (int t = 0; t < TREES; ++t) lone[(r * TREES + t) * 64 + lane] = smt::wave_sum4(v[t][0], v[t][1], v[t][2], v[t][3], lane);
        float a[3][4], b[2][4], sa[3], sb[2], hb[2];
        for (int j = 0; j < 4; ++j) {
            a[0][j] = v[0][j]; a[1][j] = v[1][j]; a[2][j] = v[2][j];
            b[0][j] = v[3][j]; b[1][j] = v[4][j];
        }
        smt::wave_sum4_multi<3>(a, sa, lane);
        smt::wave_sum4_multi_head<2>(b, hb, lane);
        smt::wave_sum4_multi_tail<2>(hb, sb);
        for (int t = 0; t < 3; ++t) multi[(r * TREES + t) * 64 + lane] = sa[t];
        for (int t = 0; t < 2; ++t) multi[(r * TREES + 3 + t) * 64 + lane] = sb[t];
    }
}
int main()
{
    constexpr int N_IN = ROUNDS * TREES * 4 * 64, N_OUT = ROUNDS * TREES * 64;
    static float h[N_IN], lone[N_OUT], multi[N_OUT];
    uint32_t s = 12345u;
    for (int i = 0; i < N_IN; ++i) {
        s = s * 1664525u + 1013904223u;
        const float u = (float)((s >> 8) & 0xFFFF) / 65536.0f - 0.5f;
        s = s * 1664525u + 1013904223u;
        h[i] = u * ((float)((s >> 8) & 0xFFFF) / 65536.0f - 0.5f);
    }
    float *d_in, *d_lone, *d_multi;
    if (hipMalloc(&d_in, sizeof(h)) != hipSuccess || hipMalloc(&d_lone, sizeof(lone)) != hipSuccess ||
        hipMalloc(&d_multi, sizeof(multi)) != hipSuccess) { printf("FAIL (hipMalloc)\n"); return 2; }
    hipMemcpy(d_in, h, sizeof(h), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, d_in, d_lone, d_multi);
    if (hipMemcpy(lone, d_lone, sizeof(lone), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(multi, d_multi, sizeof(multi), hipMemcpyDeviceToHost) != hipSuccess) { printf("FAIL (hipMemcpy)\n"); return 2; }
    int bad = 0, nonzero = 0;
    for (int i = 0; i < N_OUT; ++i) {
        nonzero += lone[i] != 0.0f;
        if (memcmp(&lone[i], &multi[i], 4) != 0) {
            if (bad < 8) printf("round %d tree %d lane %d: lone %a multi %a\n", i / 64 / TREES, i / 64 % TREES, i % 64, lone[i], multi[i]);
            ++bad;
        }
    }
    if (nonzero < N_OUT / 2) { printf("FAIL (the kernel wrote nothing)\n"); return 2; }
    printf(bad ? "FAIL (%d values)\n" : "PASS wave_sum4_multi\n", bad);
    return bad != 0;
}
