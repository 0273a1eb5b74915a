// The merged tail of the grouped scan's trees (csrc/device_utils.h: wave_sum4_rows + wave_sum4_group_tail behind the heads of
// wave_sum4_multi) against wave_sum4, bit for bit: <c, c> must come out in every lane as wave_sum4 leaves it, and query tree g in
// every lane of ROW g of the wave (lanes 16 g .. 16 g + 15) as wave_sum4 leaves it there -- same additions, same operands, same
// order -- on 64 rounds of inputs whose sums DO depend on the order (products of unit-scale values of mixed sign).  Also with
// trees 2 and 3 absent (a group of two calls: the tail is fed the registers of trees 0 and 1 again): rows 0 and 1 must not change.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../semtools_amd/csrc/device_utils.h"
constexpr int TREES = 5, ROUNDS = 64;
__global__ void k(const float *in, float *lone, float *merged, float *merged2)
{
    const int lane = threadIdx.x & 63;
    for (int r = 0; r < ROUNDS; ++r) {
        float v[TREES][4];
        for (int t = 0; t < TREES; ++t)
            for (int j = 0; j < 4; ++j) v[t][j] = in[((r * TREES + t) * 4 + j) * 64 + lane];
        for (int t = 0; t < TREES; ++t) lone[(r * TREES + t) * 64 + lane] = smt::wave_sum4(v[t][0], v[t][1], v[t][2], v[t][3], lane);
        float a[3][4], b[2][4], ha[3], hb[2];
        for (int j = 0; j < 4; ++j) {
            a[0][j] = v[0][j]; a[1][j] = v[1][j]; a[2][j] = v[2][j];
            b[0][j] = v[3][j]; b[1][j] = v[4][j];
        }
        smt::wave_sum4_multi_head<3>(a, ha, lane);
        smt::wave_sum4_multi_head<2>(b, hb, lane);
        float v5[5] = {ha[0], ha[1], ha[2], hb[0], hb[1]};
        smt::wave_sum4_rows<5>(v5);
        float w5[5] = {v5[0], v5[1], v5[2], v5[1], v5[2]};   // the group of two
        smt::wave_sum4_group_tail(v5[0], v5[1], v5[2], v5[3], v5[4]);
        smt::wave_sum4_group_tail(w5[0], w5[1], w5[2], w5[3], w5[4]);
        merged[(r * 2 + 0) * 64 + lane] = v5[0];
        merged[(r * 2 + 1) * 64 + lane] = v5[1];
        merged2[(r * 2 + 0) * 64 + lane] = w5[0];
        merged2[(r * 2 + 1) * 64 + lane] = w5[1];
    }
}
int main()
{
    constexpr int N_IN = ROUNDS * TREES * 4 * 64, N_LONE = ROUNDS * TREES * 64, N_OUT = ROUNDS * 2 * 64;
    static float h[N_IN], lone[N_LONE], merged[N_OUT], merged2[N_OUT];
    uint32_t s = 12345u;
    for (int i = 0; i < N_IN; ++i) {
        s = s * 1664525u + 1013904223u;
        const float u = (float)((s >> 8) & 0xFFFF) / 65536.0f - 0.5f;
        s = s * 1664525u + 1013904223u;
        h[i] = u * ((float)((s >> 8) & 0xFFFF) / 65536.0f - 0.5f);
    }
    float *d_in, *d_lone, *d_merged, *d_merged2;
    if (hipMalloc(&d_in, sizeof(h)) != hipSuccess || hipMalloc(&d_lone, sizeof(lone)) != hipSuccess ||
        hipMalloc(&d_merged, sizeof(merged)) != hipSuccess || hipMalloc(&d_merged2, sizeof(merged2)) != hipSuccess) {
        printf("FAIL (hipMalloc)\n");
        return 2;
    }
    hipMemcpy(d_in, h, sizeof(h), hipMemcpyHostToDevice);
    hipMemset(d_merged, 0, sizeof(merged));
    hipMemset(d_merged2, 0, sizeof(merged2));
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, d_in, d_lone, d_merged, d_merged2);
    if (hipMemcpy(lone, d_lone, sizeof(lone), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(merged, d_merged, sizeof(merged), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(merged2, d_merged2, sizeof(merged2), hipMemcpyDeviceToHost) != hipSuccess) { printf("FAIL (hipMemcpy)\n"); return 2; }
    int bad = 0, nonzero = 0;
    auto check = [&](const char *what, int r, int lane, float want, float got) {
        nonzero += want != 0.0f;
        if (memcmp(&want, &got, 4) != 0) {
            if (bad < 8) printf("%s round %d lane %d: wave_sum4 %a merged %a\n", what, r, lane, want, got);
            ++bad;
        }
    };
    for (int r = 0; r < ROUNDS; ++r)
        for (int lane = 0; lane < 64; ++lane) {
            const int g = lane >> 4;
            check("<c,c>", r, lane, lone[(r * TREES + 0) * 64 + lane], merged[(r * 2 + 0) * 64 + lane]);
            check("query tree", r, lane, lone[(r * TREES + 1 + g) * 64 + lane], merged[(r * 2 + 1) * 64 + lane]);
            check("<c,c>, group of two", r, lane, lone[(r * TREES + 0) * 64 + lane], merged2[(r * 2 + 0) * 64 + lane]);
            if (g < 2) check("query tree, group of two", r, lane, lone[(r * TREES + 1 + g) * 64 + lane], merged2[(r * 2 + 1) * 64 + lane]);
        }
    if (nonzero < ROUNDS * 64 * 2) { printf("FAIL (the kernel wrote nothing)\n"); return 2; }
    printf(bad ? "FAIL (%d values)\n" : "PASS wave_sum4_group_tail\n", bad);
    return bad != 0;
}
