// The heads of scan_deep_kernel's trees on rows permuted by lane (csrc/device_utils.h: swizzle_rows4 + wave_sum4_swizzled_head) against
// wave_sum4 on the rows as they were loaded, bit for bit.  Per round every lane holds its 16 bytes of four rows and of four queries;
// the reference of tree t (<c, c> and the four queries) is wave_sum4 of the four rows' products, which leaves row j's total in the
// lanes with lane % 4 == j.  Under test, as the kernel does it: the rows permuted in place, the SAME product chain on the permuted
// registers, the heads without selects, then wave_sum4_rows<5> + wave_sum4_group_tail (a phase of the A kind: <c, c> in every lane,
// query g in row g of the wave) and wave_sum4_rows<4> + wave_sum4_group_tail_queries (a phase of the B kind, the queries in the
// opposite order).  Lane 16 g + 4 i + j must hold what wave_sum4 leaves there for query g, i.e. row j's total.  The permuted rows
// themselves are written out too and compared with c[k ^ (lane & 3)].
// Rounds 0 .. 47: elements that are products of two unit-scale values of mixed sign (sums that depend on the order); 48 .. 51: a
// quarter of the elements +0 or -0; 52 .. 55: a quarter of them denormal; 56 .. 63: one huge element per row (the rest is absorbed
// or not, by the order).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../semtools_amd/csrc/device_utils.h"
using smt::f32x4;
constexpr int ROUNDS = 64, TREES = 5;
// (SMT_ROW_DOT of csrc/scan_group.h)
#define ROW_DOT(cj, qv) __builtin_fmaf((cj).w, (qv).w, __builtin_fmaf((cj).z, (qv).z, __builtin_fmaf((cj).x, (qv).x, (cj).y * (qv).y)))
__global__ void k(const f32x4 *in, float *lone, float *got_a, float *got_b, f32x4 *swizzled)
{
    const int lane = threadIdx.x & 63;
    for (int r = 0; r < ROUNDS; ++r) {
        f32x4 c[4], q[4];
        for (int j = 0; j < 4; ++j) c[j] = in[(r * 8 + j) * 64 + lane];
        for (int g = 0; g < 4; ++g) q[g] = in[(r * 8 + 4 + g) * 64 + lane];
        // the reference: the rows as loaded, one tree at a time
        for (int t = 0; t < TREES; ++t) {
            float p[4];
            for (int j = 0; j < 4; ++j) p[j] = t == 0 ? ROW_DOT(c[j], c[j]) : ROW_DOT(c[j], q[t - 1]);
            lone[(r * TREES + t) * 64 + lane] = smt::wave_sum4(p[0], p[1], p[2], p[3], lane);
        }
        // under test
        smt::swizzle_rows4(c[0], c[1], c[2], c[3], lane);
        for (int j = 0; j < 4; ++j) swizzled[(r * 4 + j) * 64 + lane] = c[j];
        float part[3][4], part2[2][4], v3[3], v2[2];
        for (int j = 0; j < 4; ++j) {
            part[0][j] = ROW_DOT(c[j], c[j]);
            part[1][j] = ROW_DOT(c[j], q[0]);
            part[2][j] = ROW_DOT(c[j], q[1]);
            part2[0][j] = ROW_DOT(c[j], q[2]);
            part2[1][j] = ROW_DOT(c[j], q[3]);
        }
        smt::wave_sum4_swizzled_head<3>(part, v3);
        smt::wave_sum4_swizzled_head<2>(part2, v2);
        float v5[5] = {v3[0], v3[1], v3[2], v2[0], v2[1]};
        smt::wave_sum4_rows<5>(v5);
        smt::wave_sum4_group_tail(v5[0], v5[1], v5[2], v5[3], v5[4]);
        got_a[(r * 2 + 0) * 64 + lane] = v5[0];
        got_a[(r * 2 + 1) * 64 + lane] = v5[1];
        float parta[2][4], partc[2][4], w2[2], x2[2];
        for (int j = 0; j < 4; ++j) {
            parta[0][j] = ROW_DOT(c[j], q[3]);
            parta[1][j] = ROW_DOT(c[j], q[2]);
            partc[0][j] = ROW_DOT(c[j], q[1]);
            partc[1][j] = ROW_DOT(c[j], q[0]);
        }
        smt::wave_sum4_swizzled_head<2>(parta, w2);
        smt::wave_sum4_swizzled_head<2>(partc, x2);
        float v4[4] = {w2[0], w2[1], x2[0], x2[1]};
        smt::wave_sum4_rows<4>(v4);
        smt::wave_sum4_group_tail_queries(v4[0], v4[1], v4[2], v4[3]);
        got_b[r * 64 + lane] = v4[0];
    }
}
int main()
{
    constexpr int N_IN = ROUNDS * 8 * 64 * 4, N_LONE = ROUNDS * TREES * 64, N_A = ROUNDS * 2 * 64, N_B = ROUNDS * 64, N_SW = ROUNDS * 4 * 64 * 4;
    static float h[N_IN], lone[N_LONE], got_a[N_A], got_b[N_B], sw[N_SW];
    uint32_t s = 12345u;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (s >> 8) & 0xFFFFu; };
    for (int i = 0; i < N_IN; ++i) {
        const int r = i / (8 * 64 * 4), vec = i / (64 * 4) % 8, lane = i / 4 % 64, e = i % 4;
        const float u = (float)next() / 65536.0f - 0.5f;
        float x = 4.0f * u * ((float)next() / 65536.0f - 0.5f);
        const uint32_t dice = next();
        if (r >= 48 && r < 52 && (dice & 3) == 0) x = (dice & 4) ? 0.0f : -0.0f;
        if (r >= 52 && r < 56 && (dice & 3) == 0) {
            const uint32_t bits = ((dice & 4) ? 0x80000000u : 0u) | (1u + (dice >> 3) * 997u % 0x7FFFFFu);   // exponent 0: a denormal
            memcpy(&x, &bits, 4);
        }
        if (r >= 56 && vec < 4 && lane == (int)((7u * r + 13u * vec) % 64u) && e == (r + vec) % 4) x = (r & 1) ? 3.0e18f : -3.0e18f;
        h[i] = x;
    }
    float *d_in, *d_lone, *d_a, *d_b, *d_sw;
    if (hipMalloc(&d_in, sizeof(h)) != hipSuccess || hipMalloc(&d_lone, sizeof(lone)) != hipSuccess || hipMalloc(&d_a, sizeof(got_a)) != hipSuccess ||
        hipMalloc(&d_b, sizeof(got_b)) != hipSuccess || hipMalloc(&d_sw, sizeof(sw)) != hipSuccess) {
        printf("FAIL (hipMalloc)\n");
        return 2;
    }
    if (hipMemcpy(d_in, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_lone, 0, sizeof(lone)) != hipSuccess ||
        hipMemset(d_a, 0, sizeof(got_a)) != hipSuccess || hipMemset(d_b, 0, sizeof(got_b)) != hipSuccess || hipMemset(d_sw, 0, sizeof(sw)) != hipSuccess) {
        printf("FAIL (hipMemcpy to the device)\n");
        return 2;
    }
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, (const f32x4 *)d_in, d_lone, d_a, d_b, (f32x4 *)d_sw);
    if (hipMemcpy(lone, d_lone, sizeof(lone), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(got_a, d_a, sizeof(got_a), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(got_b, d_b, sizeof(got_b), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(sw, d_sw, sizeof(sw), hipMemcpyDeviceToHost) != hipSuccess) {
        printf("FAIL (hipMemcpy)\n");
        return 2;
    }
    int bad = 0, nonzero = 0, moved = 0;
    auto check = [&](const char *what, int r, int lane, float want, float got) {
        nonzero += want != 0.0f;
        if (memcmp(&want, &got, 4) != 0) {
            if (bad < 8) printf("%s round %d lane %d: wave_sum4 %a swizzled %a\n", what, r, lane, want, got);
            ++bad;
        }
    };
    for (int r = 0; r < ROUNDS; ++r)
        for (int lane = 0; lane < 64; ++lane) {
            const int g = lane >> 4;
            for (int kk = 0; kk < 4; ++kk) {   // register kk holds row kk ^ (lane & 3)
                const float *want = &h[((r * 8 + (kk ^ (lane & 3))) * 64 + lane) * 4], *got = &sw[((r * 4 + kk) * 64 + lane) * 4];
                moved += memcmp(&h[((r * 8 + kk) * 64 + lane) * 4], got, 16) != 0;
                if (memcmp(want, got, 16) != 0) {
                    if (bad < 8) printf("permuted rows round %d lane %d register %d: not row %d\n", r, lane, kk, kk ^ (lane & 3));
                    ++bad;
                }
            }
            check("<c,c>", r, lane, lone[(r * TREES + 0) * 64 + lane], got_a[(r * 2 + 0) * 64 + lane]);
            check("query tree, phase A", r, lane, lone[(r * TREES + 1 + g) * 64 + lane], got_a[(r * 2 + 1) * 64 + lane]);
            check("query tree, phase B", r, lane, lone[(r * TREES + 1 + (3 - g)) * 64 + lane], got_b[r * 64 + lane]);
        }
    if (nonzero < ROUNDS * 64 * 2 || moved < ROUNDS * 48 * 2) { printf("FAIL (the kernel wrote nothing)\n"); return 2; }
    printf(bad ? "FAIL (%d values)\n" : "PASS wave_sum4_swizzled\n", bad);
    return bad != 0;
}
