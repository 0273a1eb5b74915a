// The folded lane map of scan_deep_kernel (csrc/device_utils.h: swizzle_rows4_folded, wave_sum4_folded_slot, the mirror and ror8 row steps,
// the tail in three parts) against wave_sum4 on the rows as they were loaded, bit for bit.  Per round every lane holds its 16 bytes of
// four rows and of SIXTEEN queries; the reference of tree t (<c, c> and the sixteen queries) is wave_sum4 of the four rows' products,
// which leaves row j's total in the lanes with lane % 4 == j, and its stages: the head (the quad sums), the rotation by 4 and the
// rotation by 8, whose canonical values stand in quad 0 of each 16-lane row.  Under test, as the kernel does it: the rows permuted in
// place by m(l), the query images written to LDS where wave_sum4_folded_slot says and read back slot by slot, the SAME product chain,
// the heads without selects, V (four slots per phase), W (the mirror step), X (the rotation by 8), then the progressive tail with the
// <c, c> column beside it, for a pass of 1, 2, 3 and 4 phases (the registers of the phases that are off hold a huge constant: no lane
// of a phase that is on may see it).  Lane l must hold what wave_sum4 leaves for <row m(l), query 4 R + i'>, and <c, c> of row m(l).
// Rounds 0 .. 47: elements that are products of two unit-scale values of mixed sign (sums that depend on the order); 48 .. 51: a
// quarter of the elements +0 or -0; 52 .. 55: a quarter of them denormal; 56 .. 63: one huge element per row (the rest is absorbed
// or not, by the order).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../semtools_amd/csrc/device_utils.h"
using smt::f32x4;
constexpr int ROUNDS = 64, NQ = 16, TREES = 1 + NQ, VECS = 4 + NQ;
// (SMT_ROW_DOT of csrc/scan_group.h)
#define ROW_DOT(cj, qv) __builtin_fmaf((cj).w, (qv).w, __builtin_fmaf((cj).z, (qv).z, __builtin_fmaf((cj).x, (qv).x, (cj).y * (qv).y)))
// ref: [round][stage 0 head | 1 ror4 | 2 ror8 | 3 wave_sum4][tree][lane]; got_v [round][phase][slot][lane], got_w [round][phase][2][lane],
// got_x [round][phase][lane], got_f and got_cc [round][phases on - 1][lane]
__global__ void k(const f32x4 *in, float *ref, float *got_v, float *got_w, float *got_x, float *got_f, float *got_cc, f32x4 *swizzled)
{
    __shared__ f32x4 s_q[NQ * 64];
    const int lane = threadIdx.x & 63;
    for (int r = 0; r < ROUNDS; ++r) {
        f32x4 c[4];
        for (int j = 0; j < 4; ++j) c[j] = in[(r * VECS + j) * 64 + lane];
        __syncthreads();
        for (int n = 0; n < NQ; ++n) s_q[smt::wave_sum4_folded_slot(n, lane) * 64 + lane] = in[(r * VECS + 4 + n) * 64 + lane];
        __syncthreads();
        // the reference: the rows as loaded, one tree at a time, stage by stage
        for (int t = 0; t < TREES; ++t) {
            const f32x4 q = t == 0 ? c[0] : in[(r * VECS + 4 + (t - 1)) * 64 + lane];
            float p[1][4], v[1];
            for (int j = 0; j < 4; ++j) p[0][j] = t == 0 ? ROW_DOT(c[j], c[j]) : ROW_DOT(c[j], q);
            smt::wave_sum4_multi_head<1>(p, v, lane);
            ref[((r * 4 + 0) * TREES + t) * 64 + lane] = v[0];
            v[0] += smt::dpp_f<smt::DPP_ROW_ROR4>(v[0]);
            ref[((r * 4 + 1) * TREES + t) * 64 + lane] = v[0];
            v[0] += smt::dpp_f<smt::DPP_ROW_ROR8>(v[0]);
            ref[((r * 4 + 2) * TREES + t) * 64 + lane] = v[0];
            ref[((r * 4 + 3) * TREES + t) * 64 + lane] = smt::wave_sum4(p[0][0], p[0][1], p[0][2], p[0][3], lane);
        }
        // under test
        smt::swizzle_rows4_folded(c[0], c[1], c[2], c[3], lane);
        for (int j = 0; j < 4; ++j) swizzled[(r * 4 + j) * 64 + lane] = c[j];
        float pcc[1][4], vcc[1], x[4];
        for (int j = 0; j < 4; ++j) pcc[0][j] = ROW_DOT(c[j], c[j]);
        smt::wave_sum4_swizzled_head<1>(pcc, vcc);
        const float cc_rows = smt::wave_sum4_fold_cc_rows(vcc[0]);
        for (int h = 0; h < 4; ++h) {
            float part[4][4], v[4];
            for (int s = 0; s < 4; ++s) {
                const f32x4 q = s_q[(4 * h + s) * 64 + lane];
                for (int j = 0; j < 4; ++j) part[s][j] = ROW_DOT(c[j], q);
            }
            smt::wave_sum4_swizzled_head<4>(part, v);
            for (int s = 0; s < 4; ++s) got_v[((r * 4 + h) * 4 + s) * 64 + lane] = v[s];
            const float w0 = smt::wave_sum4_fold_mirror(v[0], v[1]), w1 = smt::wave_sum4_fold_mirror(v[2], v[3]);
            got_w[((r * 4 + h) * 2 + 0) * 64 + lane] = w0;
            got_w[((r * 4 + h) * 2 + 1) * 64 + lane] = w1;
            x[h] = smt::wave_sum4_fold_ror8(w0, w1);
            got_x[(r * 4 + h) * 64 + lane] = x[h];
        }
        for (int on = 1; on <= 4; ++on) {   // the pass serves 4 on - 3 .. 4 on calls: phases 0 .. on - 1
            float cc = cc_rows, t[4];
            for (int h = 0; h < 4; ++h) t[h] = h < on ? x[h] : 3.0e38f;
            smt::wave_sum4_fold_tail16_cc(cc, t[0], t[1]);
            if (on > 2) smt::wave_sum4_fold_tail16(t[2], t[3]);
            smt::wave_sum4_fold_tail32_cc(cc, t[0], t[2]);
            got_f[(r * 4 + on - 1) * 64 + lane] = t[0];
            got_cc[(r * 4 + on - 1) * 64 + lane] = cc;
        }
    }
}
int main()
{
    constexpr int N_IN = ROUNDS * VECS * 64 * 4, N_REF = ROUNDS * 4 * TREES * 64, N_V = ROUNDS * 16 * 64, N_W = ROUNDS * 8 * 64, N_X = ROUNDS * 4 * 64, N_SW = ROUNDS * 4 * 64 * 4;
    static float h[N_IN], ref[N_REF], got_v[N_V], got_w[N_W], got_x[N_X], got_f[N_X], got_cc[N_X], sw[N_SW];
    uint32_t s = 12345u;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (s >> 8) & 0xFFFFu; };
    for (int i = 0; i < N_IN; ++i) {
        const int r = i / (VECS * 64 * 4), vec = i / (64 * 4) % VECS, lane = i / 4 % 64, e = i % 4;
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
    struct Buf { void *host; size_t bytes; float *dev; } bufs[] = {{h, sizeof(h), nullptr}, {ref, sizeof(ref), nullptr}, {got_v, sizeof(got_v), nullptr}, {got_w, sizeof(got_w), nullptr},
                                                                   {got_x, sizeof(got_x), nullptr}, {got_f, sizeof(got_f), nullptr}, {got_cc, sizeof(got_cc), nullptr}, {sw, sizeof(sw), nullptr}};
    for (Buf &b : bufs)
        if (hipMalloc(&b.dev, b.bytes) != hipSuccess || (b.host == h ? hipMemcpy(b.dev, h, b.bytes, hipMemcpyHostToDevice) : hipMemset(b.dev, 0, b.bytes)) != hipSuccess) {
            printf("FAIL (hipMalloc or the copy to the device)\n");
            return 2;
        }
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, (const f32x4 *)bufs[0].dev, bufs[1].dev, bufs[2].dev, bufs[3].dev, bufs[4].dev, bufs[5].dev, bufs[6].dev, (f32x4 *)bufs[7].dev);
    for (Buf &b : bufs)
        if (b.host != h && hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost) != hipSuccess) {
            printf("FAIL (hipMemcpy)\n");
            return 2;
        }
    int bad = 0, nonzero = 0, moved = 0;
    auto check = [&](const char *what, int r, int lane, int a, float want, float got) {
        nonzero += want != 0.0f;
        if (memcmp(&want, &got, 4) != 0) {
            if (bad < 12) printf("%s round %d lane %d (%d): wave_sum4 %a folded %a\n", what, r, lane, a, want, got);
            ++bad;
        }
    };
    auto stage = [&](int r, int st, int t, int lane) { return ref[((r * 4 + st) * TREES + t) * 64 + lane]; };
    int seen[NQ][4] = {};
    for (int r = 0; r < ROUNDS; ++r)
        for (int lane = 0; lane < 64; ++lane) {
            // the map as the issue states it, written out here and not taken from device_utils.h
            const int R = lane >> 4, i = (lane >> 2) & 3, j = lane & 3, m = j ^ ((i & 1) ? 3 : 0), ip = (4 - i) & 3;
            if (r == 0) ++seen[4 * R + ip][m];
            for (int kk = 0; kk < 4; ++kk) {   // register kk holds row kk ^ m
                const float *want = &h[((r * VECS + (kk ^ m)) * 64 + lane) * 4], *got = &sw[((r * 4 + kk) * 64 + lane) * 4];
                moved += memcmp(&h[((r * VECS + kk) * 64 + lane) * 4], got, 16) != 0;
                if (memcmp(want, got, 16) != 0) {
                    if (bad < 12) printf("permuted rows round %d lane %d register %d: not row %d\n", r, lane, kk, kk ^ m);
                    ++bad;
                }
            }
            for (int hh = 0; hh < 4; ++hh) {
                // V: the quad's sum of row m, which the frozen head leaves in lane m of the same quad
                for (int sl = 0; sl < 4; ++sl)
                    check("V", r, lane, 4 * hh + sl, stage(r, 0, 1 + 4 * hh + (sl ^ ip), (lane & ~3) | m), got_v[((r * 4 + hh) * 4 + sl) * 64 + lane]);
                // W: q_i + q_{3-i}; the rotation by 4 leaves q_0 + q_3 in quad 0 and q_2 + q_1 in quad 2
                const int wq = (i == 0 || i == 3) ? 0 : 2;
                check("W0", r, lane, hh, stage(r, 1, 1 + 4 * hh + ip, 16 * R + 4 * wq + m), got_w[((r * 4 + hh) * 2 + 0) * 64 + lane]);
                check("W1", r, lane, hh, stage(r, 1, 1 + 4 * hh + (2 ^ ip), 16 * R + 4 * wq + m), got_w[((r * 4 + hh) * 2 + 1) * 64 + lane]);
                // X: the row's sum, canonical in quad 0 behind the rotation by 8
                check("X", r, lane, hh, stage(r, 2, 1 + 4 * hh + ip, 16 * R + m), got_x[(r * 4 + hh) * 64 + lane]);
            }
            for (int on = 1; on <= 4; ++on) {
                check("<c,c>", r, lane, on, stage(r, 3, 0, m), got_cc[(r * 4 + on - 1) * 64 + lane]);
                if (R < on) check("final", r, lane, on, stage(r, 3, 1 + 4 * R + ip, m), got_f[(r * 4 + on - 1) * 64 + lane]);
            }
        }
    for (int n = 0; n < NQ; ++n)
        for (int m = 0; m < 4; ++m)
            if (seen[n][m] != 1) { printf("pair (query %d, row %d) is held by %d lanes\n", n, m, seen[n][m]); ++bad; }
    if (nonzero < ROUNDS * 64 * 20 || moved < ROUNDS * 48 * 2) { printf("FAIL (the kernel wrote nothing)\n"); return 2; }
    printf(bad ? "FAIL (%d values)\n" : "PASS wave_sum4_folded\n", bad);
    return bad != 0;
}
