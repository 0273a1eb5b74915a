// What does v_pk_fma_f32 cost in a plain vector loop (no MFMA beside it)?  N independent v_pk_fma_f32 with an op_sel broadcast of one
// half of src0 against 2 N independent v_fmac_f32 -- the same flops -- at one and at two waves per SIMD on every CU, timed with
// events; and the bit equality of the two forms of the grouped scan's per-lane products (y qy, then fused adds of x, z, w; two
// queries in one register pair) on inputs with denormals, signed zeros, infinities and NaNs.
// Prints one JSON line; exit code 1 if the bits differ.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cmath>
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int ITERS = 4096;

#define R16(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15)
#define R8(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7)
#define FMAC(i) "v_fmac_f32 %" #i ", %16, %17\n\t"
#define PKFMA(i) "v_pk_fma_f32 %" #i ", %8, %9, %" #i " op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"

__global__ void scalar_loop(float *out, float x, float y)
{
    float a[16];
    for (int i = 0; i < 16; ++i) a[i] = (float)threadIdx.x + i;
    for (int it = 0; it < ITERS; ++it)   // 32 v_fmac_f32, sixteen accumulators: the same register comes back after 16 instructions
        asm volatile(R16(FMAC) R16(FMAC)
                     : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]),
                       "+v"(a[9]), "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]), "+v"(a[14]), "+v"(a[15])
                     : "v"(x), "v"(y));
    float s = 0.0f;
    for (int i = 0; i < 16; ++i) s += a[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}
__global__ void packed_loop(float *out, float x, float y)
{
    f32x2 a[8];
    for (int i = 0; i < 8; ++i) a[i] = f32x2{(float)threadIdx.x + i, (float)threadIdx.x - i};
    const f32x2 c = {x, y}, q = {y, x};
    for (int it = 0; it < ITERS; ++it)   // 16 v_pk_fma_f32, eight accumulator pairs: the same flops as the 32 above
        asm volatile(R8(PKFMA) R8(PKFMA)
                     : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7])
                     : "v"(c), "v"(q));
    float s = 0.0f;
    for (int i = 0; i < 8; ++i) s += a[i].x + a[i].y;
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// bits: lane i takes row (x, y, z, w) = in[i][0..3] and the queries q0 = in[i][4..7], q1 = in[i][8..11]
__global__ void bits(const float *in, float *scalar_out, float *packed_out, int n)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *v = in + (size_t)i * 12;
    const float x = v[0], y = v[1], z = v[2], w = v[3];
    float r0 = y * v[5], r1 = y * v[9];
    r0 = __builtin_fmaf(x, v[4], r0); r1 = __builtin_fmaf(x, v[8], r1);
    r0 = __builtin_fmaf(z, v[6], r0); r1 = __builtin_fmaf(z, v[10], r1);
    r0 = __builtin_fmaf(w, v[7], r0); r1 = __builtin_fmaf(w, v[11], r1);
    scalar_out[2 * i] = r0;
    scalar_out[2 * i + 1] = r1;
    const f32x2 xy = {x, y}, zw = {z, w};
    const f32x2 qx = {v[4], v[8]}, qy = {v[5], v[9]}, qz = {v[6], v[10]}, qw = {v[7], v[11]};   // the two queries interleaved
    f32x2 acc;
    asm volatile("v_pk_mul_f32 %0, %1, %3 op_sel:[1,0] op_sel_hi:[1,1]\n\t"           // y * (q0.y, q1.y)
                 "v_pk_fma_f32 %0, %1, %4, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"   // x
                 "v_pk_fma_f32 %0, %2, %5, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]\n\t"   // z
                 "v_pk_fma_f32 %0, %2, %6, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]"       // w
                 : "=&v"(acc)
                 : "v"(xy), "v"(zw), "v"(qy), "v"(qx), "v"(qz), "v"(qw));
    packed_out[2 * i] = acc.x;
    packed_out[2 * i + 1] = acc.y;
}

static float time_ms(void (*kern)(float *, float, float), int blocks, int threads, float *d_out)
{
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    float best = 1e30f;
    for (int rep = 0; rep < 5; ++rep) {
        hipEventRecord(e0, 0);
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, 0, d_out, 1.0000001f, 0.9999999f);
        hipEventRecord(e1, 0);
        hipEventSynchronize(e1);
        float ms = 0.0f;
        hipEventElapsedTime(&ms, e0, e1);
        if (rep && ms < best) best = ms;
    }
    return best;
}

int main()
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { printf("FAIL (no device)\n"); return 2; }
    const int cus = prop.multiProcessorCount;
    float *d_out;
    if (hipMalloc(&d_out, (size_t)cus * 512 * sizeof(float)) != hipSuccess) { printf("FAIL (hipMalloc)\n"); return 2; }
    // one block per CU: 256 threads = one wave per SIMD, 512 = two
    const float s1 = time_ms(scalar_loop, cus, 256, d_out), p1 = time_ms(packed_loop, cus, 256, d_out);
    const float s2 = time_ms(scalar_loop, cus, 512, d_out), p2 = time_ms(packed_loop, cus, 512, d_out);

    // special values in every position, then pseudo-random finite values of mixed sign and scale
    const float special[] = {0.0f, -0.0f, 1e-40f, -1e-40f, 1.17549435e-38f, 1.0f, -1.0f, 3.0e38f, -3.0e38f, INFINITY, -INFINITY, NAN,
                             1e-20f, -1e-20f, 0.33333334f, 16777217.0f};
    constexpr int NS = sizeof(special) / sizeof(special[0]), N = NS * NS * 12 + 4096;
    static float h[N * 12], hs[N * 2], hp[N * 2];
    uint32_t s = 777u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((float)((s >> 8) & 0xFFFF) / 65536.0f - 0.5f); };
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < 12; ++j) h[i * 12 + j] = rnd() * (j & 1 ? 1.0f : 1e-19f) * (i & 1 ? 1e19f : 1.0f);
    for (int a = 0; a < NS; ++a)
        for (int b = 0; b < NS; ++b)
            for (int pos = 0; pos < 12; ++pos) {
                float *v = h + (size_t)((a * NS + b) * 12 + pos) * 12;
                v[pos] = special[a];
                v[(pos + 5) % 12] = special[b];
            }
    float *d_in, *d_s, *d_p;
    if (hipMalloc(&d_in, sizeof(h)) != hipSuccess || hipMalloc(&d_s, sizeof(hs)) != hipSuccess || hipMalloc(&d_p, sizeof(hp)) != hipSuccess) {
        printf("FAIL (hipMalloc)\n");
        return 2;
    }
    hipMemcpy(d_in, h, sizeof(h), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(bits, dim3((N + 255) / 256), dim3(256), 0, 0, d_in, d_s, d_p, N);
    if (hipMemcpy(hs, d_s, sizeof(hs), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hp, d_p, sizeof(hp), hipMemcpyDeviceToHost) != hipSuccess) {
        printf("FAIL (hipMemcpy)\n");
        return 2;
    }
    int bad = 0, nans = 0, denormal = 0;
    for (int i = 0; i < N * 2; ++i) {
        nans += hs[i] != hs[i];
        denormal += hs[i] != 0.0f && fabsf(hs[i]) < 1.17549435e-38f;
        if (memcmp(&hs[i], &hp[i], 4) != 0) {
            if (bad < 8) fprintf(stderr, "input %d query %d: scalar %a packed %a\n", i / 2, i & 1, hs[i], hp[i]);
            ++bad;
        }
    }
    const double flops = (double)cus * 64.0 * ITERS * 32.0;   // fused operations per lane-wave: per wave ITERS * 32 lane-fmas
    printf("{\"cus\": %d, \"iters\": %d, \"fmac_per_iter\": 32, \"pk_fma_per_iter\": 16, "
           "\"one_wave_per_simd_ms\": {\"v_fmac_f32\": %.4f, \"v_pk_fma_f32_op_sel\": %.4f}, "
           "\"two_waves_per_simd_ms\": {\"v_fmac_f32\": %.4f, \"v_pk_fma_f32_op_sel\": %.4f}, "
           "\"packed_over_scalar_time\": [%.3f, %.3f], \"bit_check\": {\"values\": %d, \"differ\": %d, \"nan_results\": %d, \"denormal_results\": %d}}\n",
           cus, ITERS, s1, p1, s2, p2, p1 / s1, p2 / s2, N * 2, bad, nans, denormal);
    (void)flops;
    return bad != 0;
}
