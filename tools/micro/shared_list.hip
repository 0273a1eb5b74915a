// shared_list_insert (csrc/shared_list.h), the routine scan_wide_kernel keeps its block lists with, alone: eight waves push a fixed
// pseudo-random stream of 4096 keys -- 256 different distances, so every distance comes many times, with different rows -- into ONE
// list, all through one lock.  Whatever the schedule, the list must end as the sorted kp smallest keys, KEY_PAD behind them, the
// threshold must be the kp-th key, the lock must be free and the error word 0, for kp = 1, 9, 18 and 32.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../semtools_amd/csrc/shared_list.h"
constexpr int N_KEYS = 4096, WAVES = 8;
__global__ void __launch_bounds__(64 * WAVES) k(const float *dist, int kp, unsigned long long *out, unsigned long long *err)
{
    __shared__ smt::key_t64 s_list[smt::SHARED_LIST_KEYS];
    __shared__ unsigned long long s_thr;
    __shared__ unsigned int s_lock;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < smt::SHARED_LIST_KEYS) s_list[threadIdx.x] = smt::KEY_PAD;
    if (threadIdx.x == 0) {
        s_thr = smt::SHARED_LIST_OPEN;
        s_lock = 0u;
    }
    __syncthreads();
    for (int i = wave; i < N_KEYS; i += WAVES) {   // (i < N_KEYS: the stream's bound)
        const float d = smt::readlane_f(dist[i], 0);
        smt::shared_list_insert(s_list, &s_lock, &s_thr, d, (uint32_t)i, kp, lane, err);
    }
    __syncthreads();
    if (threadIdx.x < smt::SHARED_LIST_KEYS) out[threadIdx.x] = s_list[threadIdx.x];
    if (threadIdx.x == 0) {
        out[smt::SHARED_LIST_KEYS] = s_thr;
        out[smt::SHARED_LIST_KEYS + 1] = s_lock;
    }
}
int main()
{
    static float h[N_KEYS];
    std::vector<unsigned long long> all(N_KEYS);
    uint32_t s = 2463534242u;
    for (int i = 0; i < N_KEYS; ++i) {
        s = s * 1664525u + 1013904223u;
        h[i] = (float)((s >> 12) & 0xFF) / 256.0f;
        uint32_t bits;
        memcpy(&bits, &h[i], 4);
        all[i] = ((unsigned long long)bits << 32) | (unsigned long long)i;
    }
    std::sort(all.begin(), all.end());
    float *d_in;
    unsigned long long *d_out, *d_err;
    constexpr int N_OUT = smt::SHARED_LIST_KEYS + 2;
    if (hipMalloc(&d_in, sizeof(h)) != hipSuccess || hipMalloc(&d_out, N_OUT * 8) != hipSuccess || hipMalloc(&d_err, 8) != hipSuccess) {
        printf("FAIL (hipMalloc)\n");
        return 2;
    }
    (void)hipMemcpy(d_in, h, sizeof(h), hipMemcpyHostToDevice);
    int bad = 0;
    for (int kp : {1, 9, 18, 32}) {
        unsigned long long out[N_OUT], err = 7;
        (void)hipMemset(d_out, 0, N_OUT * 8);
        (void)hipMemset(d_err, 0, 8);
        hipLaunchKernelGGL(k, dim3(1), dim3(64 * WAVES), 0, 0, d_in, kp, d_out, d_err);
        if (hipMemcpy(out, d_out, sizeof(out), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(&err, d_err, 8, hipMemcpyDeviceToHost) != hipSuccess) {
            printf("FAIL (hipMemcpy)\n");
            return 2;
        }
        int wrong = 0;
        for (int i = 0; i < smt::SHARED_LIST_KEYS; ++i) {
            const unsigned long long want = i < kp ? all[i] : smt::KEY_PAD;
            if (out[i] != want) {
                if (wrong < 4) printf("kp %d place %d: %016llx, want %016llx\n", kp, i, out[i], want);
                ++wrong;
            }
        }
        const unsigned long long thr = (all[kp - 1] << 32) | (all[kp - 1] >> 32);
        if (out[smt::SHARED_LIST_KEYS] != thr) { printf("kp %d threshold %016llx, want %016llx\n", kp, out[smt::SHARED_LIST_KEYS], thr); ++wrong; }
        if (out[smt::SHARED_LIST_KEYS + 1] != 0) { printf("kp %d: the lock is held\n", kp); ++wrong; }
        if (err != 0) { printf("kp %d: error word %llu\n", kp, err); ++wrong; }
        printf("kp %d: %s\n", kp, wrong ? "wrong" : "ok");
        bad += wrong;
    }
    printf(bad ? "FAIL (%d)\n" : "PASS shared_list\n", bad);
    return bad != 0;
}
