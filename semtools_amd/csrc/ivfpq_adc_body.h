// ivfpq_adc_body.h -- the ADC scan kernel of the IVF index, included TWICE by ivfpq_search.hip (no include guard):
//   IVF_ADC_KERNEL = ivf_adc_kernel,      IVF_ADC_POOL 0   the narrow route (top_k <= 56): stage 2 keeps the kp best re-scored rows
//   IVF_ADC_KERNEL = ivf_adc_pool_kernel, IVF_ADC_POOL 1   the wide route (57 ... 1024): stage 2 keeps EVERY re-scored row
// Stage 1 is the same text for both, hence the same shortlist, the same 16-bit selection and the same scan-order ties, bit for bit.
// Why an include and not one inlined __device__ body with an `if constexpr` switch: that form was tried and moved the narrow
// kernels' registers (93 -> 101 VGPRs for the PQ kind, 67 -> 76 for the per-list PCA kind at 256 threads), which
// tests/test_ivf_ranges_resources.py pins; as the text of a __global__ function the narrow instantiations compile to what they were.
//
// The pool form: the f32 distance of the row taken from lane `src` goes back to lane `src`, and after the loop each wave writes one
// coalesced 512 B line of keys (d32 bits << 32 | row) to its 64 fixed slots of the block's region of the pool,
// p.lists + (query x lists + list segment) x ADC_THREADS.  No lane list, no s_keys block merge, no atomics.
#if !defined(IVF_ADC_KERNEL) || !defined(IVF_ADC_POOL)
#error "define IVF_ADC_KERNEL and IVF_ADC_POOL before including ivfpq_adc_body.h"
#endif

template <int ADC_THREADS, int KIND, bool RANGED>
__global__ void __launch_bounds__(ADC_THREADS) IVF_ADC_KERNEL(AdcParams p)
{
    __shared__ __attribute__((aligned(16))) float s_lut[KIND == 0 ? PQ_M * PQ_K : 4];
    __shared__ key_t64 s_keys[(ADC_THREADS / 64) * 64];
    // XCD-aware block order.  Workgroups go to the 8 XCDs round-robin by their linear id, and each XCD has its own L2: with one grid
    // row per query the P = nprobe x n_seg blocks of a query landed on P different XCDs and every one of them fetched the query's
    // 32 KiB LUT (kind 0) from HBM again -- 262 MB of a 2.4 GB launch (profiles/r05_ivf/, r06_ivf/).  The grid is one line of
    // ceil(nq / 8) x 8 x P blocks: XCD x takes the queries q = 8 j + x, and the P blocks of a query follow each other ON that XCD.
    const uint32_t P = p.nprobe * p.n_seg;
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
    const uint32_t qi = (slot / P) * 8u + xcd, pblk = slot % P;
    if (qi >= p.nq) return;   // (the last group of eight queries may be short)
    const uint32_t pi = pblk / p.n_seg, seg = pblk % p.n_seg;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#if !IVF_ADC_POOL
    const int kp = (int)p.kp;
#endif
    const int ks = (int)p.shortlist;
#if IVF_ADC_POOL
    // this block's region of the pool, one slot per thread (slot = wave * 64 + lane).  (The per-list PCA kind uses it for the early
    // exit below only: its store at the end works the address out again, see there.)
    key_t64 *out = p.lists + ((size_t)qi * p.nprobe * p.n_seg + pblk) * ADC_THREADS;
#else
    key_t64 *out = p.lists + ((size_t)qi * p.nprobe * p.n_seg + pblk) * kp;
#endif
    {
        // this block's segment of the probed list; most lists are shorter than n_seg segments: leave an empty list
        const uint32_t l0 = p.probe_list[(size_t)qi * p.nprobe + pi];
        const uint64_t b0 = p.list_offsets[l0], e0 = p.list_offsets[l0 + 1];
        if (b0 + (uint64_t)seg * p.seg_len >= e0) {  // block-uniform
#if IVF_ADC_POOL
            out[threadIdx.x] = KEY_PAD;
#else
            if ((int)threadIdx.x < kp) out[threadIdx.x] = KEY_PAD;
#endif
            return;
        }
    }

    if constexpr (KIND == 0) {
        const f32x4 *lsrc = reinterpret_cast<const f32x4 *>(p.lut + (size_t)qi * PQ_M * PQ_K);
        for (int e = threadIdx.x; e < PQ_M * PQ_K / 4; e += ADC_THREADS) reinterpret_cast<f32x4 *>(s_lut)[e] = lsrc[e];
    }
    // kind 1: the 32 weights of this (query, list) pair, block-uniform (scalar loads)
    float lw[PQ_M];
    if constexpr (KIND == 1) {
        const float *src = p.lw + ((size_t)qi * p.nprobe + pi) * PQ_M;
#pragma unroll
        for (int k = 0; k < PQ_M; ++k) lw[k] = src[k];
    } else {
#pragma unroll
        for (int k = 0; k < PQ_M; ++k) lw[k] = 0.0f;
    }
    float lw_bias = 0.0f;
    if constexpr (KIND == 1) {
#pragma unroll
        for (int k = 0; k < PQ_M; ++k) lw_bias += lw[k];
        lw_bias *= 128.0f;
    }
    const uint32_t rot = (uint32_t)lane & 31u;   // KIND 0: this lane's walk through the sub-quantisers starts at rot
    const uint32_t m16 = (rot & 16u) ? 0xFFFFFFFFu : 0u, m8 = (rot & 8u) ? 0xFFFFFFFFu : 0u, m4 = (rot & 4u) ? 0xFFFFFFFFu : 0u;
    auto bfi = [](uint32_t m, uint32_t a, uint32_t b) -> uint32_t {   // (a & m) | (b & ~m) in ONE instruction, and opaque to the optimiser
        uint32_t d;
        asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(d) : "v"(m), "v"(a), "v"(b));
        return d;
    };
    const f32x4 qv = reinterpret_cast<const f32x4 *>(p.queries + (size_t)qi * 256)[lane];
    const float a2 = wave_sum(qv.x * qv.x + qv.y * qv.y + qv.z * qv.z + qv.w * qv.w);
    const bool qz = a2 == 0.0f;
    const float rq = qz ? 0.0f : __frsqrt_rn(a2);
    const uint32_t list = p.probe_list[(size_t)qi * p.nprobe + pi];
    const float base = p.probe_dot[(size_t)qi * p.nprobe + pi];
    const uint64_t begin = p.list_offsets[list] + (uint64_t)seg * p.seg_len;
    const uint64_t list_end = p.list_offsets[list + 1];
    const uint64_t end = seg + 1 == p.n_seg ? list_end : min(list_end, begin + (uint64_t)p.seg_len);  // the last segment takes the rest
    __syncthreads();

#if !IVF_ADC_POOL
    // wave-uniform insert of (cd, cr) into a lane-distributed sorted list of `cap` entries
    auto insert = [&](float cd, uint32_t cr, float &ld, uint32_t &lr, float &thr_d, uint32_t &thr_r, int cap) {
        if (cd < thr_d || (cd == thr_d && cr < thr_r)) {
            const bool less = (ld < cd) || (ld == cd && lr < cr);
            const int pos = __popcll(__ballot(less));
            const float sd = dpp_f<DPP_WAVE_SHR1>(ld);
            const uint32_t sr = dpp_u<DPP_WAVE_SHR1>(lr);
            if (lane > pos) { ld = sd; lr = sr; }
            else if (lane == pos) { ld = cd; lr = cr; }
            thr_d = readlane_f(ld, cap - 1);
            thr_r = (uint32_t)__builtin_amdgcn_readlane((int)lr, cap - 1);
        }
    };
#endif

    // ---- stage 1: ADC scan of the list's codes -> the wave's `ks` best approximate candidates (an unordered SET:
    // lane i < n_short ends up holding one of them in (ld, lr)).  A wave takes 64 x ADC_R codes per pass, keeps
    // their ADC distances in registers next to the set carried over from the previous pass, finds the ks-th
    // smallest by bisection on the distance bits (one ballot + scalar popcount per register and step) and
    // compacts the winners through LDS.  (The first version inserted candidates one at a time into a sorted
    // lane-distributed list: ~160 serial inserts per wave at ks = 64 -- that, not the re-score reads, was what
    // bounded this kernel.)
    constexpr int ADC_R = 8;
    float ld = __builtin_inff();       // carried set: lane i < n_carry holds a real entry
    uint32_t lr = 0xFFFFFFFFu;
    key_t64 *s_short = s_keys + wave * 64;  // per-wave compaction scratch (s_keys is reused by the block merge later)
    // RANGED: a lane's positions lie whole multiples of 64 apart, so its mask bits share ONE bit index and their words follow from
    // one per-lane pointer that moves with the passes -- three VGPRs; the kernel argument's two SGPRs are free again after this line
    // (the per-list PCA kind keeps its 32 weights in SGPRs and has none to spare)
    const uint64_t *mword = nullptr;
    uint32_t mshift = 0;
    if constexpr (RANGED) {
        const uint64_t first = begin + (uint64_t)wave * 64 + (uint64_t)lane;
        mword = p.mask + (first >> 6);
        mshift = (uint32_t)first & 63u;
    }
    // (64-code groups are dealt to the waves round-robin, so every wave sees codes from the whole list: lists are in
    // row order and neighbours cluster -- contiguous 512-code chunks per wave cost a point of recall)
    for (uint64_t base_i = begin; base_i < end; base_i += (uint64_t)(ADC_THREADS / 64) * 64 * ADC_R) {
        uint32_t kd[ADC_R + 1], kpos[ADC_R + 1];  // orderable distance bits (0xFFFFFFFF = empty) and list positions
#pragma unroll
        for (int r = 0; r < ADC_R; ++r) {
            const uint64_t i = base_i + ((uint64_t)r * (ADC_THREADS / 64) + wave) * 64 + lane;
            kd[r] = 0xFFFFFFFFu;
            kpos[r] = 0xFFFFFFFFu;
            bool take = i < end;
            if constexpr (RANGED) {   // bit i of the mask (a wave reads at most two adjacent words; none is read past the list's end)
                if (take) take = ((mword[r * (ADC_THREADS / 64)] >> mshift) & 1ull) != 0ull;
            }
            if (take) {
                const uint4 c0 = reinterpret_cast<const uint4 *>(p.codes + i * PQ_M)[0];
                const uint4 c1 = reinterpret_cast<const uint4 *>(p.codes + i * PQ_M)[1];
                const uint32_t w[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
                float acc = base;
                if constexpr (KIND == 1) {   // signed bytes times the pair's weights
                    // s = u - 128 with u = s ^ 0x80 as an unsigned byte: one v_cvt_f32_ubyteN per byte instead of a sign-extending
                    // bit-field extract + convert, and 128 x sum(lw) comes off the block-uniform base (lw_bias)
                    acc = base - lw_bias;
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const uint32_t x = w[u] ^ 0x80808080u;
                        acc += lw[4 * u + 0] * (float)(x & 0xFF);
                        acc += lw[4 * u + 1] * (float)((x >> 8) & 0xFF);
                        acc += lw[4 * u + 2] * (float)((x >> 16) & 0xFF);
                        acc += lw[4 * u + 3] * (float)(x >> 24);
                    }
                } else {
                    // the record rotated left by rot = lane % 32 bytes: byte t of x[] is the code of sub-quantiser (t + rot) % 32
                    // (bit selects through lane masks, one v_bfi_b32 each, as inline asm: written as `rot & 16 ? a : b` clang folds the three stages into ONE
                    // dynamically indexed pick per dword -- seven compare + select pairs each, 1400 of them per pass, 0.36 of HBM)
                    uint32_t x[8], y[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) y[u] = bfi(m16, w[(u + 4) & 7], w[u]);
#pragma unroll
                    for (int u = 0; u < 8; ++u) x[u] = bfi(m8, y[(u + 2) & 7], y[u]);
#pragma unroll
                    for (int u = 0; u < 8; ++u) y[u] = bfi(m4, x[(u + 1) & 7], x[u]);
#pragma unroll
                    for (int u = 0; u < 8; ++u) x[u] = __builtin_amdgcn_alignbyte(y[(u + 1) & 7], y[u], rot & 3);
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        acc += s_lut[((x[u] & 0xFF) << 5) | ((4 * u + 0 + rot) & 31)];
                        acc += s_lut[(((x[u] >> 8) & 0xFF) << 5) | ((4 * u + 1 + rot) & 31)];
                        acc += s_lut[(((x[u] >> 16) & 0xFF) << 5) | ((4 * u + 2 + rot) & 31)];
                        acc += s_lut[((x[u] >> 24) << 5) | ((4 * u + 3 + rot) & 31)];
                    }
                }
                const float d = fmaxf(1.0f - acc * rq, 0.0f);  // rows are unit-norm (model2vec output), zero rows score ~0
                if (acc == acc) {                                // a NaN score never becomes a candidate
                    kd[r] = min(__float_as_uint(d), 0xFFFFFFFEu);  // d >= 0: the bit pattern orders like the value
                    kpos[r] = (uint32_t)i;                         // position in list order (codes / ids / int8 rows share it)
                }
            }
        }
        kd[ADC_R] = lr != 0xFFFFFFFFu ? __float_as_uint(ld) : 0xFFFFFFFFu;  // (ld keeps only the top 16 bits: enough here)
        kpos[ADC_R] = lr;
        // (wave-wide counts through ballots: the compare writes a lane mask to SGPRs and s_bcnt1 counts it on the scalar unit --
        // 9 VALU instructions per bisection step instead of 9 + 9 + an 11-instruction lane reduction)
        uint32_t total = 0;
#pragma unroll
        for (int r = 0; r <= ADC_R; ++r) total += (uint32_t)__popcll(__ballot(kd[r] != 0xFFFFFFFFu));
        // The ADC distance is itself an approximation (error ~1e-2): its top 16 bits (relative step 2^-8 of the value)
        // are all the selection needs, which halves the bisection; ties in that bucket go by scan order.
#pragma unroll
        for (int r = 0; r <= ADC_R; ++r) kd[r] = kd[r] == 0xFFFFFFFFu ? 0xFFFFFFFFu : (kd[r] >> 16);
        uint32_t T = 0xFFFFFFFEu, need_eq = 0xFFFFFFFFu;  // winners: kd < T, plus the first need_eq entries with kd == T
        if (total > (uint32_t)ks) {
            uint32_t lo = 0u, hi = 0xFFFFu;               // smallest T with #(kd <= T) >= ks
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                uint32_t cnt = 0;
#pragma unroll
                for (int r = 0; r <= ADC_R; ++r) cnt += (uint32_t)__popcll(__ballot(kd[r] <= mid));
                if (cnt >= (uint32_t)ks) hi = mid; else lo = mid + 1u;
            }
            T = lo;
            uint32_t n_lt = 0;
#pragma unroll
            for (int r = 0; r <= ADC_R; ++r) n_lt += (uint32_t)__popcll(__ballot(kd[r] < T));
            need_eq = (uint32_t)ks - n_lt;
        }
        // compaction: winners take consecutive LDS slots, then lane i reads slot i
        uint32_t n_out = 0, n_eq_seen = 0;
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (int r = 0; r <= ADC_R; ++r) {
            const bool valid = kd[r] != 0xFFFFFFFFu;
            const bool lt = valid && kd[r] < T;
            const bool eq = valid && kd[r] == T;
            const unsigned long long m_eq = __ballot(eq);
            const bool eq_win = eq && (n_eq_seen + (uint32_t)__popcll(m_eq & below)) < need_eq;
            const unsigned long long m_win = __ballot(lt || eq_win);
            if (lt || eq_win) s_short[n_out + (uint32_t)__popcll(m_win & below)] = ((key_t64)kd[r] << 32) | kpos[r];
            n_out += (uint32_t)__popcll(m_win);
            n_eq_seen += (uint32_t)__popcll(m_eq);
        }
        __builtin_amdgcn_wave_barrier();
        const key_t64 mine = (uint32_t)lane < n_out ? reinterpret_cast<volatile key_t64 *>(s_short)[lane] : KEY_PAD;
        __builtin_amdgcn_wave_barrier();
        ld = mine != KEY_PAD ? __uint_as_float((uint32_t)(mine >> 32) << 16) : __builtin_inff();
        lr = mine != KEY_PAD ? (uint32_t)(mine & 0xFFFFFFFFull) : 0xFFFFFFFFu;
        if constexpr (RANGED) mword += (ADC_THREADS / 64) * ADC_R;
    }

    // (An int8 refinement stage between the two -- a 260 B/row copy of the rows ranking the shortlist so that only a few
    // candidates need their 1 KiB row -- was built in round 1, measured at +6 % queries/s for a 7x larger index, kept opt-in
    // for two rounds and removed in round 3.)
    const int n_short = __popcll(__ballot(lr != 0xFFFFFFFFu));  // the set sits in lanes 0..n_short-1
    unsigned long long go = n_short >= 64 ? ~0ull : ((1ull << n_short) - 1ull);  // lanes whose candidate is re-scored

    // ---- stage 2: re-score the survivors with the full-precision rows (coalesced 1 KiB loads, f32),
    //      keep the kp best; the select stage then recomputes those exactly in f64
    // RANGED: the two pointers of this stage are read from the kernel arguments HERE.  Left to the compiler they are loaded at the
    // kernel's entry and held in SGPRs across the scan loop, where the mask test's second level of lane masks takes two more than
    // the per-list PCA kind has (its 32 weights live there): it spilled p.corpus.  (The kernel's only argument is p, by value, so it
    // sits at offset 0 of the kernel-argument segment; AdcParams is standard-layout, see the static_assert below it.  What guards
    // this workaround is tests/test_ivf_ranges_resources.py: 0 spills and the twin's occupancy step for every RANGED instantiation --
    // a compiler that no longer needs it shows there as well, and the block can then go.)
    const uint32_t *ids = p.ids;
    const float *corpus = p.corpus;
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (RANGED) {
        const char *ka = reinterpret_cast<const char *>(__builtin_amdgcn_kernarg_segment_ptr());
        asm volatile("" : "+s"(ka));   // (opaque: nothing read through it moves above this line)
        ids = *reinterpret_cast<const uint32_t *const *>(ka + offsetof(AdcParams, ids));
        corpus = *reinterpret_cast<const float *const *>(ka + offsetof(AdcParams, corpus));
    }
#endif
    const uint32_t my_row = (lane < n_short && ((go >> lane) & 1ull)) ? ids[lr] : 0xFFFFFFFFu;  // one gather, before the loop
#if IVF_ADC_POOL
    float my_d = __builtin_nanf("");   // this lane's own re-scored distance, once its row has been taken
#else
    float ld2 = __builtin_inff();
    uint32_t lr2 = 0xFFFFFFFFu;
    float thr2_d = __builtin_inff();
    uint32_t thr2_r = 0xFFFFFFFFu;
#endif
    // Rows in flight per wave: the reads are random 1 KiB rows, i.e. latency, and what hides it is rows in flight per CU.  The PQ
    // kind's 32 KiB LUT keeps it at 4 waves per SIMD where the per-list PCA kind runs 7, so its waves keep EIGHT rows in flight
    // instead of four (round 6: the re-scored rows are 60 % of this kernel's bytes -- 128 KiB per block against 88 KiB of codes --
    // and their latency, not the LUT gathers, was what held the PQ kind at 0.57 of HBM).
    constexpr int RS = KIND == 0 ? 8 : 4;
    while (go) {
        f32x4 c[RS];
        uint32_t rr[RS];
        bool ok[RS];
#pragma unroll
        for (int u = 0; u < RS; ++u) {
            ok[u] = go != 0ull;
            const int src = ok[u] ? __ffsll((long long)go) - 1 : 0;
            if (ok[u]) go &= go - 1;
            rr[u] = (uint32_t)__builtin_amdgcn_readlane((int)my_row, src);
            c[u] = reinterpret_cast<const f32x4 *>(corpus + (uint64_t)(ok[u] ? rr[u] : 0u) * 256)[lane];
        }
        // four rows' norms and dot products reduced together (device_utils.h wave_sum4: lane l ends with the sum of row l % 4)
#pragma unroll
        for (int g4 = 0; g4 < RS; g4 += 4) {
            float pb[4], pa[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const f32x4 cu = c[g4 + u];
                pb[u] = cu.x * cu.x + cu.y * cu.y + cu.z * cu.z + cu.w * cu.w;
                pa[u] = cu.x * qv.x + cu.y * qv.y + cu.z * qv.z + cu.w * qv.w;
            }
            const float b2s = wave_sum4(pb[0], pb[1], pb[2], pb[3], lane);
            const float abs4 = wave_sum4(pa[0], pa[1], pa[2], pa[3], lane);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float b2 = readlane_f(b2s, u), ab = readlane_f(abs4, u);
#if IVF_ADC_POOL
                // (wave-uniform) back to the lane the row came from: the one lane that holds this row -- a row has one list position.
                // (Told by the row, not by a kept lane number: the per-list PCA kind has no SGPR to spare for four of those.)
                const float d = dist_f32(ab, b2, rq, qz);
                if (ok[g4 + u] && my_row == rr[g4 + u]) my_d = d;
#else
                if (ok[g4 + u]) insert(dist_f32(ab, b2, rq, qz), rr[g4 + u], ld2, lr2, thr2_d, thr2_r, kp);
#endif
            }
        }
    }

#if IVF_ADC_POOL
    // one coalesced 512 B line per wave.  my_d is a number only in a lane whose row was re-scored (lanes at or past n_short hold
    // my_row = 0xFFFFFFFF, which is no row of a taken candidate), and such a lane holds a corpus row the index covers: no real key
    // equals KEY_PAD.  Lanes without a candidate, or with a NaN score, write KEY_PAD: every slot is written exactly once per launch.
    if constexpr (KIND == 0) out[wave * 64 + lane] = my_d == my_d ? make_key(my_d, my_row) : KEY_PAD;
    // Per-list PCA kind: the slot's address is worked out HERE, from the block id and the kernel arguments read again (the way the
    // RANGED re-score stage reads its two pointers above).  Held from the kernel's entry, `out` sat in two SGPRs across the scan loop,
    // where this kind -- its 32 weights live there -- has none left, and spilled them.  (The PQ kind has SGPRs to spare, and the
    // address arithmetic done again in VGPRs would take its <256, RANGED> instantiation one register past its twin's occupancy step.)
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (KIND == 1) {
        const char *ka = reinterpret_cast<const char *>(__builtin_amdgcn_kernarg_segment_ptr());
        uint32_t bx = blockIdx.x;
        asm volatile("" : "+s"(ka), "+s"(bx));   // (opaque: nothing below is computed or loaded above this line)
        const uint32_t P2 = *reinterpret_cast<const uint32_t *>(ka + offsetof(AdcParams, nprobe)) *
                            *reinterpret_cast<const uint32_t *>(ka + offsetof(AdcParams, n_seg));
        key_t64 *pool = *reinterpret_cast<key_t64 *const *>(ka + offsetof(AdcParams, lists));
        const uint32_t slot2 = bx >> 3, qi2 = (slot2 / P2) * 8u + (bx & 7u), pblk2 = slot2 % P2;
        pool[((size_t)qi2 * P2 + pblk2) * ADC_THREADS + threadIdx.x] = my_d == my_d ? make_key(my_d, my_row) : KEY_PAD;
    }
#endif
#else
    // block merge of the wave lists (rank by counting), as in K2
    s_keys[wave * 64 + lane] = (lane < kp && lr2 != 0xFFFFFFFFu) ? make_key(ld2, lr2) : KEY_PAD;
    if ((int)threadIdx.x < kp) out[threadIdx.x] = KEY_PAD;
    __syncthreads();
    const key_t64 mine = s_keys[wave * 64 + lane];
    if (mine != KEY_PAD) {
        int rank = 0;
        for (int w = 0; w < ADC_THREADS / 64; ++w)
            for (int i = 0; i < kp; ++i) rank += (s_keys[w * 64 + i] < mine) ? 1 : 0;
        if (rank < kp) out[rank] = mine;
    }
#endif
}
