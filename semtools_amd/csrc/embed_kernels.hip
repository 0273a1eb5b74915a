// embed_kernels.hip -- K1: model2vec static embedding on gfx950.
//
// Replaces the pool step of StaticModel::encode_with_args / encode_single
// (model2vec-rs 0.1.3; reference call sites src/search/mod.rs:69,138,153 and
// src/cmds/search.rs:136,154): for every line, gather the token rows of the
// table [V x 256] (f32, IEEE half or int8 as stored; narrow rows are widened in registers, which is exact), sum them IN TOKEN ORDER in f32, divide by the token
// count, then divide by max(sqrt(sum_d v_d^2), 1e-12) with the squares summed
// IN DIMENSION ORDER -- i.e. exactly the serial f32 chains of the CPU code, so
// the output is bit-identical to the oracle (oracle/semtools_oracle.c
// orc_pool_ids), not merely close.
//
// Mapping: 16 lanes (one DPP row) form a GROUP; lane a of a group owns dims {64c + 4a .. 64c + 4a + 3 : c = 0..3}:
// every gather instruction reads 16 lanes x 16 B = 256 contiguous bytes of a table row (4 instructions cover the
// 1 KiB row; tools/micro/gather_patterns.hip: this shape pulls random 1 KiB rows at 6.9 TB/s, the streaming ceiling of
// the part, also with the row number loaded from memory first), and each lane's 16 accumulators are independent
// per-dimension chains, so token order is preserved trivially.  The norm's dimension-order chain runs around the
// group with DPP row_ror:1 (64 steps x 4 adds).
//
// Work: a group owns a CONTIGUOUS RUN of lines and walks it on its own -- the four groups of a wave share an
// instruction stream but not a position: each step a group gathers the next 4 tokens of ITS current line, and a
// group whose line is complete finalises it (mean, norm, store) and moves on while the others keep gathering.  The
// first version gave a wave four lines and iterated to the longest of them: with ragged lines (0..32 tokens) a third of
// the gather slots sat idle and the kernel stopped at 5.3 TB/s on uniform ids (0.76 of what the probe shows the part
// delivers for this access pattern).
//
// Typed tables: the kernel is a template over the table element.  The f32 instantiation is the mapping above, behind
// `if constexpr`.  A half row is 512 B = 2 gather instructions (lane a owns dims {128c + 8a .. 128c + 8a + 7 : c = 0, 1}), an
// int8 row 256 B = 1 (lane a owns dims 16a .. 16a + 15): the same 16 lanes x 16 B contiguous pieces, 32 / 16 row registers in
// flight instead of 64.  half -> f32 and int8 -> f32 lose nothing (half subnormals are normal f32 values; the FP16 denormal
// mode stays at its default, on), the 16 accumulators per lane are the same independent f32 chains, and the norm chain walks
// the dimensions in order whatever the ownership -- so a typed model gives the bits of the f32 model built from the widened table.
//
// Indexed tables (vocabulary-quantised models): the model also holds tok[n_tokens] = {row, weight bits}, built and validated once by
// embed_pack_tokens_kernel from `mapping` (token id -> row) and `weights` (one scalar per token).  embed_indexed_kernel is the same body
// with one more link: id -> tok[id] -> row pieces, each widened, multiplied by the weight (the product rounded to f32; contraction is
// off, so no FMA) and added to the same 16 accumulators.  An id >= n_tokens adds nothing and still counts in the mean.  The output
// is bit-identical to plain pooling over E'[t] = fl32(weights[t] * widen(table[mapping[t]])).  These semantics are this project's
// restatement of newer model2vec versions; they are not pinned against a crate.
#include "common.h"

namespace smt {

// row_ror:n rotates the 16-lane DPP row right by n: lane i receives lane (i - n) mod 16.
constexpr int DPP_ROW_ROR1 = 0x121;
// 32-bit positions of the PF kernel step up to TU + 3 past a line's end before they are compared
constexpr uint64_t EMBED_SPAN_LIMIT = (1ull << 32) - 16;
template <int CTRL>
__device__ __forceinline__ float dppf(float v)
{
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef signed char char16_t_ __attribute__((ext_vector_type(16)));

// what a lane holds of one table row while it is in flight: NC 16-byte pieces
template <typename T> struct RowPiece;
template <> struct RowPiece<float> { using type = float4; static constexpr int NC = 4; };
template <> struct RowPiece<_Float16> { using type = half8_t; static constexpr int NC = 2; };
template <> struct RowPiece<signed char> { using type = char16_t_; static constexpr int NC = 1; };

// accumulator k = 4 c + j of a lane lives in component j of acc[c]
__device__ __forceinline__ float &comp(float4 &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

struct EmbedParams {
    const unsigned char *table; // rows of 256 elements of `kind`, as stored
    uint64_t V;
    const uint32_t *ids;
    const uint64_t *offsets;
    uint64_t n_lines;
    uint32_t max_tokens;
    int normalize;
    int batched;                // 1: parked lines wait for a wave-wide epilogue (0: each line is finished when it completes; A/B)
    float *out;
    uint64_t lines_per_group;   // a group of 16 lanes walks lines [g * lines_per_group, ...) -- unless:
    const uint64_t *run_start;  // [n_groups + 1] or nullptr: group g walks lines [run_start[g], run_start[g + 1]) (embed_runs_kernel)
    uint64_t n_groups;
    uint64_t span_limit;        // PF kernel: runs spanning this many tokens or more are left to the generic kernel (2^32; tests: small)
    int only_large;             // generic kernel: 1 = walk only the runs the PF kernel left
    int kind;                   // SMT_TABLE_F32 / F16 / I8: which instantiation the launch picked
};

// PF: the token ids of step s + 1 are requested while the rows of step s are in flight (the next position is pure arithmetic on the
// prefetched offsets), so a step waits for ONE memory round trip -- the rows -- instead of two in a row (ids, then rows).
// The PF kernel keeps token positions as 32-bit counts from the first token of its run (six position registers instead of twelve:
// that is what takes it under the 128-VGPR line of four waves per SIMD without spilling); a run spanning 2^32 tokens or more --
// 16 GiB of ids under one group -- is skipped here and walked by the generic kernel, launched behind it with only_large = 1.
// Runs of equal WORK instead of equal line counts.  A group's time is its tokens plus ~4 token-steps per line (the epilogue), and
// line lengths of real text have a heavy tail: with equal line counts a run that holds one 2048-token line among four-token ones
// takes three times as long as its neighbours and the launch waits for it (8 M lines of 4 tokens with 0.2 % of 2048: 6.6 ms against
// 4.7 for the same tokens spread evenly).  key(i) = offsets[i] - offsets[0] + 4 i is strictly increasing; run_start[g] = the first
// line whose key reaches g / n_groups of key(n_lines) -- a binary search per group, one thread each.  (The truncation to
// max_tokens is not in the key: a line far beyond it spreads its share over groups that then find nothing to do.)
constexpr uint64_t EMBED_LINE_WEIGHT = 4;
__global__ void __launch_bounds__(256) embed_runs_kernel(const uint64_t *__restrict__ offsets, uint64_t n_lines, uint64_t n_groups,
                                                         uint64_t *__restrict__ run_start)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g > n_groups) return;
    const uint64_t o0 = offsets[0];
    const uint64_t total = offsets[n_lines] - o0 + EMBED_LINE_WEIGHT * n_lines;
    // target = total * g / n_groups without overflow: total < 2^52 in practice, g <= 2^20 -- 128-bit to be safe
    const uint64_t target = (uint64_t)(((unsigned __int128)total * g) / n_groups);
    uint64_t lo = 0, hi = n_lines;   // first i in [0, n_lines] with key(i) >= target (key(n_lines) = total >= target)
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] - o0 + EMBED_LINE_WEIGHT * mid >= target) hi = mid; else lo = mid + 1;
    }
    run_start[g] = g == n_groups ? n_lines : lo;
}

// what embed_pack_tokens_kernel stores for nothing and the indexed PF kernel for a position without a known token: no table has 2^32 - 1 rows
constexpr uint32_t EMBED_NO_ROW = 0xFFFFFFFFu;

// where a group stands one step on (known before any row has arrived): whether this step completes its line, and the next step's
// active flag, first token and line end
__device__ __forceinline__ void one_step_on(bool active, uint32_t t, uint32_t t_end, uint32_t li, uint32_t n_run, uint32_t o_end,
                                            uint32_t o_next, uint32_t max_tokens, bool &d0, bool &a1, uint32_t &t1, uint32_t &e1)
{
    d0 = active && t + 4 >= t_end;
    a1 = d0 ? li + 1 < n_run : active;
    t1 = d0 ? o_end : t + 4;
    e1 = d0 ? o_next : t_end;
    if (d0 && max_tokens != 0 && e1 - t1 > max_tokens) e1 = t1 + max_tokens;
}

// IX: the indexed form (header comment): token id -> tok[id] = {row, weight} -> row pieces, each widened, multiplied by the weight
// (rounded to f32, no FMA) and added.  The plain form is the IX = false instantiation, unchanged.
template <typename T, bool PF, bool IX>
__device__ __forceinline__ void embed_body(const EmbedParams p, const uint2 *__restrict__ tok)
{
#pragma clang fp contract(off)
    constexpr bool F32 = std::is_same<T, float>::value;
    using piece_t = typename RowPiece<T>::type;
    constexpr int NC = RowPiece<T>::NC;        // gather instructions per token
    constexpr int EPL = 16 / NC;               // dims per 16-byte piece
    constexpr uint64_t ROW_BYTES = 256 * sizeof(T);
    const int lane = threadIdx.x & 63;
    const int a = lane & 15;        // position inside the group
    const uint64_t group = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    // (register diet: the kernel sits at the 128-VGPR edge of four waves per SIMD -- the position inside the run is a 32-bit count,
    // the parked line is always the one before the current, its token count is kept as the float the mean divides by)
    uint64_t line0;
    uint32_t n_run;
    if (p.run_start) {   // (kernel-uniform)
        const bool mine = group < p.n_groups;
        line0 = mine ? p.run_start[group] : 0;
        n_run = mine ? (uint32_t)(p.run_start[group + 1] - line0) : 0u;
    } else {
        line0 = group * p.lines_per_group;
        n_run = line0 < p.n_lines ? (uint32_t)min(p.n_lines - line0, p.lines_per_group) : 0u;
    }
    // positions are counted from `tb`: the run's first token in the PF kernel, 0 in the generic one
    using pos_t = typename std::conditional<PF, uint32_t, uint64_t>::type;
    uint64_t tb = 0;
    if (n_run != 0) {
        const uint64_t first = p.offsets[line0];
        const bool large = p.offsets[line0 + n_run] - first >= p.span_limit;
        if constexpr (PF) {
            tb = first;
            if (large) n_run = 0;
        } else if (p.only_large && !large) n_run = 0;
    }
    uint32_t li = 0;                                     // current line = line0 + li
    bool active = li < n_run;                            // group-uniform

    // token range of the current line [t, t_end) (max_tokens applied), its token count, and the NEXT line's end (read one
    // line ahead: a group that moves on must not wait for a dependent offsets load)
    pos_t t = 0, t_end = 0, o_end = 0, o_next = 0;
    pos_t o_next2 = 0;               // indexed PF kernel: the end of the line after the next (it looks two steps ahead)
    if (active) {
        t = (pos_t)(p.offsets[line0] - tb);
        o_end = (pos_t)(p.offsets[line0 + 1] - tb);
        o_next = 1 < n_run ? (pos_t)(p.offsets[line0 + 2] - tb) : o_end;
        if constexpr (PF && IX) o_next2 = 2 < n_run ? (pos_t)(p.offsets[line0 + 3] - tb) : o_next;
        t_end = o_end;
        if (p.max_tokens != 0 && t_end - t > (pos_t)p.max_tokens) t_end = t + p.max_tokens;
    }
    float cnt_cur = (float)(t_end - t > 0 ? t_end - t : 1);   // what the current line's sums are divided by (max(cnt, 1))

    float4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);

    float4 pend[4];                  // the sums of a complete line waiting for its epilogue
    float pend_cnt = 1.0f;
    bool has_pend = false;           // group-uniform; the parked line is line0 + li - 1
#pragma unroll
    for (int c = 0; c < 4; ++c) pend[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    auto finalize = [&]() __attribute__((always_inline)) {
        if (has_pend) {
            const float cnt = pend_cnt;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                pend[c].x = pend[c].x / cnt; pend[c].y = pend[c].y / cnt;
                pend[c].z = pend[c].z / cnt; pend[c].w = pend[c].w / cnt;
            }
            if (p.normalize) {
                // ss = (((0 + v0^2) + v1^2) + ... + v255^2), dimension order.
                // step s = 16*c + a': the true chain value sits in lane a' of the group;
                // every lane runs the same instruction stream, only lane a' matters.
                float sq[4][4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    sq[c][0] = pend[c].x * pend[c].x; sq[c][1] = pend[c].y * pend[c].y;
                    sq[c][2] = pend[c].z * pend[c].z; sq[c][3] = pend[c].w * pend[c].w;
                }
                float s = 0.0f;
                if constexpr (F32) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
#pragma unroll
                        for (int step = 0; step < 16; ++step) {
                            // take the running sum from the previous lane of the row (lane 15 -> lane 0 wraps
                            // into the next 64-dim chunk); at the very first step everyone holds 0.
                            const float in = (c == 0 && step == 0) ? 0.0f : dppf<DPP_ROW_ROR1>(s);
                            s = (((in + sq[c][0]) + sq[c][1]) + sq[c][2]) + sq[c][3];
                        }
                    }
                } else {
                    // the lane's piece c holds EPL consecutive dims (accumulators EPL c .. EPL c + EPL - 1): NC x 16 steps of EPL adds
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
#pragma unroll
                        for (int step = 0; step < 16; ++step) {
                            s = (c == 0 && step == 0) ? 0.0f : dppf<DPP_ROW_ROR1>(s);
#pragma unroll
                            for (int e = 0; e < EPL; ++e) s = s + sq[(EPL * c + e) >> 2][(EPL * c + e) & 3];
                        }
                    }
                }
                // after the last step the full chain value is in lane 15 of each group
                const float ss = __shfl(s, (lane & 48) | 15);
                float norm = sqrtf(ss);
                if (!(norm > 1e-12f)) norm = 1e-12f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    pend[c].x = pend[c].x / norm; pend[c].y = pend[c].y / norm;
                    pend[c].z = pend[c].z / norm; pend[c].w = pend[c].w / norm;
                }
            }
            float4 *o = reinterpret_cast<float4 *>(p.out + (line0 + li - 1) * 256);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if constexpr (F32) o[c * 16 + a] = pend[c];
                else if constexpr (NC == 2) o[(c >> 1) * 32 + 2 * a + (c & 1)] = pend[c];   // dims 128 c' + 8 a + 4 h ..
                else o[4 * a + c] = pend[c];                                                // dims 16 a + 4 c ..
            }
            has_pend = false;
        }
    };

    constexpr int TU = 4;  // tokens in flight per group
    // PF: the ids of the step about to run -- ONE per lane (lane a holds token a & 3 of its group's step; the gather reads it with a
    // DPP quad broadcast), so the prefetch costs one register and a quarter of the id loads
    static_assert(TU == 4, "one id per lane of a quad");
    uint32_t nid = 0;
    const uint32_t *ids = p.ids + tb;
    if constexpr (PF) nid = (active && (t + (a & 3)) < t_end) ? ids[t + (a & 3)] : 0u;
    // Indexed PF: a three-link chain ids -> tok[] -> rows.  The lane holds tok[id] of ITS token of the step about to run (`ntk`, fetched one
    // step ahead) and the id of its token of the step after (`nid`, fetched two steps ahead), so a step still waits for one round trip.
    // A position without a token, or with an id >= n_tokens, holds {EMBED_NO_ROW, +0}.
    uint2 ntk = make_uint2(EMBED_NO_ROW, 0u);
    if constexpr (PF && IX) {   // (prologue, once per run: two dependent loads)
        const bool v0 = active && (t + (a & 3)) < t_end && (uint64_t)nid < p.V;
        if (v0) ntk = tok[nid];
        bool d0, a1;
        pos_t t1, e1;
        one_step_on(active, t, t_end, li, n_run, o_end, o_next, p.max_tokens, d0, a1, t1, e1);
        nid = (a1 && (t1 + (a & 3)) < e1) ? ids[t1 + (a & 3)] : 0u;
    }
    while (__any(active)) {
        piece_t r[TU][NC];
        uint32_t idq[TU] = {0u, 0u, 0u, 0u};
        uint32_t wcur = 0u;   // IX: the weight of the lane's token of this step (broadcast over the quad when it is added)
        if constexpr (IX && !PF) {   // generic: both links inside the step, still one token per lane of a quad
            const bool onq = active && (t + (a & 3)) < t_end;
            const uint32_t idv = onq ? ids[t + (a & 3)] : 0u;
            ntk = (onq && (uint64_t)idv < p.V) ? tok[idv] : make_uint2(EMBED_NO_ROW, 0u);
        }
        if constexpr (IX) {   // idq = the ROWS of the step's tokens
            idq[0] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ntk.x, 0x00, 0xF, 0xF, false);
            idq[1] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ntk.x, 0x55, 0xF, 0xF, false);
            idq[2] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ntk.x, 0xAA, 0xF, 0xF, false);
            idq[3] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ntk.x, 0xFF, 0xF, 0xF, false);
            wcur = ntk.y;
        } else if constexpr (PF) {   // quad_perm broadcasts of lane u of every quad
            idq[0] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)nid, 0x00, 0xF, 0xF, false);
            idq[1] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)nid, 0x55, 0xF, 0xF, false);
            idq[2] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)nid, 0xAA, 0xF, 0xF, false);
            idq[3] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)nid, 0xFF, 0xF, 0xF, false);
        }
#pragma unroll
        for (int u = 0; u < TU; ++u) {
            const bool on = active && (t + u) < t_end;
            uint64_t id;
            if constexpr (PF || IX) id = idq[u];
            else id = on ? (uint64_t)ids[t + u] : 0;
            bool ok;
            if constexpr (!IX) ok = on && id < p.V;  // out-of-vocab ids contribute nothing
            else ok = on && idq[u] != EMBED_NO_ROW;  // (the pack kernel checked every row against the table: no guard here)
            // (plain loads, not nontemporal: natural text is Zipf-distributed and its hot rows must stay in L2 / MALL --
            // measured with the nt policy: Zipf ids 3.50 -> 4.59 ms, uniform ids 5.97 -> 6.27 ms; round 4: 3.18 -> 4.68, 6.56 -> 6.77)
            if constexpr (F32) {
                const float4 *row = reinterpret_cast<const float4 *>(p.table + (ok ? id : 0) * ROW_BYTES);
#pragma unroll
                for (int c = 0; c < 4; ++c) r[u][c] = ok ? row[c * 16 + a] : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                const piece_t *row = reinterpret_cast<const piece_t *>(p.table + (ok ? id : 0) * ROW_BYTES);
#pragma unroll
                for (int c = 0; c < NC; ++c) r[u][c] = ok ? row[c * 16 + a] : piece_t(0);   // (all-zero bits are +0 in every type)
            }
        }
        // where the group stands after this step -- known before any row has arrived
        const bool done = active && t + TU >= t_end;
        if constexpr (PF && IX) {
            bool d0, a1;
            pos_t t1, e1;
            one_step_on(active, t, t_end, li, n_run, o_end, o_next, p.max_tokens, d0, a1, t1, e1);
            // tok[] of the next step's token, from the id fetched a step ago
            const bool v1 = a1 && (t1 + (a & 3)) < e1 && (uint64_t)nid < p.V;
            ntk = v1 ? tok[nid] : make_uint2(EMBED_NO_ROW, 0u);
            // the id of the token of the step after that: the next step may complete a line too
            const bool d1 = a1 && t1 + TU >= e1;
            const bool a2 = d1 ? li + (d0 ? 2u : 1u) < n_run : a1;
            const pos_t t2 = d1 ? (d0 ? o_next : o_end) : t1 + TU;
            pos_t e2 = d1 ? (d0 ? o_next2 : o_next) : e1;
            if (d1 && p.max_tokens != 0 && e2 - t2 > (pos_t)p.max_tokens) e2 = t2 + p.max_tokens;
            nid = (a2 && (t2 + (a & 3)) < e2) ? ids[t2 + (a & 3)] : 0u;
        } else if constexpr (PF) {
            const bool n_active = done ? li + 1 < n_run : active;
            const pos_t nt = done ? o_end : t + TU;
            pos_t nt_end = done ? o_next : t_end;
            if (done && p.max_tokens != 0 && nt_end - nt > (pos_t)p.max_tokens) nt_end = nt + p.max_tokens;
            nid = (n_active && (nt + (a & 3)) < nt_end) ? ids[nt + (a & 3)] : 0u;
        }
#pragma unroll
        for (int u = 0; u < TU; ++u) {
            if (active && (t + u) < t_end) {  // token order: u ascending
                if constexpr (IX) {   // the product is rounded to f32, then added (contract off: no FMA); an unknown id adds +0 * +0
                    const float w =   // (u is a constant once unrolled: one quad broadcast remains)
                            __builtin_bit_cast(float, u == 0   ? __builtin_amdgcn_update_dpp(0, (int)wcur, 0x00, 0xF, 0xF, false)
                                                      : u == 1 ? __builtin_amdgcn_update_dpp(0, (int)wcur, 0x55, 0xF, 0xF, false)
                                                      : u == 2 ? __builtin_amdgcn_update_dpp(0, (int)wcur, 0xAA, 0xF, 0xF, false)
                                                               : __builtin_amdgcn_update_dpp(0, (int)wcur, 0xFF, 0xF, 0xF, false));
                    if constexpr (F32) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            acc[c].x = acc[c].x + w * r[u][c].x;
                            acc[c].y = acc[c].y + w * r[u][c].y;
                            acc[c].z = acc[c].z + w * r[u][c].z;
                            acc[c].w = acc[c].w + w * r[u][c].w;
                        }
                    } else {
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
#pragma unroll
                            for (int e = 0; e < EPL; ++e) {
                                float &d = comp(acc[(EPL * c + e) >> 2], (EPL * c + e) & 3);
                                d = d + w * (float)r[u][c][e];
                            }
                        }
                    }
                } else if constexpr (F32) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        acc[c].x = acc[c].x + r[u][c].x;
                        acc[c].y = acc[c].y + r[u][c].y;
                        acc[c].z = acc[c].z + r[u][c].z;
                        acc[c].w = acc[c].w + r[u][c].w;
                    }
                } else {   // widened in registers (exact), then the same f32 add
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
#pragma unroll
                        for (int e = 0; e < EPL; ++e) {
                            float &d = comp(acc[(EPL * c + e) >> 2], (EPL * c + e) & 3);
                            d = d + (float)r[u][c][e];
                        }
                    }
                }
            }
        }
        t += TU;
        // ---- a complete line is PARKED (its sums move to `pend`) and the group goes on gathering its next line; the epilogue --
        // mean, norm chain, store: ~640 instructions, the bulk of a line's instruction count -- runs for all parked lines of the
        // wave at once: when every group has one parked, or when a group completes a second line before that.  (Run at once per
        // completion it executed with 16 of 64 lanes enabled, once per line; measured: Zipf ids 3.75 -> 3.39 ms)
        if (__any(done && has_pend)) finalize();
        if (done) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                pend[c] = acc[c];
                acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            pend_cnt = cnt_cur;
            has_pend = true;
            // ---- next line of the run
            ++li;
            active = li < n_run;
            t = o_end;
            o_end = o_next;
            // (register diet of the indexed f32 kernels: left alone the compiler keeps &offsets[line0] in two registers of its own across the
            // loop -- and spills them; behind the empty asm the address is rebuilt from line0 where it is used, one instruction per line)
            uint64_t lb = line0;
            if constexpr (IX) asm volatile("" : "+v"(lb));
            if constexpr (PF && IX) {
                o_next = o_next2;
                if (li + 2 < n_run) o_next2 = (pos_t)(p.offsets[lb + li + 3] - tb);
            } else if (li + 1 < n_run) o_next = (pos_t)(p.offsets[lb + li + 2] - tb);
            t_end = o_end;
            if (p.max_tokens != 0 && t_end - t > (pos_t)p.max_tokens) t_end = t + p.max_tokens;
            cnt_cur = (float)(t_end - t > 0 ? t_end - t : 1);
        }
        if (__any(has_pend) && (!p.batched || __all(has_pend || !active))) finalize();
    }
    if (__any(has_pend)) finalize();
}

template <typename T, bool PF>
__global__ void __launch_bounds__(256, 4) embed_kernel(EmbedParams p)
{
    embed_body<T, PF, false>(p, nullptr);
}

// the same over a model with a token array (a kernel name of its own: the plain instantiations stay what they are)
template <typename T, bool PF>
__global__ void __launch_bounds__(256, 4) embed_indexed_kernel(EmbedParams p, const uint2 *__restrict__ tok)
{
    embed_body<T, PF, true>(p, tok);
}

// The token array of an indexed model: tok[i] = {mapping[i] or i, bits of weights[i] or 1.0f}.  Validation happens here, once, so that
// the gather needs none: the smallest i whose row is outside the table or whose weight is not finite goes to *first_bad (preset to
// 2^64 - 1), and such an entry is stored as {EMBED_NO_ROW, +0}.
__global__ void __launch_bounds__(256) embed_pack_tokens_kernel(const uint32_t *__restrict__ mapping, const float *__restrict__ weights,
                                                                uint64_t n_tokens, uint64_t n_rows, uint2 *__restrict__ tok,
                                                                unsigned long long *__restrict__ first_bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_tokens) return;
    const uint32_t row = mapping ? mapping[i] : (uint32_t)i;
    const uint32_t wbits = weights ? __builtin_bit_cast(uint32_t, weights[i]) : 0x3F800000u;
    const bool bad = (uint64_t)row >= n_rows || (wbits & 0x7F800000u) == 0x7F800000u;   // (exponent all ones: inf or NaN)
    if (bad) atomicMin(first_bad, (unsigned long long)i);
    tok[i] = bad ? make_uint2(EMBED_NO_ROW, 0u) : make_uint2(row, wbits);
}

int build_token_array(smt_ctx *ctx, const uint32_t *mapping_dev, const float *weights_dev, uint64_t n_tokens, uint64_t n_rows,
                      void **tok_out)
{
    *tok_out = nullptr;
    SMT_REQUIRE(n_tokens > 0 && n_tokens <= (1ull << 32), "n_tokens must be in 1 .. 2^32 (token ids are 32-bit)");
    SMT_REQUIRE(n_rows < EMBED_NO_ROW, "an indexed table has fewer than 2^32 - 1 rows");
    uint2 *tok = nullptr;
    unsigned long long *d_bad = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&tok), n_tokens * sizeof(uint2));
    if (e != hipSuccess) { set_error("hipMalloc(%llu) for the token array: %s", (unsigned long long)(n_tokens * sizeof(uint2)), hipGetErrorString(e)); return SMT_E_NOMEM; }
    e = hipMalloc(reinterpret_cast<void **>(&d_bad), sizeof(unsigned long long));
    if (e != hipSuccess) { (void)hipFree(tok); set_error("hipMalloc for the token array: %s", hipGetErrorString(e)); return SMT_E_NOMEM; }
    unsigned long long bad = ~0ull;
    e = hipMemsetAsync(d_bad, 0xFF, sizeof(unsigned long long), ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(embed_pack_tokens_kernel, dim3((unsigned)((n_tokens + 255) / 256)), dim3(256), 0, ctx->stream, mapping_dev, weights_dev,
                           n_tokens, n_rows, tok, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    uint32_t row = 0;
    float w = 1.0f;
    if (e == hipSuccess && bad != ~0ull) {   // what the offending token holds, for the message
        if (mapping_dev) e = hipMemcpy(&row, mapping_dev + bad, sizeof(row), hipMemcpyDeviceToHost);
        else row = (uint32_t)bad;
        if (e == hipSuccess && weights_dev) e = hipMemcpy(&w, weights_dev + bad, sizeof(w), hipMemcpyDeviceToHost);
    }
    (void)hipFree(d_bad);
    if (e != hipSuccess) { (void)hipFree(tok); set_error("building the token array: %s", hipGetErrorString(e)); return SMT_E_HIP; }
    if (bad != ~0ull) {
        (void)hipFree(tok);
        if ((uint64_t)row >= n_rows)
            set_error("token %llu: mapping entry %u is outside the table (n_rows %llu)", bad, row, (unsigned long long)n_rows);
        else set_error("token %llu: weight %g is not finite", bad, (double)w);
        return SMT_E_INVALID;
    }
    *tok_out = tok;
    return SMT_OK;
}

template <typename T>
static void launch_embed_indexed(smt_ctx *ctx, EmbedParams &p, const uint2 *tok, unsigned blocks, uint64_t n_tokens_known)
{
    p.only_large = 0;
    if (ctx->tune.embed_batched & 2) {
        hipLaunchKernelGGL((embed_indexed_kernel<T, true>), dim3(blocks), dim3(256), 0, ctx->stream, p, tok);
        if (n_tokens_known == 0 || n_tokens_known >= p.span_limit) {
            p.only_large = 1;
            hipLaunchKernelGGL((embed_indexed_kernel<T, false>), dim3(blocks), dim3(256), 0, ctx->stream, p, tok);
        }
    } else hipLaunchKernelGGL((embed_indexed_kernel<T, false>), dim3(blocks), dim3(256), 0, ctx->stream, p, tok);
}

template <typename T>
static void launch_embed_typed(smt_ctx *ctx, EmbedParams &p, const uint2 *tok, unsigned blocks, uint64_t n_tokens_known)
{
    if (tok) return launch_embed_indexed<T>(ctx, p, tok, blocks, n_tokens_known);
    // (A/B: embed_batched bit 1 = ids prefetched one step ahead.  Probed in round 4 and removed: the same kernel at three waves per
    // SIMD without spills -- Zipf 3.11 -> 3.32 ms -- and nontemporal row loads -- 4.68 / 6.77 ms; profiles/r04_k1/)
    p.only_large = 0;
    if (ctx->tune.embed_batched & 2) {
        hipLaunchKernelGGL((embed_kernel<T, true>), dim3(blocks), dim3(256), 0, ctx->stream, p);
        // the runs it left: none when the caller knows the batch holds fewer tokens than the limit (n_tokens_known = 0: offsets
        // only exist on the device -- the launch finds nothing to do and costs a few microseconds)
        if (n_tokens_known == 0 || n_tokens_known >= p.span_limit) {
            p.only_large = 1;
            hipLaunchKernelGGL((embed_kernel<T, false>), dim3(blocks), dim3(256), 0, ctx->stream, p);
        }
    } else hipLaunchKernelGGL((embed_kernel<T, false>), dim3(blocks), dim3(256), 0, ctx->stream, p);
}

int launch_embed(smt_ctx *ctx, const void *table, int table_dtype, uint64_t V, int normalize, const uint32_t *ids,
                 const uint64_t *offsets, uint64_t n_lines, uint32_t max_tokens, float *out, uint64_t n_tokens_known,
                 const void *tok_array, uint64_t n_tok)
{
    const uint2 *tok = static_cast<const uint2 *>(tok_array);
    if (n_lines == 0) return SMT_OK;
    SMT_REQUIRE(table_dtype == SMT_TABLE_F32 || table_dtype == SMT_TABLE_F16 || table_dtype == SMT_TABLE_I8, "unknown table dtype");
    EmbedParams p;
    p.table = static_cast<const unsigned char *>(table);
    p.kind = table_dtype;
    p.V = tok ? n_tok : V;   // what an id is checked against: the token array's length in the indexed form
    p.ids = ids;
    p.offsets = offsets;
    p.n_lines = n_lines;
    p.max_tokens = max_tokens;
    p.normalize = normalize;
    p.batched = ctx->tune.embed_batched & 1;
    p.out = out;
    // a run of lines per group: enough groups to fill the chip (16 waves x 4 groups per CU), runs long enough that ragged
    // lines average out inside a run (a group with 100 lines of 0..32 tokens ends within ~5 % of its neighbours)
    const uint64_t want_groups = (uint64_t)std::max(ctx->num_cus, 1) * 64;
    p.lines_per_group = std::max<uint64_t>(1, (n_lines + want_groups - 1) / want_groups);
    uint64_t groups = (n_lines + p.lines_per_group - 1) / p.lines_per_group;
    p.run_start = nullptr;
    p.n_groups = 0;
    // more than one line per group: the runs are cut by work, not by line count (embed_runs_kernel; tuning key embed_batched bit 3
    // turns it off for A/B)
    const bool balanced = p.lines_per_group > 1 && !(ctx->tune.embed_batched & 8);
    if (balanced) {
        groups = want_groups;
        if (ctx->embed_runs_cap < groups + 1) {
            SMT_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            if (ctx->d_embed_runs) SMT_HIP_CHECK(hipFree(ctx->d_embed_runs));
            ctx->d_embed_runs = nullptr;
            ctx->embed_runs_cap = 0;
            SMT_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&ctx->d_embed_runs), (groups + 1) * sizeof(uint64_t)));
            ctx->embed_runs_cap = groups + 1;
        }
        p.run_start = ctx->d_embed_runs;
        p.n_groups = groups;
    }
    const uint64_t blocks = (groups + 15) / 16;    // 256 threads = 16 groups
    SMT_REQUIRE(blocks < (1ull << 24), "too many lines for one embed launch");
    prof_begin(ctx, "embed");
    if (balanced)
        hipLaunchKernelGGL(embed_runs_kernel, dim3((unsigned)((groups + 1 + 255) / 256)), dim3(256), 0, ctx->stream, offsets, n_lines, groups,
                           ctx->d_embed_runs);
    // embed_batched bit 2 (tests): the PF kernel leaves every run of 64 tokens or more to the generic kernel
    p.span_limit = (ctx->tune.embed_batched & 4) ? 64ull : EMBED_SPAN_LIMIT;
    if (table_dtype == SMT_TABLE_F16) launch_embed_typed<_Float16>(ctx, p, tok, (unsigned)blocks, n_tokens_known);
    else if (table_dtype == SMT_TABLE_I8) launch_embed_typed<signed char>(ctx, p, tok, (unsigned)blocks, n_tokens_known);
    else launch_embed_typed<float>(ctx, p, tok, (unsigned)blocks, n_tokens_known);
    prof_end(ctx, "embed");
    SMT_HIP_CHECK(hipGetLastError());
    return SMT_OK;
}

}  // namespace smt
