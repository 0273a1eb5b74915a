// device_utils.h -- wave64 / DPP helpers shared by the gfx950 kernels.
#pragma once
#include "common.h"

namespace smt {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ DPP helpers
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v)
{
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ float readlane_f(float v, int lane)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

constexpr int DPP_XOR1 = 0xB1;         // quad_perm [1,0,3,2]
constexpr int DPP_XOR2 = 0x4E;         // quad_perm [2,3,0,1]
constexpr int DPP_HALF_MIRROR = 0x141; // lane i <-> 7-i within 8
constexpr int DPP_MIRROR = 0x140;      // lane i <-> 15-i within 16
constexpr int DPP_WAVE_SHR1 = 0x138;   // lane i <- lane i-1 across the wave

// Sum over the 64 lanes, result in every lane.  Fixed tree => deterministic.
__device__ __forceinline__ float wave_sum(float v)
{
    v += dpp_f<DPP_XOR1>(v);
    v += dpp_f<DPP_XOR2>(v);
    v += dpp_f<DPP_HALF_MIRROR>(v);
    v += dpp_f<DPP_MIRROR>(v);
    const float s0 = readlane_f(v, 0), s1 = readlane_f(v, 16);
    const float s2 = readlane_f(v, 32), s3 = readlane_f(v, 48);
    return (s0 + s1) + (s2 + s3);
}

// FOUR sums over the 64 lanes at once: lane l of the result holds the sum over all lanes of the input with index l % 4 (a, b, c, d).
// A transposing tree: the xor-1 and xor-2 steps halve the number of live values instead of repeating each step per value, rotations
// by 4 and 8 finish the 16-lane rows, v_permlane16_swap / v_permlane32_swap (gfx950) add the rows -- 15 VALU instructions for four
// sums against 4 x 11 of wave_sum (whose four v_readlane + scalar adds per value are most of its cost).  Fixed tree => deterministic.
constexpr int DPP_ROW_ROR4 = 0x124, DPP_ROW_ROR8 = 0x128;   // lane i of a row <- lane (i - n) mod 16
// (v_permlane{16,32}_swap_b32 through inline asm: __builtin_amdgcn_permlane*_swap of clang 22 / ROCm 7.2 hands back its FIRST result
// for both elements -- the generated code added v + v -- so the builtin cannot give "lane + partner".  The two wait states a VALU
// write needs before the swap reads the register are in the asm, the assembler adds none for inline code.
// tools/micro/wave_sum4.hip is the on-device test of what comes out.)
__device__ __forceinline__ float add_lane_xor32(float v)
{
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32_e32 %0, %1" : "+v"(a), "+v"(b));   // a = {lo, lo}, b = {hi, hi}
    return a + b;
}
__device__ __forceinline__ float add_lane_xor16(float v)
{
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32_e32 %0, %1" : "+v"(a), "+v"(b));   // a = rows {0, 0, 2, 2}, b = rows {1, 1, 3, 3}
    return a + b;
}
__device__ __forceinline__ float wave_sum4(float a, float b, float c, float d, int lane)
{
    const bool odd = lane & 1, upper = lane & 2;
    // xor 1: even lanes keep a (c), odd lanes keep b (d), each adds its neighbour's share of the value it keeps
    const float ab = (odd ? b : a) + dpp_f<DPP_XOR1>(odd ? a : b);
    const float cd = (odd ? d : c) + dpp_f<DPP_XOR1>(odd ? c : d);
    // xor 2: lanes 0, 1 of a quad keep a | b, lanes 2, 3 keep c | d
    float v = (upper ? cd : ab) + dpp_f<DPP_XOR2>(upper ? ab : cd);
    v += dpp_f<DPP_ROW_ROR4>(v);
    v += dpp_f<DPP_ROW_ROR8>(v);
    v = add_lane_xor16(v);
    return add_lane_xor32(v);
}

// T wave_sum4 trees at once: out[t] is bit for bit wave_sum4(in[t][0], in[t][1], in[t][2], in[t][3], lane) -- every tree performs the
// same operations in the same order -- with the trees' instructions interleaved level by level, so that each DPP step of one tree
// stands in the wait states of the others', and ONE s_nop in front of each level's permlane swaps covers all T of them.
template <int T>
__device__ __forceinline__ void swap_lanes_xor16(float (&a)[T], float (&b)[T]);
template <int T>
__device__ __forceinline__ void swap_lanes_xor32(float (&a)[T], float (&b)[T]);
template <>
__device__ __forceinline__ void swap_lanes_xor16<2>(float (&a)[2], float (&b)[2])
{
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32_e32 %0, %1\n\tv_permlane16_swap_b32_e32 %2, %3"
                 : "+v"(a[0]), "+v"(b[0]), "+v"(a[1]), "+v"(b[1]));
}
template <>
__device__ __forceinline__ void swap_lanes_xor32<2>(float (&a)[2], float (&b)[2])
{
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32_e32 %0, %1\n\tv_permlane32_swap_b32_e32 %2, %3"
                 : "+v"(a[0]), "+v"(b[0]), "+v"(a[1]), "+v"(b[1]));
}
template <>
__device__ __forceinline__ void swap_lanes_xor16<3>(float (&a)[3], float (&b)[3])
{
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32_e32 %0, %1\n\tv_permlane16_swap_b32_e32 %2, %3\n\tv_permlane16_swap_b32_e32 %4, %5"
                 : "+v"(a[0]), "+v"(b[0]), "+v"(a[1]), "+v"(b[1]), "+v"(a[2]), "+v"(b[2]));
}
template <>
__device__ __forceinline__ void swap_lanes_xor32<3>(float (&a)[3], float (&b)[3])
{
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32_e32 %0, %1\n\tv_permlane32_swap_b32_e32 %2, %3\n\tv_permlane32_swap_b32_e32 %4, %5"
                 : "+v"(a[0]), "+v"(b[0]), "+v"(a[1]), "+v"(b[1]), "+v"(a[2]), "+v"(b[2]));
}
// (in two halves, so that a caller short of registers can place work between them: the head leaves ONE live value per tree)
template <int T>
__device__ __forceinline__ void wave_sum4_multi_head(const float (&in)[T][4], float (&v)[T], int lane)
{
    const bool odd = lane & 1, upper = lane & 2;
    float ab[T], cd[T];
#pragma unroll
    for (int t = 0; t < T; ++t) ab[t] = (odd ? in[t][1] : in[t][0]) + dpp_f<DPP_XOR1>(odd ? in[t][0] : in[t][1]);
#pragma unroll
    for (int t = 0; t < T; ++t) cd[t] = (odd ? in[t][3] : in[t][2]) + dpp_f<DPP_XOR1>(odd ? in[t][2] : in[t][3]);
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = (upper ? cd[t] : ab[t]) + dpp_f<DPP_XOR2>(upper ? ab[t] : cd[t]);
}
// The same heads without their selects (scan_deep_kernel).  What a lane keeps and what it sends at the xor-1 and xor-2 steps is
// decided by the lane alone, m = lane & 3, not by the tree: so the caller permutes the chunk's four ROWS by lane once
// (swizzle_rows4: register k holds row k ^ m) and every tree's products come out in the registers the steps want --
// in[t][k] = the partial of row k ^ m in this lane, p_{k ^ m}[m] -- whatever the number of trees behind the one permutation:
//   ab = in[0] + xor1(in[1])   lane m: p_m[m] + p_m[m ^ 1]                  (kept + received)
//   cd = in[2] + xor1(in[3])   lane m: p_{m ^ 2}[m] + p_{m ^ 2}[m ^ 1]
//   v  = ab + xor2(cd)         lane m: ab + (p_m[m ^ 2] + p_m[m ^ 3])       (kept + received)
// the additions of wave_sum4_multi_head, same operands, same order: v[t] is bit for bit what that head leaves.
// (tools/micro/wave_sum4_swizzled.hip is the on-device test.)
template <int T>
__device__ __forceinline__ void wave_sum4_swizzled_head(const float (&in)[T][4], float (&v)[T])
{
    float ab[T], cd[T];
#pragma unroll
    for (int t = 0; t < T; ++t) ab[t] = in[t][0] + dpp_f<DPP_XOR1>(in[t][1]);
#pragma unroll
    for (int t = 0; t < T; ++t) cd[t] = in[t][2] + dpp_f<DPP_XOR1>(in[t][3]);
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] = ab[t] + dpp_f<DPP_XOR2>(cd[t]);
}
// swizzle_rows4: c_k <- c_{k ^ (lane & 3)}, in place: odd lanes exchange (c0, c1) and (c2, c3), then the lanes with bit 1 set
// exchange (c0, c2) and (c1, c3) -- 32 selects on the sixteen row registers, once per chunk, for the six selects per tree that the
// heads no longer have.  The caller must let the permuted rows END behind their last use (an empty asm that defines the buffer
// anew): rows that stay live into the next turn of a loop are copied about, and the copies do not fit the deep kernel's 64 VGPRs.
// (Tried and not kept: the same exchanges as sixteen v_swap_b32 under two exec masks.  Fewer instructions, but a slower pass --
// profiles/scan_deep_heads.json.)
__device__ __forceinline__ void swizzle_rows4(f32x4 &c0, f32x4 &c1, f32x4 &c2, f32x4 &c3, int lane)
{
    const bool odd = lane & 1, upper = lane & 2;
    f32x4 t;
    t = odd ? c1 : c0; c1 = odd ? c0 : c1; c0 = t;
    t = odd ? c3 : c2; c3 = odd ? c2 : c3; c2 = t;
    t = upper ? c2 : c0; c2 = upper ? c0 : c2; c0 = t;
    t = upper ? c3 : c1; c3 = upper ? c1 : c3; c1 = t;
}
template <int T>
__device__ __forceinline__ void wave_sum4_multi_tail(float (&v)[T], float (&out)[T])
{
    float w[T];
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] += dpp_f<DPP_ROW_ROR4>(v[t]);
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] += dpp_f<DPP_ROW_ROR8>(v[t]);
#pragma unroll
    for (int t = 0; t < T; ++t) w[t] = v[t];
    swap_lanes_xor16<T>(v, w);   // v = rows {0, 0, 2, 2}, w = rows {1, 1, 3, 3}
#pragma unroll
    for (int t = 0; t < T; ++t) { v[t] = v[t] + w[t]; w[t] = v[t]; }
    swap_lanes_xor32<T>(v, w);   // v = {lo, lo}, w = {hi, hi}
#pragma unroll
    for (int t = 0; t < T; ++t) out[t] = v[t] + w[t];
}
template <int T>
__device__ __forceinline__ void wave_sum4_multi(const float (&in)[T][4], float (&out)[T], int lane)
{
    float v[T];
    wave_sum4_multi_head<T>(in, v, lane);
    wave_sum4_multi_tail<T>(v, out);
}

// The trees of a GROUP (scan_pair_kernel): <c, c> and four query trees whose totals are wanted in ONE row of the wave each -- tree g
// in row g, where lane 16 g + j tests row j of the chunk against query g -- so the four query trees share one tail.
// wave_sum4_rows: the rotations by 4 and 8 of wave_sum4 on T trees, interleaved; every lane then holds its 16-lane row's sum r_R.
template <int T>
__device__ __forceinline__ void wave_sum4_rows(float (&v)[T])
{
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] += dpp_f<DPP_ROW_ROR4>(v[t]);
#pragma unroll
    for (int t = 0; t < T; ++t) v[t] += dpp_f<DPP_ROW_ROR8>(v[t]);
}
// wave_sum4_group_tail: cc and t0 .. t3 come from wave_sum4_rows.  v_permlane16_swap(t0, t1) and one add leave
// t0.(r0 + r1) | t1.(r0 + r1) | t0.(r2 + r3) | t1.(r2 + r3) in the four rows, the same with (t2, t3); v_permlane32_swap of the two
// results and one add leave tree g's (r0 + r1) + (r2 + r3) in row g: the additions of wave_sum4's tail, same operands, same order,
// six instructions for the four trees and no copy.  cc keeps the replicating tail (every row needs <c, c>).  Returns: cc = what
// wave_sum4 leaves, in every lane; t0 = in row g what wave_sum4 leaves for tree g.  t1 .. t3 are used up.  A tree that does not
// exist (a group of fewer than four calls) may be any register: its row holds a sum nobody reads, the other rows never see it.
// (One block of assembly so that the order is the one written: a swap may read a register two wait states after a VALU write at
// the earliest, and the independent instructions of the other trees stand in those states -- two s_nop 0 are left.)
__device__ __forceinline__ void wave_sum4_group_tail(float &cc, float &t0, float &t1, float &t2, float &t3)
{
    float w;
    asm volatile("v_mov_b32 %5, %0\n\t"
                 "s_nop 0\n\t"
                 "v_permlane16_swap_b32_e32 %1, %2\n\t"
                 "v_permlane16_swap_b32_e32 %3, %4\n\t"
                 "v_permlane16_swap_b32_e32 %0, %5\n\t"
                 "v_add_f32 %1, %1, %2\n\t"
                 "v_add_f32 %3, %3, %4\n\t"
                 "v_add_f32 %0, %0, %5\n\t"
                 "v_mov_b32 %5, %0\n\t"
                 "v_permlane32_swap_b32_e32 %1, %3\n\t"
                 "s_nop 0\n\t"
                 "v_permlane32_swap_b32_e32 %0, %5\n\t"
                 "v_add_f32 %1, %1, %3\n\t"
                 "v_add_f32 %0, %0, %5"
                 : "+v"(cc), "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3), "=&v"(w));
}

// The same tail for four query trees whose <c, c> is already known (scan_wide_kernel's second four queries of a chunk): the
// additions of wave_sum4_group_tail on t0 .. t3, same operands, same order, without the cc column.  t0 = in row g what wave_sum4
// leaves for tree g; t1 .. t3 are used up.  (The callers' last VALU writes stand directly in front: two wait states before the
// first swaps, and two between the adds and the swap that reads them.)
__device__ __forceinline__ void wave_sum4_group_tail_queries(float &t0, float &t1, float &t2, float &t3)
{
    asm volatile("s_nop 1\n\t"
                 "v_permlane16_swap_b32_e32 %0, %1\n\t"
                 "v_permlane16_swap_b32_e32 %2, %3\n\t"
                 "v_add_f32 %0, %0, %1\n\t"
                 "v_add_f32 %2, %2, %3\n\t"
                 "s_nop 1\n\t"
                 "v_permlane32_swap_b32_e32 %0, %2\n\t"
                 "v_add_f32 %0, %0, %2"
                 : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3));
}

// ONE REGISTER FOR THE 64 (ROW, QUERY) PAIRS OF A CHUNK (scan_deep_kernel).  The group tails above deliver a chunk's sums sixteen at a
// time, in quad 0 of each 16-lane row; the rotations by 4 and 8 in front of them replicate one value over a row.  Here the QUERIES are
// permuted by lane as well, where their LDS images are written (once per pass), so that the steps at distance 4 and 8 FOLD four query
// trees into one register, and the four phases' registers go through one tail.  For lane l, with R = l >> 4 the 16-lane row,
// i = (l >> 2) & 3 the quad and j = l & 3:
//   row of the chunk   m(l) = j ^ ((i & 1) ? 3 : 0)   odd quads hold the rows in reverse; register k of the row buffer holds row
//                      k ^ m(l) (swizzle_rows4_folded).  m(l ^ 1) = m(l) ^ 1 and m(l ^ 2) = m(l) ^ 2 inside a quad, so the heads
//                      (wave_sum4_swizzled_head) stay what they are: v = the quad's sum of row m(l).
//   query              slot s (0 .. 3) of phase h holds query 4 h + (s ^ i'), i' = (4 - i) & 3 (wave_sum4_folded_slot)
//   w0 = v[0] + row_mirror(v[1])   the lane 15 - p of the row is quad 3 - i, and its reversed rows put row m(l) there: same row,
//   w1 = v[2] + row_mirror(v[3])   and 1 ^ i'(3 - i) = i'(i), 3 ^ i'(3 - i) = 2 ^ i'(i): same query.  q_i + q_{3 - i}.
//   x  = w0 + row_ror8(w1)         quad i ^ 2, same j, same row; 2 ^ i'(i ^ 2) = i'(i): same query.
// Quad i then holds (q_i + q_{3-i}) + (q_{i^2} + q_{3-(i^2)}) of row m(l) against query 4 h + i'.  wave_sum4 computes
// (q_0 + q_3) + (q_2 + q_1) at quad 0, the lanes the kernels read: in every quad the new value is that sum with operands exchanged,
// and IEEE addition is commutative bit for bit.  The swaps of the tail move lane p of a row to lane p of another, so a lane keeps
// its (row, query); after the tail of x_0 .. x_3 lane l holds what wave_sum4 leaves for <row m(l), query 4 R + i'>: 64 pairs, each
// once.  3 adds per four trees where wave_sum4_rows has 8, one tail where the phases had four.
// (tools/micro/wave_sum4_folded.hip is the on-device test.)
__device__ __forceinline__ int wave_sum4_folded_row(int lane) { return (lane & 3) ^ ((lane & 4) ? 3 : 0); }
__device__ __forceinline__ int wave_sum4_folded_query(int lane) { return 4 * (lane >> 4) + ((4 - ((lane >> 2) & 3)) & 3); }   // (of the 16)
__device__ __forceinline__ int wave_sum4_folded_slot(int n, int lane) { return (n & ~3) | ((n & 3) ^ ((4 - ((lane >> 2) & 3)) & 3)); }   // where lane keeps query n's 16 bytes
// swizzle_rows4 with the masks of m(l): c_k <- c_{k ^ m(l)}, in place, the same 32 selects (and the same rule for the caller)
__device__ __forceinline__ void swizzle_rows4_folded(f32x4 &c0, f32x4 &c1, f32x4 &c2, f32x4 &c3, int lane)
{
    const int m = wave_sum4_folded_row(lane);
    const bool odd = m & 1, upper = m & 2;
    f32x4 t;
    t = odd ? c1 : c0; c1 = odd ? c0 : c1; c0 = t;
    t = odd ? c3 : c2; c3 = odd ? c2 : c3; c2 = t;
    t = upper ? c2 : c0; c2 = upper ? c0 : c2; c0 = t;
    t = upper ? c3 : c1; c3 = upper ? c1 : c3; c1 = t;
}
// the folding row steps: wave_sum4_fold_mirror(v[0], v[1]) = w0, (v[2], v[3]) = w1, wave_sum4_fold_ror8(w0, w1) = x
__device__ __forceinline__ float wave_sum4_fold_mirror(float keep, float send) { return keep + dpp_f<DPP_MIRROR>(send); }
__device__ __forceinline__ float wave_sum4_fold_ror8(float keep, float send) { return keep + dpp_f<DPP_ROW_ROR8>(send); }
// the <c, c> column's row steps: nothing to fold, but the same two distances, so that EVERY lane of the row ends with the canonical
// (q_0 + q_3) + (q_2 + q_1) of its own row m(l) up to exchanged operands (behind ror4 and ror8 only quad 0 has it)
__device__ __forceinline__ float wave_sum4_fold_cc_rows(float v)
{
    v += dpp_f<DPP_MIRROR>(v);
    v += dpp_f<DPP_ROW_ROR8>(v);
    return v;
}
// The tail in three parts, so that a caller short of registers folds as the phases come: (x_0, x_1) as soon as phase 1 is done, then
// (x_2, x_3), then the two results -- the additions of wave_sum4_group_tail_queries, same operands, same order.  The first and the
// last part take the <c, c> column along (the replicating tail of wave_sum4_group_tail).  t0 holds the result, t1 is used up; a
// tree that does not exist may be any register.  (Wait states as in wave_sum4_group_tail: two between a VALU write and the swap.)
__device__ __forceinline__ void wave_sum4_fold_tail16_cc(float &cc, float &t0, float &t1)
{
    float w;
    asm volatile("v_mov_b32 %3, %0\n\t"
                 "s_nop 0\n\t"
                 "v_permlane16_swap_b32_e32 %1, %2\n\t"
                 "v_permlane16_swap_b32_e32 %0, %3\n\t"
                 "v_add_f32 %1, %1, %2\n\t"
                 "v_add_f32 %0, %0, %3"
                 : "+v"(cc), "+v"(t0), "+v"(t1), "=&v"(w));
}
__device__ __forceinline__ void wave_sum4_fold_tail16(float &t0, float &t1)
{
    asm volatile("s_nop 1\n\t"
                 "v_permlane16_swap_b32_e32 %0, %1\n\t"
                 "v_add_f32 %0, %0, %1"
                 : "+v"(t0), "+v"(t1));
}
__device__ __forceinline__ void wave_sum4_fold_tail32_cc(float &cc, float &t0, float &t1)
{
    float w;
    asm volatile("v_mov_b32 %3, %0\n\t"
                 "s_nop 0\n\t"
                 "v_permlane32_swap_b32_e32 %1, %2\n\t"
                 "v_permlane32_swap_b32_e32 %0, %3\n\t"
                 "v_add_f32 %1, %1, %2\n\t"
                 "v_add_f32 %0, %0, %3"
                 : "+v"(cc), "+v"(t0), "+v"(t1), "=&v"(w));
}

// Integer sum over the 64 lanes, result in every lane.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    v += dpp_u<DPP_XOR1>(v);
    v += dpp_u<DPP_XOR2>(v);
    v += dpp_u<DPP_HALF_MIRROR>(v);
    v += dpp_u<DPP_MIRROR>(v);
    const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), s1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t s2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), s3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return (s0 + s1) + (s2 + s3);
}

__device__ __forceinline__ float dist_f32(float ab, float b2, float rq, bool q_zero)
{
    // simsimd rules (oracle/semtools_oracle.c cos_finish): both zero -> 0,
    // ab == 0 -> 1, else max(0, 1 - ab * rsqrt(a2) * rsqrt(b2)).  rq = 0 when
    // the query is the zero vector, so "ab == 0 -> 1" falls out of the formula.
    if (b2 == 0.0f) return q_zero ? 0.0f : 1.0f;
    const float d = 1.0f - ab * rq * __frsqrt_rn(b2);
    return fmaxf(d, 0.0f);
}

// dist_f32 for a row that meets several queries (scan_deep_kernel's four phases): rs_b2 = __frsqrt_rn(b2) and b2_zero = (b2 == 0)
// computed once by the caller, the same expression behind them.
__device__ __forceinline__ float dist_f32_rs(float ab, float rs_b2, bool b2_zero, float rq, bool q_zero)
{
    if (b2_zero) return q_zero ? 0.0f : 1.0f;
    const float d = 1.0f - ab * rq * rs_b2;
    return fmaxf(d, 0.0f);
}

// Read-only data produced by an EARLIER kernel, addressed uniformly: loads go through the scalar cache.
typedef const uint64_t __attribute__((address_space(4))) *const_u64_ptr;

// A value that is the same in every lane, moved to SGPRs (lets address arithmetic and loads go scalar).
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ key_t64 make_key(float d, uint32_t row)
{
    return ((key_t64)__float_as_uint(d) << 32) | (key_t64)row;
}


// --------------------------------------------------- exact f64 distance (A5)
// Bit-for-bit the oracle's orc_cosine_f32_accurate: f64 accumulators, index
// order, then cos_finish.  The product of two f32 values is exact in f64, so
// fma(a, b, acc) rounds exactly like acc + a*b: letting the compiler contract
// to v_fma_f64 cannot change a bit (the oracle is built with contraction off).
// cos_finish of the oracle.  Contraction OFF here: 1 - (ab*ra)*rb must round the
// products before the subtraction exactly as the CPU code does.
__device__ __forceinline__ double cos_finish_exact(double ab, double a2, double b2)
{
#pragma clang fp contract(off)
    if (a2 == 0.0 && b2 == 0.0) return 0.0;
    if (ab == 0.0) return 1.0;
    const double ra = 1.0 / sqrt(a2);
    const double rb = 1.0 / sqrt(b2);
    const double t = ab * ra;
    const double u = t * rb;
    const double unclipped = 1.0 - u;
    return unclipped > 0.0 ? unclipped : 0.0;
}

// ab and b2 chains for one row (index order), a2 supplied by the caller (same for every row).
template <typename QP, typename RP>
__device__ __forceinline__ void exact_sums(QP q4, RP r4, double &ab_out, double &b2_out)
{
    double ab = 0.0, b2 = 0.0;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
        const f32x4 a = q4[i];
        const f32x4 b = r4[i];
        const double ax = a.x, ay = a.y, az = a.z, aw = a.w;
        const double bx = b.x, by = b.y, bz = b.z, bw = b.w;
        ab = ab + ax * bx; b2 = b2 + bx * bx;
        ab = ab + ay * by; b2 = b2 + by * by;
        ab = ab + az * bz; b2 = b2 + bz * bz;
        ab = ab + aw * bw; b2 = b2 + bw * bw;
    }
    ab_out = ab;
    b2_out = b2;
}

template <typename QP>
__device__ __forceinline__ double exact_norm2(QP q4)
{
    double a2 = 0.0;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
        const f32x4 a = q4[i];
        const double ax = a.x, ay = a.y, az = a.z, aw = a.w;
        a2 = a2 + ax * ax; a2 = a2 + ay * ay; a2 = a2 + az * az; a2 = a2 + aw * aw;
    }
    return a2;
}

template <typename QP, typename RP>
__device__ __forceinline__ double exact_distance(QP q4, RP r4)
{
    double ab, b2;
    exact_sums(q4, r4, ab, b2);
    return cos_finish_exact(ab, exact_norm2(q4), b2);
}

// Ascending bitonic sort of n (a power of two) LDS entries, compare-exchange given as a functor on two indices and the
// direction; every thread of the block calls it (topk_large.hip, ivfpq_search.hip)
template <typename CX>
__device__ __forceinline__ void bitonic_sort(uint32_t n, CX cx)
{
    for (uint32_t size = 2; size <= n; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t i = threadIdx.x; i < n / 2; i += blockDim.x) {
                const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                cx(lo, hi, (lo & size) == 0);
            }
            __syncthreads();
        }
}

}  // namespace smt
