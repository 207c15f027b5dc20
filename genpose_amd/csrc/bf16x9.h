// Exact-product split-bf16 ("bf16x9") arithmetic for the BF16 matrix pipe: an fp32 value is the sum of three bf16 terms,
//     x = hi + mid + lo,   hi = bf16(x),  mid = bf16(x - hi),  lo = bf16((x - hi) - mid)     (round to nearest even at every stage)
// which is exact for a normal fp32 x: 24 significand bits = 8 + 8 + 8, and both differences are exact in fp32 (each drops the leading
// eight bits of a value that has at most 24).  A product a_i . b_j of two bf16 terms has at most 16 significand bits, so it is exact in
// fp32; v_mfma_f32_16x16x32_bf16 forms all of them exactly and only its fp32 accumulation rounds - the error class of the fp32 MFMA path,
// at 16 / 9 of its work rate (the BF16 pipe runs at 16x the fp32 one).  Unlike bf16x3.h (three of the nine products, hi / lo pairs),
// nothing is dropped in the score trunks that pin fp32 bits (trunk_bf16x9.h's nine-product kernels, rk45.hip, heun_solve.hip): they form
// all nine (NPROD = 9, the default).
// Fewer products - the split is the same nine-term one and each product formed is exact; with |mid| <= 2^-8 |x| and |lo| <= 2^-16 |x|:
//   NPROD = 8  lo.lo is not issued: at most 2^-32 |a b| per multiply - 1 / 256 of an fp32 unit roundoff (2^-24) of that product.
//   NPROD = 6  lo.lo, lo.mid and mid.lo are not issued (the encoder kernels sa_bf16x9.hip, sa_lds_bf16x9.hip, sa_groupall_bf16x9.hip as
//              the project builds them, and the PC step's six-product kernels of trunk_bf16x9.hip): lo.mid and mid.lo are each at most
//              2^-24 |a b|, so the three together are at most (2^-23 + 2^-32) |a b| per multiply - K 2^-23 max|a||b| over a reduction
//              with all signs equal.  The classical bound on the fp32 accumulation's own rounding, K 2^-24 sum |a_i b_i| <= K^2 2^-24
//              max|a||b|, is K / 2 times that; on random data what is dropped is a random walk of steps ~2^-24 |a b|, two orders of
//              magnitude below the accumulated rounding (tests/test_x6_products_host.py: against float64 six products stay within
//              1.1x of nine, and FIVE - lo.hi dropped as well - are ten times worse: six is the boundary).  6 / 9 of the matrix-pipe
//              cycles.
#pragma once
#include <type_traits>

#include "bf16_split_common.h"

// Products per multiply in the encoder kernels: 9, 8 or 6.  A build-time choice only.  The project's build (build.py) passes
// -DGP_SA_X9_PRODUCTS=6; a translation unit compiled without the flag gets the eight-product kernels, and -DGP_SA_X9_PRODUCTS=8 / =9
// rebuild the earlier instruction streams for measurements against them.  (The score trunks name their count per kernel.)
#ifndef GP_SA_X9_PRODUCTS
#define GP_SA_X9_PRODUCTS 8
#endif

namespace gp_bf16x9 {

constexpr int SA_NPROD = GP_SA_X9_PRODUCTS;

// the three terms of eight values: t[0] = hi, t[1] = mid, t[2] = lo
struct Split8 {
    bf16x8 t[3];
};

// Values i and i + 1 (i even) of split8's eight: their hi / mid / lo terms into s.  Three v_cvt_pk_bf16_f32, two widenings back to fp32
// (shifts), four subtractions - all exact but the conversions.  On its own it is the PIECE of a split that a caller issues beside MFMAs
// (trunk_bf16x9.h: about eleven instructions).
__device__ __forceinline__ void split8_pair(Split8 &s, const int i, const float x0, const float x1) {
    const bf16x2 h = __builtin_convertvector(f32x2{x0, x1}, bf16x2);
    const f32x2 hf = __builtin_convertvector(h, f32x2);
    const float r0 = x0 - hf.x, r1 = x1 - hf.y;  // exact
    const bf16x2 m = __builtin_convertvector(f32x2{r0, r1}, bf16x2);
    const f32x2 mf = __builtin_convertvector(m, f32x2);
    const bf16x2 l = __builtin_convertvector(f32x2{r0 - mf.x, r1 - mf.y}, bf16x2);  // r - mid is exact and has <= 8 bits: l == r - mid
    s.t[0][i] = h.x, s.t[0][i + 1] = h.y;
    s.t[1][i] = m.x, s.t[1][i + 1] = m.y;
    s.t[2][i] = l.x, s.t[2][i + 1] = l.y;
}

// (a, b) = eight fp32 values of a lane (two D fragments: chunks 2m and 2m+1) -> the lane's eight k-values of k-block m as hi / mid / lo.
__device__ __forceinline__ Split8 split8(const f32x4 a, const f32x4 b) {
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    Split8 s;
#pragma unroll
    for (int i = 0; i < 8; i += 2) split8_pair(s, i, x[i], x[i + 1]);
    return s;
}

// acc[p] += W . X[p] for NT B tiles sharing one A operand W = (hi, mid, lo): the nine exact products of each tile, SMALLEST TERMS FIRST
// (lo.lo; lo.mid, mid.lo; lo.hi, mid.mid, hi.lo; mid.hi, hi.mid; hi.hi), so the small terms meet the accumulator before the large
// ones; the tiles are interleaved product by product (independent accumulation chains for the pipe).
// NPROD = 8: the first of them, lo.lo (q == 0, at most 2^-32 |a b| per multiply: see the top of the file), is not issued; the other eight
// in the same order.  NPROD = 6: neither are lo.mid and mid.lo (q == 1, 2); the other six in the same order - lo.hi, mid.mid, hi.lo,
// mid.hi, hi.mid, hi.hi.
// TRANSPOSED: acc[p] += X[p] . W, the activations as the A operand - the same products in the same order.
// `first`: acc[p] = W . X[p] - the first product issued starts from a literal-zero C operand (the bits of 0 + product), no zeroed
// registers.
template <int NT, bool TRANSPOSED = false, int NPROD = 9>
__device__ __forceinline__ void mma9(const bf16x8 (&w)[3], const Split8 (&x)[NT], f32x4 (&acc)[NT], bool first = false) {
    static_assert(NPROD == 9 || NPROD == 8 || NPROD == 6, "all nine products, all but lo.lo, or all but lo.lo, lo.mid and mid.lo");
    constexpr int WA[9] = {2, 2, 1, 2, 1, 0, 1, 0, 0};  // term of W
    constexpr int XB[9] = {2, 1, 2, 0, 1, 2, 0, 1, 0};  // term of X
    constexpr int Q0 = 9 - NPROD;                       // the first product issued
#pragma unroll
    for (int q = Q0; q < 9; ++q)
#pragma unroll
        for (int p = 0; p < NT; ++p) {
            const f32x4 c = first && q == Q0 ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[p];
            if constexpr (TRANSPOSED) acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[p].t[XB[q]], w[WA[q]], c, 0, 0, 0);
            else acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[WA[q]], x[p].t[XB[q]], c, 0, 0, 0);
        }
}

// End of a ring step: this wave's LDS writes of the step have completed (lgkmcnt), then the bare barrier.  No vmcnt wait: the slice in
// flight to the registers may stay in flight across it.  The empty asm statements keep LDS accesses on their side.
__device__ __forceinline__ void ring_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// no side work beside a ring step's MFMAs
struct RingNoSide {
    __device__ __forceinline__ void operator()(int) const {}
};

// One step of the two-slot LDS ring every bf16x9 kernel streams its weights through (slice = chunks x (hi, mid, lo) x 64 lanes of
// bf16x8; NTH threads, PER_T slice elements per thread), over the slice in `slot`: for chunk n < NCH of the slice (output chunk N0 + n
// of acc), the three weight terms (read one chunk ahead) x the two row tiles' split k-block = 2 NPROD MFMAs; beside chunk n < PER_T, element
// n of the next slice goes from the registers (`hold`, requested a step ago) to the other slot `dst` (last read one step ago) and
// element n of the slice after it, `src`, is requested; one barrier.  The caller keeps the ring's position and names the three slices.
// `first`: the step opens its accumulators (acc = W . X, mma9).
// `side(n)`: the caller's piece of other work for chunk n - values that are already final (the split of the NEXT k-block, an epilogue of
// chunks < n of a layer's last step); it must not touch acc[.][N0 + n].  With a side, the chunk's 2 NPROD MFMAs take at most two other
// instructions behind each (ring_half_step's placement), so the piece goes BETWEEN them; without one the region is left to the scheduler
// as before (sa_bf16x9.hip's kernels: several waves per SIMD fill each other's bursts).
// OTHERS: how many other instructions a side's placement takes behind each MFMA - two; a six-product caller whose side pieces were cut
// for 18 MFMAs asks for three (12 x 3 = 18 x 2 places per chunk).
template <int NTH, int PER_T, bool TRANSPOSED, int N0, int NCH, int NPROD = 9, int OTHERS = 2, int NA, class Side = RingNoSide>
__device__ __forceinline__ void ring_step(const bf16x8 *slot, bf16x8 *dst, const bf16x8 *src, bf16x8 (&hold)[PER_T], const Split8 (&xs)[2],
                                          f32x4 (&acc)[2][NA], int tid, int lane, bool first = false, Side side = Side()) {
    static_assert(NCH >= PER_T && N0 + NCH <= NA, "every slice element moves beside a chunk");
    constexpr bool SIDE = !std::is_same<Side, RingNoSide>::value;
    bf16x8 wf[2][3];
#pragma unroll
    for (int t = 0; t < 3; ++t) wf[0][t] = slot[t * 64 + lane];
#pragma unroll
    for (int n = 0; n < NCH; ++n) {
        if (n + 1 < NCH) {
#pragma unroll
            for (int t = 0; t < 3; ++t) wf[(n + 1) & 1][t] = slot[((n + 1) * 3 + t) * 64 + lane];
        }
        if (n < PER_T) {
            dst[tid + n * NTH] = hold[n];
            hold[n] = src[tid + n * NTH];
        }
        if constexpr (SIDE) side(n);
        f32x4 an[2] = {acc[0][N0 + n], acc[1][N0 + n]};
        mma9<2, TRANSPOSED, NPROD>(wf[n & 1], xs, an, first);
        acc[0][N0 + n] = an[0], acc[1][N0 + n] = an[1];
        if constexpr (SIDE) {
#pragma unroll
            for (int i = 0; i < 2 * NPROD; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
                __builtin_amdgcn_sched_group_barrier(0x096, OTHERS, 0);  // VALU | SALU | VMEM | DS
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // one chunk per region: the optimiser would hoist every fragment read of the step
    }
    ring_barrier();
}

// Half a step of the same ring over a CHUNK-MAJOR slice = (two output chunks) x (KB k-blocks) x (hi, mid, lo): chunk C of the slice in
// `slot` against the KB split k-blocks of the whole input, acc[p] = sum over kb ascending of W[C][kb] . X[kb][p] - each accumulator takes
// its k-blocks in the order of the k-major step, from a literal zero.  Sub-block u = C KB + kb: the weight terms of u + 1 are read, element
// u < PER_T of the next slice moves and the slice after it is requested as in ring_step, and `side(kb)` is the caller's piece of other
// work for this sub-block (an epilogue of accumulators that are already final); the sub-block's 2 NPROD MFMAs take at most two other
// instructions behind each, so what side() adds goes BETWEEN them (trunk_chain.h's placement: one wave per SIMD, nothing else fills a
// burst).  Chunk 0 reads chunk 1's first weight terms ahead into `w1`; the barrier follows chunk 1.  OTHERS: as in ring_step.
template <int NTH, int PER_T, int KB, int C, int NPROD = 9, int OTHERS = 2, class Side>
__device__ __forceinline__ void ring_half_step(const bf16x8 *slot, bf16x8 *dst, const bf16x8 *src, bf16x8 (&hold)[PER_T], bf16x8 (&w1)[3],
                                               const Split8 (&xs)[KB][2], f32x4 (&acc)[2], int tid, int lane, Side side) {
    static_assert(C == 0 || C == 1, "two chunks per slice");
    bf16x8 wf[2][3];
#pragma unroll
    for (int t = 0; t < 3; ++t) wf[0][t] = C == 0 ? slot[t * 64 + lane] : w1[t];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        const int u = C * KB + kb;
        if (kb + 1 < KB) {
#pragma unroll
            for (int t = 0; t < 3; ++t) wf[(kb + 1) & 1][t] = slot[((u + 1) * 3 + t) * 64 + lane];
        } else if (C == 0) {
#pragma unroll
            for (int t = 0; t < 3; ++t) w1[t] = slot[((u + 1) * 3 + t) * 64 + lane];
        }
        if (u < PER_T) {
            dst[tid + u * NTH] = hold[u];
            hold[u] = src[tid + u * NTH];
        }
        side(kb);
        mma9<2, false, NPROD>(wf[kb & 1], xs[kb], acc, kb == 0);
#pragma unroll
        for (int i = 0; i < 2 * NPROD; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
            __builtin_amdgcn_sched_group_barrier(0x096, OTHERS, 0);  // VALU | SALU | VMEM | DS
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (C == 1) ring_barrier();
}

}  // namespace gp_bf16x9
