// The score trunk as EXACT-PRODUCT split bf16 on the BF16 matrix pipe (bf16x9.h), once for its kernels: the PC step's chain plan, its
// seeded twin and the Heun step (trunk_bf16x9.hip) and the RK45 chain stage (rk45.hip).  4 waves per workgroup (one per SIMD, the whole
// 512-entry register file), each carrying TWO 16-row B tiles = 32 rows, 128 rows per workgroup.  The D fragment of a layer is the next
// layer's B operand.  All weights stream through a 2-slot LDS ring in 33 slices of 48 KB: pose_encoder.0 (1) and pose_encoder.2 (8)
// K-MAJOR (ring_step: one k-block x 16 output chunks; the fp32 input split into hi / mid / lo one k-block at a time, 128 accumulator
// registers), then the three heads (8 each) CHUNK-MAJOR (ring_half_step: two output chunks x all eight k-blocks): pose_encoder.2's output
// is split once into 192 registers that all three heads read, 16 accumulator registers are live, and a chunk's fp32 epilogue is issued
// between the MFMAs of the next chunk.  Every accumulator takes its k-blocks ascending and every head output its chunks ascending in
// both orders: the bits are those of k-major heads (tests/test_gpu_x9_chain_bits.py).
// One wave per SIMD: an instruction that is not placed between MFMAs is exposed.  So the k-major layers' own fp32 work rides beside their
// MFMAs too (ring_step's side hook, at most two other instructions behind each MFMA): pose_encoder.0's bias + ReLU chunk by chunk, the
// split of k-block kb + 1 during step kb, and pose_encoder.2's bias + ReLU + split tail pair by pair during its last step (the last pair
// on the first head chunk) - run<KSIDE>.  Same expressions on the same values, same summation orders: the bits do not move
// (tests/test_gpu_x9_chain_bits.py, tests/test_gpu_x9_chain_bits_more.py).  Still exposed (profiles/x9_kmajor_under_mfma.txt): the
// prologue up to the first MFMA (sampler update, slot 0), the part of the tail that does not fit two-per-MFMA (14 runs of 39-49
// instructions at the chunk ends of pose_encoder.2's last step, 124 before the first head chunk), the head loop's short runs, the last
// head's last chunk.
// run<KSIDE, NPROD>: NPROD = 9 is all of the above; NPROD = 6 (the PC step's six-product kernels, trunk_bf16x9.hip) issues six of the nine
// products of every multiply (bf16x9.h) - 6 336 MFMAs per wave instead of 9 504, the same ring, packs, orders and side pieces, the
// pieces in fewer instructions (DIET in run: one-instruction ReLU, the head outputs as fma chains, LDS addresses as register + immediate).
//   request : slices 0 and 1 into registers - the caller places it among its own loads (memory returns in order)
//   stage_request : the staged fp32 operands (w_out, b0, b2, cvec[cloud] + tvec) into registers, for a caller that has work of its own
//             before run() - issued BEFORE request, they arrive under that work instead of behind the 24 weight loads
//   run     : staged fp32 operands, slot 0, the layers, and once per head and tile, heads ascending, its fp32 Linear(256, 3) outputs
//             handed to the caller's functor (the callers store at once: carrying the nine outputs to the end costs 27-40 more spilled
//             registers, profiles/r9_rk45_bf16x9_resources.txt); heads 0 and 1 hand over beside the next head's first MFMAs
#pragma once
#include <type_traits>

#include "bf16x9.h"

namespace gp_x9trunk {

using namespace gp_split;
using namespace gp_bf16x9;

constexpr int X9_NW = 4, X9_NT = 64 * X9_NW, X9_RT = 2, X9_ROWS = 16 * X9_RT * X9_NW;
using X9Lds = SplitLds<3, 2>;  // 2 slots of 48 KB
constexpr int X9_SLICE = X9Lds::SLICE, X9_PER_T = X9_SLICE / X9_NT;
static_assert(X9_ROWS == 128 && X9_PER_T <= 16, "one slice element per thread and output chunk at most");

// The head epilogue's arithmetic as PLAIN fp32 instructions: beside MFMAs a packed v_pk_add_f32 / v_pk_mul_f32 costs several times its
// scalar form, and the optimiser packs adjacent fp32 adds and multiplies wherever it sees two of them.  Every result passes through an
// (empty, movable) asm statement, which it does not look through.  Values and rounding order are those of the expressions they replace.
__device__ __forceinline__ float plain(float v) {
    asm("" : "+v"(v));
    return v;
}
// relu_plain<BITS>(s) = fmaxf(s, 0) of a pinned sum.  Behind the pin the compiler no longer knows that s is canonical and puts a
// v_max_f32 s, s, s in front of the maximum: two instructions per ReLU.  BITS (the six-product kernels): the maximum of the BITS as
// signed integers, one v_max_i32 - a float with its sign set is a negative integer and gives +0, any other keeps its bits.  For every s
// that is not a NaN that is fmaxf(s, 0) to the bit (a NaN with a clear sign stays a NaN where fmaxf gives 0).
template <bool BITS>
__device__ __forceinline__ float relu_plain(float s) {
    s = plain(s);
    if constexpr (BITS) {
        const int b = __builtin_bit_cast(int, s);
        return __builtin_bit_cast(float, b > 0 ? b : 0);
    } else
        return fmaxf(s, 0.f);
}
template <bool BITS = false>
__device__ __forceinline__ f32x4 relu_sum4(const f32x4 a, const f32x4 b) {  // relu4(a + b)
    return f32x4{relu_plain<BITS>(a.x + b.x), relu_plain<BITS>(a.y + b.y), relu_plain<BITS>(a.z + b.z), relu_plain<BITS>(a.w + b.w)};
}
__device__ __forceinline__ float dot4_plain(const f32x4 v, const f32x4 w) {  // v.x * w.x + v.y * w.y + v.z * w.z + v.w * w.w
    const float m0 = plain(v.x * w.x), m1 = plain(v.y * w.y), m2 = plain(v.z * w.z), m3 = plain(v.w * w.w);
    return plain(plain(plain(m0 + m1) + m2) + m3);
}
// o + v . w as one chain of four fused multiply-adds (the six-product kernels): 4 instructions where dot4_plain and its accumulate take
// 8, the same four products, each added unrounded - and pinned like the rest (the two tiles' chains side by side would be packed)
__device__ __forceinline__ float dot4_fma(const f32x4 v, const f32x4 w, float o) {
    o = plain(__builtin_fmaf(v.x, w.x, o));
    o = plain(__builtin_fmaf(v.y, w.y, o));
    o = plain(__builtin_fmaf(v.z, w.z, o));
    return plain(__builtin_fmaf(v.w, w.w, o));
}
// operands of a head chunk's epilogue in flight between the sub-blocks of the next chunk
struct HeadEpi {
    f32x4 cv[X9_RT], w[3], v[X9_RT];
};

// slice 0 (-> slot 0 in run) and slice 1 (-> registers, written during step 0)
__device__ __forceinline__ void request(const SplitNet &w, int tid, bf16x8 (&first)[X9_PER_T], bf16x8 (&hold)[X9_PER_T]) {
#pragma unroll
    for (int u = 0; u < X9_PER_T; ++u) first[u] = split_slice<3>(w, 0)[tid + u * X9_NT];
#pragma unroll
    for (int u = 0; u < X9_PER_T; ++u) hold[u] = split_slice<3>(w, 1)[tid + u * X9_NT];
}

// xv: the nine pose components of the lane's row in each of its two tiles; row: that row (rows >= nrows are clamped duplicates);
// tvec: the step's / stage's 768 time-embedding outputs.  emit(head, tile, out): out[c] = output 3 head + c of the row, bias included, in
// every lane of the row.
// sg: the staged fp32 operands in registers (stage_request) when the caller asked for them ahead of its own work, nullptr when run() is
// to fetch them itself (split_stage).
using X9Staged = SplitStaged<X9_NT>;
__device__ __forceinline__ void stage_request(X9Staged &sg, const SplitNet &w, const float *cvec, const float *tvec, int wg_row0, int nrows, int kcand) {
    split_stage_request<X9_NT>(sg, w, cvec, tvec, wg_row0, nrows, kcand);
}

// KSIDE: how much of the k-major layers' fp32 work rides beside their MFMAs.  0 (the default; rk45.hip's stage kernels): nothing, the
// plain form - their f64 stage state leaves no room for the second live split (stages 6 and 7 would take 12-36 B more scratch).
// 1 (the Heun step): all but pose_encoder.2's tail - with it that kernel parks 117 values in AGPRs instead of 76 and loses what the
// rest gains.  2 (the PC kernels): all of it.  (profiles/x9_kmajor_under_mfma.txt)
// NPROD: the products per multiply (bf16x9.h), forwarded to both ring functions - 9 (the default: every kernel whose bits are recorded) or
// 6 (the PC step's six-product kernels).  With six, the side pieces above are issued in fewer instructions (DIET, in run) and a chunk's or
// sub-block's 12 MFMAs take two other instructions behind each like nine products' 18: 24 places where the pieces were cut for 36 - three
// behind each, which the kernels had before the pieces shrank, measures 1.8 us per launch slower (profiles/x6_issue_budget.txt).
template <int KSIDE = 0, int NPROD = 9, class Emit, class Staged = std::nullptr_t>
__device__ __forceinline__ void run(float *lds, const SplitNet &w, const float *cvec, const float *tvec, int wg_row0, int nrows, int kcand,
                                    const bf16x8 (&first)[X9_PER_T], bf16x8 (&hold)[X9_PER_T], const float (&xv)[X9_RT][POSE],
                                    const int (&row)[X9_RT], Emit emit, const Staged &sg = nullptr) {
    bf16x8 *ring = reinterpret_cast<bf16x8 *>(lds);
    const float *woutl = lds + X9Lds::OFF_WOUT, *b0l = lds + X9Lds::OFF_B0, *b2l = lds + X9Lds::OFF_B2, *cvtl = lds + X9Lds::OFF_CVT;
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
    // DIET (the six-product kernels; profiles/x6_issue_budget.txt): fewer instructions for the same side work - relu_plain<true>, dot4_fma,
    // and LDS addresses as one register + an immediate.  A ds_read's 16-bit offset does not reach the second ring slot (48 KB up) from the
    // first slot's lane address, nor the staged fp32 operands (from byte 96 K), and the compiler forms each such address with an add of
    // its own or parks it in an AGPR.  lane1 is the lane's element index IN SLOT 1 counted from slot 0, pinned: through (ring, lane1)
    // every fragment of slot 1 is a base register + an immediate, as slot 0's are.  g4 is the lane group's 4 g carried as the pinned
    // sum OFF_WOUT + 4 g: the staged operands' addresses are that register (+ what moves with the head and the cloud) + an immediate.
    constexpr bool DIET = NPROD == 6;
    int lane1 = lane + X9_SLICE, g4 = 4 * g;
    if constexpr (DIET) {
        asm("" : "+v"(lane1));
        g4 += X9Lds::OFF_WOUT;
        asm("" : "+v"(g4));
        g4 -= X9Lds::OFF_WOUT;
    }
    auto slot_of = [&](int gs) { return DIET ? ring : ring + (gs & 1) * X9_SLICE; };
    auto lane_of = [&](int gs) { return DIET && (gs & 1) ? lane1 : lane; };
    // ---- staged epilogue operands and slot 0
    if constexpr (std::is_same<Staged, X9Staged>::value) split_stage_store<X9_NT, X9Lds>(lds, sg);
    else split_stage<X9_NT, X9Lds>(lds, w, cvec, tvec, wg_row0, nrows, kcand);
#pragma unroll
    for (int u = 0; u < X9_PER_T; ++u) ring[tid + u * X9_NT] = first[u];
    __syncthreads();
    int gstep = 0;
    f32x4 acc[X9_RT][16];
    f32x4 act[X9_RT][16];
    if constexpr (KSIDE == 0) {
        // the plain form (the text rk45.hip's resource table was taken with): bias + ReLU between the layers, each k-block split before its step
        auto step = [&](const Split8 (&xs)[X9_RT], bool first) {
            const int gs = gstep++;
            ring_step<X9_NT, X9_PER_T, false, 0, 16, NPROD>(ring + (gs & 1) * X9_SLICE, ring + ((gs + 1) & 1) * X9_SLICE, split_slice<3>(w, gs + 2), hold, xs, acc,
                                                     tid, lane, first);
        };
        auto hidden = [&](const float *bias) {
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias + 16 * n + 4 * g);
#pragma unroll
                for (int p = 0; p < X9_RT; ++p) act[p][n] = relu4(acc[p][n] + bv);
            }
        };
        auto layer = [&]() {  // acc = W . act over the 8 k-blocks of a 256-wide input
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {
                Split8 xs[X9_RT];
#pragma unroll
                for (int p = 0; p < X9_RT; ++p) xs[p] = split8(act[p][2 * kb], act[p][2 * kb + 1]);
                step(xs, kb == 0);
            }
        };
        {
            Split8 xs[X9_RT];
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) {
                f32x4 pa, pb;
                split_pose_fragment(xv[p], g, pa, pb);
                xs[p] = split8(pa, pb);
            }
            step(xs, true);
        }
        hidden(b0l);
        layer();
    }
    // pose_encoder.2's output (bias + ReLU) split ONCE, all eight k-blocks: the B operand of every head chunk.  192 registers that take the
    // place of both the fp32 activations and the 128 accumulators of a k-major head
    Split8 xs_all[8][X9_RT];
    // its pieces: tail_read(m) asks LDS for the biases of chunks 2m and 2m + 1, tail_piece(m, q) is one eighth (tile q / 4, values 2 (q % 4),
    // + 1) of xs_all[m] = split8(relu4(acc[.][2m] + ba), relu4(acc[.][2m + 1] + bb))
    f32x4 tb[2][2];
    auto tail_read = [&](int m) {
        tb[m & 1][0] = *reinterpret_cast<const f32x4 *>(b2l + 32 * m + g4), tb[m & 1][1] = *reinterpret_cast<const f32x4 *>(b2l + 32 * m + 16 + g4);
    };
    auto tail_piece = [&](int m, int q) {
        const int p = q >> 2, i = 2 * (q & 3), j = i & 3;
        const f32x4 a = acc[p][2 * m + (i >> 2)], b = tb[m & 1][i >> 2];
        split8_pair(xs_all[m][p], i, relu_plain<DIET>(a[j] + b[j]), relu_plain<DIET>(a[j + 1] + b[j + 1]));
    };
    if constexpr (KSIDE == 0) {  // (written out in place, after the layers: the order rk45.hip's resource table was taken with)
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            const f32x4 ba = *reinterpret_cast<const f32x4 *>(b2l + 32 * kb + 4 * g), bb = *reinterpret_cast<const f32x4 *>(b2l + 32 * kb + 16 + 4 * g);
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) xs_all[kb][p] = split8(relu4(acc[p][2 * kb] + ba), relu4(acc[p][2 * kb + 1] + bb));
        }
    } else {
        // one ring step over slot gstep % 2: slice gstep + 1 goes from the registers to the other slot, slice gstep + 2 is requested
        // (the position advances BEFORE the call: after it, the kernels keep 20-68 B of scratch, profiles/r11_shared_ring_stage_resources.txt);
        // side(n): the caller's piece of other work beside the MFMAs of output chunk n (bf16x9.h).  first: the layer's first k-block opens
        // the accumulators (no zeroing pass)
        auto step = [&](const Split8 (&xs)[X9_RT], bool first, auto side) {
            const int gs = gstep++;
            ring_step<X9_NT, X9_PER_T, false, 0, 16, NPROD>(slot_of(gs), ring + ((gs + 1) & 1) * X9_SLICE, split_slice<3>(w, gs + 2), hold, xs, acc,
                                                     tid, lane_of(gs), first, side);
        };
        // The k-major layers keep their 256-wide input in fp32 (act) and split it one k-block at a time.  Nothing of that is issued between two
        // layers or two steps: every piece rides beside the MFMAs of a chunk that does not need it yet (one wave per SIMD - what is not placed
        // between MFMAs is exposed).
        //   bias0(n)        act[.][n] = relu(acc[.][n] + b0) of pose_encoder.0's chunk n, final after its own 18 MFMAs: beside chunk n + 1 (chunk
        //                   15: beside chunk 0 of pose_encoder.2's first step, which reopens acc[.][15] only at ITS chunk 15); the bias is read
        //                   from LDS a piece ahead
        //   split_piece     one eighth (tile q / 4, values 2 (q % 4), + 1) of split8(act[.][2 kb], act[.][2 kb + 1]): k-block kb + 1 beside
        //                   chunks 1-8 of step kb, k-block 0 beside chunks 3-10 of pose_encoder.0 - a step starts with its operand ready
        // The expressions and their order per value are those of relu4(acc + b) and split8: the bits do not move.
        f32x4 bv;
        Split8 xs[2][X9_RT];
        auto bias_read = [&](const float *bias, int n) { bv = *reinterpret_cast<const f32x4 *>(bias + 16 * n + g4); };
        auto bias0 = [&](int n) {
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) act[p][n] = relu_sum4<DIET>(acc[p][n], bv);
        };
        auto split_piece = [&](Split8 (&x)[X9_RT], int kb, int q) {
            const int p = q >> 2, i = 2 * (q & 3);
            const f32x4 v = act[p][2 * kb + (i >> 2)];
            split8_pair(x[p], i, v[i & 3], v[(i & 3) + 1]);
        };
        // ---- pose_encoder.0
        {
            Split8 x0[X9_RT];
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) {
                f32x4 pa, pb;
                split_pose_fragment(xv[p], g, pa, pb);
                x0[p] = split8(pa, pb);
            }
            step(x0, true, [&](int n) {
                if (n >= 1) bias0(n - 1);
                bias_read(b0l, n);
                if (n >= 3 && n < 11) split_piece(xs[0], 0, n - 3);
            });
        }
        // ---- pose_encoder.2: acc = W . act over the 8 k-blocks of its 256-wide input
#pragma unroll
        for (int kb = 0; kb < 8; ++kb)
            step(xs[kb & 1], kb == 0, [&](int n) {
                if (kb == 0 && n == 0) bias0(15);
                if (kb < 7 && n >= 1 && n < 9) split_piece(xs[(kb + 1) & 1], kb + 1, n - 1);
                if (KSIDE == 2 && kb == 7) {  // the tail: pair m is final after chunk 2m + 1 - its tile 0 beside chunk 2m + 2, its tile 1 beside chunk 2m + 3
                    if (n >= 2) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) tail_piece((n - 2) >> 1, 4 * (n & 1) + q);
                    }
                    if (n & 1) tail_read(n >> 1);  // a chunk ahead of its first use
                }
            });
        if constexpr (KSIDE < 2) {  // the tail in one block after the layer
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {
                const f32x4 ba = *reinterpret_cast<const f32x4 *>(b2l + 32 * kb + 4 * g), bb = *reinterpret_cast<const f32x4 *>(b2l + 32 * kb + 16 + 4 * g);
#pragma unroll
                for (int p = 0; p < X9_RT; ++p) xs_all[kb][p] = split8(relu4(acc[p][2 * kb] + ba), relu4(acc[p][2 * kb + 1] + bb));
            }
        }
    }
    // ---- the three heads, CHUNK-MAJOR: a slice is (two output chunks) x (eight k-blocks), a chunk's two accumulator tiles are final after
    // its 144 MFMAs, and its share of the fp32 Linear(256, 3) output layer - bias + ReLU against cvt, then o += v . w_out, chunks ascending,
    // the text and order of bf16_split_common.h's split_head_out - is issued beside the MFMAs of the NEXT chunk (across the ring barrier,
    // and across the change of head: the sums over lane groups, + b_out and emit() of head h ride on head h + 1's first chunk).  Only the
    // last head's last chunk and its emit() stay exposed.
    int cl[X9_RT];
#pragma unroll
    for (int p = 0; p < X9_RT; ++p) {
        const int r = row[p] < nrows ? row[p] : nrows - 1;
        cl[p] = r / kcand - wg_row0 / kcand;  // < NCL (the chain plan admits k only when a workgroup's rows span <= NCL clouds)
    }
    f32x4 fin[X9_RT] = {}, pend[X9_RT];  // the chunk under the MFMAs; the chunk before it, final
    float o[X9_RT][3];
    HeadEpi e;
    bf16x8 w1[3];
    // piece k of the epilogue of chunk n of head hp (one piece per sub-block of the next chunk: the reads, bias + ReLU, three dot products)
    auto epi = [&](int k, int hp, int n) {
        const int ch = 16 * n + g4;
        if (k == 0) {
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) e.cv[p] = *reinterpret_cast<const f32x4 *>(cvtl + cl[p] * HEADS + 256 * hp + ch);
#pragma unroll
            for (int c = 0; c < 3; ++c) e.w[c] = *reinterpret_cast<const f32x4 *>(woutl + (3 * hp + c) * HID + ch);
        } else if (k == 1) {
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) e.v[p] = relu_sum4<DIET>(pend[p], e.cv[p]);
        } else if (k <= 4) {
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) {
                if constexpr (DIET) o[p][k - 2] = dot4_fma(e.v[p], e.w[k - 2], o[p][k - 2]);
                else o[p][k - 2] = plain(o[p][k - 2] + dot4_plain(e.v[p], e.w[k - 2]));
            }
        }
    };
    auto finish = [&](int hp) {
#pragma unroll
        for (int p = 0; p < X9_RT; ++p) {
            // the four lane groups hold the four channel quarters: fixed order, every lane gets the sum
            const float out[3] = {lane_groups_sum(o[p][0]) + w.b_out[3 * hp + 0], lane_groups_sum(o[p][1]) + w.b_out[3 * hp + 1],
                                  lane_groups_sum(o[p][2]) + w.b_out[3 * hp + 2]};
            emit(hp, p, out);
        }
    };
    auto chunk = [&](auto c01, auto side) {
        constexpr int C = decltype(c01)::value;
        const int gs = gstep;
        if (C == 1) ++gstep;
#pragma unroll
        for (int p = 0; p < X9_RT; ++p) pend[p] = fin[p];
        ring_half_step<X9_NT, X9_PER_T, 8, C, NPROD>(slot_of(gs), ring + ((gs + 1) & 1) * X9_SLICE, split_slice<3>(w, gs + 2), hold, w1, xs_all,
                                              fin, tid, lane_of(gs), side);
    };
    constexpr std::integral_constant<int, 0> c0{};
    constexpr std::integral_constant<int, 1> c1{};
    chunk(c0, [&](int k) {  // xs_all[7] (final only now) is not read before sub-block 7
        if (KSIDE == 2 && k < 4) tail_piece(7, 2 * k), tail_piece(7, 2 * k + 1);
    });
#pragma unroll 1
    for (int h = 0; h < 3; ++h) {
#pragma unroll
        for (int p = 0; p < X9_RT; ++p) o[p][0] = o[p][1] = o[p][2] = 0.f;
        chunk(c1, [&](int k) { epi(k, h, 0); });
#pragma unroll
        for (int j = 1; j < 8; ++j) {
            chunk(c0, [&](int k) { epi(k, h, 2 * j - 1); });
            chunk(c1, [&](int k) { epi(k, h, 2 * j); });
        }
        if (h < 2) {  // head h + 1's first chunk carries head h's last epilogue and its outputs
            chunk(c0, [&](int k) {
                epi(k, h, 15);
                if (k == 5) finish(h);
            });
        } else {
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) pend[p] = fin[p];
#pragma unroll
            for (int k = 0; k < 5; ++k) epi(k, h, 15);
            finish(h);
        }
    }
}

}  // namespace gp_x9trunk
