// The score trunk as EXACT-PRODUCT split bf16 on the BF16 matrix pipe (bf16x9.h), once for its kernels: the PC step's chain plan, its
// seeded twin and the Heun step (trunk_bf16x9.hip) and the RK45 chain stage (rk45.hip).  4 waves per workgroup (one per SIMD, the whole
// 512-entry register file), each carrying TWO 16-row B tiles = 32 rows, 128 rows per workgroup.  The D fragment of a layer is the next
// layer's B operand.  All weights stream through a 2-slot LDS ring in 33 slices of 48 KB: pose_encoder.0 (1) and pose_encoder.2 (8)
// K-MAJOR (ring_step: one k-block x 16 output chunks; the fp32 input split into hi / mid / lo one k-block at a time, 128 accumulator
// registers), then the three heads (8 each) CHUNK-MAJOR (ring_half_step: two output chunks x all eight k-blocks): pose_encoder.2's output
// is split once into 192 registers that all three heads read, 16 accumulator registers are live, and a chunk's fp32 epilogue is issued
// between the MFMAs of the next chunk.  Every accumulator takes its k-blocks ascending and every head output its chunks ascending in
// both orders: the bits are those of k-major heads (tests/test_gpu_x9_chain_bits.py).
//   request : slices 0 and 1 into registers - the caller places it among its own loads (memory returns in order)
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
__device__ __forceinline__ f32x4 relu_sum4(const f32x4 a, const f32x4 b) {  // relu4(a + b)
    return f32x4{fmaxf(plain(a.x + b.x), 0.f), fmaxf(plain(a.y + b.y), 0.f), fmaxf(plain(a.z + b.z), 0.f), fmaxf(plain(a.w + b.w), 0.f)};
}
__device__ __forceinline__ float dot4_plain(const f32x4 v, const f32x4 w) {  // v.x * w.x + v.y * w.y + v.z * w.z + v.w * w.w
    const float m0 = plain(v.x * w.x), m1 = plain(v.y * w.y), m2 = plain(v.z * w.z), m3 = plain(v.w * w.w);
    return plain(plain(plain(m0 + m1) + m2) + m3);
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
template <class Emit>
__device__ __forceinline__ void run(float *lds, const SplitNet &w, const float *cvec, const float *tvec, int wg_row0, int nrows, int kcand,
                                    const bf16x8 (&first)[X9_PER_T], bf16x8 (&hold)[X9_PER_T], const float (&xv)[X9_RT][POSE],
                                    const int (&row)[X9_RT], Emit emit) {
    bf16x8 *ring = reinterpret_cast<bf16x8 *>(lds);
    const float *woutl = lds + X9Lds::OFF_WOUT, *b0l = lds + X9Lds::OFF_B0, *b2l = lds + X9Lds::OFF_B2, *cvtl = lds + X9Lds::OFF_CVT;
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
    // ---- staged epilogue operands and slot 0
    split_stage<X9_NT, X9Lds>(lds, w, cvec, tvec, wg_row0, nrows, kcand);
#pragma unroll
    for (int u = 0; u < X9_PER_T; ++u) ring[tid + u * X9_NT] = first[u];
    __syncthreads();
    int gstep = 0;
    f32x4 acc[X9_RT][16];
    // one ring step over slot gstep % 2: slice gstep + 1 goes from the registers to the other slot, slice gstep + 2 is requested
    // (the position advances BEFORE the call: after it, the kernels keep 20-68 B of scratch, profiles/r11_shared_ring_stage_resources.txt)
    auto step = [&](const Split8 (&xs)[X9_RT], bool first) {  // first: the layer's first k-block opens the accumulators (no zeroing pass)
        const int gs = gstep++;
        ring_step<X9_NT, X9_PER_T, false, 0, 16>(ring + (gs & 1) * X9_SLICE, ring + ((gs + 1) & 1) * X9_SLICE, split_slice<3>(w, gs + 2), hold, xs, acc,
                                                 tid, lane, first);
    };
    // bias + ReLU of a 256-wide hidden layer, kept in fp32 (split one k-block at a time as the next layer consumes it)
    f32x4 act[X9_RT][16];
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
    // ---- pose_encoder.0
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
    // ---- pose_encoder.2
    layer();
    // ---- its output (bias + ReLU) split ONCE, all eight k-blocks: the B operand of every head chunk.  192 registers that take the place of
    // both the fp32 activations and the 128 accumulators of a k-major head
    Split8 xs_all[8][X9_RT];
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) {
        const f32x4 ba = *reinterpret_cast<const f32x4 *>(b2l + 32 * kb + 4 * g), bb = *reinterpret_cast<const f32x4 *>(b2l + 32 * kb + 16 + 4 * g);
#pragma unroll
        for (int p = 0; p < X9_RT; ++p) xs_all[kb][p] = split8(relu4(acc[p][2 * kb] + ba), relu4(acc[p][2 * kb + 1] + bb));
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
        const int ch = 16 * n + 4 * g;
        if (k == 0) {
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) e.cv[p] = *reinterpret_cast<const f32x4 *>(cvtl + cl[p] * HEADS + 256 * hp + ch);
#pragma unroll
            for (int c = 0; c < 3; ++c) e.w[c] = *reinterpret_cast<const f32x4 *>(woutl + (3 * hp + c) * HID + ch);
        } else if (k == 1) {
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) e.v[p] = relu_sum4(pend[p], e.cv[p]);
        } else if (k <= 4) {
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) o[p][k - 2] = plain(o[p][k - 2] + dot4_plain(e.v[p], e.w[k - 2]));
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
        ring_half_step<X9_NT, X9_PER_T, 8, C>(ring + (gs & 1) * X9_SLICE, ring + ((gs + 1) & 1) * X9_SLICE, split_slice<3>(w, gs + 2), hold, w1, xs_all,
                                              fin, tid, lane, side);
    };
    constexpr std::integral_constant<int, 0> c0{};
    constexpr std::integral_constant<int, 1> c1{};
    chunk(c0, [](int) {});
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
