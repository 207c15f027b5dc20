// The score trunk as EXACT-PRODUCT split bf16 on the BF16 matrix pipe (bf16x9.h), once for its two kernels: the PC step's chain plan
// (trunk_bf16x9.hip) and the RK45 chain stage (rk45.hip).  4 waves per workgroup (one per SIMD, the whole 512-entry register file), each
// carrying TWO 16-row B tiles = 32 rows, 128 rows per workgroup.  The D fragment of a layer is the next layer's B operand; activations stay
// in fp32 registers and are split into hi / mid / lo one k-block at a time.  All weights stream through a 2-slot LDS ring (ring_step) in
// 33 slices of 48 KB: pose_encoder.0 (1), pose_encoder.2 (8), three heads (8 each).
//   request : slices 0 and 1 into registers - the caller places it among its own loads (memory returns in order)
//   run     : staged fp32 operands, slot 0, the layers, and after EACH head its fp32 Linear(256, 3) outputs handed to the caller's functor
//             (both callers store at once: carrying the nine outputs to the end costs 27-40 more spilled registers,
//             profiles/r9_rk45_bf16x9_resources.txt)
#pragma once
#include "bf16x9.h"

namespace gp_x9trunk {

using namespace gp_split;
using namespace gp_bf16x9;

constexpr int X9_NW = 4, X9_NT = 64 * X9_NW, X9_RT = 2, X9_ROWS = 16 * X9_RT * X9_NW;
using X9Lds = SplitLds<3, 2>;  // 2 slots of 48 KB
constexpr int X9_SLICE = X9Lds::SLICE, X9_PER_T = X9_SLICE / X9_NT;
static_assert(X9_ROWS == 128 && X9_PER_T <= 16, "one slice element per thread and output chunk at most");

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
    auto step = [&](const Split8 (&xs)[X9_RT]) {
        const int gs = gstep++;
        ring_step<X9_NT, X9_PER_T, false, 0, 16>(ring + (gs & 1) * X9_SLICE, ring + ((gs + 1) & 1) * X9_SLICE, split_slice<3>(w, gs + 2), hold, xs, acc,
                                                 tid, lane);
    };
    auto zero_acc = [&]() {
#pragma unroll
        for (int p = 0; p < X9_RT; ++p)
#pragma unroll
            for (int n = 0; n < 16; ++n) acc[p][n] = f32x4{0.f, 0.f, 0.f, 0.f};
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
        zero_acc();
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            Split8 xs[X9_RT];
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) xs[p] = split8(act[p][2 * kb], act[p][2 * kb + 1]);
            step(xs);
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
        zero_acc();
        step(xs);
    }
    hidden(b0l);
    // ---- pose_encoder.2
    layer();
    hidden(b2l);
    // ---- the three heads; their Linear(256, 3) output layers as fp32 dot products on the accumulator fragments
    int cl[X9_RT];
#pragma unroll
    for (int p = 0; p < X9_RT; ++p) {
        const int r = row[p] < nrows ? row[p] : nrows - 1;
        cl[p] = r / kcand - wg_row0 / kcand;  // < NCL (the chain plan admits k only when a workgroup's rows span <= NCL clouds)
    }
#pragma unroll 1
    for (int h = 0; h < 3; ++h) {
        layer();
#pragma unroll
        for (int p = 0; p < X9_RT; ++p) {
            // (bf16_split_common.h's split_head_out written out: through that helper these kernels, which sit on the register cliff,
            // compile to 168 spilled registers, profiles/r8_pc_rows_resources.txt)
            float o0 = 0.f, o1 = 0.f, o2 = 0.f;
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const int ch = 16 * n + 4 * g;
                const f32x4 v = relu4(acc[p][n] + *reinterpret_cast<const f32x4 *>(cvtl + cl[p] * HEADS + 256 * h + ch));
                const f32x4 w0 = *reinterpret_cast<const f32x4 *>(woutl + (3 * h + 0) * HID + ch);
                const f32x4 w1 = *reinterpret_cast<const f32x4 *>(woutl + (3 * h + 1) * HID + ch);
                const f32x4 w2 = *reinterpret_cast<const f32x4 *>(woutl + (3 * h + 2) * HID + ch);
                o0 += v.x * w0.x + v.y * w0.y + v.z * w0.z + v.w * w0.w;
                o1 += v.x * w1.x + v.y * w1.y + v.z * w1.z + v.w * w1.w;
                o2 += v.x * w2.x + v.y * w2.y + v.z * w2.z + v.w * w2.w;
            }
            // the four lane groups hold the four channel quarters: fixed order, every lane gets the sum
            const float out[3] = {lane_groups_sum(o0) + w.b_out[3 * h + 0], lane_groups_sum(o1) + w.b_out[3 * h + 1],
                                  lane_groups_sum(o2) + w.b_out[3 * h + 2]};
            emit(h, p, out);
        }
    }
}

}  // namespace gp_x9trunk
