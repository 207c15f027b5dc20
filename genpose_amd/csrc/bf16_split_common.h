// What the two split-bf16 score trunks of the PC step (trunk_bf16x9.hip: hi / mid / lo, trunk_bf16x3.hip: hi / lo) share around their
// arithmetic (bf16x9.h, bf16x3.h): the vector types, the weight stream's slice addresses, the fp32 operands staged in LDS, the first
// layer's pose fragment and the fp32 Linear(256, 3) head epilogue.  NTERM = bf16 terms per weight (3 / 2).  Rings, barriers and launch
// geometry stay with each kernel.
#pragma once
#include "score_trunk.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace gp_split {

using namespace gp_trunk;

// packed weights (weights.pack_bf16x9 / pack_bf16x3) and the fp32 operands of the epilogues
struct SplitNet {
    const bf16x8 *w0;  // pose_encoder.0 [1][16][NTERM][64]   k = component index (natural order, zero padded to 32)
    const bf16x8 *w2;  // pose_encoder.2 [8][16][NTERM][64]   k order of the register chain
    const bf16x8 *wh;  // stacked heads  NTERM = 2: [8][48][NTERM][64] (k-block, output chunk);  NTERM = 3: [3][8][2][8][NTERM][64]
                       // (head, chunk pair, chunk of the pair, k-block) - the order trunk_bf16x9.h consumes (weights.pack_heads_bf16x9)
    const float *b0, *b2, *w_out, *b_out;  // fp32: biases [256], [256]; output layers [9][256], [9]
};
// from an entry point's arguments: the three packs as they arrive over the C ABI, the fp32 operands from the network
static inline SplitNet split_net(const gp_scorenet *net, const void *w_pose0, const void *w_pose2, const void *w_headx) {
    return {reinterpret_cast<const bf16x8 *>(w_pose0), reinterpret_cast<const bf16x8 *>(w_pose2), reinterpret_cast<const bf16x8 *>(w_headx),
            net->b_pose0, net->b_pose2, net->w_out, net->b_out};
}

constexpr int NSLICES = 33;  // pose_encoder.0 (1), pose_encoder.2 (8), three heads (8 each)
constexpr int NCL = 4;       // clouds a workgroup's 128 rows may span (gp_pc_layout)

// LDS (floats): ring [SLOTS][SLICE] bf16x8 | w_out [9][256] | b0 [256] | b2 [256] | cvt [NCL][768] = cvec[cloud] + tvec
template <int NTERM, int SLOTS>
struct SplitLds {
    static constexpr int SLICE = 16 * NTERM * 64;  // bf16x8 (16 B) per slice = 16 (k-block, output chunk) sub-blocks x NTERM terms
    static constexpr int OFF_WOUT = SLOTS * SLICE * 4, OFF_B0 = OFF_WOUT + POSE * HID, OFF_B2 = OFF_B0 + HID, OFF_CVT = OFF_B2 + HID,
                         TOTAL = OFF_CVT + NCL * HEADS;
    static constexpr size_t BYTES = (size_t)TOTAL * sizeof(float);
    static_assert(BYTES <= 160 * 1024, "LDS");
};

template <int NTERM>
__device__ __forceinline__ const bf16x8 *split_slice(const SplitNet &w, int s) {
    s = s < NSLICES ? s : NSLICES - 1;  // the ring runs ahead: requests past the end re-read the last slice (never used)
    if (s == 0) return w.w0;
    if (s <= 8) return w.w2 + (size_t)(s - 1) * (16 * NTERM * 64);
    if constexpr (NTERM == 3) return w.wh + (size_t)(s - 9) * (16 * NTERM * 64);  // chunk-major: slice (head, chunk pair) as consumed
    const int h = (s - 9) >> 3, kb = (s - 9) & 7;
    return w.wh + ((size_t)kb * 48 + 16 * h) * NTERM * 64;
}

// w_out, the two hidden biases and cvec[cloud] + tvec of step i for the workgroup's (up to NCL) clouds -> LDS, by NT threads
template <int NT, typename L>
__device__ __forceinline__ void split_stage(float *lds, const SplitNet &w, const float *cvec, const float *tvec, int wg_row0, int nrows, int kcand) {
    const int tid = threadIdx.x;
    float *woutl = lds + L::OFF_WOUT, *b0l = lds + L::OFF_B0, *b2l = lds + L::OFF_B2, *cvtl = lds + L::OFF_CVT;
    for (int e = tid; e < POSE * HID; e += NT) woutl[e] = w.w_out[e];
    for (int e = tid; e < HID; e += NT) b0l[e] = w.b0[e], b2l[e] = w.b2[e];
    const int cloud0 = wg_row0 / kcand, last_cloud = (nrows - 1) / kcand;
    for (int e = tid; e < NCL * HEADS; e += NT) {
        const int c = e / HEADS, o = e - c * HEADS;
        const int cl = cloud0 + c < last_cloud ? cloud0 + c : last_cloud;
        cvtl[e] = cvec[(size_t)cl * HEADS + o] + tvec[o];
    }
}

// split_stage in two phases, for a kernel that has other work between them (trunk_bf16x9.hip: the sampler update).  None of these
// loads depends on that work: REQUEST them before it and before the weight ring's prologue (memory returns in order, so they arrive
// under it and not behind 24 weight loads), STORE them to LDS after it.  16-byte loads: w_out | b0 | b2 are contiguous in LDS and
// (POSE + 2) HID / 4 = 704 float4; cvt is NCL HEADS / 4 = 768 float4, each the sum of one float4 of cvec[cloud] and one of tvec - the
// expression and the cloud clamp of split_stage, element by element.  All five arrays must be 16-byte aligned (rows of 256 / 768 floats
// of an aligned base are; the launchers check).
template <int NT>
struct SplitStaged {
    static constexpr int NW4 = (POSE + 2) * HID / 4, NC4 = NCL * HEADS / 4, H4 = HEADS / 4;
    static constexpr int W_PER_T = (NW4 + NT - 1) / NT, C_PER_T = NC4 / NT;
    static_assert(NC4 % NT == 0, "whole float4 rounds of cvt");
    f32x4 wv[W_PER_T], cv[C_PER_T], tv[C_PER_T];
};

template <int NT>
__device__ __forceinline__ void split_stage_request(SplitStaged<NT> &sg, const SplitNet &w, const float *cvec, const float *tvec, int wg_row0, int nrows,
                                                    int kcand) {
    using S = SplitStaged<NT>;
    const int tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < S::W_PER_T; ++u) {
        const int e = tid + u * NT;  // float4 index into w_out | b0 | b2
        if (e < S::NW4) {
            const float *src = e < POSE * HID / 4 ? w.w_out + 4 * e : e < (POSE + 1) * HID / 4 ? w.b0 + 4 * e - POSE * HID : w.b2 + 4 * e - (POSE + 1) * HID;
            sg.wv[u] = *reinterpret_cast<const f32x4 *>(src);
        }
    }
    const int cloud0 = wg_row0 / kcand, last_cloud = (nrows - 1) / kcand;
#pragma unroll
    for (int u = 0; u < S::C_PER_T; ++u) {
        const int e = tid + u * NT, c = e / S::H4, o = e - c * S::H4;
        const int cl = cloud0 + c < last_cloud ? cloud0 + c : last_cloud;
        sg.cv[u] = reinterpret_cast<const f32x4 *>(cvec + (size_t)cl * HEADS)[o];
        sg.tv[u] = reinterpret_cast<const f32x4 *>(tvec)[o];
    }
}

template <int NT, typename L>
__device__ __forceinline__ void split_stage_store(float *lds, const SplitStaged<NT> &sg) {
    using S = SplitStaged<NT>;
    static_assert(L::OFF_B0 == L::OFF_WOUT + POSE * HID && L::OFF_B2 == L::OFF_B0 + HID && L::OFF_WOUT % 4 == 0 && L::OFF_CVT % 4 == 0, "LDS layout");
    const int tid = threadIdx.x;
    f32x4 *wl = reinterpret_cast<f32x4 *>(lds + L::OFF_WOUT), *cvtl = reinterpret_cast<f32x4 *>(lds + L::OFF_CVT);
#pragma unroll
    for (int u = 0; u < S::W_PER_T; ++u)
        if (tid + u * NT < S::NW4) wl[tid + u * NT] = sg.wv[u];
#pragma unroll
    for (int u = 0; u < S::C_PER_T; ++u) cvtl[tid + u * NT] = sg.cv[u] + sg.tv[u];
}

// pose_encoder.0's B operand: the row's nine components as the one (zero-padded) k-block, natural k order: lane group g holds
// k = 8g .. 8g+7
__device__ __forceinline__ void split_pose_fragment(const float (&xv)[9], int g, f32x4 &pa, f32x4 &pb) {
    pa = f32x4{0.f, 0.f, 0.f, 0.f}, pb = f32x4{0.f, 0.f, 0.f, 0.f};
    if (g == 0) pa = f32x4{xv[0], xv[1], xv[2], xv[3]}, pb = f32x4{xv[4], xv[5], xv[6], xv[7]};
    if (g == 1) pa = f32x4{xv[8], 0.f, 0.f, 0.f};
}

// Head h's Linear(256, 3) output layer as fp32 dot products on the accumulator fragments: out[c] = relu(acc + cvt) . w_out[3 h + c]
// (cvt: the row's cloud's row of the staged cvec + tvec).  The four lane groups hold the four channel quarters: fixed order, every
// lane gets the sum.
__device__ __forceinline__ void split_head_out(const f32x4 (&acc)[16], const float *cvt, const float *woutl, int h, int g, float (&out)[3]) {
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
#pragma unroll
    for (int n = 0; n < 16; ++n) {
        const int ch = 16 * n + 4 * g;
        const f32x4 v = relu4(acc[n] + *reinterpret_cast<const f32x4 *>(cvt + 256 * h + ch));
        const f32x4 w0 = *reinterpret_cast<const f32x4 *>(woutl + (3 * h + 0) * HID + ch);
        const f32x4 w1 = *reinterpret_cast<const f32x4 *>(woutl + (3 * h + 1) * HID + ch);
        const f32x4 w2 = *reinterpret_cast<const f32x4 *>(woutl + (3 * h + 2) * HID + ch);
        o0 += v.x * w0.x + v.y * w0.y + v.z * w0.z + v.w * w0.w;
        o1 += v.x * w1.x + v.y * w1.y + v.z * w1.z + v.w * w1.w;
        o2 += v.x * w2.x + v.y * w2.y + v.z * w2.z + v.w * w2.w;
    }
    out[0] = lane_groups_sum(o0), out[1] = lane_groups_sum(o1), out[2] = lane_groups_sum(o2);
}

}  // namespace gp_split
