// Forward + backward pass of the score trunk for one 16-row tile: the score of the network, or of the ENERGY model (the gradient of
// its inner-product energy), and the Skilling-Hutchinson divergence estimate - shared by gp_score_div / gp_energy_score
// (score_div.hip), the predictor-corrector step of the energy model (scorenet.hip) and the RK45 stage kernels that integrate the
// energy model's probability-flow ODE and the likelihood ODE (rk45.hip).
//
// The reference evaluates these with autograd (networks/gf_algorithms/energynet.py:200-222, samplers.py:49-71): a second network
// pass per evaluation.  Here one tile runs the forward trunk, keeps both hidden layers (post-ReLU) in LDS, seeds the backward pass
// on the head-layer fragments while they are in registers
//     g3[c] = [a3[c] > 0] * sum_i w_out[i][c] * u_i
// and pushes it back through the transposed weight packs (w_headx^T, w_pose2^T, w_pose0^T) on the same MFMA building block.
#pragma once
#include "score_trunk.h"

namespace gp_bwd {

using namespace gp_trunk;

constexpr int DP = 16, DNW = TrunkCfg<DP>::NW, DNV = TrunkCfg<DP>::NV, DNT = TrunkCfg<DP>::NT;
static_assert(DNW == 4 && DNV == 4, "the backward layers assume 4 waves x 4 chunks");
constexpr int LDG = HEADS + GP_LD_PAD;            // row stride of the head-layer gradient G3 [P][768]
constexpr int OFF_G3 = TrunkLds<DP, true>::TOTAL;  // after the trunk's own LDS
constexpr int OFF_U = OFF_G3 + DP * LDG;          // u [P][12] (backward seed, per mode), probe [P][12]
constexpr int LDS_FLOATS = OFF_U + 2 * DP * 12;
constexpr size_t LDS_BYTES = (size_t)LDS_FLOATS * sizeof(float);
constexpr int LDS_OUT = 12;                       // row stride of the result: out[r][0..8] = score, out[r][9] = divergence / energy

// what the tile computes from x (in X0) and the probe (in the second half of the U block)
//   SCORE_DIV : u = probe / (sigma + 1e-7);  score = f / (sigma + 1e-7);  extra = (J_f^T u) . probe   (likelihood, samplers.py:49-71)
//   ENERGY    : probe = x, u = x / sigma;    score = f / sigma + J_f^T u (= d/dx <x, f(x)/sigma>, energynet.py:200-222);
//               extra = <x, f / sigma> (the un-decoupled inner-product energy)
enum Mode { SCORE_DIV = 0, ENERGY = 1 };

// g_out[r][n] = mask[r][n] > 0 ? sum_k Wt[n][k] * g_in[r][k] : 0 for the wave's four 16-channel chunks; written over `mask`.
template <int KG>
__device__ __forceinline__ void backward_dense(const float *Gin, int ldg, const float *__restrict__ Wt, float *MaskOut, int ldo) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nc[4] = {wave, wave + DNW, wave + 2 * DNW, wave + 3 * DNW};
    f32x4 acc[4][1];
    mfma_tile<DNV, 1>(Gin, ldg, 0, Wt, KG, HID / 16, nc, acc);
#pragma unroll
    for (int i = 0; i < DNV; ++i) {
        float *m = MaskOut + (lane & 15) * ldo + nc[i] * 16 + 4 * (lane >> 4);
        const f32x4 h = *reinterpret_cast<const f32x4 *>(m);
        f32x4 g = acc[i][0];
        g.x = h.x > 0.f ? g.x : 0.f;
        g.y = h.y > 0.f ? g.y : 0.f;
        g.z = h.z > 0.f ? g.z : 0.f;
        g.w = h.w > 0.f ? g.w : 0.f;
        *reinterpret_cast<f32x4 *>(m) = g;
    }
}

// the probe rows of the tile -> LDS (ENERGY: the probe is x itself, taken from X0 by seed_from_x); call before the barrier that
// precedes score_vjp_tile
__device__ __forceinline__ void load_probe_tile(float *lds, const float *__restrict__ probe, int row0, int nrows) {
    float *E = lds + OFF_U + DP * 12;
    for (int e = threadIdx.x; e < DP * 12; e += DNT) {
        const int r = e / 12, j = e - r * 12;
        int g = row0 + r;
        if (g >= nrows) g = nrows - 1;
        E[e] = j < POSE ? probe[(size_t)g * POSE + j] : 0.f;
    }
}

// Preconditions: x rows in X0 (cols 0..8, zero padded to 16); MODE SCORE_DIV: probe rows loaded (load_probe_tile); ONE
// __syncthreads(); trunk_begin<DP>() issued earlier.  Result (valid after the call, which ends on a barrier): out = lds + OFF_U,
// out[r * LDS_OUT + j], j < 9 score, j == 9 divergence estimate / energy.
template <int MODE>
__device__ __forceinline__ const float *score_vjp_tile(float *lds, const gp_scorenet &net, const float *__restrict__ cvec, const float *__restrict__ tvec,
                                                       int row0, int nrows, int kcand, TrunkPre<DP> &pre, float sigma) {
    using L = TrunkLds<DP, true>;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *X0 = lds, *H1 = lds + L::OFF_H1, *H2 = lds + L::OFF_H2, *G3 = lds + OFF_G3, *U = lds + OFF_U, *E = U + DP * 12;
    // backward seed u (and, ENERGY, the probe = x)
    for (int e = tid; e < DP * 12; e += DNT) {
        const int r = e / 12, j = e - r * 12;
        if (MODE == ENERGY) {
            const float xv = j < POSE ? X0[r * L::LD0 + j] : 0.f;
            E[e] = xv;
            U[e] = xv / sigma;
        } else {
            U[e] = E[e] / (sigma + 1e-7f);
        }
    }
    __syncthreads();
    // forward; every head-layer fragment leaves its backward seed in G3 (same lane layout as the activations: one b128 store)
    trunk_ftheta<DP, true>(lds, net, cvec, tvec, row0, nrows, kcand, pre,
                           [&](int h, int, int, const f32x4 &a3, const f32x4 &w0, const f32x4 &w1, const f32x4 &w2, int ch) {
                               const float *u = U + (lane & 15) * 12 + 3 * h;
                               const float u0 = u[0], u1 = u[1], u2 = u[2];
                               f32x4 g;
                               g.x = a3.x > 0.f ? (w0.x * u0 + w1.x * u1) + w2.x * u2 : 0.f;
                               g.y = a3.y > 0.f ? (w0.y * u0 + w1.y * u1) + w2.y * u2 : 0.f;
                               g.z = a3.z > 0.f ? (w0.z * u0 + w1.z * u1) + w2.z * u2 : 0.f;
                               g.w = a3.w > 0.f ? (w0.w * u0 + w1.w * u1) + w2.w * u2 : 0.f;
                               *reinterpret_cast<f32x4 *>(G3 + (lane & 15) * LDG + ch) = g;
                           });
    // f_theta sits in X0 columns 12..20 (KEEP_H1).  backward: g2 = (Wx^T g3) . [h2 > 0] -> over H2;  g1 = (W2^T g2) . [h1 > 0] -> over H1
    backward_dense<HEADS / 16>(G3, LDG, net.w_headx_t, H2, L::LDH);
    __syncthreads();
    backward_dense<HID / 16>(H2, L::LDH, net.w_pose2_t, H1, L::LDH);
    __syncthreads();
    // gx = W0^T g1 (9 of 16 channels): one 16-channel chunk, wave 0; results over the (dead) seed block U
    if (wave == 0) {
        const int nc[4] = {0, 0, 0, 0};
        f32x4 acc[4][1];
        mfma_tile<1, 1>(H1, L::LDH, 0, net.w_pose0_t, HID / 16, 1, nc, acc);
        const int r = lane & 15, g = lane >> 4;
        const float *e = E + r * 12 + 4 * g;  // probe components 4g..4g+3 (zero beyond 8)
        const float gx[4] = {acc[0][0].x, acc[0][0].y, acc[0][0].z, acc[0][0].w};
        float extra = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = 4 * g + q;
            if (j < POSE) {
                if (MODE == SCORE_DIV) {
                    extra += gx[q] * e[q];
                    U[r * LDS_OUT + j] = X0[r * L::LD0 + 12 + j] / (sigma + 1e-7f);
                } else {
                    const float s = X0[r * L::LD0 + 12 + j] / sigma;
                    extra += e[q] * s;
                    U[r * LDS_OUT + j] = s + gx[q];
                }
            }
        }
        // lanes l, l+16, l+32 hold the three channel groups of row l: sum them (group 3 holds zeros)
        extra += __shfl_xor(extra, 16, 64);
        extra += __shfl_xor(extra, 32, 64);
        if (lane < 16) U[r * LDS_OUT + 9] = extra;
    }
    __syncthreads();
    return U;
}

// ------------------------------------------------------------------------------------------------ exact divergence
// score and the EXACT divergence tr(d score / d x) = sum_i (e_i^T J)_i of one 16-row tile: the Hutchinson probe of SCORE_DIV replaced by
// the nine unit seeds.  The forward trunk runs once and is the code SCORE_DIV runs (same f_theta, same score bits); instead of a seeded
// gradient its head-layer hook keeps the ReLU mask of the 768 head channels, one bit group per accumulator fragment.  Seed e_i reaches
// only head i / 3 (rot_x, rot_y, trans), through row i mod 3 of that head's 256 -> 3 output layer:
//     g3_i[c] = [a3[256 h + c] > 0] * w_out[i][c]            (c < 256: the head's own channels; every other head channel is zero)
// so the three seeds of a head become three 16-row M-tiles of ONE pass over that head's 256 columns of w_headx^T, then over w_pose2^T
// and w_pose0^T (mfma_tile<.., 3>): every weight fragment feeds three MFMAs, as in a 48-row tile.  Per tile the backward pass streams
// w_headx^T once (0.75 MB) and w_pose2^T three times (3 x 0.25 MB) - 1.5 MB against 9 MB for nine passes of the probe code - and
// issues 4 752 MFMA k-groups against the forward pass's 1 040.  The three seed tiles of a head run IN PLACE in one [48][256] block
// (a layer's outputs wait in the accumulators until every wave has read its inputs); H1 / H2 are only read, they serve all three heads.
// The cloud and time columns of the heads' first layers do not depend on x and take no part.
constexpr int XS = 3;                                // seeds per pass = outputs of one head
constexpr int LDM = HEADS / 4 + 4;                   // words per row of the head-layer mask: one word per 4 channels
constexpr int OFF_XM = TrunkLds<DP, true>::TOTAL;    // mask [P][LDM]
constexpr int OFF_XO = OFF_XM + DP * LDM;            // out [P][12] (score, divergence), diag [P][12] ((e_i^T J_f)_i)
constexpr int OFF_XG = OFF_XO + 2 * DP * 12;         // seed tiles [XS * P][256 + pad]
constexpr int LDS_FLOATS_EXACT = OFF_XG + XS * DP * TrunkLds<DP, true>::LDH;
constexpr size_t LDS_BYTES_EXACT = (size_t)LDS_FLOATS_EXACT * sizeof(float);
static_assert(OFF_XM % 4 == 0 && OFF_XO % 4 == 0 && OFF_XG % 4 == 0, "b128 accesses");
static_assert(LDS_BYTES_EXACT <= 160 * 1024, "one workgroup per CU");

// g_out = mask > 0 ? (Wt g_in) : 0 for the three seed tiles, written over g_in (G: [XS * P][ldg]); mask rows are shared by the tiles.
// Ends on a barrier.
__device__ __forceinline__ void backward_dense_seeds(float *G, int ldg, const float *__restrict__ Wt, const float *Mask, int ldm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nc[4] = {wave, wave + DNW, wave + 2 * DNW, wave + 3 * DNW};
    f32x4 acc[4][XS];
    mfma_tile<DNV, XS>(G, ldg, 0, Wt, HID / 16, HID / 16, nc, acc);
    __syncthreads();  // every wave has read G
#pragma unroll
    for (int i = 0; i < DNV; ++i) {
        const int col = nc[i] * 16 + 4 * (lane >> 4);
        const f32x4 h = *reinterpret_cast<const f32x4 *>(Mask + (lane & 15) * ldm + col);
#pragma unroll
        for (int p = 0; p < XS; ++p) {
            f32x4 g = acc[i][p];
            g.x = h.x > 0.f ? g.x : 0.f;
            g.y = h.y > 0.f ? g.y : 0.f;
            g.z = h.z > 0.f ? g.z : 0.f;
            g.w = h.w > 0.f ? g.w : 0.f;
            *reinterpret_cast<f32x4 *>(G + (p * DP + (lane & 15)) * ldg + col) = g;
        }
    }
    __syncthreads();
}

// Preconditions as score_vjp_tile (no probe).  Result (valid after the call, which ends on a barrier): out = lds + OFF_XO,
// out[r * LDS_OUT + j], j < 9 score (SCORE_DIV's bits), j == 9 the exact divergence.
__device__ __forceinline__ const float *score_div_exact_tile(float *lds, const gp_scorenet &net, const float *__restrict__ cvec,
                                                             const float *__restrict__ tvec, int row0, int nrows, int kcand, TrunkPre<DP> &pre,
                                                             float sigma) {
    using L = TrunkLds<DP, true>;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *X0 = lds, *H1 = lds + L::OFF_H1, *H2 = lds + L::OFF_H2, *O = lds + OFF_XO, *D = O + DP * 12, *G = lds + OFF_XG;
    const float *Wout = lds + L::OFF_WOUT;
    unsigned *M3 = reinterpret_cast<unsigned *>(lds + OFF_XM);
    // forward; every head-layer fragment leaves its ReLU mask (bit q: channel ch + q is active)
    trunk_ftheta<DP, true>(lds, net, cvec, tvec, row0, nrows, kcand, pre,
                           [&](int, int, int, const f32x4 &a3, const f32x4 &, const f32x4 &, const f32x4 &, int ch) {
                               M3[(lane & 15) * LDM + (ch >> 2)] = (a3.x > 0.f ? 1u : 0u) | (a3.y > 0.f ? 2u : 0u) | (a3.z > 0.f ? 4u : 0u) | (a3.w > 0.f ? 8u : 0u);
                           });
    // f_theta sits in X0 columns 12..20, the post-ReLU hidden layers in H1 / H2, w_out in LDS (staged by the forward pass)
#pragma unroll 1
    for (int h = 0; h < 3; ++h) {
        // seed tiles of head h: G[p][r][c] = mask3[r][256 h + c] * w_out[3 h + p][c]
        for (int e = tid; e < DP * (HID / 4); e += DNT) {
            const int r = e / (HID / 4), q = e - r * (HID / 4);
            const unsigned m = M3[r * LDM + h * (HID / 4) + q];
#pragma unroll
            for (int p = 0; p < XS; ++p) {
                const f32x4 w = *reinterpret_cast<const f32x4 *>(Wout + (3 * h + p) * HID + 4 * q);
                f32x4 g;
                g.x = (m & 1u) ? w.x : 0.f;
                g.y = (m & 2u) ? w.y : 0.f;
                g.z = (m & 4u) ? w.z : 0.f;
                g.w = (m & 8u) ? w.w : 0.f;
                *reinterpret_cast<f32x4 *>(G + (p * DP + r) * L::LDH + 4 * q) = g;
            }
        }
        __syncthreads();
        // g2 = (Wx_h^T g3) . [h2 > 0]: the head's 256 columns = k-groups [16 h, 16 h + 16) of the transposed pack;  g1 = (W2^T g2) . [h1 > 0]
        backward_dense_seeds(G, L::LDH, net.w_headx_t + (size_t)h * (HID / 16) * (HID / 16) * 256, H2, L::LDH);
        backward_dense_seeds(G, L::LDH, net.w_pose2_t, H1, L::LDH);
        // gx = W0^T g1 (9 of 16 channels), one seed tile per wave; seed i = 3 h + wave keeps component i
        if (wave < XS) {
            const int nc[4] = {0, 0, 0, 0};
            f32x4 acc[4][1];
            mfma_tile<1, 1>(G, L::LDH, wave, net.w_pose0_t, HID / 16, 1, nc, acc);
            const int i = 3 * h + wave, q = i & 3;
            const float v = q == 0 ? acc[0][0].x : q == 1 ? acc[0][0].y : q == 2 ? acc[0][0].z : acc[0][0].w;
            if ((lane >> 4) == (i >> 2)) D[(lane & 15) * 12 + i] = v;
        }
        __syncthreads();  // G is rebuilt for the next head
    }
    for (int e = tid; e < DP * 12; e += DNT) {
        const int r = e / 12, j = e - r * 12;
        if (j < POSE) {
            O[e] = X0[r * L::LD0 + 12 + j] / (sigma + 1e-7f);
        } else if (j == 9) {
            float tr = 0.f;
#pragma unroll
            for (int i = 0; i < POSE; ++i) tr += D[r * 12 + i] / (sigma + 1e-7f);
            O[e] = tr;
        }
    }
    __syncthreads();
    return O;
}

}  // namespace gp_bwd
