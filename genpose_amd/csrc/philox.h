// Counter-based Gaussian noise of the predictor-corrector sampler (replaces the two torch.randn_like draws of cond_pc_sampler,
// samplers.py:132,149, when the sampler is seeded): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as
// 1, 2, 3", SC'11) keyed by the seed, counted by (global row, run, step, stream, block), Box-Muller on top.  A row's draws depend on
// those fields only - not on the launch plan, the batch it shares a launch with or the shard it runs on - and live in registers.
//
// Counter and key (the one layout; DESIGN.md, "seeded noise"; tests/philox_reference.py restates it):
//     key[0], key[1]  = seed bits 0..31, 32..63
//     ctr[0], ctr[1]  = GLOBAL row index bits 0..31, 32..63
//     ctr[2]          = run index (32 bits)
//     ctr[3]          = step << 3 | stream << 2 | block      step < 2^29; stream 0 = Langevin corrector, 1 = predictor; block 0..2
// Every field has its own bits, so two different field tuples never share a (counter, key).
// THE TRACKER'S PRIOR (gp_track_warm_start, gp_track_prior_fill: the draw of samplers.py:180; tests/track_prior_reference.py restates it) has
// the same layout with the step field RESERVED: step = PRIOR_STEP = 2^29 - 1, stream 0, run index = the FRAME index, global row =
// (sequence * objects per frame + object) * K + candidate.  The seeded PC samplers take nsteps < 2^29, so their steps end at 2^29 - 2:
// no PC draw of a sampler shares a (counter, key) with the prior.
// THE DEPTH FRONT END'S DRAW (gp_roi_sample_seeded, preprocess.hip: which n_pts of a detection's c valid pixels form its cloud;
// genpose_amd.preprocess.seeded_ranks restates it) takes the reserved step with STREAM 1, block 0.  It uses the generator as the round
// function F(u, r) of a Feistel network, not as a source of normals: F = output word 0 of the block with
//     ctr[0] = u (the half of the Feistel state that is read)      ctr[1] = (slot & 0xFFFFFF) | r << 24      (round r < 8)
//     ctr[2] = run index (the FRAME index)                         ctr[3] = PRIOR_STEP << 3 | 1 << 2 | 0
// slot = the detection's global slot = seed state word [4] + instance of the launch (a tracker: sequence * objects per frame + object).
// The prior draws on stream 0 of that step and no PC step reaches it, so the stream bit alone keeps these (counter, key) apart from both.
// One row, stream and step take three blocks = 12 words w[0..11]; pair k = (w[2k], w[2k+1]) gives
//     u1 = ((w[2k] >> 8) + 1) * 2^-24,  u2 = ((w[2k+1] >> 8) + 1) * 2^-24        both in (0, 1]
//     z[2k] = sqrt(-2 log u1) * cos(2 pi u2),  z[2k+1] = sqrt(-2 log u1) * sin(2 pi u2)
// and the row keeps z[0..8] (of the sixth pair nothing is used).  TRUNCATION: u1 >= 2^-24, so log u1 is finite and
// |z| <= sqrt(48 log 2) = 5.768: the tails beyond 5.77 sigma (probability 8e-9 per draw) are absent.
// logf / sqrtf / sincosf are the precise library functions: a few hundred VALU operations per row against the trunk's 0.53 MFLOP.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gp_philox {

constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
constexpr int STREAM_LANGEVIN = 0, STREAM_PREDICTOR = 1;
constexpr uint32_t MAX_STEPS = 1u << 29;
constexpr uint32_t PRIOR_STEP = MAX_STEPS - 1;  // the tracker's prior (header comment)
constexpr int STREAM_PRIOR = 0, STREAM_FRONT_END = 1;  // the two users of the reserved step

// The seed state in device memory (8 words, written by the host in stream order before a replay; the kernels only read it):
//     [0], [1] seed lo / hi   [2] run index   [3] 0   [4], [5] row base lo / hi (global row = row base + row of the launch)   [6], [7] 0
constexpr int SEED_WORDS = 8;
struct Seed {
    uint32_t k0, k1, run;
    uint64_t row_base;
};
__device__ __forceinline__ Seed load_seed(const uint32_t *__restrict__ s) {
    Seed sd;
    sd.k0 = s[0], sd.k1 = s[1], sd.run = s[2];
    sd.row_base = (uint64_t)s[4] | ((uint64_t)s[5] << 32);
    return sd;
}

__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0], hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
        c[0] = hi1 ^ c[1] ^ k0, c[1] = lo1, c[2] = hi0 ^ c[3] ^ k1, c[3] = lo0;
        k0 += W0, k1 += W1;
    }
}

// block `blk` of (row, run, step, stream): four raw words
__device__ __forceinline__ void block_words(const Seed &sd, uint32_t step, int stream, int blk, uint64_t row, uint32_t (&w)[4]) {
    w[0] = (uint32_t)row, w[1] = (uint32_t)(row >> 32), w[2] = sd.run, w[3] = step << 3 | (uint32_t)stream << 2 | (uint32_t)blk;
    philox4x32_10(w, sd.k0, sd.k1);
}

__device__ __forceinline__ float uniform24(uint32_t w) { return (float)((w >> 8) + 1u) * 5.9604644775390625e-8f; }  // (0, 1]

// The nine normals of global row `row` for one stream at one step (step = index into the reference's loop, 0 .. nsteps - 1).
__device__ __forceinline__ void draw9(const Seed &sd, uint32_t step, int stream, uint64_t row, float (&z)[9]) {
    float v[10];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        uint32_t w[4];
        block_words(sd, step, stream, b, row, w);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * b + h;
            if (k >= 5) continue;
            const float r = sqrtf(-2.f * logf(uniform24(w[2 * h])));
            float sn, cs;
            sincosf(6.2831854820251465f * uniform24(w[2 * h + 1]), &sn, &cs);
            v[2 * k] = r * cs, v[2 * k + 1] = r * sn;
        }
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) z[j] = v[j];
}

}  // namespace gp_philox
