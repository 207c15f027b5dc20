// Vanilla PointNet encoder (networks/pts_encoder/pointnets.py:45-123, PointNetfeat without BatchNorm): the per-point MLP chains of the
// input transform net (3 -> 64 -> 128 -> 1024) and of the trunk (3 -> 64 -> 128 -> 512 -> 1024) with the maximum over the cloud's points,
// and the small-row dense layer of the transform net's head and of the agent's fusion layer.
//
// One workgroup (4 waves) owns a tile of PN_P = 48 points of ONE cloud.  The layers before the last one go LDS -> LDS through
// dense_to_lds_w (gp_common.h: fp32 MFMA, packed weights streamed L2 -> registers through the three-stage pipeline, bias after the
// product, ReLU); their activations never leave the CU.  The last layer (-> 1024) keeps its outputs in the accumulators: rows that pad the
// tile are masked to -inf, the maximum over the tile's rows is taken in registers, and the tiles of a cloud combine through an integer
// atomic max on an ORDER-PRESERVING KEY of the float (the trunk's pooled values are signed: conv4 has no ReLU), into a buffer zeroed
// by a kernel in front (0 is below every key).  A last small kernel turns the keys back into floats and adds the last layer's bias, once
// per channel and after the pooling (exact: rounding is monotone, max_j fl(a_j + b) = fl(max_j a_j + b)) - and the ReLU of the
// transform net's conv3 likewise.  Neither [b, n, 1024] nor [b, n, 512] exists outside LDS / registers.
//
// 48 rows: the trunk's [48][512 + 8] conv3 output and [48][128 + 8] conv2 output fill 123 KB of the CU's 160 KB LDS (64 rows do not fit);
// every wave then multiplies 4 channel chunks x 3 row chunks per weight fragment it loads (12 MFMAs per 4 global_load_dwordx4).
#include "gp_common.h"

namespace {

constexpr int PN_P = 48;        // points per tile
constexpr int PN_PT = PN_P / 16;
constexpr int PN_COUT = 1024;   // pooled width of both chains
constexpr int PN_LD0 = 16 + GP_LD_PAD, PN_LD1 = 64 + GP_LD_PAD, PN_LD2 = 128 + GP_LD_PAD, PN_LD3 = 512 + GP_LD_PAD;

struct PNArgs {
    int n, ntiles;
    const float *xyz, *trans;
    const float *w1, *b1, *w2, *b2, *w3, *b3, *w4;
    unsigned *keys;
};

// float -> unsigned whose integer order is the float order (negative values: all bits flipped, others: sign bit set); 0 is below every key
__device__ __forceinline__ unsigned order_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// Last layer over the tile in LDS: [PN_P rows] x K -> 1024 channels, bias-free; the maximum over the tile's first `nvalid` rows goes to
// keys[0..1023] by atomic max.  Wave w computes chunks w, w + 4, ... (four at a time) over all three row chunks.
__device__ __forceinline__ void pooled_last_layer(const float *Xs, int ld, const float *__restrict__ Wp, int K, int nvalid, unsigned *keys) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int KG = K / 16, NC = PN_COUT / 16;
    const float ninf = -__builtin_inff();
    for (int ncb = wave; ncb < NC; ncb += 16) {
        const int nc[4] = {ncb, ncb + 4, ncb + 8, ncb + 12};
        f32x4 acc[4][PN_PT];
        mfma_tile<4, PN_PT>(Xs, ld, 0, Wp, KG, NC, nc, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 m = f32x4{ninf, ninf, ninf, ninf};
#pragma unroll
            for (int p = 0; p < PN_PT; ++p) {
                const bool valid = p * 16 + (lane & 15) < nvalid;  // D fragment: lane = row p * 16 + (lane & 15), registers = four channels
                m.x = fmaxf(m.x, valid ? acc[i][p].x : ninf);
                m.y = fmaxf(m.y, valid ? acc[i][p].y : ninf);
                m.z = fmaxf(m.z, valid ? acc[i][p].z : ninf);
                m.w = fmaxf(m.w, valid ? acc[i][p].w : ninf);
            }
            m.x = row16_max(m.x);
            m.y = row16_max(m.y);
            m.z = row16_max(m.z);
            m.w = row16_max(m.w);
            // every lane of a 16-lane row now holds the four maxima of channels nc * 16 + 4 (lane >> 4) + 0..3: lanes 0..3 of the row store one each
            const int r = lane & 15;
            const float v = r == 0 ? m.x : (r == 1 ? m.y : (r == 2 ? m.z : m.w));
            if (r < 4) atomicMax(keys + nc[i] * 16 + 4 * (lane >> 4) + r, order_key(v));
        }
    }
}

// TRUNK = false: the transform net's chain  relu(conv1) relu(conv2) [conv3 pooled]          (pointnets.py:60-63)
// TRUNK = true:  x . trans, relu(conv1) relu(conv2) relu(conv3) [conv4 pooled]              (pointnets.py:101-117)
template <bool TRUNK>
__global__ __launch_bounds__(256) void pointnet_pool_kernel(PNArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int cloud = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const int p0 = tile * PN_P;
    const int nvalid = a.n - p0 < PN_P ? a.n - p0 : PN_P;
    // LDS: [big region: X0 | H1, later H3 (trunk)] [H2]
    float *X0 = smem;                          // [PN_P][PN_LD0]
    float *H1 = smem + PN_P * PN_LD0;          // [PN_P][PN_LD1]
    float *H3 = smem;                          // [PN_P][PN_LD3], trunk only: written when X0 and H1 are dead
    float *H2 = smem + (TRUNK ? PN_P * PN_LD3 : PN_P * (PN_LD0 + PN_LD1));  // [PN_P][PN_LD2]

    // the tile's points as rows of 16 floats (x, y, z, zeros): conv1 is a K = 16 MFMA layer with zero-padded weights.  Rows past the
    // cloud's end are zero points - finite values all the way down, masked out of the maximum at the end.
    for (int e = threadIdx.x; e < PN_P * 16; e += 256) {
        const int r = e >> 4, c = e & 15;
        float v = 0.f;
        if (c < 3 && r < nvalid) {
            const float *x = a.xyz + ((size_t)cloud * a.n + p0 + r) * 3;
            if constexpr (TRUNK) {
                const float *t = a.trans + (size_t)cloud * 9;  // torch.bmm(x, trans): x'[c] = sum_i x[i] trans[i][c]
                v = x[0] * t[c] + x[1] * t[3 + c] + x[2] * t[6 + c];
            } else {
                v = x[c];
            }
        }
        X0[r * PN_LD0 + c] = v;
    }
    __syncthreads();
    dense_to_lds_w<PN_PT, 4, true>(X0, PN_LD0, a.w1, a.b1, 3, 64, H1, PN_LD1);
    __syncthreads();
    dense_to_lds_w<PN_PT, 4, true>(H1, PN_LD1, a.w2, a.b2, 64, 128, H2, PN_LD2);
    __syncthreads();
    unsigned *keys = a.keys + (size_t)cloud * PN_COUT;
    if constexpr (TRUNK) {
        dense_to_lds_w<PN_PT, 4, true>(H2, PN_LD2, a.w3, a.b3, 128, 512, H3, PN_LD3);
        __syncthreads();
        pooled_last_layer(H3, PN_LD3, a.w4, 512, nvalid, keys);
    } else {
        pooled_last_layer(H2, PN_LD2, a.w3, 128, nvalid, keys);
    }
}

__global__ void pointnet_zero_keys_kernel(unsigned *keys, size_t count4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count4) reinterpret_cast<uint4 *>(keys)[i] = uint4{0u, 0u, 0u, 0u};
}

// keys -> floats in place, + the pooled layer's bias, ReLU where the layer has one
template <bool RELU>
__global__ void pointnet_finish_kernel(float *out, const float *__restrict__ bias, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float v = order_key_value(reinterpret_cast<const unsigned *>(out)[i]) + bias[i % PN_COUT];
    out[i] = RELU ? fmaxf(v, 0.f) : v;
}

constexpr size_t lds_floats(bool trunk) { return trunk ? (size_t)PN_P * (PN_LD3 + PN_LD2) : (size_t)PN_P * (PN_LD0 + PN_LD1 + PN_LD2); }
static_assert(lds_floats(true) * sizeof(float) <= 160 * 1024, "trunk tile must fit the CU's LDS");
static_assert(PN_P * (PN_LD0 + PN_LD1) <= PN_P * PN_LD3, "X0 and H1 alias the H3 region");

template <bool TRUNK>
int launch_pool(PNArgs a, int b, const float *bias_last, float *out, hipStream_t st) {
    const long long blocks = (long long)b * a.ntiles;
    if (blocks > 0x7fffffffLL) return GP_EINVAL;
    constexpr size_t lds = lds_floats(TRUNK) * sizeof(float);
    if (lds > 64 * 1024 && gp_prepare_lds<pointnet_pool_kernel<TRUNK>>(lds)) return GP_ELAUNCH;
    const size_t count = (size_t)b * PN_COUT;
    hipLaunchKernelGGL(pointnet_zero_keys_kernel, dim3((unsigned)((count / 4 + 255) / 256)), dim3(256), 0, st, a.keys, count / 4);
    hipLaunchKernelGGL(pointnet_pool_kernel<TRUNK>, dim3((unsigned)blocks), dim3(256), lds, st, a);
    hipLaunchKernelGGL(pointnet_finish_kernel<!TRUNK>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, out, bias_last, count);
    return gp_launch_status();
}

// out[row][c] = act(bias[c] + sum_k x[row][k] W[c][k]) with x = [xa | xb] (the second part optional): one wave owns DR_NT channels x
// DR_RT rows, the lanes stride over k four floats at a time, fixed-order wave sum at the end.  Rows / channels past the end are clamped
// for the loads and not stored.
constexpr int DR_NT = 4, DR_RT = 8;

__global__ __launch_bounds__(256) void dense_rows_kernel(int rows, int ka, int kb, int n_out, const float *__restrict__ xa, const float *__restrict__ xb,
                                                         const float *__restrict__ W, const float *__restrict__ bias, int act, float *__restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = (blockIdx.x * 4 + wave) * DR_NT, r0 = blockIdx.y * DR_RT;
    if (c0 >= n_out) return;
    const int K = ka + kb;
    float acc[DR_NT][DR_RT];
#pragma unroll
    for (int c = 0; c < DR_NT; ++c)
#pragma unroll
        for (int r = 0; r < DR_RT; ++r) acc[c][r] = 0.f;
    const float *wrow[DR_NT];
#pragma unroll
    for (int c = 0; c < DR_NT; ++c) wrow[c] = W + (size_t)(c0 + c < n_out ? c0 + c : n_out - 1) * K;
    for (int part = 0; part < 2; ++part) {
        const float *x = part ? xb : xa;
        const int kp = part ? kb : ka, koff = part ? ka : 0;
        for (int k = lane * 4; k < kp; k += 256) {
            f32x4 w[DR_NT];
#pragma unroll
            for (int c = 0; c < DR_NT; ++c) w[c] = *reinterpret_cast<const f32x4 *>(wrow[c] + koff + k);
#pragma unroll
            for (int r = 0; r < DR_RT; ++r) {
                const int row = r0 + r < rows ? r0 + r : rows - 1;
                const f32x4 v = *reinterpret_cast<const f32x4 *>(x + (size_t)row * kp + k);
#pragma unroll
                for (int c = 0; c < DR_NT; ++c) acc[c][r] += (w[c].x * v.x + w[c].y * v.y) + (w[c].z * v.z + w[c].w * v.w);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < DR_NT; ++c)
#pragma unroll
        for (int r = 0; r < DR_RT; ++r) {
            const float s = wave_sum_f32(acc[c][r]);
            if (lane == 0 && c0 + c < n_out && r0 + r < rows) {
                const float v = s + bias[c0 + c];
                out[(size_t)(r0 + r) * n_out + c0 + c] = act == GP_ACT_RELU ? fmaxf(v, 0.f) : v;
            }
        }
}

}  // namespace

extern "C" {

int gp_pointnet_stn_pool(int b, int n, const float *xyz, const float *wpack1, const float *bias1, const float *wpack2, const float *bias2,
                         const float *wpack3, const float *bias3, float *g, gp_stream_t s) {
    if (b < 0 || n <= 0 || !xyz || !wpack1 || !bias1 || !wpack2 || !bias2 || !wpack3 || !bias3 || !g) return GP_EINVAL;
    if (b == 0) return GP_OK;
    PNArgs a{n, (n + PN_P - 1) / PN_P, xyz, nullptr, wpack1, bias1, wpack2, bias2, wpack3, nullptr, nullptr, reinterpret_cast<unsigned *>(g)};
    return launch_pool<false>(a, b, bias3, g, (hipStream_t)s);
}

int gp_pointnet_feat_pool(int b, int n, const float *xyz, const float *trans, const float *wpack1, const float *bias1, const float *wpack2,
                          const float *bias2, const float *wpack3, const float *bias3, const float *wpack4, const float *bias4, float *feat,
                          gp_stream_t s) {
    if (b < 0 || n <= 0 || !xyz || !trans || !wpack1 || !bias1 || !wpack2 || !bias2 || !wpack3 || !bias3 || !wpack4 || !bias4 || !feat) return GP_EINVAL;
    if (b == 0) return GP_OK;
    PNArgs a{n, (n + PN_P - 1) / PN_P, xyz, trans, wpack1, bias1, wpack2, bias2, wpack3, bias3, wpack4, reinterpret_cast<unsigned *>(feat)};
    return launch_pool<true>(a, b, bias4, feat, (hipStream_t)s);
}

int gp_dense_rows(int rows, int k_a, int k_b, int n_out, const float *xa, const float *xb, const float *W, const float *bias, int act, float *out,
                  gp_stream_t s) {
    if (rows < 0 || k_a <= 0 || (k_a & 3) || k_b < 0 || (k_b & 3) || n_out <= 0 || !xa || (k_b > 0 && !xb) || !W || !bias || !out) return GP_EINVAL;
    if (act != GP_ACT_NONE && act != GP_ACT_RELU) return GP_EINVAL;
    if (rows == 0) return GP_OK;
    const int row_tiles = (rows + DR_RT - 1) / DR_RT;
    if (row_tiles > 65535) return GP_EINVAL;
    hipLaunchKernelGGL(dense_rows_kernel, dim3((n_out + 4 * DR_NT - 1) / (4 * DR_NT), row_tiles), dim3(256), 0, (hipStream_t)s, rows, k_a, k_b, n_out, xa,
                       xb, W, bias, act, out);
    return gp_launch_status();
}

}  // extern "C"
