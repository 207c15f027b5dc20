// Depth + instance mask -> per-instance point clouds on the device: the per-detection body of
// detect_mrcnn_genpose (runners/evaluation_single.py:162-216) - nearest-neighbour crop-and-resize of depth / mask / pixel
// coordinates to img x img (cv2.warpAffine fixed point, utils/datasets_utils.py:82-94), back-projection of the valid
// pixels (depth_to_pcl, :107-118) in raster order, then sample_points (:120-133).  Byte-sized work: one workgroup per
// detection, compaction in raster order of the crop so that the points come out in the reference's order.
#include "gp_common.h"
#include "philox.h"

namespace {

constexpr int AB_BITS = 10;  // OpenCV's fixed-point fraction for warpAffine coordinates

struct RoiArgs {
    int H, W, ninst, img;
    const uint16_t *depth;   // [H,W] millimetres, 0 = no reading
    const uint8_t *masks;    // [H,W,ninst] (Mask-RCNN layout), non-zero = inside the instance
    const double *minv;      // [ninst][6] destination -> source map (the INVERTED affine matrix, row major 2x3)
    float fx, fy, cx, cy;
    float *pcl;              // [ninst][img*img][3] metres, first count[i] rows valid
    int *count;              // [ninst] valid masked pixels
    int *depth_count;        // [ninst] pixels of the crop with a depth reading
};

// One 16-wave workgroup per detection.  Every wave owns a contiguous block of crop rows and walks it twice without any
// workgroup barrier in the loops: pass 1 counts its valid pixels, one barrier publishes the per-wave totals (= each
// wave's base offset in raster order), pass 2 recomputes the pixels and writes them at base + ballot prefix.
constexpr int ROI_WAVES = 16;

struct RoiPixel {
    bool valid, has_depth;
    int sx, sy;
    float d;
};

// Where a detection's pixels and its draw come from: the addressing argument of roi_pixel and of roi_sample_body.
struct RoiSrc {
    const uint16_t *depth;  // the detection's depth image [H,W]
    const uint8_t *mask;    // pixel 0 of the detection's channel = its mask block + the channel
    int stride;             // channels of that block = bytes from a pixel's entry to the next pixel's
    uint32_t run, slot;     // the draw's (run, slot) of philox.h (roi_sample_body alone)
};

__device__ __forceinline__ RoiPixel roi_pixel(const RoiArgs &a, const RoiSrc &src, long long X0, long long Y0, double m00, double m10, int x) {
    RoiPixel p{false, false, 0, 0, 0.f};
    if (x >= a.img) return p;
    // adelta[x] = cvRound(M00 * x * 1024), source = (X0 + adelta[x]) >> 10 (arithmetic shift), saturate_cast<short>
    long long sxl = (X0 + llrint(m00 * x * (double)(1 << AB_BITS))) >> AB_BITS;
    long long syl = (Y0 + llrint(m10 * x * (double)(1 << AB_BITS))) >> AB_BITS;
    sxl = sxl < -32768 ? -32768 : (sxl > 32767 ? 32767 : sxl);
    syl = syl < -32768 ? -32768 : (syl > 32767 ? 32767 : syl);
    if (sxl >= 0 && sxl < a.W && syl >= 0 && syl < a.H) {
        p.sx = (int)sxl, p.sy = (int)syl;
        const size_t q = (size_t)p.sy * a.W + p.sx;
        const uint16_t dv = src.depth[q];
        p.has_depth = dv > 0;
        p.d = (float)dv;
        p.valid = p.has_depth && src.mask[q * src.stride] != 0;
    }
    return p;
}

// depth_to_pcl, all float32: (x - cx) * d / fx, (y - cy) * d / fy, d; then / 1000
__device__ __forceinline__ void roi_point(const RoiArgs &a, const RoiPixel &p, float *o) {
    o[0] = (((float)p.sx - a.cx) * p.d / a.fx) / 1000.0f;
    o[1] = (((float)p.sy - a.cy) * p.d / a.fy) / 1000.0f;
    o[2] = p.d / 1000.0f;
}

__global__ __launch_bounds__(64 * ROI_WAVES) void roi_cloud_kernel(RoiArgs a) {
    __shared__ int wave_tot[ROI_WAVES], wave_dep[ROI_WAVES];
    const int inst = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *M = a.minv + (size_t)inst * 6;
    const double m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5];
    float *out = a.pcl + (size_t)inst * a.img * a.img * 3;
    const RoiSrc src{a.depth, a.masks + inst, a.ninst, 0, 0};
    const int rpw = (a.img + ROI_WAVES - 1) / ROI_WAVES;
    const int r0 = wave * rpw, r1 = (r0 + rpw < a.img) ? r0 + rpw : a.img;
    int cnt = 0, dep = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int off = 0;
        if (pass == 1) {
            if (lane == 0) wave_tot[wave] = cnt, wave_dep[wave] = dep;
            __syncthreads();
            for (int w = 0; w < wave; ++w) off += wave_tot[w];
        }
        for (int y = r0; y < r1; ++y) {
            // X0 = cvRound((M01*y + M02) * 1024) + 512   (rint = round half to even = cvRound)
            const long long X0 = llrint((m01 * y + m02) * (double)(1 << AB_BITS)) + (1 << (AB_BITS - 1));
            const long long Y0 = llrint((m11 * y + m12) * (double)(1 << AB_BITS)) + (1 << (AB_BITS - 1));
            for (int x0 = 0; x0 < a.img; x0 += 64) {
                const RoiPixel p = roi_pixel(a, src, X0, Y0, m00, m10, x0 + lane);
                const unsigned long long bal = __ballot(p.valid);
                if (pass == 0) {
                    cnt += __popcll(bal);
                    dep += __popcll(__ballot(p.has_depth));
                } else {
                    if (p.valid) roi_point(a, p, out + (size_t)(off + __popcll(bal & ((1ull << lane) - 1))) * 3);
                    off += __popcll(bal);
                }
            }
        }
    }
    if (threadIdx.x == 0) {
        int c = 0, d = 0;
        for (int w = 0; w < ROI_WAVES; ++w) c += wave_tot[w], d += wave_dep[w];
        a.count[inst] = c, a.depth_count[inst] = d;
    }
}

// sample_points: count < n -> tile (row k % count); count > n -> rows ids[k] (first n of a host permutation); else copy
__global__ void cloud_sample_kernel(int cap, int npts, const float *__restrict__ pcl, const int *__restrict__ count,
                                    const int32_t *__restrict__ ids, float *__restrict__ out) {
    const int inst = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= npts) return;
    const int c = count[inst];
    if (c <= 0) return;
    int src = c > npts ? (ids ? ids[(size_t)inst * npts + k] : k) : k % c;
    src = src < 0 ? 0 : (src >= c ? c - 1 : src);
    const float *s = pcl + ((size_t)inst * cap + src) * 3;
    float *o = out + ((size_t)inst * npts + k) * 3;
    o[0] = s[0], o[1] = s[1], o[2] = s[2];
}

// ---- gp_roi_sample_seeded: depth + masks -> the SAMPLED [n_pts, 3] clouds in one launch, no [img*img, 3] buffer in between.
// Pass 1 is roi_cloud_kernel's counting pass on the same roi_pixel, except that every (crop row, 64-column segment) keeps its ballot of
// valid pixels in LDS; an exclusive scan of the segments' popcounts in raster order gives every segment its base rank and the workgroup
// c (valid pixels) and d (pixels with depth).  Pass 2: output row k takes the valid pixel of rank
//     c < n: k % c (sample_points' tiling)     c == n: k     c > n: sigma(k)
// sigma: a keyed bijection of [0, c) - cycle walking over an alternating Feistel network of b = max(2, bit_length(c - 1)) bits whose
// round function is word 0 of a Philox block (philox.h, "THE DEPTH FRONT END'S DRAW") - so the n ranks are distinct by construction.
// The rank's segment is found by binary search in the scanned table, its column is the (rank - base)-th set bit of the ballot, the pixel
// is recomputed and written with roi_cloud_kernel's float expressions (roi_point): row k is bit for bit row `rank` of gp_roi_to_cloud.
constexpr int SAMPLE_MAX_IMG = 512;  // 512 rows x 8 segments: 32 KB of ballots + 16 KB of base ranks in LDS
constexpr int FEISTEL_ROUNDS = 8;

__device__ __forceinline__ uint32_t feistel_f(const gp_philox::Seed &sd, uint32_t slot, uint32_t u, uint32_t r) {
    uint32_t w[4] = {u, (slot & 0xFFFFFFu) | r << 24, sd.run, gp_philox::PRIOR_STEP << 3 | (uint32_t)gp_philox::STREAM_FRONT_END << 2};
    gp_philox::philox4x32_10(w, sd.k0, sd.k1);
    return w[0];
}

__device__ __forceinline__ uint32_t seeded_rank(const gp_philox::Seed &sd, uint32_t slot, uint32_t c, uint32_t k) {  // c > n > k
    const int b = max(2, 32 - __clz((int)(c - 1))), ha = b / 2, hb = b - ha;
    const uint32_t ma = (1u << ha) - 1, mb = (1u << hb) - 1;
    uint32_t x = k;
    do {  // (the walk stays on the cycle of a permutation of [0, 2^b) that holds k < c, so it ends; 2^b <= 2 c)
        uint32_t a = x >> hb, v = x & mb;
#pragma unroll 1
        for (uint32_t r = 0; r < FEISTEL_ROUNDS; r += 2) {
            a ^= feistel_f(sd, slot, v, r) & ma;
            v ^= feistel_f(sd, slot, a, r + 1) & mb;
        }
        x = a << hb | v;
    } while (x >= c);
    return x;
}

// Pass 1, the scan and pass 2 for detection `inst` of the launch (its minv row, its output rows), written once: roi_sample_kernel and
// roi_sample_frames_kernel differ in `src` alone.  a.depth, a.masks and a.ninst are not read here.
__device__ __forceinline__ void roi_sample_body(const RoiArgs &a, const RoiSrc &src, int inst, const uint32_t *__restrict__ seed, int npts,
                                                uint8_t *__restrict__ valid) {
    extern __shared__ unsigned long long seg_bal[];  // [nseg] ballots, then [nseg] int base ranks
    __shared__ int wave_tot[ROI_WAVES], wave_dep[ROI_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int segs = (a.img + 63) >> 6, nseg = a.img * segs;
    int *seg_base = reinterpret_cast<int *>(seg_bal + nseg);
    const double *M = a.minv + (size_t)inst * 6;
    const double m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5];
    // ---- pass 1: the segments go round the waves
    int dep = 0;
    for (int s = wave; s < nseg; s += ROI_WAVES) {
        const int y = s / segs, x0 = (s - y * segs) << 6;
        const long long X0 = llrint((m01 * y + m02) * (double)(1 << AB_BITS)) + (1 << (AB_BITS - 1));
        const long long Y0 = llrint((m11 * y + m12) * (double)(1 << AB_BITS)) + (1 << (AB_BITS - 1));
        const RoiPixel p = roi_pixel(a, src, X0, Y0, m00, m10, x0 + lane);
        const unsigned long long bal = __ballot(p.valid);
        dep += __popcll(__ballot(p.has_depth));
        if (lane == 0) seg_bal[s] = bal;
    }
    if (lane == 0) wave_dep[wave] = dep;
    __syncthreads();
    // ---- exclusive scan of the popcounts in raster order: a thread owns `per` consecutive segments
    const int per = (nseg + 64 * ROI_WAVES - 1) / (64 * ROI_WAVES), s0 = tid * per;
    int local = 0;
    for (int j = 0; j < per; ++j)
        if (s0 + j < nseg) local += __popcll(seg_bal[s0 + j]);
    int inc = local;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    int run = inc - local, c = 0, d = 0;
    for (int w = 0; w < ROI_WAVES; ++w) {
        if (w < wave) run += wave_tot[w];
        c += wave_tot[w], d += wave_dep[w];
    }
    for (int j = 0; j < per; ++j)
        if (s0 + j < nseg) {
            seg_base[s0 + j] = run;
            run += __popcll(seg_bal[s0 + j]);
        }
    __syncthreads();
    const bool ok = c > 1 && d > 1;  // evaluation_single.py:201-208
    if (tid == 0) a.count[inst] = c, a.depth_count[inst] = d, valid[inst] = ok;
    // ---- pass 2
    float *out = a.pcl + (size_t)inst * npts * 3;
    gp_philox::Seed sd = gp_philox::load_seed(seed);  // (the key; run and slot are the source's)
    sd.run = src.run;
    const uint32_t slot = src.slot;
    for (int k = tid; k < npts; k += 64 * ROI_WAVES) {
        float *o = out + (size_t)k * 3;
        if (!ok) {
            o[0] = o[1] = o[2] = 0.f;
            continue;
        }
        const int rank = c < npts ? k % c : (c == npts ? k : (int)seeded_rank(sd, slot, (uint32_t)c, (uint32_t)k));
        int lo = 0, hi = nseg - 1;  // the last segment whose base rank is <= rank (it holds the rank: the next base is above it)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (seg_base[mid] <= rank) lo = mid; else hi = mid - 1;
        }
        unsigned long long m = seg_bal[lo];
        int j = rank - seg_base[lo], pos = 0;  // the j-th set bit of the ballot
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) {
            const int below = __popcll(m & ((1ull << w) - 1));
            if (j >= below) j -= below, m >>= w, pos += w;
        }
        const int y = lo / segs, x = ((lo - y * segs) << 6) + pos;
        const long long X0 = llrint((m01 * y + m02) * (double)(1 << AB_BITS)) + (1 << (AB_BITS - 1));
        const long long Y0 = llrint((m11 * y + m12) * (double)(1 << AB_BITS)) + (1 << (AB_BITS - 1));
        roi_point(a, roi_pixel(a, src, X0, Y0, m00, m10, x), o);
    }
}

// One frame: the launch's detections are the channels of its one mask block; run and the slot of detection 0 from the seed state.
__global__ __launch_bounds__(64 * ROI_WAVES) void roi_sample_kernel(RoiArgs a, const uint32_t *__restrict__ seed, int npts, uint8_t *__restrict__ valid) {
    const int inst = blockIdx.x;
    const RoiSrc src{a.depth, a.masks + inst, a.ninst, seed[2], seed[4] + (uint32_t)inst};
    roi_sample_body(a, src, inst, seed, npts, valid);
}

// Many frames of one size: detection i's frame, channel, block and (run, slot) from the tables (genpose_hip.h, gp_roi_sample_frames).  An
// entry that does not name a channel of a block inside `masks` is a detection without a cloud - zero rows, zero counts, valid = 0 - decided
// by the whole workgroup before anything is read through it.
struct FrameTables {
    int nframes;
    long long mask_bytes;
    const long long *mask_off;  // [nframes]
    const int32_t *det;         // [ndet][3] frame, channel, channels of the frame's block
    const uint32_t *draw;       // [ndet][2] run, slot
};

__global__ __launch_bounds__(64 * ROI_WAVES) void roi_sample_frames_kernel(RoiArgs a, FrameTables t, const uint32_t *__restrict__ seed, int npts,
                                                                           uint8_t *__restrict__ valid) {
    const int inst = blockIdx.x;
    const int f = t.det[3 * inst], ch = t.det[3 * inst + 1], nf = t.det[3 * inst + 2];
    bool ok = f >= 0 && f < t.nframes && nf > 0 && ch >= 0 && ch < nf;
    long long off = 0;
    if (ok) {  // (H, W <= 32767 and nf < 2^31: the block's size stays below 2^61)
        off = t.mask_off[f];
        ok = off >= 0 && off <= t.mask_bytes && (long long)a.H * a.W * nf <= t.mask_bytes - off;
    }
    if (!ok) {
        float *out = a.pcl + (size_t)inst * npts * 3;
        for (int k = threadIdx.x; k < npts; k += 64 * ROI_WAVES) out[(size_t)k * 3] = out[(size_t)k * 3 + 1] = out[(size_t)k * 3 + 2] = 0.f;
        if (threadIdx.x == 0) a.count[inst] = 0, a.depth_count[inst] = 0, valid[inst] = 0;
        return;
    }
    const RoiSrc src{a.depth + (size_t)f * a.H * a.W, a.masks + off + ch, nf, t.draw[2 * inst], t.draw[2 * inst + 1]};
    roi_sample_body(a, src, inst, seed, npts, valid);
}

}  // namespace

extern "C" {

int gp_roi_to_cloud(int h, int w, int ninst, int img, const uint16_t *depth, const uint8_t *masks, const double *minv, float fx, float fy,
                    float cx, float cy, float *pcl, int32_t *count, int32_t *depth_count, gp_stream_t s) {
    if (h <= 0 || w <= 0 || ninst < 0 || img <= 0 || !depth || !masks || !minv || !pcl || !count || !depth_count) return GP_EINVAL;
    if (h > 32767 || w > 32767) return GP_EINVAL;
    if (ninst == 0) return GP_OK;
    RoiArgs a{h, w, ninst, img, depth, masks, minv, fx, fy, cx, cy, pcl, count, depth_count};
    hipLaunchKernelGGL(roi_cloud_kernel, dim3(ninst), dim3(64 * ROI_WAVES), 0, (hipStream_t)s, a);
    return gp_launch_status();
}

int gp_cloud_sample(int ninst, int cap, int npts, const float *pcl, const int32_t *count, const int32_t *ids, float *out, gp_stream_t s) {
    if (ninst < 0 || cap <= 0 || npts <= 0 || !pcl || !count || !out) return GP_EINVAL;
    if (ninst == 0) return GP_OK;
    hipLaunchKernelGGL(cloud_sample_kernel, dim3((npts + 255) / 256, ninst), dim3(256), 0, (hipStream_t)s, cap, npts, pcl, count, ids, out);
    return gp_launch_status();
}

int gp_roi_sample_seeded(int h, int w, int ninst, int img, int npts, const uint16_t *depth, const uint8_t *masks, const double *minv, float fx,
                         float fy, float cx, float cy, const uint32_t *seed_state, float *out, int32_t *count, int32_t *depth_count, uint8_t *valid,
                         gp_stream_t s) {
    if (h <= 0 || w <= 0 || ninst < 0 || img <= 0 || npts <= 0 || !depth || !masks || !minv || !seed_state || !out || !count || !depth_count || !valid)
        return GP_EINVAL;
    if (h > 32767 || w > 32767 || img > SAMPLE_MAX_IMG) return GP_EINVAL;
    if (ninst == 0) return GP_OK;
    RoiArgs a{h, w, ninst, img, depth, masks, minv, fx, fy, cx, cy, out, count, depth_count};
    const size_t lds = (size_t)img * ((img + 63) / 64) * (sizeof(unsigned long long) + sizeof(int));
    hipLaunchKernelGGL(roi_sample_kernel, dim3(ninst), dim3(64 * ROI_WAVES), lds, (hipStream_t)s, a, seed_state, npts, valid);
    return gp_launch_status();
}

int gp_roi_sample_frames(int h, int w, int nframes, int ndet, int img, int npts, const uint16_t *depth, const uint8_t *masks, int64_t mask_bytes,
                         const int64_t *mask_off, const int32_t *det, const uint32_t *draw, const double *minv, float fx, float fy, float cx, float cy,
                         const uint32_t *seed_state, float *out, int32_t *count, int32_t *depth_count, uint8_t *valid, gp_stream_t s) {
    if (h <= 0 || w <= 0 || ndet < 0 || img <= 0 || npts <= 0 || mask_bytes < 0 || !depth || !masks || !mask_off || !det || !draw || !minv || !seed_state ||
        !out || !count || !depth_count || !valid)
        return GP_EINVAL;
    if (h > 32767 || w > 32767 || img > SAMPLE_MAX_IMG) return GP_EINVAL;
    if (ndet == 0) return GP_OK;
    if (nframes <= 0) return GP_EINVAL;
    RoiArgs a{h, w, ndet, img, depth, masks, minv, fx, fy, cx, cy, out, count, depth_count};
    FrameTables t{nframes, (long long)mask_bytes, (const long long *)mask_off, det, draw};
    const size_t lds = (size_t)img * ((img + 63) / 64) * (sizeof(unsigned long long) + sizeof(int));
    hipLaunchKernelGGL(roi_sample_frames_kernel, dim3(ndet), dim3(64 * ROI_WAVES), lds, (hipStream_t)s, a, t, seed_state, npts, valid);
    return gp_launch_status();
}

}  // extern "C"
