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
__device__ __forceinline__ void pixel_point(float fx, float fy, float cx, float cy, const RoiPixel &p, float *o) {
    o[0] = (((float)p.sx - cx) * p.d / fx) / 1000.0f;
    o[1] = (((float)p.sy - cy) * p.d / fy) / 1000.0f;
    o[2] = p.d / 1000.0f;
}
__device__ __forceinline__ void roi_point(const RoiArgs &a, const RoiPixel &p, float *o) { pixel_point(a.fx, a.fy, a.cx, a.cy, p, o); }

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

// Pass 1, the scan and pass 2 over a grid of rows x cols candidate pixels, written once; `src` says where a pixel's validity and point
// come from and where the counts go:
//     src.row(y) -> Row            what a grid row's pixels share
//     src.pixel(row, x) -> RoiPixel   grid pixel (x, y): its source pixel, depth and validity (x >= cols: not valid)
//     src.point(pixel, o)          the valid pixel's point
//     src.publish(c, d) -> bool    the workgroup's counts (valid pixels, pixels with depth) -> whether the rows are written; thread 0 stores
// Output row k takes the valid pixel of rank r in the grid's raster order (c < npts: k % c, c == npts: k, else the seeded walk of (run, slot)).
template <class Src>
__device__ __forceinline__ void sample_body(const Src &src, int rows, int cols, const uint32_t *__restrict__ seed, uint32_t draw_run, uint32_t slot, int npts,
                                            float *__restrict__ out) {
    extern __shared__ unsigned long long seg_bal[];  // [nseg] ballots, then [nseg] int base ranks
    __shared__ int wave_tot[ROI_WAVES], wave_dep[ROI_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int segs = (cols + 63) >> 6, nseg = rows * segs;
    int *seg_base = reinterpret_cast<int *>(seg_bal + nseg);
    // ---- pass 1: the segments go round the waves
    int dep = 0;
    for (int s = wave; s < nseg; s += ROI_WAVES) {
        const int y = s / segs, x0 = (s - y * segs) << 6;
        const RoiPixel p = src.pixel(src.row(y), x0 + lane);
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
    const bool ok = src.publish(c, d);
    // ---- pass 2
    gp_philox::Seed sd = gp_philox::load_seed(seed);  // (the key; run and slot are the source's)
    sd.run = draw_run;
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
        src.point(src.pixel(src.row(y), x), o);
    }
}

// The mask front end's source: the img x img crop of detection `inst` (its minv row), validity = depth & mask.
struct RoiCrop {
    const RoiArgs &a;
    const RoiSrc &src;
    int inst;
    uint8_t *valid;
    double m00, m01, m02, m10, m11, m12;
    struct Row {
        long long X0, Y0;
    };
    __device__ __forceinline__ RoiCrop(const RoiArgs &a_, const RoiSrc &src_, int inst_, uint8_t *valid_) : a(a_), src(src_), inst(inst_), valid(valid_) {
        const double *M = a.minv + (size_t)inst * 6;
        m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5];
    }
    __device__ __forceinline__ Row row(int y) const {
        return Row{llrint((m01 * y + m02) * (double)(1 << AB_BITS)) + (1 << (AB_BITS - 1)), llrint((m11 * y + m12) * (double)(1 << AB_BITS)) + (1 << (AB_BITS - 1))};
    }
    __device__ __forceinline__ RoiPixel pixel(const Row &r, int x) const { return roi_pixel(a, src, r.X0, r.Y0, m00, m10, x); }
    __device__ __forceinline__ void point(const RoiPixel &p, float *o) const { roi_point(a, p, o); }
    __device__ __forceinline__ bool publish(int c, int d) const {
        const bool ok = c > 1 && d > 1;  // evaluation_single.py:201-208
        if (threadIdx.x == 0) a.count[inst] = c, a.depth_count[inst] = d, valid[inst] = ok;
        return ok;
    }
};

// roi_sample_kernel and roi_sample_frames_kernel differ in `src` alone.  a.depth, a.masks and a.ninst are not read here.
__device__ __forceinline__ void roi_sample_body(const RoiArgs &a, const RoiSrc &src, int inst, const uint32_t *__restrict__ seed, int npts,
                                                uint8_t *__restrict__ valid) {
    sample_body(RoiCrop(a, src, inst, valid), a.img, a.img, seed, src.run, src.slot, npts, a.pcl + (size_t)inst * npts * 3);
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

// ---- mask-free tracking (ours): an object's cloud from a depth frame and its previous pose, gp_cloud_extent + gp_box_sample.
// THE OBJECT-FRAME EXPRESSION, written once for both kernels: camera-frame point p, pose rt (row major 4x4, object -> camera) ->
//     u_j = p_j - t_j      q_j = ((u_0 R[0][j]) + (u_1 R[1][j])) + (u_2 R[2][j])
// every product and sum its own float32 rounding (no contraction): numpy float32 restates it bit for bit, and a point that
// gp_cloud_extent measured at |q_j| <= half_j is a point gp_box_sample finds inside the box of those half-extents.
struct ObjPose {
    float R[3][3], t[3];
};
__device__ __forceinline__ ObjPose load_pose(const float *__restrict__ rt) {
    ObjPose m;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) m.R[i][j] = rt[4 * i + j];
        m.t[i] = rt[4 * i + 3];
    }
    return m;
}
__device__ __forceinline__ void object_frame(const ObjPose &m, const float *p, float *q) {
    const float u0 = __fsub_rn(p[0], m.t[0]), u1 = __fsub_rn(p[1], m.t[1]), u2 = __fsub_rn(p[2], m.t[2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] = __fadd_rn(__fadd_rn(__fmul_rn(u0, m.R[0][j]), __fmul_rn(u1, m.R[1][j])), __fmul_rn(u2, m.R[2][j]));
}

// gp_cloud_extent: one wave per cloud, PER points per lane in registers (point k = i * 64 + lane), the three |q_j| as their bit patterns -
// non-negative floats order like them.  The (trim + 1)-th largest is the largest v with #{a >= v} >= trim + 1: built bit by bit from the
// top value bit, 31 trips of PER ballots per axis whatever the data.  Slots past n hold 0 and no candidate is 0, so they never count.
template <int PER>
__global__ __launch_bounds__(64) void cloud_extent_kernel(int n, const float *__restrict__ pts, const float *__restrict__ rt, int trim,
                                                          const int8_t *__restrict__ sym, float *__restrict__ half_out) {
    const int cloud = blockIdx.x, lane = threadIdx.x;
    const ObjPose m = load_pose(rt + (size_t)cloud * 16);
    const bool radial = sym && sym[cloud] != 0;
    const float *P = pts + (size_t)cloud * n * 3;
    uint32_t a[3][PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int k = i * 64 + lane;
        a[0][i] = a[1][i] = a[2][i] = 0u;
        if (k < n) {
            const float p[3] = {P[3 * k], P[3 * k + 1], P[3 * k + 2]};
            float q[3];
            object_frame(m, p, q);
            // (sqrtf: the correctly rounded root, np.sqrt's bits - __fsqrt_rn is the native approximation on this target, an ulp off)
            if (radial) q[0] = q[2] = sqrtf(__fadd_rn(__fmul_rn(q[0], q[0]), __fmul_rn(q[2], q[2])));
#pragma unroll
            for (int j = 0; j < 3; ++j) a[j][i] = __float_as_uint(q[j]) & 0x7FFFFFFFu;
        }
    }
    const int need = trim + 1;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        uint32_t v = 0;
#pragma unroll 1
        for (int bit = 30; bit >= 0; --bit) {
            const uint32_t cand = v | 1u << bit;
            int cnt = 0;
#pragma unroll
            for (int i = 0; i < PER; ++i) cnt += __popcll(__ballot(a[j][i] >= cand));
            if (cnt >= need) v = cand;
        }
        if (lane == 0) half_out[3 * cloud + j] = __uint_as_float(v);
    }
}

// gp_box_sample: the grid is the pixel rectangle of the box's projection (only an accelerator: a superset of the inside pixels), a pixel is
// valid when it has depth and its point lies inside the oriented box - decided on the point pixel_point gives, through object_frame.
constexpr int BOX_MAX_SEGS = 8192;    // 12 bytes a segment: 96 KB of the CU's 160 KB
constexpr float BOX_NEAR = 0.05f;     // a corner nearer than this (metres): the projection is no bound, the grid is the whole image
constexpr float BOX_ORTHO_TOL = 1e-5f;  // |R^T R - I| above this: rt is no rotation and its corners no bound, the grid is the whole image

struct BoxArgs {
    int H, W, nframes, npts, min_count;
    const uint16_t *depth;
    const int32_t *frame_of;
    const float *rt, *half;
    float inflate, pad, fx, fy, cx, cy;
    const uint32_t *draw;
    float *points;
    int32_t *count;
    uint8_t *valid;
};

struct BoxGrid {
    const BoxArgs &a;
    const uint16_t *depth;  // the object's frame
    ObjPose m;
    float hh[3];
    int x0, y0, cols, inst;
    bool fin;
    struct Row {
        int sy;
    };
    __device__ __forceinline__ BoxGrid(const BoxArgs &a_) : a(a_) {}
    __device__ __forceinline__ Row row(int y) const { return Row{y0 + y}; }
    __device__ __forceinline__ RoiPixel pixel(const Row &r, int x) const {
        RoiPixel p{false, false, 0, 0, 0.f};
        if (x >= cols) return p;
        p.sx = x0 + x, p.sy = r.sy;
        const uint16_t dv = depth[(size_t)p.sy * a.W + p.sx];
        p.d = (float)dv;
        if (dv > 0) {
            float pt[3], q[3];
            pixel_point(a.fx, a.fy, a.cx, a.cy, p, pt);
            object_frame(m, pt, q);
            p.valid = p.has_depth = fabsf(q[0]) <= hh[0] && fabsf(q[1]) <= hh[1] && fabsf(q[2]) <= hh[2];
        }
        return p;
    }
    __device__ __forceinline__ void point(const RoiPixel &p, float *o) const { pixel_point(a.fx, a.fy, a.cx, a.cy, p, o); }
    __device__ __forceinline__ bool publish(int c, int) const {
        const bool ok = fin && c >= (a.min_count > 2 ? a.min_count : 2);
        if (threadIdx.x == 0) a.count[inst] = c, a.valid[inst] = ok;
        return ok;
    }
};

__global__ __launch_bounds__(64 * ROI_WAVES) void box_sample_kernel(BoxArgs a, const uint32_t *__restrict__ seed) {
    const int inst = blockIdx.x;
    float *out = a.points + (size_t)inst * a.npts * 3;
    BoxGrid g(a);
    g.inst = inst;
    const int f = a.frame_of ? a.frame_of[inst] : 0;
    int rows = 0, code = 0;  // (code: the count of an object that gets no scan)
    bool scan = f >= 0 && f < a.nframes;
    if (scan) {
        g.depth = a.depth + (size_t)f * a.H * a.W;
        g.m = load_pose(a.rt + (size_t)inst * 16);
        g.fin = true;
#pragma unroll
        for (int j = 0; j < 16; ++j) g.fin = g.fin && isfinite(a.rt[(size_t)inst * 16 + j]);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            g.hh[j] = __fadd_rn(__fmul_rn(a.half[3 * inst + j], a.inflate), a.pad);
            g.fin = g.fin && isfinite(g.hh[j]) && g.hh[j] > 0.f;
        }
        // the rectangle: the eight corners t + R (+-hh) projected, widened by two pixels, clipped
        bool whole = !g.fin;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) {
                const float e = g.m.R[0][i] * g.m.R[0][j] + g.m.R[1][i] * g.m.R[1][j] + g.m.R[2][i] * g.m.R[2][j] - (i == j ? 1.f : 0.f);
                whole = whole || !(fabsf(e) <= BOX_ORTHO_TOL);
            }
        float u0 = 3e38f, u1 = -3e38f, v0 = 3e38f, v1 = -3e38f;
#pragma unroll
        for (int cnr = 0; cnr < 8; ++cnr) {
            const float s0 = cnr & 1 ? g.hh[0] : -g.hh[0], s1 = cnr & 2 ? g.hh[1] : -g.hh[1], s2 = cnr & 4 ? g.hh[2] : -g.hh[2];
            const float px = g.m.t[0] + g.m.R[0][0] * s0 + g.m.R[0][1] * s1 + g.m.R[0][2] * s2;
            const float py = g.m.t[1] + g.m.R[1][0] * s0 + g.m.R[1][1] * s1 + g.m.R[1][2] * s2;
            const float pz = g.m.t[2] + g.m.R[2][0] * s0 + g.m.R[2][1] * s1 + g.m.R[2][2] * s2;
            const float u = a.fx * px / pz + a.cx, v = a.fy * py / pz + a.cy;
            whole = whole || !(pz >= BOX_NEAR) || !isfinite(u) || !isfinite(v);
            u0 = fminf(u0, u), u1 = fmaxf(u1, u), v0 = fminf(v0, v), v1 = fmaxf(v1, v);
        }
        int x0 = 0, x1 = a.W - 1, y0 = 0, y1 = a.H - 1;
        if (!whole) {  // (clamped as floats first: the conversions stay in range)
            const float lim = 40000.f;
            x0 = max(x0, (int)floorf(fminf(fmaxf(u0, -lim), lim)) - 2), x1 = min(x1, (int)ceilf(fminf(fmaxf(u1, -lim), lim)) + 2);
            y0 = max(y0, (int)floorf(fminf(fmaxf(v0, -lim), lim)) - 2), y1 = min(y1, (int)ceilf(fminf(fmaxf(v1, -lim), lim)) + 2);
        }
        g.x0 = x0, g.y0 = y0;
        g.cols = x1 >= x0 && y1 >= y0 ? x1 - x0 + 1 : 0;
        rows = g.cols ? y1 - y0 + 1 : 0;
        if ((long long)rows * ((g.cols + 63) >> 6) > BOX_MAX_SEGS) scan = false, code = -1;  // no truncated scan
    }
    if (!scan) {  // (decided by the whole workgroup, before a barrier and before anything is read through frame_of)
        for (int k = threadIdx.x; k < a.npts; k += 64 * ROI_WAVES) out[(size_t)k * 3] = out[(size_t)k * 3 + 1] = out[(size_t)k * 3 + 2] = 0.f;
        if (threadIdx.x == 0) a.count[inst] = code, a.valid[inst] = 0;
        return;
    }
    const uint32_t run = a.draw ? a.draw[2 * inst] : seed[2], slot = a.draw ? a.draw[2 * inst + 1] : seed[4] + (uint32_t)inst;
    sample_body(g, rows, g.cols, seed, run, slot, a.npts, out);
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

int gp_cloud_extent(int b, int n, const float *pts, const float *rt, int trim, const int8_t *sym, float *half_out, gp_stream_t s) {
    if (b < 0 || n < 1 || n > GP_EXTENT_MAX_N || trim < 0 || trim >= n || !pts || !rt || !half_out) return GP_EINVAL;
    if (b == 0) return GP_OK;
    if (n <= 1024)
        hipLaunchKernelGGL(cloud_extent_kernel<16>, dim3(b), dim3(64), 0, (hipStream_t)s, n, pts, rt, trim, sym, half_out);
    else
        hipLaunchKernelGGL(cloud_extent_kernel<GP_EXTENT_MAX_N / 64>, dim3(b), dim3(64), 0, (hipStream_t)s, n, pts, rt, trim, sym, half_out);
    return gp_launch_status();
}

int gp_box_sample_max_segments(void) { return BOX_MAX_SEGS; }

int gp_box_sample(int h, int w, int nframes, int nobj, int npts, const uint16_t *depth, const int32_t *frame_of, const float *rt, const float *half,
                  float inflate, float pad, int min_count, float fx, float fy, float cx, float cy, const void *seed_state, const uint32_t *draw,
                  float *points, int32_t *count, uint8_t *valid, gp_stream_t s) {
    if (h < 1 || w < 1 || h > 32767 || w > 32767 || nframes < 1 || nobj < 0 || npts < 1 || min_count < 0) return GP_EINVAL;
    if (!(inflate > 0.f && inflate <= 3.4028234664e38f) || !(pad >= 0.f && pad <= 3.4028234664e38f)) return GP_EINVAL;  // (finite; NaN fails both)
    if (!depth || !rt || !half || !seed_state || !points || !count || !valid) return GP_EINVAL;
    if (nobj == 0) return GP_OK;
    // the largest request this entry point serves, on the first call - a runner's warm-up, outside any stream capture
    constexpr size_t lds_max = (size_t)BOX_MAX_SEGS * (sizeof(unsigned long long) + sizeof(int));
    static_assert(lds_max <= 128 * 1024, "the segment table must fit the CU's LDS beside the static arrays");
    if (gp_prepare_lds<box_sample_kernel>(lds_max)) return GP_ELAUNCH;
    const long long whole = (long long)h * ((w + 63) / 64);  // (no rectangle has more segments than the image)
    const size_t lds = (size_t)(whole < BOX_MAX_SEGS ? whole : BOX_MAX_SEGS) * (sizeof(unsigned long long) + sizeof(int));
    BoxArgs a{h, w, nframes, npts, min_count, depth, frame_of, rt, half, inflate, pad, fx, fy, cx, cy, draw, points, count, valid};
    hipLaunchKernelGGL(box_sample_kernel, dim3(nobj), dim3(64 * ROI_WAVES), lds, (hipStream_t)s, a, (const uint32_t *)seed_state);
    return gp_launch_status();
}

}  // extern "C"
