/*
 * genpose_hip.h - C ABI of libgenpose_hip.so (MI355X / gfx950 only).
 *
 * This is the drop-in boundary for GenPose's inference hot path.  Every entry point
 *   - takes raw DEVICE pointers, plain ints/floats and a hipStream_t passed as void* (0 = null stream),
 *   - is stateless, allocation-free, never synchronises and never reads results back on the host
 *     (safe to capture in a hipGraph),
 *   - returns 0 on success or a negative GP_E* code (never exit()s, unlike the reference launchers,
 *     e.g. ball_query_gpu.cu:62-66).
 * Caller owns every buffer, outputs included (same convention as the reference's pybind wrappers,
 * pointnet2_utils.py:26-27,56,95-96,129,173,219).
 *
 * Section A replaces, one for one, the nine pybind functions of the reference's CUDA extension
 * `pointnet2_cuda` (networks/pts_encoder/pointnet2_utils/pointnet2/src/pointnet2_api.cpp:10-24).
 * Sections B-D are the fused MI355X-native entry points that replace the Python/ATen glue above them
 * (pointnet2_modules.py:19-56, scorenet.py:178-222, samplers.py:102-227, reward.py:131-155,
 * sgpa_utils.py:897-954).
 */
#ifndef GENPOSE_HIP_H
#define GENPOSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GP_OK 0
#define GP_EINVAL (-1)   /* bad size / null pointer / unsupported shape */
#define GP_ELAUNCH (-2)  /* hipGetLastError() != hipSuccess after a launch */
#define GP_EARCH (-3)    /* device is not gfx950 */

typedef void *gp_stream_t; /* hipStream_t */

/* ---------------------------------------------------------------------------------------------------------------
 * Arithmetic convention of the reference's three-product sums.  The reference's kernels say
 *     d = dx*dx + dy*dy + dz*dz          sampling_gpu.cu:133, ball_query_gpu.cu:33, interpolate_gpu.cu:36
 *     o = w0*p0 + w1*p1 + w2*p2          interpolate_gpu.cu:95
 * and are built with plain `nvcc -O2` (setup.py:19-20: --fmad=true), so nvcc decides how they contract - and which product
 * is fused decides, for distances that agree to an ulp, WHICH index furthest point sampling or a ball query returns.  There is
 * no CUDA toolchain here to settle it, so the convention is an explicit, tested parameter (compile-time inside every kernel):
 *     GP_ARITH_A   fma(c,c, fma(b,b, a*a))   the first product rounded on its own, the other two fused left to right
 *     GP_ARITH_B   fma(c,c, fma(a,a, b*b))   what LLVM's DAG combiner and GCC's widening-mul pass emit for this text: the
 *                                            inner fadd fuses its LEFT operand's multiply, the outer one the remaining product
 *     GP_ARITH_C   (a*a + b*b) + c*c         no contraction (nvcc --fmad=false)
 * GP_ARITH_DEFAULT is what every entry point WITHOUT an `_arith` suffix uses (DESIGN.md section 5 has the evidence and the
 * measured index differences between the conventions); the `_arith` twin of an entry point takes the convention first. */
#define GP_ARITH_A 0
#define GP_ARITH_B 1
#define GP_ARITH_C 2
#define GP_ARITH_DEFAULT GP_ARITH_B
int gp_arith_default(void); /* the GP_ARITH_DEFAULT this library was built with */

/* ---------------------------------------------------------------------------------------------------------------
 * E. Depth + instance mask -> point clouds (the step right before the path).
 * Replaces the per-detection body of detect_mrcnn_genpose (runners/evaluation_single.py:162-216):
 *   crop_resize_by_warp_affine(INTER_NEAREST) of raw depth, mask & (depth > 0) and the pixel-coordinate map
 *   (utils/datasets_utils.py:82-94; OpenCV's 10-bit fixed-point nearest sampling), depth_to_pcl (:107-118, float32) on the
 *   pixels with depth > 0 inside the mask, in raster order of the img x img crop, divided by 1000 (metres).
 *   depth [h,w] uint16 mm; masks [h,w,ninst] uint8 (Mask-RCNN layout); minv [ninst][6] = the INVERSE of the 2x3 matrix that
 *   get_affine_transform (:96-136) builds from get_bbox's window (doubles, row major): source = minv . (x, y, 1);
 *   pcl [ninst][img*img][3] f32 (first count[i] rows written); count / depth_count [ninst] = number of valid masked pixels /
 *   of crop pixels with a depth reading (the reference skips an instance when either is <= 1, :201-208).
 * gp_cloud_sample = sample_points (:120-133): out[i][k] = pcl[i][k % count] when count <= npts (tiling), else pcl[i][ids[i][k]]
 *   (ids = first npts entries of a permutation of count, drawn by the caller; NULL -> the first npts rows). */
int gp_roi_to_cloud(int h, int w, int ninst, int img, const uint16_t *depth, const uint8_t *masks, const double *minv, float fx, float fy,
                    float cx, float cy, float *pcl, int32_t *count, int32_t *depth_count, gp_stream_t s);
int gp_cloud_sample(int ninst, int cap, int npts, const float *pcl, const int32_t *count, const int32_t *ids, float *out, gp_stream_t s);
/* gp_roi_sample_seeded (ours): the two above in ONE launch with the draw made on the device - depth + masks -> out [ninst][npts][3], no
 *   [ninst][img*img][3] buffer, no count read back, no host permutation.  depth, masks, minv, the intrinsics, count and depth_count as in
 *   gp_roi_to_cloud; valid [ninst] uint8 = count > 1 && depth_count > 1 (the reference's skip, :201-208, as a device flag); a detection
 *   with valid = 0 gets all-zero rows.  Row k of a valid detection with c = count is, bit for bit, row rank(k) of what gp_roi_to_cloud
 *   writes for it:  c < npts: rank = k % c (sample_points' tiling);  c == npts: rank = k;  c > npts: rank = sigma(k), a keyed bijection of
 *   [0, c) (cycle walking over an 8-round alternating Feistel network on max(2, bit_length(c - 1)) bits whose round function is a
 *   Philox4x32-10 block: genpose_amd/csrc/philox.h, "the depth front end's draw"; genpose_amd.preprocess.seeded_ranks restates it in
 *   numpy), so the npts pixels are distinct by construction.  NO random-number parity with numpy's permutation is claimed.
 *   seed_state: the 8 uint32 words of the seeded samplers in device memory ([0], [1] seed lo / hi, [2] run = the frame index, [4] the
 *   slot of detection 0: detection i draws as global slot [4] + i, whatever shares its launch); only read.
 *   img <= 512 (the per-segment ballots and base ranks live in LDS: 12 bytes per 64 crop pixels of a row, 48 KB at 512).  NULL pointers,
 *   npts <= 0, img outside [1, 512] or h, w outside [1, 32767]: GP_EINVAL, nothing written; ninst == 0: GP_OK.  One 16-wave workgroup per
 *   detection; no allocation, no synchronisation, no host read: capturable. */
int gp_roi_sample_seeded(int h, int w, int ninst, int img, int npts, const uint16_t *depth, const uint8_t *masks, const double *minv, float fx,
                         float fy, float cx, float cy, const uint32_t *seed_state, float *out, int32_t *count, int32_t *depth_count, uint8_t *valid,
                         gp_stream_t s);
/* gp_roi_sample_frames (ours): gp_roi_sample_seeded over the detections of MANY depth images in ONE launch - ndet detections that belong
 *   to nframes images of one size h x w and one set of intrinsics; one 16-wave workgroup per detection, the same device code (the body of
 *   pass 1, the scan and pass 2 exists once; the two kernels differ in the addressing they hand it).
 *   depth [nframes][h][w] uint16 mm; masks: the frames' [h][w][n_f] uint8 blocks one after the other (n_f differs from frame to frame
 *   and may be 0), mask_bytes the size of the whole packed buffer; mask_off [nframes] int64 = the byte offset of each frame's block;
 *   det [ndet][3] int32 = {frame index, mask channel inside that frame's block, n_f = the block's channel count};
 *   draw [ndet][2] uint32 = {run, slot} of the detection's draw; minv [ndet][6] as above (row i = detection i);
 *   seed_state: the 8 words as above, of which ONLY [0], [1] (the seed) are read - run and slot come from `draw`.
 *   out [ndet][npts][3], count, depth_count, valid [ndet] as gp_roi_sample_seeded.  Detection i's four outputs are, bit for bit, what
 *   gp_roi_sample_seeded writes for it given depth + det[i][0] * h * w, masks + mask_off[det[i][0]] with ninst = det[i][2], instance
 *   det[i][1], seed_state[2] = draw[i][0] and seed_state[4] + instance = draw[i][1] - whatever shares its launch, in any order.
 *   A table entry that is out of range - frame outside [0, nframes), n_f <= 0, channel outside [0, n_f), or a block that does not lie
 *   inside [0, mask_bytes) - is a detection without a cloud: zero rows, count = depth_count = 0, valid = 0; nothing is read through it.
 *   NULL pointers, npts <= 0, img outside [1, 512], h or w outside [1, 32767], ndet < 0, mask_bytes < 0, nframes <= 0 with ndet > 0:
 *   GP_EINVAL, nothing written; ndet == 0: GP_OK.  No allocation, no synchronisation, no host read: capturable. */
int gp_roi_sample_frames(int h, int w, int nframes, int ndet, int img, int npts, const uint16_t *depth, const uint8_t *masks, int64_t mask_bytes,
                         const int64_t *mask_off, const int32_t *det, const uint32_t *draw, const double *minv, float fx, float fy, float cx, float cy,
                         const uint32_t *seed_state, float *out, int32_t *count, int32_t *depth_count, uint8_t *valid, gp_stream_t s);
/* MASK-FREE TRACKING (ours; opt-in; NO counterpart in the reference, whose tracking loop takes its clouds from the dataset's ground-truth
 * masks, evaluation_tracking.py:262-337): once an object has a pose, its pose and size say where its cloud is in the next depth frame.
 * THE OBJECT-FRAME EXPRESSION both entry points share (one device function): camera-frame point p, pose rt (float32 [4][4] row major,
 * object -> camera: the layout of gp_rank_aggregate_rt's avg_rt), R = rt[:3][:3], t = rt[:3][3]:
 *     u_j = p_j - t_j      q_j = ((u_0 * R[0][j]) + (u_1 * R[1][j])) + (u_2 * R[2][j])      j = 0, 1, 2
 *   every product and every sum rounded to float32 on its own (numpy float32 restates the bits: tests/box_front_end_reference.py).
 * gp_cloud_extent: half-extents of a cloud in its object frame.  pts [b][n][3], rt [b][4][4], half_out [b][3].  For cloud i,
 *   a_j[k] = |q_j(pts[i][k])| and half_out[i][j] = the (trim + 1)-th LARGEST of a_j[0..n-1] (trim = 0: the maximum; duplicated points count
 *   as often as they occur) - EXACT: a value of the array, the bits np.sort gives.  sym [b] int8 or NULL (gp_consensus_energy's
 *   convention): sym[i] != 0 = symmetric about the y axis, then half_out[i][0] = half_out[i][2] = that order statistic of
 *   sqrt_rn(add_rn(mul_rn(q_0, q_0), mul_rn(q_2, q_2))).  The frame is centred on the object, so 2 * half is its size also when only the
 *   camera-facing side was seen.  One wave per cloud, the values in registers, a bisection over the 31 value bits with wave-wide counts:
 *   no sort, no barrier, the same trip count on every bit pattern; non-finite input neither faults nor hangs (its result is unspecified).
 *   1 <= n <= GP_EXTENT_MAX_N, 0 <= trim < n, b >= 0, pts / rt / half_out non-NULL - else GP_EINVAL, nothing written; b == 0: GP_OK.  A
 *   cloud's row does not depend on the rest of the batch.  No allocation, no synchronisation: capturable.
 * gp_box_sample: depth + oriented boxes -> the sampled clouds, one launch, no mask.  depth [nframes][h][w] uint16 mm; frame_of [nobj] =
 *   each object's frame (NULL: frame 0); rt [nobj][4][4], half [nobj][3]; points [nobj][npts][3], count / valid [nobj].  For object i on
 *   its frame, hh_j = add_rn(mul_rn(half[i][j], inflate), pad); pixel (sx, sy) with depth word dv is INSIDE when dv > 0 and
 *   |q_j(p)| <= hh_j for j = 0, 1, 2, p = gp_roi_to_cloud's float32 back-projection ((sx - cx) * d / fx) / 1000, ((sy - cy) * d / fy) /
 *   1000, d / 1000.  count[i] = c = the inside pixels of the WHOLE image; valid[i] = c >= max(2, min_count) and every entry of rt[i] and
 *   hh finite and every hh_j > 0; a valid object's row k is the inside pixel of rank r in the image's raster order, c < npts: r = k % c,
 *   c == npts: r = k, c > npts: r = gp_roi_sample_seeded's seeded walk sigma(k) under (seed, run, slot) - draw [nobj][2] = {run, slot},
 *   or NULL: seed_state words [2] and [4] + i as gp_roi_sample_seeded; seed_state: its 8 uint32 words.  valid[i] == 0: all-zero rows.
 *   The kernel scans only the pixel rectangle of the box's eight projected corners, widened by two pixels and clipped - the whole image
 *   where a corner lies nearer than 0.05 m, projects to something non-finite or rt[i] is no rotation (|R^T R - I| > 1e-5): the rectangle
 *   is an accelerator, membership is the inside test alone, the result is the whole-image definition bit for bit.  The rectangle's
 *   (row, 64-column segment) table lives in LDS, 12 bytes a segment: a clipped rectangle of more than gp_box_sample_max_segments()
 *   segments (a whole 640 x 480 frame has 4 800) gets count = -1, valid = 0 and zero rows, never a truncated scan.  A frame_of entry
 *   outside [0, nframes) is an object without a cloud (count = 0, valid = 0, zero rows), decided before anything is read through it.
 *   1 <= h, w <= 32767, nframes >= 1, nobj >= 0, npts >= 1, inflate finite > 0, pad finite >= 0, min_count >= 0, depth / rt / half /
 *   seed_state / points / count / valid non-NULL - else GP_EINVAL, nothing written; nobj == 0: GP_OK.  One 16-wave workgroup per object
 *   running gp_roi_sample_seeded's ballot / scan / select code (one template, two pixel sources); an object's outputs do not depend on
 *   what shares its launch.  The first call raises the kernel's dynamic-LDS limit (make it outside a stream capture); then capturable. */
#define GP_EXTENT_MAX_N 4096
int gp_cloud_extent(int b, int n, const float *pts /*[b,n,3]*/, const float *rt /*[b,4,4]*/, int trim, const int8_t *sym /*[b] or NULL*/,
                    float *half_out /*[b,3]*/, gp_stream_t s);
int gp_box_sample_max_segments(void);
int gp_box_sample(int h, int w, int nframes, int nobj, int npts, const uint16_t *depth /*[nframes,h,w] mm*/, const int32_t *frame_of /*[nobj] or NULL*/,
                  const float *rt /*[nobj,4,4]*/, const float *half /*[nobj,3]*/, float inflate, float pad, int min_count, float fx, float fy, float cx,
                  float cy, const void *seed_state, const uint32_t *draw /*[nobj][2] run, slot; or NULL*/, float *points /*[nobj,npts,3]*/,
                  int32_t *count /*[nobj]*/, uint8_t *valid /*[nobj]*/, gp_stream_t s);

/* Library / device identification: returns ABI version; writes gcnArchName of the current device. */
int gp_version(void);
int gp_device_arch(char *buf, int buflen);

/* ------------------------------------------------------------------------------------------------
 * A. pointnet2_cuda operator API (reference: pointnet2_api.cpp:10-24)
 * ------------------------------------------------------------------------------------------------ */

/* furthest_point_sampling_wrapper (sampling.cpp:40-51, sampling_gpu.cu:86-253).
 * xyz [b,n,3] f32; temp [b,n] f32 in/out (caller fills 1e10, pointnet2_utils.py:27; must be >= 0);
 * idx [b,m] i32 out.  idx[:,0] = 0; ties resolved exactly as the reference's shared-memory tree does. */
int gp_furthest_point_sampling(int b, int n, int m, const float *xyz, float *temp, int32_t *idx, gp_stream_t s);
int gp_furthest_point_sampling_arith(int arith, int b, int n, int m, const float *xyz, float *temp, int32_t *idx, gp_stream_t s);

/* gather_points_wrapper (sampling.cpp:13-23, sampling_gpu.cu:8-44): points [b,c,n], idx [b,m] -> out [b,c,m]. */
int gp_gather_points(int b, int c, int n, int m, const float *points, const int32_t *idx, float *out, gp_stream_t s);
/* gather_points_grad_wrapper (sampling_gpu.cu:46-83): grad_out [b,c,m], idx [b,m] -> grad_points [b,c,n] (+=, atomic). */
int gp_gather_points_grad(int b, int c, int n, int m, const float *grad_out, const int32_t *idx, float *grad_points, gp_stream_t s);

/* ball_query_wrapper (ball_query.cpp:16-27, ball_query_gpu.cu:9-67).
 * new_xyz [b,m,3], xyz [b,n,3] -> idx [b,m,nsample] i32.  First `nsample` points in index order with
 * d2 < radius^2 (strict, radius^2 in f32); the first hit pre-fills every slot; rows with no hit are
 * left untouched (caller pre-zeroes idx, pointnet2_utils.py:219). */
int gp_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz, int32_t *idx, gp_stream_t s);
int gp_ball_query_arith(int arith, int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz, int32_t *idx,
                        gp_stream_t s);

/* group_points_wrapper (group_points.cpp:26-37, group_points_gpu.cu:47-86): points [b,c,n], idx [b,np,ns] -> out [b,c,np,ns]. */
int gp_group_points(int b, int c, int n, int npoints, int nsample, const float *points, const int32_t *idx, float *out, gp_stream_t s);
/* group_points_grad_wrapper (group_points_gpu.cu:8-45): grad_out [b,c,np,ns] -> grad_points [b,c,n] (+=, atomic). */
int gp_group_points_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int32_t *idx, float *grad_points, gp_stream_t s);

/* three_nn_wrapper (interpolate.cpp, interpolate_gpu.cu:9-74): unknown [b,n,3], known [b,m,3] -> dist2 [b,n,3] f32, idx [b,n,3] i32. */
int gp_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2, int32_t *idx, gp_stream_t s);
int gp_three_nn_arith(int arith, int b, int n, int m, const float *unknown, const float *known, float *dist2, int32_t *idx, gp_stream_t s);
/* three_interpolate_wrapper (interpolate_gpu.cu:77-117): points [b,c,m], idx/weight [b,n,3] -> out [b,c,n]. */
int gp_three_interpolate(int b, int c, int m, int n, const float *points, const int32_t *idx, const float *weight, float *out, gp_stream_t s);
int gp_three_interpolate_arith(int arith, int b, int c, int m, int n, const float *points, const int32_t *idx, const float *weight, float *out,
                               gp_stream_t s);
/* three_interpolate_grad_wrapper (interpolate_gpu.cu:120-160): grad_out [b,c,n] -> grad_points [b,c,m] (+=, atomic). */
int gp_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int32_t *idx, const float *weight, float *grad_points, gp_stream_t s);

/* ------------------------------------------------------------------------------------------------
 * B. Fused PointNet++(MSG) encoder (replaces Pointnet2ClsMSG.forward, pointnet2.py:203-211, and
 *    _PointnetSAModuleBase.forward, pointnet2_modules.py:19-56).  Features are kept POINT-MAJOR
 *    [b, n, C] on the device (the reference keeps [b, C, n]).
 * ------------------------------------------------------------------------------------------------ */

/* FPS + gather for up to 3 consecutive set-abstraction levels in one launch (one workgroup per cloud).
 * xyz [b,n0,3]; level l selects m[l] points out of the previous level's selection.
 * idx_l [b,m_l] i32 (indices into the previous level's point list), new_xyz_l [b,m_l,3].  Unused levels: m = 0.
 * Limits: 1 <= n0 <= 1024 (one wave holds a level in registers), 1 <= nlevels <= 3, 1 <= m[0] <= n0 and 1 <= m[l] <= m[l-1], and a
 * non-null idx_l / new_xyz_l for every level l < nlevels (those of the unused levels are not read: NULL).  Anything else returns
 * GP_EINVAL before any launch: no output is written.  Larger clouds: one gp_furthest_point_sampling per level. */
int gp_fps_chain(int b, int n0, int nlevels, const int *m, const float *xyz, int32_t *idx0, float *new_xyz0,
                 int32_t *idx1, float *new_xyz1, int32_t *idx2, float *new_xyz2, gp_stream_t s);
int gp_fps_chain_arith(int arith, int b, int n0, int nlevels, const int *m, const float *xyz, int32_t *idx0, float *new_xyz0,
                       int32_t *idx1, float *new_xyz1, int32_t *idx2, float *new_xyz2, gp_stream_t s);

/* Ball query for the two scales of one MSG level in a single pass; rows with no hit are zero-filled (the caller need not zero idx0 /
 * idx1 beforehand).  The workgroup keeps the cloud and its staging rows in LDS, 12 n + 16 (nsample0 + nsample1 + 2) bytes, and the
 * entry takes what fits 60 KiB: n <= 5053 at 16 + 32 samples.  gp_ball_query_msg_fits says so (1 / 0; host only, no device needed); for
 * a shape that does not fit, gp_ball_query_msg[_arith] returns GP_EINVAL before any launch and writes nothing - the caller runs
 * gp_ball_query once per scale on zeroed buffers instead (any n). */
int gp_ball_query_msg_fits(int n, int nsample0, int nsample1);
int gp_ball_query_msg(int b, int n, int m, float radius0, int nsample0, float radius1, int nsample1, const float *new_xyz,
                      const float *xyz, int32_t *idx0, int32_t *idx1, gp_stream_t s);
int gp_ball_query_msg_arith(int arith, int b, int n, int m, float radius0, int nsample0, float radius1, int nsample1, const float *new_xyz,
                            const float *xyz, int32_t *idx0, int32_t *idx1, gp_stream_t s);

/* One scale of one set-abstraction level: gather neighbourhood -> 3-layer shared MLP (BN folded, ReLU) on
 * fp32 MFMA -> max over the neighbourhood.  Never materialises the grouped [b,C+3,np,ns] tensor.
 *   xyz [b,n,3]; feats_in [b,n,cin] or NULL (cin = 0); new_xyz [b,np,3] and idx [b,np,ns] (grouping mode)
 *   or new_xyz = idx = NULL with np = 1 (GroupAll mode: ns must equal n, absolute xyz, pointnet2_utils.py:268-291).
 *   wpack*: weights packed by gp_pack_weight_size/gp_pack_weight (layer input order = [feats..., dx,dy,dz]);
 *   bias*: folded BN shift per output channel (padded to a multiple of 16).
 *   out [b,np,cout_total]: this scale writes channels [cout_off, cout_off + c3).
 * GroupAll mode accumulates with an integer atomic max (post-ReLU values are >= 0): out must be zeroed first. */
int gp_sa_mlp_max(int b, int n, int np, int ns, int cin, int c1, int c2, int c3, const float *xyz, const float *feats_in,
                  const float *new_xyz, const int32_t *idx, const float *wpack1, const float *bias1, const float *wpack2,
                  const float *bias2, const float *wpack3, const float *bias3, float *out, int cout_total, int cout_off,
                  gp_stream_t s);

/* Hoisted first layer of a grouping level (exact algebra: W1.[feat_j ; xyz_j - c] = W1f.feat_j + W1x.(xyz_j - c)):
 * gp_point_linear computes z[row, 0:n_out] = x[row, 0:k_in] . W1f^T once per SOURCE point (rows = b*n; wpack from gp_pack_weight);
 * gp_sa_pre_mlp_max then gathers z rows (channels [zoff, zoff+c1) of a zstride-wide row; z = NULL for a level without input
 * features), adds wxyz[c][0..2].(xyz_j - centre) + bias1[c], ReLU, and runs layers 2, 3 + max-pool as gp_sa_mlp_max does.
 * wxyz is [round16(c1)][4] (x, y, z, 0), BN scale folded in.  new_xyz = idx = NULL with np = 1, ns = n selects GroupAll
 * (every point once, absolute xyz; out must be zeroed first - the tiles of a cloud combine by integer atomic max).
 * This is the encoder's production path for every level; gp_sa_mlp_max remains as the unhoisted form. */
int gp_point_linear(int rows, int k_in, int n_out, const float *x, const float *wpack, float *z, gp_stream_t s);
int gp_sa_pre_mlp_max(int b, int n, int np, int ns, int c1, int c2, int c3, const float *xyz, const float *new_xyz, const int32_t *idx,
                      const float *z, int zstride, int zoff, const float *wxyz, const float *bias1, const float *wpack2, const float *bias2,
                      const float *wpack3, const float *bias3, float *out, int cout_total, int cout_off, gp_stream_t s);
/* The same with a choice of HIDDEN-LAYER LAYOUT for widths c2 that are not a multiple of 16 (light encoder level 2: 196 = 12 x 16 + 4).
 * GP_SA_TAIL_PLAIN: channel c of the hidden layer is row c of wpack2 / bias2 and column c of wpack3 (what gp_sa_pre_mlp_max assumes).
 * GP_SA_TAIL_SPREAD: the r = c2 % 16 channels of the last, partly filled 16-channel block are moved to positions
 * 4 (c % 4) + c / 4 of that block (gp_sa_tail_position(c2, channel) gives the padded index; the caller packs a [round16(c2), c1]
 * layer-2 matrix / bias and a [c3, round16(c2)] layer-3 matrix with the channels there and zeros elsewhere).  The network is the same
 * function; the register-chain kernels then skip the MFMAs of the last block that only multiply padding (196: one k-step of four). */
#define GP_SA_TAIL_PLAIN 0
#define GP_SA_TAIL_SPREAD 1
int gp_sa_pre_mlp_max_layout(int hidden_layout, int b, int n, int np, int ns, int c1, int c2, int c3, const float *xyz, const float *new_xyz,
                             const int32_t *idx, const float *z, int zstride, int zoff, const float *wxyz, const float *bias1, const float *wpack2,
                             const float *bias2, const float *wpack3, const float *bias3, float *out, int cout_total, int cout_off, gp_stream_t s);
int gp_sa_tail_position(int c2, int channel);

/* OPT-IN, EXPLORATORY (round 5; csrc/sa_bf16x3.hip): gp_sa_pre_mlp_max for the level-2 shapes of the light encoder (c1, c2, c3 = 128, 196, 256;
 * ns = 16 | 32; hoisted first layer: z required) with layers 2 and 3 on the BF16 matrix pipe as three-term split products
 * (a.b ~= a_hi.b_hi + a_lo.b_hi + a_hi.b_lo, fp32 accumulate; relative error ~2^-17 per product instead of 2^-24).  w2_split / w3_split: the
 * weights as hi / lo bf16 pairs in the fragment order of v_mfma_f32_16x16x32_bf16 (genpose_amd/weights.py: pack_bf16x3 -
 * [c1/32][13][2][64][8] and [2][7][8][2][64][8] bf16); bias2 [224] zero padded, channel order as trained.  Never the default: the fp32 entry
 * points above are what every parity claim and the headline bench line run.  b * np * ns must be a multiple of 32. */
int gp_sa_pre_mlp_max_bf16x3(int b, int n, int np, int ns, int c1, int c2, int c3, const float *xyz, const float *new_xyz, const int32_t *idx,
                             const float *z, int zstride, int zoff, const float *wxyz, const float *bias1, const void *w2_split, const float *bias2,
                             const void *w3_split, const float *bias3, float *out, int cout_total, int cout_off, gp_stream_t s);

/* gp_sa_pre_mlp_max for grouping level 2 (c1, c2, c3 = 128, 196, 256; ns = 16 | 32; hoisted first layer: z required) with layers 2 and 3 as
 * EXACT-PRODUCT split bf16 on the BF16 matrix pipe (csrc/sa_bf16x9.hip: every fp32 operand = hi + mid + lo, all nine bf16 cross products on
 * v_mfma_f32_16x16x32_bf16, fp32 accumulation - the error class of the fp32 MFMA kernel, as gp_pc_step_bf16x9 is to gp_pc_step_plan).  Layer 1,
 * the pooling, the inputs and the [b, np, c3] output columns are gp_sa_pre_mlp_max's.  w23_x9: both layers' weights as hi / mid / lo bf16
 * triples in the kernel's streaming order (genpose_amd/weights.py: pack_sa_bf16x9 - [22 slices][8 chunks][3][64][8] bf16: layer 2 as
 * (k-block, chunk half), layer 3 as (half, k-block)); bias2 [224] zero padded, bias3 [256], channel order as trained.  Layer-3 columns >= 196
 * and, of slices 14 / 21 (layer 3's seventh k-block), everything beyond k = 195 are not read.  b * np * ns must be
 * a multiple of 32.  What an agent of the PC sampler runs for this level by default (genpose_amd/config.py: encoder_level2); the fp32 entry points above stay selectable. */
int gp_sa_pre_mlp_max_bf16x9(int b, int n, int np, int ns, int c1, int c2, int c3, const float *xyz, const float *new_xyz, const int32_t *idx,
                             const float *z, int zstride, int zoff, const float *wxyz, const float *bias1, const void *w23_x9, const float *bias2,
                             const float *bias3, float *out, int cout_total, int cout_off, gp_stream_t s);

/* gp_sa_pre_mlp_max for grouping level 1 of the light / dense encoders ((c1, c2, c3), ns = (64, 64, 128), 16 | (64, 96, 128), 32; hoisted first
 * layer: z required) with layers 2 and 3 as EXACT-PRODUCT split bf16 on the BF16 matrix pipe (csrc/sa_lds_bf16x9.hip; the arithmetic of
 * gp_sa_pre_mlp_max_bf16x9), both layers' weights LDS-resident as hi / mid / lo, no barrier in the row loop.  Layer 1, the pooling, the inputs
 * and the [b, np, c3] output columns are gp_sa_pre_mlp_max's.  w2_x9 / w3_x9: the weights as hi / mid / lo bf16 triples in the fragment order
 * of v_mfma_f32_16x16x32_bf16 (genpose_amd/weights.py: pack_bf16x9 - [c1 / 32][c2 / 16][3][64][8] and [c2 / 32][c3 / 16][3][64][8] bf16);
 * bias2 [c2], bias3 [c3], channel order as trained.  b * np * ns must be a multiple of 32; GP_EINVAL (nothing launched) for any other shape,
 * a null pointer or offsets that are not multiples of four floats; b = 0 returns GP_OK.  What an agent of the PC sampler runs for this
 * level by default (genpose_amd/config.py: encoder_level1); the fp32 entry points above stay selectable. */
int gp_sa_lds_bf16x9(int b, int n, int np, int ns, int c1, int c2, int c3, const float *xyz, const float *new_xyz, const int32_t *idx, const float *z,
                     int zstride, int zoff, const float *wxyz, const float *bias1, const void *w2_x9, const float *bias2, const void *w3_x9,
                     const float *bias3, float *out, int cout_total, int cout_off, gp_stream_t s);

/* The GroupAll level of the light encoder (n = 128 points, cin = 512 features, c1 = 256, c3 = 512, c2 = 256 | 384 per scale) in ONE launch
 * with all three dense layers as EXACT-PRODUCT split bf16 on the BF16 matrix pipe (csrc/sa_groupall_bf16x9.hip; the arithmetic of
 * gp_sa_pre_mlp_max_bf16x9): the job of gp_point_linear (hoisted feature half of layer 1) + gp_sa_pre_mlp_max_layout per scale, from
 * feat [b, 128, 512] directly - no hoisted rows in memory, no zeroed output, no atomics; out[b, cout_off : cout_off + 512] of every scale
 * is written whole, and a cloud's values do not depend on b or on its position.  xyz [b, 128, 3] absolute coordinates.  Per scale (_a, and
 * _b unless c2_b = 0 = one scale): w = the three matrices as hi / mid / lo bf16 triples in the kernel's streaming order
 * (genpose_amd/weights.py: pack_groupall_bf16x9 - [80 | 104 slices][8 chunks][3][64][8] bf16), wxyz [256][4] rows (wx, wy, wz, 0), biases
 * [256], [c2], [512], channel order as trained.  GP_EINVAL for any other shape, a misaligned pointer (16 bytes: feat, w, wxyz; 4 the rest),
 * overlapping or out-of-range output columns; b = 0 returns GP_OK. */
int gp_sa_groupall_bf16x9(int b, int n, int cin, int c1, int c3, const float *xyz, const float *feat, int c2_a, const void *w_a, const float *wxyz_a,
                          const float *bias1_a, const float *bias2_a, const float *bias3_a, int cout_off_a, int c2_b, const void *w_b,
                          const float *wxyz_b, const float *bias1_b, const float *bias2_b, const float *bias3_b, int cout_off_b, float *out,
                          int cout_total, gp_stream_t s);

/* Vanilla PointNet encoder, PointNetfeat(num_points, out_dim=1024) without BatchNorm (networks/pts_encoder/pointnets.py:83-123; the agent's
 * cfg.pts_encoder = 'pointnet' | 'pointnet_and_pointnet2', networks/posenet.py:36-46, 79-90).  csrc/pointnet.hip: per-point MLP chains on
 * fp32 MFMA over 48-point tiles, bias after the product, ReLU where the reference has it; the [b, n, 1024] and [b, n, 512] activations of
 * the reference never reach memory.  Any n >= 1; all weights wpack* from gp_pack_weight ([Cout, Cin] of the Conv1d's [Cout, Cin, 1]),
 * biases as trained; outputs 16-byte aligned.  The output buffer doubles as the scratch of the cross-tile maximum (atomic max on
 * order-preserving integer keys, zeroed and decoded by the entry point itself): it holds no meaningful value until the call's last
 * kernel has run.
 *
 * gp_pointnet_stn_pool: the convolutions of the input transform net STNkd(k=3) and its pooling (pointnets.py:60-64)
 *     g[b, 1024] = max over the cloud's n points of relu(conv3(relu(conv2(relu(conv1(xyz))))))       widths 3 -> 64 -> 128 -> 1024
 * gp_pointnet_feat_pool: the trunk (pointnets.py:101-118), trans [b, 3, 3] = the transform net's output
 *     x' = torch.bmm(x, trans), i.e. x'[j] = sum_i x[i] trans[i][j]                                    (pointnets.py:102-104)
 *     feat[b, 1024] = max over the n points of conv4(relu(conv3(relu(conv2(relu(conv1(x')))))))       widths 3 -> 64 -> 128 -> 512 -> 1024
 *     conv4 has NO ReLU (pointnets.py:116): the pooled values are signed. */
int gp_pointnet_stn_pool(int b, int n, const float *xyz, const float *wpack1, const float *bias1, const float *wpack2, const float *bias2,
                         const float *wpack3, const float *bias3, float *g, gp_stream_t s);
int gp_pointnet_feat_pool(int b, int n, const float *xyz, const float *trans, const float *wpack1, const float *bias1, const float *wpack2,
                          const float *bias2, const float *wpack3, const float *bias3, const float *wpack4, const float *bias4, float *feat,
                          gp_stream_t s);

/* Small-row dense layer with bias and activation: out[rows, n_out] = act([xa | xb] . W^T + bias), W [n_out, k_a + k_b] row-major as trained
 * (NOT packed), xa [rows, k_a], xb [rows, k_b] or NULL with k_b = 0; k_a, k_b multiples of 4; act = GP_ACT_NONE | GP_ACT_RELU.
 * Serves the transform net's head fc1 -> fc2 -> fc3 (pointnets.py:66-68; the caller folds `+ iden`, :70-77, into fc3's bias) and the
 * agent's fusion_layer over cat(pointnet_feat, pointnet2_feat) without materialising the concatenation (posenet.py:87-88).
 * gp_point_linear above (no bias, no activation, packed weights, many rows) is unchanged. */
#define GP_ACT_NONE 0
#define GP_ACT_RELU 1
int gp_dense_rows(int rows, int k_a, int k_b, int n_out, const float *xa, const float *xb, const float *W, const float *bias, int act, float *out,
                  gp_stream_t s);

/* Weight packing for the MFMA layers (host-callable helpers operating on HOST memory):
 * W is [n_out, k_in] row-major (torch Linear / 1x1 conv layout).  Packed size in floats = gp_pack_weight_size(). */
int64_t gp_pack_weight_size(int n_out, int k_in);
int gp_pack_weight(int n_out, int k_in, const float *W, int ldw, float *packed);

/* ------------------------------------------------------------------------------------------------
 * C. Score / energy network and the samplers (scorenet.py:178-222, energynet.py:143-198,
 *    samplers.py:102-160 PC, samplers.py:163-227 PF-ODE with scipy RK45 semantics).
 * ------------------------------------------------------------------------------------------------ */

/* Parameter block shared by the score/energy entry points (all device pointers). */
typedef struct gp_scorenet {
    const float *w_pose0; /* packed [256 x 9]   pose_encoder.0 */
    const float *b_pose0; /* [256] */
    const float *w_pose2; /* packed [256 x 256] pose_encoder.2 */
    const float *b_pose2; /* [256] */
    const float *w_headx; /* packed [768 x 256]: pose_feat columns of fusion_tail_{rot_x,rot_y,trans}.0 stacked */
    const float *w_out;   /* [9 x 256]: rows 0-2 rot_x.2, 3-5 rot_y.2, 6-8 trans.2 */
    const float *b_out;   /* [9] */
    const float *fourier_w; /* [64] t_encoder.0.W */
    const float *w_t1;    /* [128 in][128 out]: t_encoder.1.weight TRANSPOSED */
    const float *b_t1;    /* [128] */
    const float *w_headt; /* [128 in][768 out]: t_feat columns of the three head first layers, TRANSPOSED */
    const float *w_headp; /* packed [768 x 1024]: pts_feat columns of the three head first layers */
    const float *b_head;  /* [768] */
    /* transposed packs for the backward pass of gp_score_div (d score / d pose); unused by every other entry point */
    const float *w_headx_t; /* packed [256 x 768] = w_headx^T */
    const float *w_pose2_t; /* packed [256 x 256] = pose_encoder.2.weight^T */
    const float *w_pose0_t; /* packed [9 x 256]   = pose_encoder.0.weight^T */
} gp_scorenet;

/* cvec[b,768] = W_headp . pts_feat[b] + b_head  (hoisted once per cloud; exact algebra). */
int gp_cloud_embed(int b, const gp_scorenet *net, const float *pts_feat, float *cvec, gp_stream_t s);
/* tvec[nt,768] = W_headt . relu(W_t1 . fourier(t) + b_t1) for nt time values read from DEVICE memory (f32). */
int gp_time_embed(int nt, const gp_scorenet *net, const float *t, float *tvec, gp_stream_t s);
/* ngroups sets of nt time values, set g at t + g * t_stride_floats -> tvec[(g*nt + i), 768] (the grouped RK45 driver reads its stage
 * times straight out of the per-group solver states). */
int gp_time_embed_strided(int nt, int ngroups, int64_t t_stride_floats, const gp_scorenet *net, const float *t, float *tvec, gp_stream_t s);

/* f_theta / score / energy for R = nclouds*k rows.  x [R,9] f32; tvec [768]; sigma = *sigma_dev (f32).
 * mode 0: out[R,9] = f_theta/(sigma+1e-7) (score, scorenet.py:217); mode 1: out[R,2] = IP energy (energynet.py:180-185). */
int gp_score_eval(int nclouds, int k, const gp_scorenet *net, const float *cvec, const float *tvec, const float *x,
                  const float *sigma_dev, int mode, float *out, gp_stream_t s);

/* Score and the Skilling-Hutchinson divergence estimate of cond_ode_likelihood (samplers.py:49-71) in one launch:
 *   score[R,9] = f_theta(x)/(sigma+1e-7);  div[R] = eps^T (d score / d x) eps  - the reference gets it from
 *   torch.autograd.grad(sum(score * eps), x); here the vector-Jacobian product runs through the transposed weight packs
 *   (ReLU masks from the forward activations kept in LDS).  x, eps [R,9] f32; tvec [768]; sigma = *sigma_dev. */
int gp_score_div(int nclouds, int k, const gp_scorenet *net, const float *cvec, const float *tvec, const float *x, const float *eps,
                 const float *sigma_dev, float *score, float *div, gp_stream_t s);

/* Score and the EXACT divergence of the score field in one launch - what gp_score_div estimates with one probe:
 *   score[R,9] = f_theta(x)/(sigma+1e-7), the bits gp_score_div writes;  div[R] = tr(d score / d x) = sum_{i<9} d score_i / d x_i.
 * One forward pass per 16-row tile, then the backward pass for the nine unit seeds: seed e_i selects row i mod 3 of the 256 -> 3 output
 * layer of head i / 3 (rot_x, rot_y, trans) and runs through that head's 256 pose-feature columns of w_headx_t, then w_pose2_t and
 * w_pose0_t; the three seeds of a head are three 16-row MFMA tiles of one pass over those weights (csrc/score_bwd.h).  Same fp32 MFMA
 * arithmetic and transposed packs as gp_score_div; no probe.  x [R,9] f32; tvec [768]; sigma = *sigma_dev.  Null pointers, k <= 0 or a
 * net without the transposed packs: GP_EINVAL, nothing written; R == 0: GP_OK.  Cost (MI355X, profiles/exact_likelihood.txt): 2.45 x the
 * time of gp_score_div, 103.7 against 42.3 us at 800 rows and 821 against 335 us at 32 000 rows; bound by the matrix pipe. */
int gp_score_div_exact(int nclouds, int k, const gp_scorenet *net, const float *cvec, const float *tvec, const float *x, const float *sigma_dev,
                       float *score, float *div, gp_stream_t s);

/* Score of the ENERGY model (PoseEnergyNet.forward(return_item='score'), energynet.py:200-222): the gradient of the un-decoupled
 * inner-product energy <x, f_theta(x)/sigma> with respect to the pose, which the reference obtains by autograd:
 *   score[R,9] = f_theta/sigma + J_f^T (x/sigma);  energy[R] (may be NULL) = <x, f_theta/sigma>.  `net` = the energy net's block. */
int gp_energy_score(int nclouds, int k, const gp_scorenet *net, const float *cvec, const float *tvec, const float *x, const float *sigma_dev,
                    float *score, float *energy, gp_stream_t s);

/* gp_score_eval with the launch plan chosen by the caller: tile = 0 (automatic, = gp_score_eval), 16 / 32 / 64 (tile form: one 16-, 32-
 * or 64-row tile per workgroup, activations through LDS), 128 (chain form: 4 waves x 32 rows per workgroup, activations
 * register-resident, weights through an LDS ring - csrc/trunk_chain.h; pays from ~32 000 rows; needs k >= 43 so that the rows of a
 * workgroup span at most 4 clouds, else GP_EINVAL). */
int gp_score_eval_plan(int tile, int nclouds, int k, const gp_scorenet *net, const float *cvec, const float *tvec, const float *x,
                       const float *sigma_dev, int mode, float *out, gp_stream_t s);

/* Rows per workgroup tile of the TILE-form score kernels (the RK45 driver and the backward kernels use the tile form only). */
int gp_score_tile_rows(int nrows);

/* One launch of the predictor-corrector sampler (cond_pc_sampler, samplers.py:102-160), score evaluation fused in.
 * Launch `step` = 0 .. nsteps (nsteps+1 launches, stream order is the only synchronisation):
 *   step > 0      : finishes step-1 for every row - Langevin corrector with the BATCH-MEAN gradient norm
 *                   (samplers.py:130-132; reduced in fixed order from partials[step-1][*]), renormalisation (:142-143),
 *                   Euler-Maruyama predictor with the pre-corrector score (:146-149), normalize_rotation (:152);
 *   step < nsteps : evaluates score(x, t_step) -> score[R,9] and this tile's sum of row norms -> partials[step][tile];
 *   step == nsteps: additionally writes mean_x (+centre, normalised: :157-158).
 * sched [nsteps][4] f32 = {sigma(t_i), g(t_i), step_size, sqrt(step_size)} (host schedule table);
 * tvec_all [nsteps][768] from gp_time_embed; z_* [nsteps][R][9] standard-normal draws; centre [nclouds][3];
 * traj: NULL or [nsteps][R][9] (in-process samples, centre added).
 * partials: [nsteps][ceil(R / gp_score_tile_rows(R))] floats.  gp_pc_step, gp_pc_step_grouped and gp_pc_step_coupled always run the TILE
 * form (one partial per 16- / 32-row workgroup), so this size holds for every R; the chain form of large launches (one partial per
 * wave) is reached through gp_pc_layout + gp_pc_step_plan, whose nparts_out is then the size to allocate. */
int gp_pc_step(int nclouds, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec, const float *tvec_all,
               const float *sched, const float *z_langevin, const float *z_predictor, const float *centre, float *x, float *mean_x,
               float *score, float *partials, float *traj, gp_stream_t s);

/* The same launch over `ngroups` independent batches of `nclouds_per_group` clouds laid out back to back (rows, clouds,
 * noise: group-major).  Everything is row-local except the batch-mean gradient norm, which stays PER GROUP, so every
 * group's result is what gp_pc_step returns for it alone (up to the summation order of the norm partials); serving
 * several batches per launch lets the kernel use 32-row tiles or the chain form (MFMA-bound) where one batch only fills 16-row
 * tiles (weight-stream-bound).  Rows of one group must be a multiple of the tile; partials: [nsteps][ngroups * ceil(rows per group /
 * tile)] with tile = gp_pc_tile_rows() = the TILE-form choice (16 or 32, or GP_EINVAL), which gp_pc_step_grouped / _coupled run and the
 * RK45 driver uses.  (gp_pc_layout + gp_pc_step_plan additionally offer the chain form, with their own partials size.) */
int gp_pc_tile_rows(int ngroups, int nclouds_per_group, int k);
int gp_pc_step_grouped(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                       const float *tvec_all, const float *sched, const float *z_langevin, const float *z_predictor,
                       const float *centre, float *x, float *mean_x, float *score, float *partials, float *traj, gp_stream_t s);

/* OPT-IN, EXPLORATORY (round 5; csrc/trunk_bf16x3.hip): one launch of the PC sampler - gp_pc_step_grouped's contract (step = 0 .. nsteps, per-group
 * batch-mean coupling, the same buffers) - with the score network's three dense layers on the BF16 matrix pipe as three-term split products
 * (a.b ~= a_hi.b_hi + a_lo.b_hi + a_hi.b_lo, fp32 accumulate).  128 rows per workgroup (k >= 43: a workgroup's rows span at most four clouds;
 * rows per group a multiple of 128 when ngroups > 1), one partial sum per wave: partials [nsteps][*nparts_out of gp_pc_layout_bf16x3].
 * w_*_split: hi / lo bf16 pairs in the fragment order of v_mfma_f32_16x16x32_bf16 (genpose_amd/weights.py: pack_bf16x3 - pose_encoder.0
 * [1][16][2][64][8] in natural k order, pose_encoder.2 [8][16]..., stacked heads [8][48]... in the register chain's k order); b_*, w_out [9][256],
 * b_out [9] fp32.  PC sampler of the score model only (the RK45 driver and every default path keep the fp32 trunk). */
int gp_pc_layout_bf16x3(int ngroups, int nclouds_per_group, int k, int *nparts_out);
/* The chain plan (128 rows per workgroup) of gp_pc_step_plan for the score model (model 0), with the network's three dense layers as
 * EXACT-PRODUCT split bf16 (csrc/trunk_bf16x9.hip: every fp32 operand = hi + mid + lo, all nine bf16 cross products on
 * v_mfma_f32_16x16x32_bf16, fp32 accumulation).  gp_pc_step_plan's contract with tile = 128: the same buffers, gn_ext / gn_rows_total
 * coupling, partials [nsteps][*nparts_out of gp_pc_layout(0, 128, ...)]; GP_EINVAL where that plan does not apply.  w_*_x9: hi / mid / lo
 * bf16 triples in the fragment order of v_mfma_f32_16x16x32_bf16 (genpose_amd/weights.py: pack_bf16x9 - pose_encoder.0 [1][16][3][64][8]
 * in natural k order, pose_encoder.2 [8][16][3][64][8] (k-block, output chunk) in the register chain's k order; the stacked heads in the
 * order the kernel consumes them, [head 3][chunk pair 8][chunk 2][k-block 8][3][64][8] - pack_heads_bf16x9, a permutation of
 * pack_bf16x9(W, 48, 8); this w_headx_x9 layout holds for every gp_*_bf16x9 entry point); biases and output layers
 * from `net`.  The default for that plan (genpose_amd/samplers.py); gp_pc_step_plan keeps the fp32-MFMA chain kernel.
 * ALIGNMENT: cvec, tvec_all and net->b_pose0, b_pose2, w_out must be 16-byte aligned (the kernel stages them with 16-byte loads; rows of
 * 256 / 768 floats of an aligned base are); GP_EINVAL otherwise.  The same holds for gp_pc_step_bf16x9_seeded and gp_heun_step_bf16x9. */
int gp_pc_step_bf16x9(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec, const float *tvec_all,
                      const float *sched, const float *z_langevin, const float *z_predictor, const float *centre, float *x, float *mean_x, float *score,
                      float *partials, float *traj, const float *gn_ext, int gn_rows_total, const void *w_pose0_x9, const void *w_pose2_x9,
                      const void *w_headx_x9, gp_stream_t s);
/* gp_pc_step_bf16x9 with SIX of the nine products of every multiply (csrc/bf16x9.h: lo.lo, lo.mid and mid.lo are not issued - at most
 * (2^-23 + 2^-32) |a b| per multiply, below the fp32 accumulation's own rounding; still the fp32 error class, 6 / 9 of the matrix-pipe
 * work).  Arguments, weight packs (the lo terms are still read), plan, alignment rule and results contract are gp_pc_step_bf16x9's; the bits
 * are its own.  What a score-model PC agent takes by default (config.sampler_products). */
int gp_pc_step_bf16x6(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec, const float *tvec_all,
                      const float *sched, const float *z_langevin, const float *z_predictor, const float *centre, float *x, float *mean_x, float *score,
                      float *partials, float *traj, const float *gn_ext, int gn_rows_total, const void *w_pose0_x9, const void *w_pose2_x9,
                      const void *w_headx_x9, gp_stream_t s);
int gp_pc_step_bf16x3(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const float *cvec, const float *tvec_all, const float *sched,
                      const float *z_langevin, const float *z_predictor, const float *centre, float *x, float *mean_x, float *score, float *partials,
                      float *traj, const void *w_pose0_split, const void *w_pose2_split, const void *w_headx_split, const float *b_pose0, const float *b_pose2,
                      const float *w_out, const float *b_out, gp_stream_t s);

/* Launch plan of the PC sampler for (ngroups x nclouds_per_group clouds x k candidates) and a model (see gp_pc_step_plan): tile = 0 asks for the automatic choice, else
 * 16 / 32 / 64 / 128 as in gp_score_eval_plan.  *tile_out = the plan taken, *nparts_out = partial sums of |score| per step
 * (`partials` must hold nsteps * nparts floats: one per workgroup in the tile form, one per wave in the chain form).  GP_EINVAL when a
 * workgroup of the plan would straddle two groups.  In the latency regime (score model, tiles x 3 <= CUs) the automatic choice is
 * 16 | GP_PLAN_HEADSPLIT (defined with the RK45 driver below): three workgroups per 16-row tile, one head of the network each; in its
 * `partials` every step keeps, per row, the three heads' sums of squares AND its own copies of the score and the state (nparts = 21 x rows:
 * three workgroups read a tile's state and score and each writes a part, so nothing a launch reads is written by the same launch; `x`
 * keeps the INITIAL state), and it refuses gn_ext (a sharded batch's caller sums per-tile partials: force tile = 16 there). */
int gp_pc_layout(int model, int tile, int ngroups, int nclouds_per_group, int k, int *tile_out, int *nparts_out);
/* gp_pc_step_coupled with the plan chosen by the caller (tile as above; 0 = automatic; every launch of one chain must use the same
 * plan) and the MODEL whose score drives the sampler: 0 = the score network (f / (sigma + 1e-7), scorenet.py:217); 1 = the ENERGY
 * network (`net` = its parameter block): the reference samples from it with the autograd gradient of its inner-product energy
 * (posenet.py:94-130 with PoseEnergyNet.forward(return_item='score'), energynet.py:200-222) - here the forward pass and the
 * vector-Jacobian product run inside the step kernel (tile = 16: through LDS, csrc/score_bwd.h; tile = 128: the register-resident chain
 * form, csrc/trunk_chain_vjp.h, which large launches take), so the energy model gets the same one-graph launch chain.
 * gn_ext / gn_rows_total: as gp_pc_step_coupled when gn_rows_total = 0 (gn_ext = the mean); with gn_rows_total > 0, gn_ext [nsteps][ngroups]
 * holds the SUM of |score| over all rows of the batch (this rank's per-group sum of `partials`, all-reduced in place) and
 * gn_rows_total that row count: one device-side sum and one all-reduce per step, both capturable in the sampler's hipGraph. */
int gp_pc_step_plan(int model, int tile, int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                    const float *tvec_all, const float *sched, const float *z_langevin, const float *z_predictor, const float *centre, float *x,
                    float *mean_x, float *score, float *partials, float *traj, const float *gn_ext, int gn_rows_total, gp_stream_t s);

/* SEEDED NOISE (opt-in; csrc/philox.h, csrc/noise.hip).  Replaces the two torch.randn_like draws of cond_pc_sampler (samplers.py:132,149)
 * by Philox4x32-10 + Box-Muller keyed by (seed, run, step, stream, GLOBAL row): a row draws the same values under every plan, in any
 * batch of a launch and on any shard, and no [nsteps][R][9] noise buffers exist.
 * seed_state: 8 x uint32 in DEVICE memory, read by the kernels at run time (a captured launch chain follows what the host copies there
 * in stream order before each replay): [0],[1] seed lo / hi, [2] run index, [4],[5] row base lo / hi (global row = row base + row of the
 * launch), [3],[6],[7] zero.  Normals are truncated at |z| <= 5.77 (uniforms on a 2^-24 grid in (0, 1]).
 *
 * gp_pc_step_plan_seeded / gp_pc_step_bf16x9_seeded: gp_pc_step_plan (score model: model 0) / gp_pc_step_bf16x9 with seed_state in place of
 * z_langevin / z_predictor; every other argument, plan and result as there, nsteps < 2^29.  Given buffers filled by gp_pc_noise_fill for
 * the same seed state, the unseeded entry points compute the same bits. */
int gp_pc_step_plan_seeded(int tile, int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                           const float *tvec_all, const float *sched, const void *seed_state, const float *centre, float *x, float *mean_x, float *score,
                           float *partials, float *traj, const float *gn_ext, int gn_rows_total, gp_stream_t s);
int gp_pc_step_bf16x9_seeded(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                             const float *tvec_all, const float *sched, const void *seed_state, const float *centre, float *x, float *mean_x, float *score,
                             float *partials, float *traj, const float *gn_ext, int gn_rows_total, const void *w_pose0_x9, const void *w_pose2_x9,
                             const void *w_headx_x9, gp_stream_t s);
/* gp_pc_step_bf16x6 with seed_state in place of the noise buffers, as gp_pc_step_bf16x9_seeded is to gp_pc_step_bf16x9. */
int gp_pc_step_bf16x6_seeded(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                             const float *tvec_all, const float *sched, const void *seed_state, const float *centre, float *x, float *mean_x, float *score,
                             float *partials, float *traj, const float *gn_ext, int gn_rows_total, const void *w_pose0_x9, const void *w_pose2_x9,
                             const void *w_headx_x9, gp_stream_t s);
/* The draws themselves (the values torch.randn_like returns at samplers.py:132 -> z_lang_out, :149 -> z_pred_out): for steps step0 ..
 * step0 + nsteps - 1 and rows row0 .. row0 + nrows - 1 of a launch, [nsteps][nrows][9] each (either may be NULL), exactly what the seeded
 * step kernels draw for them (the same device function). */
int gp_pc_noise_fill(const void *seed_state, int step0, int nsteps, int64_t row0, int64_t nrows, float *z_lang_out, float *z_pred_out, gp_stream_t s);
/* THE TRACKER'S PRIOR ON THE DEVICE (opt-in; csrc/noise.hip).  The reference's tracking loop (evaluation_tracking.py:262-337) starts every
 * frame's candidates at the previous frame's pose plus sigma(T0) times a standard normal draw (samplers.py:180); here the draw is the
 * seeded generator's, on counters no PC draw uses: step field = 2^29 - 1 (PC steps stay below it), stream 0, the seed state's run word = the
 * FRAME index, global row = row base + i * k + candidate (csrc/philox.h).
 * gp_track_warm_start: for cloud i < n and candidate c < k, x0[i * k + c] = init_i + sigma * z, the product and the sum rounded separately
 * (fp32 host arithmetic reproduces the bits), with init_i = [R[:,0], R[:,1], t - centre[i]] of prev_sRT[src[i]] when src[i] >= 0, else of
 * fallback_sRT[i] (evaluation_tracking.py:302-310).  prev_sRT, fallback_sRT [.,4,4] f32 row-major; src [n] int32; centre [n][3]; sigma: ONE
 * device float (the Heun schedule's first word, sigma(T0): a run-time value); x0 [n * k][9].
 * gp_track_prior_fill: the same draws as a buffer, z_out [nrows][9] for rows row0 .. row0 + nrows - 1 of the launch.
 * Both: GP_EINVAL on null pointers or negative sizes (k <= 0 included), GP_OK with nothing written for zero rows. */
int gp_track_warm_start(int n, int k, const void *seed_state, const float *sigma, const float *prev_sRT, const int *src, const float *fallback_sRT,
                        const float *centre, float *x0, gp_stream_t s);
int gp_track_prior_fill(const void *seed_state, int64_t row0, int64_t nrows, float *z_out, gp_stream_t s);
/* Raw Philox4x32-10 blocks (tests: bit-exactness against the published generator): counters [n][4], keys [n][2] -> out [n][4], uint32. */
int gp_philox_raw(int64_t n, const void *counters, const void *keys, void *out, gp_stream_t s);

/* FIXED-STEP HEUN SOLVER of the probability-flow ODE (opt-in).  Heun's second-order method on a sigma grid - the algorithm of
 * cond_edm_sampler (samplers.py:230-290), which the reference wires to a decoder only - driven by the VE score model through
 * denoised = x + sigma^2 score: slope d = -sigma score, fp32 state, no rotation renormalisation between steps, and after the last step the
 * reverse-diffusion predictor at eps, normalize_rotation and the cloud centre of cond_ode_sampler (:209-226).  Deterministic and ROW-LOCAL
 * (no noise, no batch statistic): a row's result does not depend on the rows that share its launch.  A solve of nsteps steps is a chain of
 * gp_heun_launches(nsteps, denoise) = 2 nsteps + 1 (+ 1 with denoise) launches, NFE = launches - 1:
 *     launch 0       evaluates score(x_0, t_0)
 *     launch 2i + 1  d_i = c score -> d;  evaluates score(x_i + h d_i, t_{i+1})                                  (kind 1)
 *     launch 2i + 2  x_{i+1} = x_i + h (0.5 d_i + 0.5 c score) -> x (and traj[i], rotation normalised, centre added);
 *                    evaluates score(x_{i+1}, t_{i+1})                                                            (kind 2)
 *     launch 2 nsteps      without denoise: the same update, finishes: -> out, no evaluation                      (kind 3)
 *     launch 2 nsteps + 1  with denoise: out = normalise(x + (0 - c^2 score) h) + centre                          (kind 4)
 * The kernels know nothing about the grid.  sched [launches][4] (device, f32): the sigma of the launch's evaluation (the score's divisor),
 * the slope factor c, the step h, the kind as above (0 for launch 0); tvec_all [nsteps + 1][768]: gp_time_embed of t_0 .. t_nsteps (launch l
 * evaluates at row (l + 1) / 2).  x [R,9] in / state; d, score [R,9] scratch; out [R,9]; traj [nsteps][R][9] or NULL; centre [clouds][3].
 * Plans: 16 / 32 / 64-row tiles and the 128-row chain form (tile as in gp_pc_layout, 0 = gp_heun_layout's choice); every launch of a
 * chain uses the same plan.  Not served: the head-split plan (GP_EINVAL; gp_heun_layout gives such sizes whole 16-row tiles), the energy
 * model (the _model forms below serve it), bf16x3.  GP_EINVAL with nothing written for nsteps < 1, launch outside [0, launches), null buffers or a plan that does not fit. */
int gp_heun_launches(int nsteps, int denoise);
/* The plan of a Heun chain (samplers.py:230-290): gp_pc_layout's row thresholds for the score model minus head-split; tile = 0 asks for
 * the choice, else 16 / 32 / 64 / 128.  GP_EINVAL when a workgroup of the plan would straddle two groups. */
int gp_heun_layout(int tile, int ngroups, int nclouds_per_group, int k, int *tile_out);
/* One launch of the chain (samplers.py:230-290) on plan `tile`; the chain plan (128) runs the fp32 MFMA chain kernel. */
int gp_heun_step_plan(int tile, int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                      const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                      gp_stream_t s);
/* The chain plan's launch (samplers.py:230-290) with the trunk as exact-product split bf16 (as gp_pc_step_bf16x9 is to gp_pc_step_plan):
 * the same buffers, w_*_x9 as there. */
int gp_heun_step_bf16x9(int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                        const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                        const void *w_pose0_x9, const void *w_pose2_x9, const void *w_headx_x9, gp_stream_t s);

/* The WHOLE solve in one launch, tile plans (csrc/heun_solve.hip; samplers.py:230-290).  The update is row-local, so the workgroup that owns
 * a tile's rows takes them through every launch index 0 .. gp_heun_launches(nsteps, denoise) - 1 of the chain above itself: the same row
 * update, the same trunk, the same divisor per index in the same order - x, out and traj hold afterwards, BIT FOR BIT, what the chain of
 * gp_heun_step_plan calls on the same plan leaves there (x = x_nsteps, out = the final pose, traj = x_1 .. x_nsteps).  Between the indices
 * x_i and d_i stay in registers and the score in LDS: `d` and `score` must be valid buffers (the chain's contract) but are not written.
 * sched and tvec_all are the chain's device buffers, so T0 and eps stay run-time values.  tile: 16 / 32 / 64, or 0 = gp_heun_layout's choice
 * provided that is one of them; GP_EINVAL with nothing written for the 128-row chain form (it keeps its per-launch kernels), the head-split
 * plan, nsteps < 1, null buffers or a plan that does not fit; zero rows: GP_OK.  Stateless, capturable. */
int gp_heun_solve_tile(int tile, int ngroups, int nclouds_per_group, int k, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                       const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                       gp_stream_t s);

/* DPM-SOLVER++(2M) FIXED-STEP SOLVER of the same probability-flow ODE (opt-in; ours - the reference has no multistep sampler).  The
 * second-order multistep exponential integrator in lambda = -ln sigma on the denoiser D = x + sigma^2 score: ONE evaluation per step, the
 * previous step's denoiser carried along, the linear part of the VE flow integrated exactly.  On gp_heun_launches' grid t_0 .. t_nsteps,
 * with h_i = lambda_{i+1} - lambda_i > 0 and r_i = (lambda_i - lambda_{i-1}) / h_i:
 *     D_i = x_i + sigma_i^2 score(x_i, t_i);   D~_i = D_0 (i = 0),  (1 + 1/(2 r_i)) D_i - (1/(2 r_i)) D_{i-1} (i >= 1)
 *     x_{i+1} = (sigma_{i+1} / sigma_i) x_i - expm1(-h_i) D~_i
 * fp32 state, no rotation renormalisation between steps; after step nsteps exactly what the Heun solver does (the reverse-diffusion
 * predictor at eps with denoise, normalize_rotation, the cloud centre).  Deterministic and ROW-LOCAL.  A solve of nsteps steps is a chain
 * of gp_dpm2m_launches(nsteps, denoise) = nsteps + 1 (+ 1 with denoise) launches, NFE = launches - 1:
 *     launch 0            evaluates score(x_0, t_0)
 *     launch i = 1 .. nsteps  D_{i-1} from the stored score and x_{i-1}; x_i = ratio x_{i-1} + (wc D_{i-1} + wp D_{i-2}) -> x, D_{i-1} -> d,
 *                         traj[i-1] (rotation normalised, centre added); evaluates score(x_i, t_i)                      (kind 2)
 *     launch nsteps       the same update -> out as well; evaluates at (x_nsteps, eps) only with denoise                  (kind 3)
 *     launch nsteps + 1   with denoise: out = normalise(x + (0 - c^2 score) h) + centre                                   (kind 4)
 * The kernels know nothing about the grid.  sched [launches][8] (device, f32; host float64 rounded once): [0] the sigma of the launch's
 * evaluation (the score's divisor), [1] sigma_{i-1}^2 (kind 4: c = g(eps)), [2] ratio = sigma_i / sigma_{i-1} (kind 4: the step h), [3] the
 * kind as above (0 for launch 0), [4] wc and [5] wp: the weights of D_{i-1} and D_{i-2} times -expm1(-h_{i-1}) - wp = 0 marks the first step,
 * whose launch does not read d - [6], [7] zero.  tvec_all [nsteps + 1][768]: gp_time_embed of t_0 .. t_nsteps (launch l evaluates at row l).
 * Buffers, plans (gp_heun_layout) and refusals as gp_heun_step_plan's; d holds the previous denoiser between launches. */
int gp_dpm2m_launches(int nsteps, int denoise);
/* One launch of the DPM-Solver++(2M) chain on plan `tile`; the chain plan (128) runs the fp32 MFMA chain kernel. */
int gp_dpm2m_step_plan(int tile, int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                       const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                       gp_stream_t s);
/* The chain plan's DPM-Solver++(2M) launch with the trunk as exact-product split bf16 (as gp_heun_step_bf16x9 is to gp_heun_step_plan):
 * the same buffers, w_*_x9 as there. */
int gp_dpm2m_step_bf16x9(int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                         const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                         const void *w_pose0_x9, const void *w_pose2_x9, const void *w_headx_x9, gp_stream_t s);
/* The WHOLE DPM-Solver++(2M) solve in one launch, tile plans (csrc/heun_solve.hip), as gp_heun_solve_tile is to gp_heun_step_plan: x, out
 * and traj hold afterwards, BIT FOR BIT, what the chain of gp_dpm2m_step_plan calls on the same plan leaves there; x_i, D_{i-1} and the
 * centre stay on chip, `d` and `score` are not written.  GP_EINVAL with nothing written for the 128-row chain form, the head-split plan,
 * nsteps < 1, null buffers or a plan that does not fit; zero rows: GP_OK.  Stateless, capturable. */
int gp_dpm2m_solve_tile(int tile, int ngroups, int nclouds_per_group, int k, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                        const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                        gp_stream_t s);

/* THE FIXED-STEP SOLVERS ON THE ENERGY MODEL (opt-in; ours).  The `_model` forms of the five entry points above take a leading `model`:
 * 0 launches exactly what the unsuffixed entry point launches; 1 drives the same solver, schedule, buffers and launch chain with the
 * ENERGY network's score - the gradient of its inner-product energy, f / sigma + J_f^T (x / sigma) (energynet.py:200-222), evaluated
 * inside the kernels by the forward + vector-Jacobian pass gp_pc_step_plan(model = 1) uses - in place of the score model's
 * f / (sigma + 1e-7) (samplers.py:230-290).  `net` then holds the energy network's weights and must carry the transposed packs
 * (w_headx_t, w_pose2_t, w_pose0_t): GP_EINVAL without them.  Model 1 has the 16-row tile form and the 128-row chain form only (fp32
 * MFMA; no 32 / 64-row tiles, no head-split, no bf16x9): GP_EINVAL for any other plan, and for a model other than 0 / 1. */
/* The plan of a fixed-step chain for `model` (samplers.py:230-290, energynet.py:200-222): model 0 is gp_heun_layout; model 1 takes
 * gp_pc_layout(model = 1)'s choice for tile = 0 (16 or 128), else 16 / 128.  GP_EINVAL for 32 / 64 / head-split under model 1, when the
 * chain form's workgroups would span more clouds than it stages (small k), or when a workgroup would straddle two groups. */
int gp_heun_layout_model(int model, int tile, int ngroups, int nclouds_per_group, int k, int *tile_out);
/* One launch of the Heun chain for `model` (samplers.py:230-290, energynet.py:200-222); arguments after `model` as gp_heun_step_plan. */
int gp_heun_step_plan_model(int model, int tile, int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net,
                            const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out,
                            float *traj, gp_stream_t s);
/* One launch of the DPM-Solver++(2M) chain for `model` (samplers.py:230-290's grid, energynet.py:200-222); arguments after `model` as
 * gp_dpm2m_step_plan. */
int gp_dpm2m_step_plan_model(int model, int tile, int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net,
                             const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out,
                             float *traj, gp_stream_t s);
/* The whole Heun / DPM-Solver++(2M) solve in one launch for `model` (samplers.py:230-290, energynet.py:200-222): the contract of
 * gp_heun_solve_tile / gp_dpm2m_solve_tile - x, out and traj BIT FOR BIT what the chain of gp_*_step_plan_model calls on the same plan
 * leaves.  Model 1 on plan 16 only (tile 16, or 0 where gp_heun_layout_model chooses 16): GP_EINVAL for the chain form. */
int gp_heun_solve_tile_model(int model, int tile, int ngroups, int nclouds_per_group, int k, int nsteps, int denoise, const gp_scorenet *net,
                             const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score,
                             float *out, float *traj, gp_stream_t s);
int gp_dpm2m_solve_tile_model(int model, int tile, int ngroups, int nclouds_per_group, int k, int nsteps, int denoise, const gp_scorenet *net,
                              const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score,
                              float *out, float *traj, gp_stream_t s);

/* SCHEDULE CLASSES ON THE FIXED-STEP SOLVERS (opt-in; ours): clouds that start from DIFFERENT times share the launches of one solve - a
 * tracker's objects continue from T0 = 0.15 around their previous pose while a newly seen one starts from the prior at T0 = 0.55 .. 1.
 * The `_classes` forms take the arguments of the `_model` forms above plus `ncls` (1 .. GP_MAX_SCHED_CLASSES) and `cls` [clouds] (device,
 * int32): the class of every cloud, clamped into [0, ncls - 1] on the device, so a bad table reads nothing outside the buffers.
 *     sched     [ncls][launches][row]     one schedule per class, each as gp_heun_step_plan / gp_dpm2m_step_plan describe it
 *     tvec_all  [ncls][nsteps + 1][768]   gp_time_embed of every class's times
 * Row r belongs to cloud r / k and class cls[r / k]; per row and launch it reads ITS class's values where the other entry points read the
 * launch's: the score's divisor sched[c][l][0], the update's coefficients (c, h; s2, ratio, wc, wp) and the time embedding added to the
 * cloud's cvec.  Control flow stays uniform: the launch kind - and DPM-Solver++(2M)'s "there is a previous denoiser", sched[.][l][5] != 0 -
 * is read from class 0, and the caller keeps the kind column identical in every class (the same nsteps and denoise for all).
 * CONTRACT: for every row of a cloud of class c, x, out and traj (and d, score on the chain) hold BIT FOR BIT what the entry point without
 * classes leaves for that row on the same plan and form when run uniformly on class c's sched / tvec_all; with ncls = 1 a `_classes` entry
 * equals its twin.  Served: model 0, the 16 / 32 / 64-row tile plans, per-launch chain and one-launch solve.  GP_EINVAL with nothing
 * written for model 1, the 128-row chain form (tile 128, or tile 0 where gp_heun_layout chooses it), the head-split plan, ncls outside
 * 1 .. GP_MAX_SCHED_CLASSES, a null cls, and everything the twins refuse.  Stateless, allocation-free, capturable. */
#define GP_MAX_SCHED_CLASSES 8
/* One launch of the Heun chain with schedule classes (samplers.py:230-290; the denoising launch: :209-218). */
int gp_heun_step_classes(int model, int tile, int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net,
                         const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out,
                         float *traj, int ncls, const int *cls, gp_stream_t s);
/* One launch of the DPM-Solver++(2M) chain with schedule classes (samplers.py:230-290's grid; the denoising launch: :209-218). */
int gp_dpm2m_step_classes(int model, int tile, int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net,
                          const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out,
                          float *traj, int ncls, const int *cls, gp_stream_t s);
/* The whole Heun solve in one launch with schedule classes (samplers.py:230-290, :209-218): gp_heun_solve_tile's contract per class. */
int gp_heun_solve_classes(int model, int tile, int ngroups, int nclouds_per_group, int k, int nsteps, int denoise, const gp_scorenet *net,
                          const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score,
                          float *out, float *traj, int ncls, const int *cls, gp_stream_t s);
/* The whole DPM-Solver++(2M) solve in one launch with schedule classes (samplers.py:230-290's grid, :209-218). */
int gp_dpm2m_solve_classes(int model, int tile, int ngroups, int nclouds_per_group, int k, int nsteps, int denoise, const gp_scorenet *net,
                           const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score,
                           float *out, float *traj, int ncls, const int *cls, gp_stream_t s);
/* The tracker's start states with a class per cloud (csrc/noise.hip): gp_track_warm_start that can ACQUIRE.  sched: the solve's schedule
 * block [ncls][launches][row], class_stride = launches * row floats; sigma_c = sched[c * class_stride], class c's sigma(T0_c).
 *     src[i] >= 0               x0 = init_i + sigma_0 z: gp_track_warm_start's arithmetic and bits (evaluation_tracking.py:302-310)
 *     src[i] < 0, acquire != 0  x0 = sigma_1 z: the pure prior of cond_ode_sampler with init_x = None (samplers.py:180) on class 1's T0, z the
 *                               draw the warm start would have used for the row (the same counters); fallback_sRT is not read, may be NULL
 *     src[i] < 0, acquire == 0  gp_track_warm_start's fallback_sRT[i], class 0
 * (acquire != 0 reads class 1's row: the block holds at least two classes.)
 * cls_out [n] (int32) <- the class of cloud i for the solve: src[i] < 0 when acquire != 0, else 0 - the class table is made on the device.
 * GP_EINVAL on null pointers (fallback_sRT only when acquire == 0), negative sizes, k <= 0, class_stride < 1; zero rows: GP_OK, nothing written. */
int gp_track_start_classes(int n, int k, const void *seed_state, const float *sched, int class_stride, const float *prev_sRT, const int *src,
                           const float *fallback_sRT, const float *centre, float *x0, int *cls_out, int acquire, gp_stream_t s);

/* FIXED-STEP HEUN SOLVE OF THE EXACT-LIKELIHOOD ODE (opt-in; csrc/heun_likelihood.hip).  cond_ode_likelihood's system (samplers.py:22-99)
 * d[x; logp]/dt = -g^2/2 [score; div_x score] with the exact divergence of gp_score_div_exact, integrated in sigma from sigma(eps) UP to
 * sigma(T) by Heun's method on a fixed grid (-g^2/2 dt = -sigma dsigma: slope d = -sigma [score; div]).  x and the slopes are fp32, the
 * log-density change is accumulated in float64; no rotation renormalisation, no denoise step, no centre.  Deterministic and ROW-LOCAL: the
 * result of a row is a function of its cloud, its pose and the schedule alone, whatever rows share the launch.  A solve of nsteps steps is
 * a chain of gp_heun_likelihood_launches(nsteps) = 2 nsteps + 1 launches, NFE = 2 nsteps (stream order is the only synchronisation):
 *     launch | update from the stored score / div                      | stores        | evaluates
 *     0      | -                                                       | -             | (x_0, t_0)
 *     2i + 1 | d = c (score, div), c = -sigma_i                        | d [R,10]      | (x_i + h_i d[x], t_{i+1})      (kind 1)
 *     2i + 2 | x, l += h_i (0.5 d + 0.5 c (score, div)), c = -sigma_{i+1} | x, logp    | (x_{i+1}, t_{i+1})             (kind 2)
 *     2N     | the same update                                         | z_out, logp   | nothing                        (kind 3)
 * The kernel knows nothing about the grid.  sched [launches][4] (device, f32): the sigma of the launch's evaluation (the divisor of score and
 * div), the factor c, the step h = sigma_{i+1} - sigma_i > 0, the kind as above (0 for launch 0); tvec_all [nsteps + 1][768]: gp_time_embed of
 * the ascending times t_0 = eps .. t_nsteps = T (launch l evaluates at row (l + 1) / 2).  x [R,9] in / state; d [R,10], score [R,9], div [R]
 * scratch; logp [R] f64: the log-density change, l_0 = 0 is part of the chain (launch 2 does not read it); z_out [R,9]: x at T.
 * 16-row tiles only.  GP_EINVAL with nothing written for null buffers, k <= 0, nsteps < 1, launch outside [0, launches) or a net without
 * the transposed packs; R == 0: GP_OK.  Stateless, capturable. */
int gp_heun_likelihood_launches(int nsteps);
/* One launch of that chain (samplers.py:22-99; the table above). */
int gp_heun_likelihood_step(int nclouds, int k, int launch, int nsteps, const gp_scorenet *net, const float *cvec, const float *tvec_all,
                            const float *sched, float *x, float *d, float *score, float *div, double *logp, float *z_out, gp_stream_t s);

/* The same launch with the batch-mean gradient norm SUPPLIED: gn_ext [nsteps][ngroups] (device) holds, for step i, the mean of
 * |score_i| over ALL rows of the batch each group belongs to.  For a batch that is sharded over several GPUs (SURVEY §8e caveat): the
 * host sums this rank's `partials` of step i, all-reduces the sum across the ranks and writes gn_ext[i] before launching step i+1, so
 * every shard takes the Langevin step size the unsharded batch would take (samplers.py:130-132).  gn_ext == NULL: gp_pc_step_grouped. */
int gp_pc_step_coupled(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                       const float *tvec_all, const float *sched, const float *z_langevin, const float *z_predictor,
                       const float *centre, float *x, float *mean_x, float *score, float *partials, float *traj, const float *gn_ext,
                       gp_stream_t s);

/* Probability-flow ODE sampler = cond_ode_sampler (samplers.py:163-227) over scipy's RK45 (rk.py / common.py):
 * Dormand-Prince 5(4), f64 state and controller resident in device memory, f32 score network, batch-global RMS
 * error norm, SAFETY 0.9 / MIN_FACTOR 0.2 / MAX_FACTOR 10, Hairer initial step.
 *   state   : opaque device block of gp_rk45_state_bytes() bytes (field offsets: gp_rk45_state_layout)
 *   y, ynew : [R*9] f64;  K : [7][R*9] f64;  partials : [3][ceil(R/tile)] f64;  tvec : [8][768] f32
 *   traj    : NULL or [traj_cap][R*9] f64 (accepted states; slot 0 = y0)
 * gp_rk45_phase launches one fixed, capture-safe sequence per call:
 *   0 reset(t0 -> t_bound, rtol, atol)   1 f0 + d0,d1 -> h0   2 f1 + d2 -> h_abs, first stage times
 *   3 ONE attempt: 6 fused stage kernels (stage update + score evaluation) + controller (+ trajectory record);
 *     a no-op once the device-side status word is non-zero
 *   4 set evaluation slot 0 to time `t0` (the denoise evaluation at eps)
 *   5 finish: denoise step (samplers.py:209-218) with scale `denoise_scale`, normalize_rotation, + centre -> x_out [R,9] f64,
 *     and the same post-processing of the first `nstates` trajectory states.
 * tvec is scratch owned by the solver: every kernel that decides stage times (reset, step controller, phase 4) writes their time
 * embeddings there itself (the arithmetic of gp_time_embed), so no launch separates the controller from the next stage kernel. */
int64_t gp_rk45_state_bytes(void);
/* Dense-output mode = solve_ivp(..., t_eval=np.linspace(T0, eps, n)) (samplers.py:201-205): call after phase 0 with traj = NULL
 * there; t_eval_dev [n_eval] f64 on the device, P_host = RK45's 7x4 dense-output matrix (row-major, HOST memory).  traj
 * [n_eval][R*9] then receives the 4th-order interpolant at every t_eval point (scipy RkDenseOutput). */
int gp_rk45_set_dense(void *state, const double *t_eval_dev, int n_eval, const double *P_host, gp_stream_t s);
int gp_rk45_state_layout(int64_t *offsets, int n); /* n >= 13: t,h_abs,status,n_attempts,n_accepted,nfev,err_norm,log_t,log_h,log_err,log_acc,stage_t,last_accepted */
int gp_rk45_phase(int phase, int nclouds, int k, const gp_scorenet *net, const float *cvec, float *tvec, const float *centre,
                  void *state, double *y, double *ynew, double *K, double *partials, double *traj, int traj_cap, double t0,
                  double t_bound, double rtol, double atol, double denoise_scale, int do_denoise, int nstates, double *x_out,
                  gp_stream_t s);

/* The same driver over `ngroups` independent batches that share every launch while keeping their OWN step controllers (error norm,
 * accept / reject and step size per group, exactly as separate solve_ivp calls); a finished group's workgroups exit at once.
 * Rows, clouds and solver states are laid out group-major: state = ngroups * gp_rk45_state_bytes(), tvec [ngroups][8][768]
 * (scratch), partials [3][nblocks] with
 * nblocks = ngroups * ceil(rows_per_group / tile), tile = gp_pc_tile_rows(ngroups, nclouds_per_group, k) (rows of a group must be
 * a multiple of it).  traj: every group writes its own rows at its own accepted-step slot. */
int gp_rk45_phase_grouped(int phase, int ngroups, int nclouds_per_group, int k, const gp_scorenet *net, const float *cvec, float *tvec,
                          const float *centre, void *state, double *y, double *ynew, double *K, double *partials, double *traj, int traj_cap,
                          double t0, double t_bound, double rtol, double atol, double denoise_scale, int do_denoise, int nstates, double *x_out,
                          gp_stream_t s);
/* The same driver for the right-hand sides it can integrate (`model`):
 *   0  gp_rk45_phase_grouped: probability-flow ODE of the score network;
 *   1  the same ODE driven by the ENERGY network's score, the gradient of its inner-product energy (posenet.py:94-130 on a
 *      PoseEnergyNet, energynet.py:200-222; `net` = the energy net's block) - forward + vector-Jacobian product inside the stage kernel;
 *   2  the likelihood ODE of cond_ode_likelihood (samplers.py:22-99): state [R][10] = pose and accumulated log-density change,
 *      d logp / dt = -g^2/2 probe^T (d score / d x) probe with the fixed Skilling-Hutchinson `probe` [R][9] (device); y, ynew [R*10],
 *      K [7][R*10]; one error norm over all R*10 components (scipy integrates the concatenated vector); phase 5 copies the final
 *      state to x_out [R][10] (no denoise / normalisation); phases 4 and the trajectory arguments are unused.
 *   4  GP_RK45_MODEL_LIKELIHOOD_EXACT: model 2 with the EXACT divergence, d logp / dt = -g^2/2 tr(d score / d x) (the stage arithmetic of
 *      gp_score_div_exact): the same ten-component state, controller, error norm, status words and phase 5; `probe` must be NULL; plan 16
 *      (or 0) only - it has no chain form.  (3 stays an unknown model: GP_EINVAL.)
 * Models 1, 2 and 4 run on 16-row tiles: partials [3][ngroups * ceil(rows_per_group / 16)].
 * A batch SHARDED over several GPUs (SURVEY §8e caveat: scipy's error norm runs over the whole batch): ext_sums [2][ngroups] (device,
 * f64) and ext_rows_per_group = rows of a group over all ranks.  Phases 1, 2, 3 then stop after writing this rank's per-group sums of
 * squares to ext_sums; the caller all-reduces ext_sums (RCCL: capturable with the launches) and runs phase 11, 12 or 13 = the step
 * controller on the reduced sums (+ trajectory record).  Every shard then takes the accept / reject sequence of the unsharded batch.
 * ext_sums = NULL: the controller reduces the local partials itself (phases 11-13 are GP_EINVAL).
 * plan: rows per workgroup of the stage kernels - 16 / 32 / 64 = tile form (models 1 and 2, which need the backward pass: 16 only), 128 = the
 * chain form of the trunk (every model; k >= 43, rows_per_group % 128 == 0 when ngroups > 1); 16 | GP_PLAN_HEADSPLIT = the latency
 * regime's head-split plan (score model): THREE workgroups per 16-row tile, each recomputing pose_encoder and evaluating one head
 * (scorenet.py:178-222: the three fusion tails are independent given the pose features) - half the weight stream and half the MFMA issue
 * per workgroup, 3x the CUs; every stage of an attempt is then a launch of its own (a stage reads all nine components of the previous
 * one); recommended by gp_rk45_plan_rows() while tiles x 3 <= CUs (gp_plan_headsplit_pays).  0 = a whole-tile plan is picked.
 * partials: gp_rk45_partials_count() doubles ([3][ngroups * ceil(rows_per_group / rows per workgroup) * (3 under the head-split plan)]). */
#define GP_PLAN_HEADSPLIT 0x100
#define GP_RK45_MODEL_LIKELIHOOD_EXACT 4
/* 16 | GP_PLAN_SHARED or 48 | GP_PLAN_SHARED (round 6; score model, one group; picked by gp_rk45_plan_rows() when it applies): the SHARED-CHUNK plan for
 * launches whose 16-row chunks do not divide over the CUs - T chunks on C CUs with T / C = 1 or 3 and 6 (T mod C) <= C, e.g. the 12 800 rows
 * of scripts/eval_single.sh's batches (800 chunks on 256 CUs).  An attempt is ONE launch of C workgroups: each owns T / C whole chunks for
 * all six stages, and the 6 x (T mod C) (chunk, stage) units of the left-over chunks are dealt out one per workgroup, so the busiest CU
 * evaluates 6 x (T / C) + 1 chunk-stages per attempt instead of 6 x (T / C + 1) (csrc/rk45.hip: rk45_attempt_shared_kernel).  The other
 * phases run on the whole-tile plan.  Results: every row's right-hand side is the 32- / 64-row tile plans' bit for bit (the four-wave tiles form
 * the output sums in their order, score_trunk.h ORDER8); the error norm's partial sums add in another order (poses within 1e-13 of theirs). */
#define GP_PLAN_SHARED 0x200
int gp_plan_headsplit_pays(int ntiles16); /* 1 while three workgroups per 16-row tile still get a CU each */
/* The plan the driver recommends for a launch (may carry GP_PLAN_HEADSPLIT / GP_PLAN_SHARED) and the number of doubles `partials` must hold
 * under a plan (plan = 0: what gp_rk45_phase_model resolves 0 to - always a WHOLE-tile plan, so that a buffer of 3 x ceil(rows / 16) doubles
 * per group, the size the entry points without a plan argument document, stays sufficient; the head-split and shared-chunk plans are taken
 * only when passed explicitly - ABI note in INTEGRATION.md section 3). */
int gp_rk45_plan_rows(int model, int ngroups, int nclouds_per_group, int k);
int gp_rk45_plan_rows_unshared(int model, int ngroups, int nclouds_per_group, int k); /* the same without GP_PLAN_SHARED (ext_sums callers) */
int gp_rk45_partials_count(int model, int plan, int ngroups, int nclouds_per_group, int k);
int gp_rk45_phase_model(int model, int plan, const float *probe, int phase, int ngroups, int nclouds_per_group, int k, const gp_scorenet *net, const float *cvec,
                        float *tvec, const float *centre, void *state, double *y, double *ynew, double *K, double *partials, double *traj,
                        int traj_cap, double t0, double t_bound, double rtol, double atol, double denoise_scale, int do_denoise, int nstates,
                        double *x_out, double *ext_sums, int ext_rows_per_group, gp_stream_t s);
/* The score model's chain plan (gp_rk45_phase_model(model = 0, plan = 128)) with a second ARITHMETIC of the stage kernels' trunk: the three
 * dense layers as exact-product split bf16 on the BF16 matrix pipe (csrc/rk45.hip: rk45_stage_chain_kernel_bf16x9; every fp32 operand is
 * hi + mid + lo, all nine cross products are exact, only the fp32 accumulation rounds - the error class of the fp32 MFMA stage kernels, as
 * gp_pc_step_bf16x9 is to gp_pc_step_plan).  w_*_x9: the packs of weights.pack_bf16x9 (device).  No new plan: phases 1, 2 and 3 launch the
 * split-bf16 stage kernels; the step controller, the time embeddings, the trajectory / dense-output record, the sharded batch's group sums
 * (ext_sums, phases 11-13) and phases 0, 4 and 5 are plan 128's own code, on the same grid, state and buffers (partials:
 * gp_rk45_partials_count(0, 128, ...) doubles).  Serves the shapes plan 128 serves - k >= 43, rows_per_group % 128 == 0 when ngroups > 1 -
 * and returns GP_EINVAL for every other.  Opt-in (ODESampler(trunk="bf16x9")): results differ from the fp32 chain's in the last bits. */
int gp_rk45_phase_bf16x9(int phase, int ngroups, int nclouds_per_group, int k, const gp_scorenet *net, const float *cvec, float *tvec, const float *centre,
                         void *state, double *y, double *ynew, double *K, double *partials, double *traj, int traj_cap, double t0, double t_bound,
                         double rtol, double atol, double denoise_scale, int do_denoise, int nstates, double *x_out, double *ext_sums,
                         int ext_rows_per_group, const void *w_pose0_x9, const void *w_pose2_x9, const void *w_headx_x9, gp_stream_t s);
/* Ragged variant: groups with different numbers of clouds (tracking: the objects of one frame form a group, frames of different
 * sequences share the launches).  grp_info [ngroups][4] = {first workgroup, workgroups, rows, first row}; blk_info [nblocks][3] =
 * {group, first row, end row (exclusive) of the group} per workgroup of `tile` (16 or 32) rows; both device int32.  Rows stay
 * cloud-major (k rows per cloud), groups occupy consecutive row ranges. */
int gp_rk45_phase_ragged(int phase, int ngroups, const int32_t *grp_info, int nblocks, const int32_t *blk_info, int tile, int nclouds_total, int k,
                         const gp_scorenet *net, const float *cvec, float *tvec, const float *centre, void *state, double *y, double *ynew,
                         double *K, double *partials, double *traj, int traj_cap, double t0, double t_bound, double rtol, double atol,
                         double denoise_scale, int do_denoise, int nstates, double *x_out, gp_stream_t s);
int gp_rk45_set_dense_grouped(int ngroups, void *state, const double *t_eval_dev, int n_eval, const double *P_host, gp_stream_t s);

/* ------------------------------------------------------------------------------------------------
 * D. Ranking and aggregation (reward.py:131-155, sgpa_utils.py:897-954, evaluation_tracking.py:60-77)
 * ------------------------------------------------------------------------------------------------ */

/* poses [b,k,9] f32/f64 (is_f64), energy [b,k,2] f32 -> sorted_poses (same dtype), sorted_energy [b,k,2],
 * order [b,k,2] i32 (stable descending), avg_pose [b,7] f32 (w,x,y,z,tx,ty,tz) over the top `sel` candidates.
 * Limits: 1 <= k <= GP_RANK_MAX_K; 1 <= sel <= k when avg_pose is given (sel is ignored without it); b >= 0, b == 0 launches nothing.
 * Anything else returns GP_EINVAL before a launch.  Every (k, sel) inside the limits is served: one wave per cloud keeps the energies,
 * the ranking and the selected quaternions in 16 k + 16 + 32 sel bytes of LDS - above the 64 KB default from sel = k = 1366 on, 98 320 at
 * sel = k = GP_RANK_MAX_K - and the entry point raises both kernels' dynamic-LDS limit to that maximum on its first call with b > 0, which
 * therefore has to come outside a stream capture (the runners' warm-up); GP_ELAUNCH when the runtime refuses.  The ranking compares
 * k (k - 1) pairs per column on ONE wave: meant for tens to hundreds of candidates, milliseconds at the limit. */
#define GP_RANK_MAX_K 2048
int gp_rank_aggregate(int b, int k, int sel, int is_f64, const void *poses, const float *energy, void *sorted_poses,
                      float *sorted_energy, int32_t *order, float *avg_pose, gp_stream_t s);
/* The same launch with the 4x4 forms the runners hand on written by it as well (either may be NULL): sorted_rt [b,k,4,4] f64 =
 * gp_pose9_to_rt(sorted_poses), avg_rt [b,4,4] f32 = gp_quat_trans_to_rt(avg_pose) - bit for bit; the ranking step of a tracking frame
 * (evaluation_tracking.py:316-330: energies -> sort -> average) is then one launch behind the energy evaluation. */
int gp_rank_aggregate_rt(int b, int k, int sel, int is_f64, const void *poses, const float *energy, void *sorted_poses,
                         float *sorted_energy, int32_t *order, float *avg_pose, double *sorted_rt, float *avg_rt, gp_stream_t s);

/* The 4x4 homogeneous matrices the runners hand on (evaluation_single.py:325-332, evaluation_tracking.py:60-77), one launch each instead of
 * ~15 tensor operations: poses [n][9] (f32 or f64: is_f64) -> out [n][4][4] f64 (Gram-Schmidt of the two rotation columns in f64, as
 * get_rot_matrix on float64 rows); quat_trans [n][7] f32 (w, x, y, z, t - gp_rank_aggregate's avg_pose) -> out [n][4][4] f32 (pytorch3d
 * quaternion_to_matrix). */
int gp_pose9_to_rt(int n, int is_f64, const void *pose, double *out, gp_stream_t s);
int gp_quat_trans_to_rt(int n, const float *quat_trans, float *out, gp_stream_t s);

/* Consensus ranker (ours): an "energy" array [b,k,2] f32 for gp_rank_aggregate(_rt) that needs no network - a candidate's score is minus
 * its mean distance to the cloud's other candidates (higher = closer to the rest = first), rotation (column 0) and translation (column 1)
 * independently.  In float64, for cloud b with candidates i = 0..k-1:
 *   R_i   the Gram-Schmidt matrix of pose[0:6] (gp_pose9_to_rt's, same 1e-12 floors), t_i = pose[6:9];
 *   candidate i is finite when all nine inputs are; m = the cloud's finite candidates;
 *   dR_ij = 2 asin(min(1, |R_i - R_j|_F / (2 sqrt 2)))   the geodesic angle in chordal form (sym[b] == 0), or
 *           2 asin(min(1, |y_i - y_j| / 2))              y = the second column of R (sym[b] != 0: symmetric about the y axis);
 *   dT_ij = |t_i - t_j|_2;
 *   s_i[c] = -(sum over finite j != i, ascending j, of d_ij) / max(1, m - 1), stored as float32.
 * A non-finite candidate scores -inf in both columns and enters no other sum.  d_ij is bitwise symmetric (element differences squared and
 * summed in one fixed order), so duplicates and k = 2 tie exactly and the stable ranking keeps candidate order.  No tunable.
 * One wave per cloud; every candidate's R and t sit in LDS in float64 (100 bytes each, + 8 for the ranking), which serves
 * k <= GP_CONSENSUS_MAX_K within the default 64 KB; a larger k returns GP_EINVAL.  sym: int8 [b] or NULL (no cloud symmetric).
 * Cost: k (k - 1) float64 distances per cloud on ONE wave - measured (profiles/consensus_ranker.txt) 29 us at k = 50 and 2.2 ms at the cap,
 * whatever b up to the device's wave slots; it is meant for tens of candidates. */
#define GP_CONSENSUS_MAX_K 512
int gp_consensus_energy(int b, int k, int is_f64, const void *poses, const int8_t *sym, float *energy_out, gp_stream_t s);
/* The score followed by everything gp_rank_aggregate_rt does, in ONE launch: bit for bit gp_consensus_energy + gp_rank_aggregate_rt.
 * energy_out [b,k,2] is optional like every output; argument rules as gp_rank_aggregate_rt.  It saves a launch and the round trip of the
 * array (1.2 - 1.5 us of 51 - 54 at k = 50); at k = 512 it was measured SLOWER than the two launches (2.62 against 2.54 ms). */
int gp_consensus_rank_aggregate_rt(int b, int k, int sel, int is_f64, const void *poses, const int8_t *sym, float *energy_out, void *sorted_poses,
                                   float *sorted_energy, int32_t *order, float *avg_pose, double *sorted_rt, float *avg_rt, gp_stream_t s);

/* Mode-seeking aggregation (ours): a kernel density over a cloud's candidates and a mean shift from the densest one, in place of the mean
 * over the selected candidates - a mean over two modes is a pose of neither.  Rotation (c = 0) and translation (c = 1) independently, as
 * the ranking treats them; float64 throughout.  For cloud b:
 *   R_i, t_i, "finite", dR_ij, dT_ij   exactly gp_consensus_energy's (sym[b] != 0: dR is the angle between the y axes);
 *   w_j[c] = weight[b][j][c] if it is > 0 and candidate j is finite, else 0 (weight == NULL: 1 for every finite j); W[c] = sum_j w_j[c];
 *   kappa_c(d) = exp(-d^2 / (2 h_c^2)), h_0 = bw_rot (radians), h_1 = bw_trans (metres);
 *   density[b][i][c] = (sum over j, ascending, i included, of w_j kappa_c(d_ij)) / W, stored as float32; -inf for a non-finite i.  Every i
 *                      sums in the same order, so duplicates tie exactly; the array ranks through gp_rank_aggregate like any energy;
 *   start[b][c]      = the lowest index with w_i > 0 that maximises the float64 density;
 *   mean shift, `iters` times from the start candidate, u_j = w_j kappa_c(d(centre, x_j)):
 *     translation     centre <- sum u_j t_j / sum u_j;
 *     rotation        A = sum u_j q_j q_j^T / sum u_j, q_j = pytorch3d matrix_to_quaternion(R_j); centre <- the eigenvector of A's largest
 *                     eigenvalue (float64 Jacobi), w >= 0, as a matrix (quaternion_to_matrix);
 *     symmetric cloud y <- normalize(sum u_j y_j); when iters > 0 the rotation written is the start candidate's R turned by the minimal
 *                     rotation that takes its y axis onto y (opposite axes, 1 + y_s . y < 1e-12: the half turn about R's x axis);
 *     sum u_j == 0, or a new axis of norm < 1e-12: the centre stays where it is;
 *   mass[b][c]       = sum_j w_j kappa_c(d(final centre, x_j)) / W in [0, 1]: the weighted share of the candidates the mode explains.
 * mode_pose [b,7] f32 = (w, x, y, z, t) with w >= 0, avg_pose's layout; mode_rt [b,4,4] f32 = gp_quat_trans_to_rt(mode_pose) bit for bit;
 * mass [b,2] f32; start [b,2] i32; density [b,k,2] f32.  W[c] == 0: the identity quaternion (c = 0) / the zero translation (c = 1),
 * mass 0, start -1, density 0 for the finite candidates.  The weights have to be finite.  Every output is optional (NULL).
 * Limits: 1 <= k <= GP_CONSENSUS_MAX_K; bw_rot, bw_trans finite and > 0; 0 <= iters <= GP_MODE_MAX_ITERS; b >= 0, b == 0 launches
 * nothing; poses != NULL.  Anything else returns GP_EINVAL before a launch.  No allocation, no synchronisation: capture-safe; a cloud's
 * outputs do not depend on the rest of the batch.
 * One wave per cloud.  LDS: R, t and the flag as gp_consensus_energy stages them and the two effective weights, 108 bytes a candidate,
 * 55 296 at the cap - within the default 64 KB.  The quaternions are not staged beside the matrices (that passes 64 KB at k = 512): each
 * iteration recomputes them from the matrices.
 * Cost per cloud on ONE wave: 2 k^2 float64 distances and exp for the density (lanes over i, serial over j), then (iters + 1) passes of
 * 2 k distances and exp (lanes over j, a wave reduction) with one 4x4 Jacobi each - measured (profiles/mode_aggregate.txt) 144 - 160 us at
 * k = 50 with 8 iterations (the density 26 - 29 us, an iteration ~14 us, 12 of them the Jacobi) and 2.0 ms at the cap, whatever b up to the
 * device's wave slots; gp_rank_aggregate_rt took 23 - 25 us and 0.38 ms in the same session.  Meant for tens of candidates. */
#define GP_MODE_MAX_ITERS 64
int gp_mode_aggregate(int b, int k, int is_f64, const void *poses, const int8_t *sym, const float *weight, double bw_rot, double bw_trans,
                      int iters, float *density, float *mode_pose, float *mode_rt, float *mass, int32_t *start, gp_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* GENPOSE_HIP_H */
