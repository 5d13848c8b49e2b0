/*
 * r3d.h -- C ABI of lib3d_reconstruction_project_amd (libr3d_hip.so): the MI355X (gfx950) hot path of the
 * stereo-depth + point-cloud fusion pipeline.
 *
 * The reference (aagsi/3D_Reconstruction_Project) has NO FFI of its own: it is Python glue that calls
 * third-party C++ (OpenCV, Open3D) through their Python bindings.  Each entry point below therefore cites the
 * reference call site (file:line under /root/reference) whose third-party call it replaces; INTEGRATION.md
 * shows the ctypes stub a maintainer would add at that call site.
 *
 * Conventions: plain pointers and sizes only (no torch / numpy types); every function returns 0 (R3D_OK) or a
 * negative R3D_E_* code and leaves a message retrievable by r3d_last_error().  "not converged" is NOT an error.
 * One r3d_ctx = one HIP device + one HIP stream + a grow-only device workspace; calls on one ctx must be
 * serialised by the caller (the reference issues its hot calls from one worker thread, main.py:56-61);
 * different ctxs may be used from different threads.  `_dev` variants take DEVICE pointers, enqueue on the
 * ctx stream and do not synchronise; the others take HOST pointers, copy in/out and return after completion.
 */
#ifndef R3D_H
#define R3D_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R3D_OK 0
#define R3D_E_BADARG (-1)      /* null pointer, bad size, parameter outside the documented domain */
#define R3D_E_HIP (-2)         /* a HIP runtime call failed; message holds hipGetErrorString */
#define R3D_E_OOM (-3)         /* device or host allocation failed */
#define R3D_E_UNSUPPORTED (-4) /* valid for the reference, outside this library's exact-arithmetic envelope */
#define R3D_E_NODEVICE (-5)    /* no gfx950 device visible */
#define R3D_E_INTERNAL (-6)    /* a capped device loop ran over its cap: a defect of the library, reported in place of a hang */

typedef struct r3d_ctx r3d_ctx;

/* ---- context ------------------------------------------------------------------------------------------- */
/* replaces: o3d.core.Device("CUDA:0") literals (normal_estimation.py:10, pointcloud_processing.py:12) */
int r3d_init(int device, r3d_ctx **out);
void r3d_destroy(r3d_ctx *ctx);
const char *r3d_last_error(const r3d_ctx *ctx); /* ctx may be NULL: returns the last r3d_init error */
int r3d_sync(r3d_ctx *ctx);                     /* hipStreamSynchronize on the ctx stream */
/* hip_stream: a hipStream_t.  NULL = back to the ctx-owned stream (created hipStreamNonBlocking: NOT ordered against the null
 * stream).  The legacy null stream is therefore not selectable as 0: pass hipStreamLegacy ((hipStream_t)1) for it, or -- what the
 * Python layer does (distributed.shared_stream) -- make a named stream current on the caller's side and pass that. */
int r3d_set_stream(r3d_ctx *ctx, void *hip_stream);
void *r3d_get_stream(r3d_ctx *ctx);
/* the ctx stream waits for a hipEvent_t (created by r3d_event_create on any ctx of this device, or by the caller): the join
 * between two contexts / streams without a host synchronisation */
int r3d_stream_wait_event(r3d_ctx *ctx, void *hip_event);
/* diagnostic: prices an access shape (rows independent streams of row_bytes; mode 0 = 256 B, 1 = 1 KB per wave request) */
int r3d_debug_streambench(r3d_ctx *ctx, int32_t mode, int32_t rows, uint64_t row_bytes, int32_t write, int32_t delay, int32_t reps, float *ms);
/* diagnostic: the stable sort of point indices by (cell key, index) that every grid / voxel build starts with.  key_order 0: x
 * fastest (search grid), 1: legacy voxel index (z fastest), 2: Morton code of the cell, 3: tensor voxel index; impl 0: the
 * hand-written run-based counting sort (default path), 1: the library radix sort (fallback path).  keys_out may be NULL. */
int r3d_debug_sort_by_cell(r3d_ctx *ctx, const double *xyz, int64_t n, const double *org3, double cell, const int32_t *dims3, int32_t key_order,
                           int32_t impl, int32_t *idx_out, uint64_t *keys_out);
/* diagnostic: the hand-written exclusive scan (k_scan_sums + k_scan_apply) on n int32 host values; op 0 = sum, 1 = running maximum
 * (values >= 0).  out[i] = op over in[0 .. i-1], out[0] = 0. */
int r3d_debug_exclusive_scan(r3d_ctx *ctx, const int32_t *in, int64_t n, int32_t op, int32_t *out);
/* diagnostic: the registration's correspondence search on its own.  Runs r3d_icp's set-up in the point-to-point mode (target grid,
 * packed / exact candidate selection, Morton sort of the source; the same R3D_ICP_* and R3D_CELL_TABLE switches) and ONE
 * evaluation at pose T4x4 (NULL: identity).  corr_out[i]: index into tgt of the target nearest to T * src[i] under (squared
 * distance, index), or -1 when that distance is not below max_correspondence_distance; d2_out (may be NULL): the squared
 * distance, 1e300 where there is none. */
int r3d_debug_icp_correspondences(r3d_ctx *ctx, const double *src, int64_t ns, const double *tgt, int64_t nt,
                                  double max_correspondence_distance, const double *T4x4, int32_t *corr_out, double *d2_out);
/* checks the cross-lane primitives (DPP shifts, permlane swaps, wave reductions) the kernels rely on */
int r3d_selftest(r3d_ctx *ctx);

/* device memory + timing helpers so that a host language without a HIP binding (Python/ctypes) can keep
 * inputs resident in HBM and time kernels with HIP events on the ctx stream */
int r3d_dev_alloc(r3d_ctx *ctx, uint64_t bytes, void **out_dev_ptr);
int r3d_dev_free(r3d_ctx *ctx, void *dev_ptr);
int r3d_copy_h2d(r3d_ctx *ctx, void *dev_dst, const void *host_src, uint64_t bytes);
int r3d_copy_d2h(r3d_ctx *ctx, void *host_dst, const void *dev_src, uint64_t bytes);
int r3d_event_create(r3d_ctx *ctx, void **out_event);
int r3d_event_destroy(r3d_ctx *ctx, void *event);
int r3d_event_record(r3d_ctx *ctx, void *event);                        /* on the ctx stream */
int r3d_event_elapsed_ms(r3d_ctx *ctx, void *start, void *stop, float *out_ms); /* synchronises `stop` */

/* diagnostic: what this library holds on the GPU right now, summed over every context, model and volume of the process (a leak
 * shows as a count that does not return to its earlier value once they are destroyed).  device_allocs counts r3d_dev_alloc
 * handles too; device_bytes only the buffers the library owns itself.  Needs no context and no device. */
typedef struct r3d_resource_counts {    /* 40 bytes */
    int64_t device_allocs, device_bytes, pinned_allocs, events, streams;
} r3d_resource_counts;
int r3d_debug_resources(r3d_resource_counts *out);

/* ---- stereo: semi-global block matching, 3-way ------------------------------------------------------------
 * replaces: cv2.StereoSGBM_create(**kwargs) + matcher.compute(gray_left, gray_right)
 *   Calib_depth/depth1.py:202-214,331  depth2.py:146-158,251  depth3.py:234-246,339
 *   Calib_depth/depth4.py:156-168,254  depth_test.py:162-174,260
 * Field names and meaning equal the StereoSGBM_create keyword arguments the reference passes.
 * mode: R3D_SGBM_MODE_3WAY (cv2.STEREO_SGBM_MODE_SGBM_3WAY == 2) or R3D_SGBM_MODE_HH (cv2.STEREO_SGBM_MODE_HH == 1: eight
 * full-image paths, no stripes); MODE_SGBM (0) and MODE_HH4 (3) are refused with R3D_E_UNSUPPORTED. */
#define R3D_SGBM_MODE_HH 1
#define R3D_SGBM_MODE_3WAY 2
typedef struct {
    int32_t minDisparity;
    int32_t numDisparities; /* multiple of 16, <= 512 (above 256: default kernel generation only; 1 KB per cost column and volume) */
    int32_t blockSize;      /* odd, 1..11 */
    int32_t P1, P2;
    int32_t disp12MaxDiff;
    int32_t preFilterCap;
    int32_t uniquenessRatio;
    int32_t speckleWindowSize;
    int32_t speckleRange;
    int32_t mode;
} r3d_sgbm_params;

/* left/right: uint8 single-channel rectified images, `stride` bytes per row; disp: int16 w*h, disparity x16,
 * invalid = (minDisparity-1)*16, columns outside [max(minD+D,0), w+min(minD,0)) invalid -- as matcher.compute */
int r3d_sgbm_compute(r3d_ctx *ctx, const r3d_sgbm_params *p, const uint8_t *left, const uint8_t *right, int32_t w,
                     int32_t h, int32_t stride, int16_t *disp);
int r3d_sgbm_compute_dev(r3d_ctx *ctx, const r3d_sgbm_params *p, const uint8_t *d_left, const uint8_t *d_right,
                         int32_t w, int32_t h, int32_t stride, int16_t *d_disp);

/* The same for pairs of `cn` channels, as cv2.StereoSGBM.compute takes CV_8UC1 or CV_8UC3: cn = 1 (the calls above) or cn = 3,
 * interleaved (pixel x of a row at byte x*cn, any channel order), `stride` bytes per row >= w*cn; any other cn: R3D_E_BADARG.
 * A 3-channel pair's pixel cost is the sum over the channels of the single-channel cost of that channel's plane (OpenCV's
 * calcPixelCostBT with cn == 3; hence the 3 in the usual P1 = 8*3*bs^2, P2 = 32*3*bs^2); everything after the block cost is
 * unchanged.  The exact-int16 envelope carries the channel count: cn * blockSize^2 * (2*ftzero + 63) > 32767 is refused
 * (R3D_E_UNSUPPORTED), above 16383 the call fails only if this pair's summed block cost really passes 16383 (preFilterCap 63,
 * cn = 3: blockSize <= 5 always fits, 7 depends on the images, >= 9 is refused).  Default kernel generation only. */
int r3d_sgbm_compute_cn(r3d_ctx *ctx, const r3d_sgbm_params *p, const uint8_t *left, const uint8_t *right, int32_t w,
                        int32_t h, int32_t stride, int32_t cn, int16_t *disp);
int r3d_sgbm_compute_cn_dev(r3d_ctx *ctx, const r3d_sgbm_params *p, const uint8_t *d_left, const uint8_t *d_right,
                            int32_t w, int32_t h, int32_t stride, int32_t cn, int16_t *d_disp);

/* n independent pairs of equal size (a multi-view batch, BASELINE config C5, or consecutive video frames): the maps
 * are spread over up to 3 internal lanes (own stream + workspace each) so that kernels of different maps overlap;
 * forks from / joins into the ctx stream, i.e. to the caller it behaves like n r3d_sgbm_compute_dev calls. */
int r3d_sgbm_compute_batch_dev(r3d_ctx *ctx, const r3d_sgbm_params *p, int32_t n, const uint8_t *const *d_left,
                               const uint8_t *const *d_right, int32_t w, int32_t h, int32_t stride, int16_t *const *d_disp);
/* the same, and map i's completion is recorded into done_events[i] (hipEvent_t, may be NULL per entry) on the lane that ran it:
 * a consumer on ANOTHER stream / context (r3d_stream_wait_event) can start on map i while later maps are still in flight
 * (the C5 view chain on one GPU: the cloud stages of view i run underneath the SGM kernels of views i+1 ...) */
int r3d_sgbm_compute_batch_events_dev(r3d_ctx *ctx, const r3d_sgbm_params *p, int32_t n, const uint8_t *const *d_left,
                                      const uint8_t *const *d_right, int32_t w, int32_t h, int32_t stride, int16_t *const *d_disp,
                                      void *const *done_events);

/* the batch for pairs of cn channels (1 or 3, as r3d_sgbm_compute_cn); done_events may be NULL (no events) */
int r3d_sgbm_compute_batch_cn_dev(r3d_ctx *ctx, const r3d_sgbm_params *p, int32_t n, const uint8_t *const *d_left,
                                  const uint8_t *const *d_right, int32_t w, int32_t h, int32_t stride, int32_t cn,
                                  int16_t *const *d_disp, void *const *done_events);

/* cv2.filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) on an int16 image, in place (host buffer): the last stage of
 * StereoSGBM.compute when speckleWindowSize > 0 (Calib_depth/depth4.py:164-165, depth_test.py:170-171) */
int r3d_filter_speckles(r3d_ctx *ctx, int16_t *img, int32_t w, int32_t h, int32_t new_val, int32_t max_speckle_size, int32_t max_diff);

/* per-kernel HIP-event timing (events on the ctx stream around every kernel launch while profiling is enabled).
 * r3d_sgbm_profile returns, and then resets, the AVERAGE launch duration per kernel over all r3d_sgbm_compute*
 * calls since the previous r3d_sgbm_profile.  names: NUL-separated list, one entry per slot; ms: one float per
 * slot.  Returns the number of slots.  (Events live in a 4-deep ring, so profiling never stalls the stream.) */
int r3d_set_profiling(r3d_ctx *ctx, int enabled);
int r3d_sgbm_profile(r3d_ctx *ctx, float *ms, int32_t max_slots, char *names, int32_t names_bytes);

/* debug / stage parity: copies intermediate results of the LAST sgbm call to HOST buffers (NULL = skip).
 *   cost   int16 [h][w1][dp]  aggregated block cost C, summed over the channels of a colour pair (dp = the smallest of 32 / 64 / 128 / 256 / 512
 *                             that holds D; entries d>=D undefined).  A volume is h*w1*dp*2 bytes, which
 *                             passes 4 GiB at 8 MP with dp = 512: the host buffers must hold that much.
 *   hsum   int16 [h][w1][dp]  MODE_SGBM_3WAY: L_left + L_right; MODE_HH: S after the first seven directions (the eighth is fused
 *                             with the selection and never stored)
 *   raw    int16 [h][w]       disparity after the row LR check, before the 3x3 median */
int r3d_sgbm_debug_fetch(r3d_ctx *ctx, int16_t *cost, int16_t *hsum, int16_t *raw);

/* debug / stage parity, MODE_HH only: S after the first n_dirs directions (1..8, contract order) of the LAST
 * r3d_sgbm_compute* call on this context, int16 [h][w1][dp] to a HOST buffer (layout and dp, up to 512, as r3d_sgbm_debug_fetch).
 * Runs those directions again over the cost volume that call left behind, with the same launches as the call itself except
 * that every direction stores S (the eighth too), then synchronises and copies.  Overwrites what r3d_sgbm_debug_fetch returns
 * as hsum; cost and raw stay valid.  R3D_E_BADARG: no call yet, the last call was not MODE_HH or had an empty matching range,
 * n_dirs outside 1..8, S_out NULL. */
int r3d_sgbm_debug_hh_partial(r3d_ctx *ctx, int32_t n_dirs, int16_t *S_out);

/* debug / stage parity: the selection stage alone (vertical path, winner-take-all, uniqueness, sub-pixel, LR check) on volumes
 * the CALLER hands in, HOST arrays, single-channel geometry of a w x h compute call with these params (w1, the four stripes and
 * dp as there; MODE_HH: one stripe):
 *   cost   int16 [h][w1][D]       block cost C, every entry in 0..16383 (the kernels' envelope)
 *   hsum   int16 [h][w1][D]       MODE_SGBM_3WAY: L_left + L_right; MODE_HH: S after seven directions
 *   cspec  int16 [3][SH2][w1][D]  the block-cost rows that stripes 1..3 read in place of `cost` for their first SH2 =
 *                                 blockSize/2 rows (the cost kernel replicates the box at a stripe's top); NULL = copies of the
 *                                 rows of `cost` at those positions; ignored at blockSize 1 and in MODE_HH
 * The arrays are expanded to dp slots per column, slots D..dp-1 filled with cost_pad (0..16383) / hsum_pad (an int16): no
 * result may depend on either.  raw, mins and lrd are filled with the invalid marker (minDisparity-1)*16, then the product's own
 * launches run: MODE_SGBM_3WAY k_vscan2 once (for a tiny image this is the first of a compute call's two runs, without the row
 * assembly), MODE_HH the eighth direction over `cost` with `hsum` as the running S, fused with the selection; then
 * k_lrcheck.  Outputs, int16 [h][w], each may be NULL: raw_out = the winner-take-all disparity x16 before the LR check,
 * mins_out = min_d S at every pixel of the matching columns, lrd_out = after the LR check (before the 3x3 median).
 * Afterwards r3d_sgbm_debug_fetch returns the expanded volumes (MODE_HH hsum: the S handed in, the eighth direction stores none).
 * R3D_E_BADARG: cost or hsum NULL, a cost or cost_pad outside 0..16383, hsum_pad outside int16, w1 <= 0; params as compute. */
int r3d_sgbm_debug_select(r3d_ctx *ctx, const r3d_sgbm_params *params, int32_t w, int32_t h, const int16_t *cost, const int16_t *cspec,
                          const int16_t *hsum, int32_t cost_pad, int32_t hsum_pad, int16_t *raw_out, int16_t *mins_out, int16_t *lrd_out);

/* debug / stage parity: the three int16 [h][w] planes of the LAST r3d_sgbm_compute* (lane 0) or r3d_sgbm_debug_select call, to HOST
 * buffers (NULL = skip): raw_wta = disparity x16 before the LR check, mins = min_d S (both written at columns [minX1, maxX1) only;
 * the rest is whatever the buffer held, the invalid marker after r3d_sgbm_debug_select), lrd = after the LR check (what
 * r3d_sgbm_debug_fetch returns as raw).  After a tiny-image MODE_SGBM_3WAY compute raw_wta and mins are those of its second,
 * one-stripe run.  R3D_E_BADARG: no call yet, or the last call had an empty matching range. */
int r3d_sgbm_debug_fetch_select(r3d_ctx *ctx, int16_t *raw_wta, int16_t *mins, int16_t *lrd);

/* ---- point clouds (float64 xyz triplets, like the legacy open3d.geometry.PointCloud the reference passes) ----- */

/* replaces: pcd.voxel_down_sample(voxel_size)   pointcloud_alignment.py:22-23, test/check84.py:180
 * origin = min_bound - voxel/2, key = floor((p-origin)/voxel); out = per-voxel mean of points (and colors /
 * normals when given; pass NULL otherwise).  Output arrays need room for n triplets; *out_n = voxels written, in
 * lexicographic key order (the original's order is hash-map order, i.e. unspecified). */
int r3d_voxel_downsample(r3d_ctx *ctx, const double *xyz, const double *colors, const double *normals, int64_t n, double voxel,
                         double *out_xyz, double *out_colors, double *out_normals, int64_t *out_n);

/* replaces: o3d.t.geometry.PointCloud.voxel_down_sample(voxel) on a Float32 tensor cloud   pointcloud_processing.py:26-27,
 * test/GICP1.py:71-72   [recalled, Open3D 0.18 reduction "mean"].  Unlike the legacy grid above: coordinates and attributes are
 * rounded to float32, key = floor(p / voxel) evaluated in float32 with the grid origin at 0, sums and the division in float32
 * (members added in their original order; the original's order is that of device atomics).  Outputs hold float32 values. */
int r3d_voxel_downsample_tensor(r3d_ctx *ctx, const double *xyz, const double *colors, const double *normals, int64_t n, double voxel,
                                double *out_xyz, double *out_colors, double *out_normals, int64_t *out_n);

/* replaces: pcd.estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))   pointcloud_alignment.py:27-28,
 * test/GICP1.py:77,95,97,148; tensor estimate_normals(max_nn, radius)   normal_estimation.py:20.
 * radius <= 0 selects KDTreeSearchParamKNN(max_nn).  <= max_nn nearest neighbours with distance < radius (query
 * included, nearest first); covariance and normal as legacy Open3D computes them -- one pass of nine cumulants over the raw
 * coordinates, then FastEigen3x3 (closed form), with the fused multiply-adds of the build that recorded the reference's frames:
 * the normals of those frames are reproduced SIGN INCLUDED to <= 5e-12 (oracle/normals.c has the derivation); the sign is the
 * one the closed form produces.  Fewer than 3 neighbours (or an all-zero covariance) -> (0,0,1).
 * prev_normals (may be NULL): when given, each normal is flipped to agree with it and a degenerate one keeps it (legacy
 * behaviour of a cloud that already carries normals). */
int r3d_estimate_normals(r3d_ctx *ctx, const double *xyz, int64_t n, double radius, int32_t max_nn, const double *prev_normals,
                         double *normals);

/* per-point neighbourhood score used by remove_statistical_outlier / remove_radius_outlier
 * (pointcloud_processing.py:35,39; test/check_lama1.py:175): count_radius <= 0: mean distance to the k nearest
 * points, the point itself included; count_radius > 0: number of points within that radius, itself included. */
int r3d_neighbor_score(r3d_ctx *ctx, const double *xyz, int64_t n, int32_t k, double count_radius, double *score);

/* disparity map -> point cloud, cv2.reprojectImageTo3D semantics ([X Y Z W]^T = Q [x y disp/16 1]^T, point = XYZ/W).
 * The reference computes / loads Q (Calib_depth/depth1.py:169,183, depth2.py:49,66) but never calls reprojectImageTo3D;
 * this is the join between its two halves.  Pixels with disp < min_valid_x16 are dropped;
 * out_xyz needs room for w*h triplets, out_pixel (may be NULL) receives the row-major pixel index of each point. */
int r3d_reproject_disparity(r3d_ctx *ctx, const int16_t *disp, int32_t w, int32_t h, const double *Q4x4, int32_t min_valid_x16,
                            double *out_xyz, int32_t *out_pixel, int64_t *out_n);

/* Device-resident join of the two halves ("SGM -> disparity -> cloud -> voxel -> normals, all
 * device-resident"): takes the DEVICE disparity map r3d_sgbm_compute_dev wrote and chains reprojectImageTo3D semantics
 * -> |z| <= max_depth filter (max_depth <= 0: only points at infinity, W = 0, are dropped) -> rigid pose (pose4x4 may be NULL) -> voxel_down_sample(voxel)
 * (voxel <= 0: off) -> estimate_normals(KDTreeSearchParamHybrid(normal_radius, max_nn)) (max_nn <= 0: off; radius <= 0: kNN)
 * without leaving HBM; only the final cloud is copied to the host arrays (room for `capacity` triplets each; out_normals
 * may be NULL when max_nn <= 0).  *out_n = points produced; R3D_E_BADARG if they exceed capacity.  Same kernels and
 * arithmetic as the separate host-buffer entry points, so the results are identical to chaining those. */
int r3d_disparity_to_cloud_dev(r3d_ctx *ctx, const int16_t *d_disp, int32_t w, int32_t h, const double *Q4x4, int32_t min_valid_x16,
                               double max_depth, const double *pose4x4, double voxel, double normal_radius, int32_t max_nn,
                               int64_t capacity, double *out_xyz, double *out_normals, int64_t *out_n);

/* r3d_disparity_to_cloud_dev with colours (the scanner half's clouds all carry them: create_from_rgbd_image, main.py:42-45).
 * d_color: DEVICE uint8 image of the map's size, color_channels (1 or 3) interleaved bytes per pixel, rows color_stride BYTES
 * apart (>= w * color_channels); typically the rectified left image that is in HBM next to the map.  A point's colour is
 * (double)byte / 255.0 of the pixel it was reprojected from, in r, g, b order: color_bgr != 0 reverses a 3-channel pixel (cv2
 * images are BGR, Open3D colours RGB), one channel gives r = g = b.  With the voxel grid on, a voxel's colour is the mean of its
 * members' colours summed in index order (legacy voxel_down_sample), read straight from the image bytes: the extra device
 * memory is the pixel-index array (4 w h bytes) and the output, never a [w*h,3] float64 colour array.  The pose does not touch
 * colours; max_depth and the W = 0 drop apply as to the points.  out_colors: room for `capacity` triplets.  Points and normals
 * are bit for bit those of r3d_disparity_to_cloud_dev.  R3D_E_BADARG: d_color or out_colors NULL (the colourless function is the
 * way to get no colours), color_channels not 1 or 3, color_stride < w * color_channels. */
int r3d_disparity_to_cloud_color_dev(r3d_ctx *ctx, const int16_t *d_disp, int32_t w, int32_t h, const double *Q4x4, int32_t min_valid_x16,
                                     double max_depth, const double *pose4x4, double voxel, double normal_radius, int32_t max_nn,
                                     const uint8_t *d_color, int32_t color_stride, int32_t color_channels, int32_t color_bgr,
                                     int64_t capacity, double *out_xyz, double *out_normals, double *out_colors, int64_t *out_n);

/* k-nearest-neighbour graph (indices in the caller's numbering, nearest first, the point itself first; missing
 * entries -1 / 1e300).  radius <= 0: unbounded.  Feeds orient_normals_consistent_tangent_plane(k)
 * (normal_estimation.py:21), whose spanning-tree propagation is sequential host work.  d2 may be NULL. */
int r3d_knn_graph(r3d_ctx *ctx, const double *xyz, int64_t n, int32_t k, double radius, int32_t *nbr, double *d2);

/* replaces: pcd.orient_normals_consistent_tangent_plane(k)   normal_estimation.py:21   (Open3D legacy
 * OrientNormalsConsistentTangentPlane [recalled]; the tensor method converts to legacy and calls it).
 * r3d_orient_normals_graph is the exact form: `delaunay_edges` = n_edges (a, b) index pairs, the edges of the Delaunay
 * tetrahedralisation of the cloud (Open3D obtains it from Qhull on the host; the Python layer does the same).  The library
 * builds the Euclidean MST of those edges, adds the k-nearest-neighbour edges from the device graph (the point itself is one
 * of the k) that are not Delaunay edges, weights 1 - |n_a . n_b|, takes the spanning tree and propagates the sign from the
 * highest point (turned towards +z).  Equal weights are visited in (a, b) order (the original's order is unspecified).
 * r3d_orient_normals is the k-NN-graph-only variant for callers without a tetrahedralisation: no Euclidean-MST edges, every
 * connected component is rooted at its own highest point -- a DEVIATION from Open3D, not used by the drop-in classes.
 * Spanning trees and propagation are sequential host work inside the library; normals are flipped in place. */
int r3d_orient_normals(r3d_ctx *ctx, const double *xyz, int64_t n, int32_t k, double *normals);
int r3d_orient_normals_graph(r3d_ctx *ctx, const double *xyz, int64_t n, int32_t k, const int32_t *delaunay_edges, int64_t n_edges,
                             double *normals);

/* replaces: pcd.transform(T)   pointcloud_alignment.py:42  (rotate_only != 0 for normals) ; T row-major 4x4 */
int r3d_transform_points(r3d_ctx *ctx, const double *xyz, int64_t n, const double *T4x4, int32_t rotate_only, double *out);

/* replaces: o3d.pipelines.registration.registration_icp(source, target, max_dist, init, PointToPoint / PointToPlane,
 *           ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration))   pointcloud_alignment.py:35-39,
 *           test/check2.py:151-154;  registration_generalized_icp(...)   test/GICP1.py:99-102 */
#define R3D_ICP_POINT_TO_POINT 0
#define R3D_ICP_POINT_TO_PLANE 1
#define R3D_ICP_GENERALIZED 2
typedef struct {
    int32_t mode;
    int32_t max_iteration;              /* Open3D default 30; pointcloud_alignment.py passes 100 */
    double max_correspondence_distance; /* 1-NN accepted iff distance < this */
    double relative_fitness;            /* 1e-6 */
    double relative_rmse;               /* 1e-6 */
    double gicp_epsilon;                /* 1e-3; <= 0 selects the default */
} r3d_icp_params;
typedef struct {
    int32_t iterations; /* ComputeTransformation calls performed */
    int32_t converged;  /* stopped by the relative criteria (not an error when 0) */
    int64_t correspondences;
    double fitness;     /* correspondences / source points */
    double inlier_rmse; /* Euclidean, over correspondences */
    double setup_ms;    /* host wall time: uploads, target grid build, source sort */
    double loop_ms;     /* host wall time of the evaluate / solve loop (iterations + 1 evaluations) */
} r3d_icp_stats;
/* src_normals: GICP only (covariances C = I - (1-eps) n n^T, as Open3D derives them from normals);
 * tgt_normals: point-to-plane and GICP.  init4x4 may be NULL (identity).  T4x4: row-major result.
 * The loop (correspondences, statistics, convergence test, update) runs on the device; the host enqueues evaluations in batches
 * and reads the loop state once per batch, so `iterations` / `converged` are exactly those of the sequential loop.
 * The point-to-point update is Eigen's umeyama(src, dst, false) of the correspondences.  Its moments are accumulated relative to
 * the centre of the target grid's box (r3d_debug_icp_sums), so the result does not degrade with the clouds' distance from the world origin.
 * A singular value of the covariance below 1e-6 of the largest counts as zero: planar correspondences (a wall, three pairs) give
 * the proper rotation that completes the plane's, collinear ones the smallest rotation that maps the line, one pair a pure
 * translation.  The plane and GICP updates solve the 6x6 system and keep the pose when |det J^T J| < 1e-6. */
int r3d_icp(r3d_ctx *ctx, const r3d_icp_params *p, const double *src, int64_t ns, const double *src_normals, const double *tgt,
            int64_t nt, const double *tgt_normals, const double *init4x4, double *T4x4, r3d_icp_stats *stats);
/* diagnostic: what one evaluation of the registration loop accumulates.  Runs r3d_icp's set-up for p->mode (0, 1 or 2) and ONE
 * evaluation at pose T4x4 (NULL: identity) through the loop's own launch: the same search form, the same number of workgroups and
 * the same layout of partial sums.  sums_out[29] is the DEVICE's reduction of those partial sums, by the code k_icp_step runs (a
 * kernel of its own stores them; no host sum is involved); no step is taken.  p->max_iteration and the relative criteria are unused.
 * Refuses like r3d_icp: missing normals for the mode, ns / nt <= 0, distance <= 0, mode outside 0..2.
 * Slots, over the correspondences (source i, its nearest target j within the distance; p = T * src[i], t = tgt[j]):
 *   [0] their count   [1] sum of the squared distances, as the search formed them
 *   point-to-point: with q = p - o, u = t - o,  [2..4] sum q   [5..7] sum u   [8 + 3a + b] sum q_a u_b;  [17..28] zero.
 *     o is the centre of the box the target's search grid is laid out in (the target's bounding box for this call), written to
 *     origin_out[3] (may be NULL).  The means are o + [2..4] / n and o + [5..7] / n, and sigma_ab = [8 + 3b + a] / n - ([5 + a] / n) ([2 + b] / n) is the
 *     covariance (1/n) sum (t - mean t)_a (p - mean p)_b that Umeyama decomposes: it does not depend on o.
 *   point-to-plane and GICP: [2..22] the upper triangle of J^T J (6x6, row by row: 00 01 .. 05 11 12 ..), [23..28] J^T r, in
 *     ABSOLUTE coordinates like Open3D (origin_out is still written, and means nothing here).  Point-to-plane: the row
 *     J = [p x n, n], r = (p - t) . n with n the target normal.  GICP: J^T J = sum Jb^T M^-1 Jb and J^T r = sum Jb^T M^-1 (p - t)
 *     with Jb = [-[p]x | I], M = C_t + R C_s R^T, C = I - (1 - eps) n n^T, R the rotation of T, and a normal with n_x < -0.99
 *     replaced by e1 (Open3D's GetRotationFromE1ToX) on both sides; eps = p->gicp_epsilon, <= 0 selecting 1e-3. */
int r3d_debug_icp_sums(r3d_ctx *ctx, const r3d_icp_params *p, const double *src, int64_t ns, const double *src_normals,
                       const double *tgt, int64_t nt, const double *tgt_normals, const double *T4x4, double *sums_out,
                       double *origin_out);

/* replaces: o3d.pipelines.registration.registration_colored_icp(source, target, max_dist, init,
 *           TransformationEstimationForColoredICP(lambda_geometric), ICPConvergenceCriteria(...))   [recalled, Open3D 0.18
 *           ColoredICP.cpp; the reference never calls it: the consumer of the colours its clouds carry, main.py:42-45].
 * The point-to-plane loop with a second, photometric residual per correspondence: intensity I = (r + g + b) / 3; once per call
 * every target point gets the least-squares gradient of I in its tangent plane over its hybrid neighbourhood
 * (gradient_radius, gradient_max_nn; fewer than 4 neighbours or a singular system: zero gradient); each iteration minimises
 * lambda (geometric)^2 + (1 - lambda) (photometric)^2.  Correspondences, fitness, inlier_rmse (Euclidean) and the convergence
 * test are those of r3d_icp.  lambda_geometric = 1 is point-to-plane bit for bit.  DESIGN.md section 4 ("Coloured ICP") has the contract.
 * r3d_icp and r3d_icp_params are unchanged: r3d_icp keeps refusing mode 3, the coloured mode has entry points of its own. */
#define R3D_ICP_COLORED 3
typedef struct {
    r3d_icp_params icp;       /* icp.mode must be R3D_ICP_COLORED; gicp_epsilon unused; Open3D's criteria default 1e-6 / 1e-6 / 30 */
    double lambda_geometric;  /* in [0, 1]; Open3D default 0.968 */
    double gradient_radius;   /* <= 0: 2 * icp.max_correspondence_distance (Open3D's choice) */
    int32_t gradient_max_nn;  /* <= 0: 30 (Open3D's choice); at most 128 */
    int32_t reserved;
} r3d_colored_icp_params;
/* stage parity: the set-up alone.  colors: [n,3] in [0,1]; out_intensity [n]; out_gradient [n,3].  radius > 0, max_nn in 1..128 */
int r3d_color_gradients(r3d_ctx *ctx, const double *xyz, const double *normals, const double *colors, int64_t n, double radius,
                        int32_t max_nn, double *out_intensity, double *out_gradient);
/* Required: source colours, target colours, target normals (no source normals).  R3D_E_BADARG: one of them missing,
 * lambda_geometric outside [0, 1], gradient_max_nn > 128.  The _dev form takes DEVICE clouds and, like r3d_icp_dev, returns when
 * the loop has finished. */
int r3d_icp_colored(r3d_ctx *ctx, const r3d_colored_icp_params *p, const double *src, const double *src_colors, int64_t ns,
                    const double *tgt, const double *tgt_normals, const double *tgt_colors, int64_t nt, const double *init4x4,
                    double *T4x4, r3d_icp_stats *stats);
int r3d_icp_colored_dev(r3d_ctx *ctx, const r3d_colored_icp_params *p, const double *d_src, const double *d_src_colors, int64_t ns,
                        const double *d_tgt, const double *d_tgt_normals, const double *d_tgt_colors, int64_t nt, const double *init4x4,
                        double *T4x4, r3d_icp_stats *stats);
/* diagnostic: r3d_debug_icp_sums for the coloured mode.  Runs r3d_icp_colored's checks and set-up (the target's gradients, the source
 * intensities) and ONE evaluation at pose T4x4 (NULL: identity) through the loop's own launch; sums_out[29] is the device's
 * reduction, as for r3d_debug_icp_sums; no step is taken.  Refuses like r3d_icp_colored.
 * Slots over the correspondences (p = T * src[i], t, n = its nearest target and that target's normal, (I_t, d) the target's
 * record, I_s the source's intensity, sg = sqrt(lambda), sp = sqrt(1 - lambda)):  [0] count  [1] sum of squared distances
 *   [2..22] the upper triangle of J_G^T J_G + J_I^T J_I, row by row   [23..28] J_G^T r_G + J_I^T r_I,  in absolute coordinates, with
 *   e = (p - t).n    J_G = sg [p x n, n]   r_G = sg e
 *   m = -(d - (d.n) n)   J_I = sp [p x m, m]   r_I = sp (I_s - (d.((p - e n) - t) + I_t)).
 * tgt_records_out (may be NULL): [nt][4], the records that set-up computed for the target, (I_t, d_x, d_y, d_z) per point in the
 * caller's numbering: r3d_color_gradients' output for (tgt, tgt_normals, tgt_colors, the resolved radius and max_nn). */
int r3d_debug_icp_sums_colored(r3d_ctx *ctx, const r3d_colored_icp_params *p, const double *src, const double *src_colors, int64_t ns,
                               const double *tgt, const double *tgt_normals, const double *tgt_colors, int64_t nt, const double *T4x4,
                               double *sums_out, double *tgt_records_out);

/* replaces: o3d.pipelines.registration.compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn)) (test/check_lama1.py:246-281,
 *           mini1.py, check8.py) and the nearest-neighbour search of CorrespondencesFromFeatures   [recalled, Open3D 0.18 Feature.cpp;
 *           DESIGN.md section 4 ("FPFH") restates the contract, tests/fpfh_ref.py executes it].
 * Feature rows are [n][33] float64: the memory of Open3D's 33 x N column-major Feature.data.  The neighbourhood of a point is
 * r3d_knn_graph(k = max_nn, radius)'s (the point itself first; radius <= 0: plain kNN).  spfh (optional) receives the first
 * stage's simplified histograms.  R3D_E_BADARG: a missing array (the normals included), n <= 0, max_nn < 1.
 * R3D_E_UNSUPPORTED: max_nn > 128.  The _dev form takes DEVICE arrays and enqueues on the ctx stream: it returns without waiting
 * for the result (the search grid's bounding box is the one value read back on the way). */
int r3d_compute_fpfh(r3d_ctx *ctx, const double *xyz, const double *normals, int64_t n, double radius, int32_t max_nn, double *fpfh,
                     double *spfh);
int r3d_compute_fpfh_dev(r3d_ctx *ctx, const double *d_xyz, const double *d_normals, int64_t n, double radius, int32_t max_nn,
                         double *d_fpfh, double *d_spfh);
/* stage parity: the second stage alone on a caller-supplied SPFH ([n][33]) */
int r3d_fpfh_from_spfh(r3d_ctx *ctx, const double *xyz, int64_t n, double radius, int32_t max_nn, const double *spfh_in, double *fpfh);
/* nn_out[i] = the target row with the smallest sum_j (src[i][j] - tgt[.][j])^2 (float64, summed in j order; the smaller index wins
 * ties), d2_out[i] (optional) that sum.  Brute force.  R3D_E_UNSUPPORTED: dim != 33, or ns * nt > 1.5e13 (more than a minute of work).
 * The mutual filter of CorrespondencesFromFeatures is host code (cloud_ops.correspondences_from_features).  _dev: device arrays,
 * enqueued on the ctx stream, no synchronisation. */
int r3d_match_features(r3d_ctx *ctx, const double *src_feat, int64_t ns, const double *tgt_feat, int64_t nt, int32_t dim,
                       int32_t *nn_out, double *d2_out);
int r3d_match_features_dev(r3d_ctx *ctx, const double *d_src_feat, int64_t ns, const double *d_tgt_feat, int64_t nt, int32_t dim,
                           int32_t *d_nn_out, double *d_d2_out);
/* diagnostic: ms3[0] k_knn_graph at the same (n, k, radius), ms3[1] / ms3[2] the two stages of r3d_compute_fpfh_dev (events) */
int r3d_debug_fpfh_stages(r3d_ctx *ctx, const double *d_xyz, const double *d_normals, int64_t n, double radius, int32_t max_nn,
                          double *d_fpfh, float *ms3);

/* replaces: o3d.pipelines.registration.registration_ransac_based_on_correspondence / ..._on_feature_matching with
 *           TransformationEstimationPointToPoint(False), CorrespondenceCheckerBasedOnEdgeLength / ...OnDistance and
 *           RANSACConvergenceCriteria(max_iteration, confidence) (test/check_lama1.py:246-281, mini1.py, check8.py)
 *           [recalled, Open3D 0.18 Registration.cpp / CorrespondenceChecker.cpp; DESIGN.md section 4 ("RANSAC") states the contract,
 *           tests/ransac_ref.py executes it].
 * Open3D's sampler and stopping rule are racy; this one is a pure function of (inputs, seed): hypothesis h = 0, 1, ... draws its
 * ransac_n pairs from a counter-based generator, passes the edge-length checker, gets Eigen::umeyama's transform, passes the
 * distance checker, is scored over all M pairs, and the best / stop rule is applied in h order on the host, whatever `batch` is. */
typedef struct r3d_ransac_params {
    double max_correspondence_distance; /* > 0; a pair is an inlier when |T s - t| < this */
    double edge_length_similarity;      /* <= 0: no edge-length checker */
    double checker_distance;            /* <= 0: no distance checker */
    double confidence;                  /* > 0; >= 1: never stop before max_iteration */
    int64_t max_iteration;              /* 1 .. 2^31 - 1 */
    uint64_t seed;
    int32_t ransac_n;                   /* 3 or 4 */
    int32_t batch;                      /* hypotheses per launch, 0: the library's choice; never changes the result */
} r3d_ransac_params;
typedef struct r3d_ransac_stats {
    double fitness;     /* inliers / M of the best hypothesis (0 if none survived) */
    double inlier_rmse;
    int64_t iterations; /* the sequential stop: hypotheses h < iterations count */
    int64_t validated;  /* of those, how many passed their checkers */
    int64_t best_hypothesis; /* -1 if none survived */
    int64_t inliers;
    double setup_ms;    /* host wall time: uploads, gather, index check */
    double loop_ms;     /* host wall time of the batches and the winner's mask */
} r3d_ransac_stats;
/* src [ns][3], tgt [nt][3], corres [M][2] int32 rows (source index, target index); T4x4 row-major (identity if nothing survived);
 * inlier_mask (optional) uint8 [M].  R3D_E_BADARG: a missing array, M < ransac_n, a pair index outside its cloud,
 * max_correspondence_distance <= 0, confidence <= 0, max_iteration < 1.  R3D_E_UNSUPPORTED: ransac_n outside 3..4,
 * max_iteration or M above 2^31 - 1.  batch is clamped to 1 .. 262144.
 * _dev: d_src, d_tgt, d_corres and d_inlier_mask are DEVICE arrays (T4x4 and stats stay host memory); the pair indices are checked
 * on the device before any hypothesis reads them; returns when the loop has finished, like r3d_icp_dev. */
int r3d_ransac_correspondence(r3d_ctx *ctx, const r3d_ransac_params *p, const double *src, int64_t ns, const double *tgt, int64_t nt,
                              const int32_t *corres, int64_t M, double *T4x4, uint8_t *inlier_mask, r3d_ransac_stats *stats);
int r3d_ransac_correspondence_dev(r3d_ctx *ctx, const r3d_ransac_params *p, const double *d_src, int64_t ns, const double *d_tgt, int64_t nt,
                                  const int32_t *d_corres, int64_t M, double *T4x4, uint8_t *d_inlier_mask, r3d_ransac_stats *stats);
/* stage parity: hypotheses h0 .. h0 + count - 1 (count <= 262144) evaluated without the best / stop rule, host arrays.
 * samples int32 [count][4] (unused entries -1); flags int32 [count]: bit 0 the edge-length checker passed (or is off), bit 1 the
 * distance checker passed (or is off; 0 when bit 0 is 0: the transform is not computed then); T [count][12], rows 0..2 of the 4x4
 * (zeros when bit 0 is 0); inliers int32 [count] and err2 [count] (0 unless both bits are set).  Any output may be NULL. */
int r3d_debug_ransac_hypotheses(r3d_ctx *ctx, const r3d_ransac_params *p, const double *src, int64_t ns, const double *tgt, int64_t nt,
                                const int32_t *corres, int64_t M, int64_t h0, int64_t count, int32_t *samples, int32_t *flags, double *T,
                                int32_t *inliers, double *err2);

/* replaces: o3d.pipelines.registration.registration_fgr_based_on_feature_matching / ..._on_correspondence with
 *           FastGlobalRegistrationOption (check8.py:244-248)   [recalled, Open3D 0.18 FastGlobalRegistration.cpp; DESIGN.md section 4
 *           ("FGR") states the contract, tests/fgr_ref.py executes it].
 * Both clouds are centred and scaled, the pairs (given, or the mutual ones of two r3d_match_features searches) go through the
 * tuple test, and a graduated-non-convexity Gauss-Newton loop runs over the surviving rows in ONE kernel launch.  Open3D's tuple
 * sampler draws from a process-wide generator; this one is a pure function of (inputs, options, seed): trial t draws its three
 * pairs from the RANSAC entry points' counter-based generator, and the first maximum_tuple_count accepted trials count in t order,
 * whatever `batch` is.  Every sum has a fixed order: the same bits on every run. */
typedef struct r3d_fgr_params {          /* 56 bytes */
    double division_factor;                  /* 1.4; > 1 */
    double maximum_correspondence_distance;  /* 0.025; > 0.  Compared with the annealing parameter as given, as Open3D does */
    double tuple_scale;                      /* 0.95; in (0, 1] */
    uint64_t seed;
    int32_t iteration_number;                /* 64; >= 0 */
    int32_t maximum_tuple_count;             /* 1000; >= 1 */
    int32_t use_absolute_scale, decrease_mu, tuple_test;   /* 0, 1, 1 */
    int32_t batch;                           /* trials per launch, 0: the library's choice; never changes the result */
} r3d_fgr_params;
typedef struct r3d_fgr_stats {           /* 96 bytes */
    double fitness, inlier_rmse;    /* the registration loop's evaluation at the result with maximum_correspondence_distance */
    double scale_global, scale_start, final_par;
    double setup_ms;                /* host wall time up to the optimisation: uploads, matching, normalisation, tuple test */
    double loop_ms;                 /* host wall time of the optimisation and the evaluation */
    int64_t correspondences;        /* of that evaluation */
    int64_t matched;                /* pairs after step 2: M given, or the mutual pairs */
    int64_t trials;                 /* tuple trials evaluated up to the cut (100 matched when the count is never reached) */
    int64_t tuples;                 /* accepted trials used */
    int64_t pairs;                  /* rows the optimisation ran on: 3 tuples, or matched with tuple_test off */
} r3d_fgr_stats;
/* src [ns][3], tgt [nt][3], corres [M][2] int32 rows (source index, target index; duplicates kept); T4x4 row-major, source ->
 * target.  With fewer than 10 rows the loop does not run and T is the centroid-to-centroid translation (Open3D's behaviour).
 * R3D_E_BADARG: a missing array, ns or nt < 1, an option outside its domain, a pair index outside its cloud (checked on the
 * device before any read), clouds without extent.  R3D_E_UNSUPPORTED: counts above 2^31 - 1; feature form: dim != 33 or a size
 * r3d_match_features refuses.  _dev: the clouds, pairs and feature rows are DEVICE arrays (T4x4 and stats stay host memory);
 * returns when the result is ready, like r3d_icp_dev. */
int r3d_fgr_correspondence(r3d_ctx *ctx, const r3d_fgr_params *p, const double *src, int64_t ns, const double *tgt, int64_t nt,
                           const int32_t *corres, int64_t M, double *T4x4, r3d_fgr_stats *stats);
int r3d_fgr_correspondence_dev(r3d_ctx *ctx, const r3d_fgr_params *p, const double *d_src, int64_t ns, const double *d_tgt, int64_t nt,
                               const int32_t *d_corres, int64_t M, double *T4x4, r3d_fgr_stats *stats);
int r3d_fgr_feature_matching(r3d_ctx *ctx, const r3d_fgr_params *p, const double *src, int64_t ns, const double *tgt, int64_t nt,
                             const double *src_feat, const double *tgt_feat, int32_t dim, double *T4x4, r3d_fgr_stats *stats);
int r3d_fgr_feature_matching_dev(r3d_ctx *ctx, const r3d_fgr_params *p, const double *d_src, int64_t ns, const double *d_tgt, int64_t nt,
                                 const double *d_src_feat, const double *d_tgt_feat, int32_t dim, double *T4x4, r3d_fgr_stats *stats);
/* stage parity, host arrays.  r3d_debug_fgr_tuples normalises, then evaluates trials t0 .. t0 + count - 1 (count <= 262144, M >= 1)
 * without the cut: samples int32 [count][3], flags int32 [count] (either may be NULL).  r3d_debug_fgr_optimize normalises, skips
 * the tuple test, runs the loop on the given pairs and returns the composed transform ([iteration_number][16]) and the annealing
 * parameter ([iteration_number]) after every iteration, in normalised units; with fewer than 10 pairs: the start state. */
int r3d_debug_fgr_tuples(r3d_ctx *ctx, const r3d_fgr_params *p, const double *src, int64_t ns, const double *tgt, int64_t nt,
                         const int32_t *corres, int64_t M, int64_t t0, int64_t count, int32_t *samples, int32_t *flags);
int r3d_debug_fgr_optimize(r3d_ctx *ctx, const r3d_fgr_params *p, const double *src, int64_t ns, const double *tgt, int64_t nt,
                           const int32_t *pairs, int64_t M, double *trace_T, double *trace_par);

/* replaces: the whole body of PointCloudAlignment.align_point_clouds (pointcloud_alignment.py:6-43; caller main.py:48) in ONE
 * call, device-resident between the stages: voxel_down_sample(voxel_size) of both clouds (:22-23) ->
 * estimate_normals(KDTreeSearchParamHybrid(normal_radius, normal_max_nn)) on both (:27-28) -> registration (:35-39) ->
 * source.transform(T) (:42).  Returns what the reference returns: the DOWN-SAMPLED, transformed source (points, colours
 * averaged per voxel, rotated normals).  out arrays need room for ns triplets; out_colors only with src_colors; out_normals
 * only when normal_max_nn > 0.  voxel_size <= 0 skips the down-sampling; stats->setup_ms then covers everything before the
 * ICP loop.  Same kernels as the separate entry points: identical results to chaining those. */
typedef struct r3d_align_params {
    r3d_icp_params icp;
    double voxel_size;
    double normal_radius;
    int32_t normal_max_nn;
    int32_t reserved;
} r3d_align_params;
int r3d_align_point_clouds(r3d_ctx *ctx, const r3d_align_params *p, const double *src, const double *src_colors, int64_t ns,
                           const double *tgt, int64_t nt, const double *init4x4, double *out_xyz, double *out_colors,
                           double *out_normals, int64_t *out_n, double *T4x4, r3d_icp_stats *stats);

/* ---- resident scan-loop model: the growing `combined_pcd` of main.py:28,34-54 and test/GICP1.py:134-155 kept in HBM -----------
 * The reference passes the whole accumulated cloud to align_point_clouds for every frame (main.py:48), which down-samples it
 * again (pointcloud_alignment.py:23), and appends the aligned frame (main.py:49).  An r3d_model owns device buffers for the
 * model's points / colours / normals: per frame only the frame goes up and the 4x4 + statistics come down.  Each call runs the
 * kernels of the one-shot entry points on the same values in the same order (the model is re-voxelised from its resident
 * points), so the results equal those of r3d_align_point_clouds / r3d_icp + `+=` on host clouds.  Attributes follow the legacy
 * operator+=: colours / normals survive an append only if the model is empty or carries them AND the appended cloud does. */
typedef struct r3d_model r3d_model;
int r3d_model_create(r3d_ctx *ctx, r3d_model **out);
void r3d_model_destroy(r3d_model *m);
int r3d_model_clear(r3d_model *m);
int r3d_model_size(r3d_model *m, int64_t *n, int32_t *has_colors, int32_t *has_normals);
/* The model keeps its legacy voxel grid (pointcloud_alignment.py:23 re-down-samples the target every frame, main.py:48) as a resident
 * table that a new frame is merged into while the model's minimum corner -- the grid's origin -- stays where it is; it is rebuilt
 * from all points otherwise (same means bit for bit either way).  Diagnostics: voxels in the table, full rebuilds and incremental
 * updates so far.  Any pointer may be NULL. */
int r3d_model_voxel_table_stats(r3d_model *m, int64_t *voxels, int32_t *rebuilds, int32_t *updates);
/* diagnostic: the model's voxel grid entry by entry.  Brings the table up to date with every model row exactly as the next
 * r3d_model_align_append with this voxel size would (the statistics above advance as they would there), then copies to host
 * buffers (NULL = skip), one entry per voxel in ascending (kx, ky, kz) order: the packed keys kx << 42 | ky << 21 | kz, the
 * running sums [n][3], the member counts, the means handed to the registration [n][3] and the model's box (min, max).
 * *n_out = voxels; when it exceeds cap nothing is copied and the call still succeeds.  *resident = 1 when a table
 * exists afterwards; 0 (more than 2^21 voxels along an axis, or R3D_MODEL_IMPL=rebuild) leaves keys / sums / counts untouched.
 * An empty model or voxel <= 0: R3D_E_BADARG. */
int r3d_model_debug_voxel_table(r3d_model *m, double voxel, int64_t cap, uint64_t *keys, double *sums, int32_t *counts, double *means,
                                double *box6, int64_t *n_out, int32_t *resident);
/* test hook: makes the model's next voxel-table call (r3d_model_debug_voxel_table or an align call with voxel_size > 0) return
 * R3D_E_HIP, "model voxel table: injected failure at step N", when it reaches point `step`, so that the state an error return
 * leaves behind can be tested.  Only the return is injected: nothing is launched differently or freed.  1: in a rebuild, after the
 * build kernel is enqueued; 2: in an update, after the slice is added to the resident sums; 3: in an update, after the merge of
 * new voxels is enqueued (an update that opens no voxel never gets there).  One shot: that call disarms the hook when it starts,
 * whether or not it reaches the point.  0 disarms; any other value: R3D_E_BADARG.  After such a return, as after any error from
 * an align call, the model's rows are unchanged, there is no table and the next call rebuilds it. */
int r3d_model_debug_fail_table_step(r3d_model *m, int32_t step);
/* combined.points = frame.points ... (main.py:42-45) and `combined += cloud` for host clouds; colors / normals may be NULL */
int r3d_model_append(r3d_model *m, const double *xyz, const double *colors, const double *normals, int64_t n);
/* main.py:48-49: aligned = align_point_clouds(frame, combined, threshold, voxel_size, max_iter); combined += aligned.
 * Normals are estimated only where they can reach a result (target normals for the plane / GICP estimators, source normals
 * for GICP or when the model carries normals): the point-to-point estimator never reads them and += drops them otherwise.
 * *appended (may be NULL) = points added (the down-sampled frame). */
int r3d_model_align_append(r3d_model *m, const r3d_align_params *p, const double *src, const double *src_colors, int64_t ns,
                           double *T4x4, r3d_icp_stats *stats, int64_t *appended);
/* replaces: o3d.geometry.PointCloud.create_from_rgbd_image(o3d.geometry.RGBDImage.create_from_color_and_depth(color, depth,
 *           depth_scale, depth_trunc, convert_rgb_to_intensity=False), intrinsic) + the flip transform   test/check84.py:155-159,
 * 172-178 -- how every recorded frame of test/output84 became a cloud (verified on all 163 frames, so this
 * entry point is PINNED by the reference's own PLY files).  z = float32(raw) / float32(depth_scale); z > depth_trunc or z == 0
 * dropped; x = (u - ppx) z / fx, y = (v - ppy) z / fy in float64; flip_yz != 0: (x, -y, -z).  Row-major pixel order.  depth:
 * uint16 [h][stride]; color (may be NULL): uint8 [h][color_stride bytes] with 3 channels per pixel, written as channel / 255 in
 * the order given.  Output arrays need room for w*h entries; out_pixel (may be NULL) = linear pixel index of every point. */
typedef struct r3d_depth_camera {
    double fx, fy, ppx, ppy;   /* camera_intrinsic.json */
    double depth_scale;        /* raw units per metre as the script passes it: 1.0 / sensor depth scale (cast to float32 inside) */
    double depth_trunc;        /* metres; 3.0 in the reference */
    int32_t flip_yz;           /* 1: the (x, -y, -z) flip of check84.py:172-178 */
    int32_t reserved;
} r3d_depth_camera;
int r3d_backproject_depth(r3d_ctx *ctx, const uint16_t *depth, int32_t w, int32_t h, int32_t stride, const r3d_depth_camera *cam,
                          const uint8_t *color, int32_t color_stride, double *out_xyz, double *out_colors, int32_t *out_pixel, int64_t *out_n);
/* the first frame / a later frame of the scanning loop given as a DEPTH IMAGE: back-projection on the device, then exactly
 * r3d_model_append / r3d_model_align_append (0.6 MB goes up instead of 6.8 MB of float64 points).  *frame_points = valid pixels;
 * a frame without any (a failed capture, main.py:53-54) changes nothing: identity, zeroed statistics, *appended = 0. */
int r3d_model_append_depth(r3d_model *m, const uint16_t *depth, int32_t w, int32_t h, int32_t stride, const r3d_depth_camera *cam,
                           const uint8_t *color, int32_t color_stride, int64_t *appended);
int r3d_model_align_append_depth(r3d_model *m, const r3d_align_params *p, const uint16_t *depth, int32_t w, int32_t h, int32_t stride,
                                 const r3d_depth_camera *cam, const uint8_t *color, int32_t color_stride, double *T4x4, r3d_icp_stats *stats,
                                 int64_t *frame_points, int64_t *appended);
/* test/GICP1.py:145-146: aligned = align_point_clouds(frame, combined) (registration of the frame against the WHOLE model with
 * its normals, :99-103, from identity); combined += aligned.  src_colors / src_normals may be NULL where the mode allows. */
int r3d_model_register_append(r3d_model *m, const r3d_icp_params *p, const double *src, const double *src_colors, const double *src_normals,
                              int64_t ns, double *T4x4, r3d_icp_stats *stats);
/* test/GICP1.py:148: combined.estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)); existing normals keep their orientation */
int r3d_model_estimate_normals(r3d_model *m, double radius, int32_t max_nn);
/* host arrays with room for r3d_model_size() triplets; colors / normals may be NULL (and are left alone when the model has none) */
int r3d_model_download(r3d_model *m, double *xyz, double *colors, double *normals);

/* ---- device-pointer forms (clouds that stay in HBM: the multi-view exchange of BASELINE config C5) -----------------------------
 * r3d_disparity_to_cloud_resident = r3d_disparity_to_cloud_dev with DEVICE output arrays (capacity triplets each): the cloud is
 * left in the caller's device buffers, ordered on the context stream (r3d_set_stream lets that be the caller's / torch's
 * stream, so an RCCL collective enqueued there afterwards sees it); only *out_n comes back to the host.
 * r3d_icp_dev = r3d_icp on device clouds (returns when the loop has finished).  r3d_transform_points_dev = r3d_transform_points
 * on device arrays, asynchronous on the context stream; d_out may equal d_xyz. */
int r3d_disparity_to_cloud_resident(r3d_ctx *ctx, const int16_t *d_disp, int32_t w, int32_t h, const double *Q4x4, int32_t min_valid_x16,
                                    double max_depth, const double *pose4x4, double voxel, double normal_radius, int32_t max_nn,
                                    int64_t capacity, double *d_out_xyz, double *d_out_normals, int64_t *out_n);
/* r3d_disparity_to_cloud_color_dev with DEVICE output arrays (d_out_colors: capacity triplets, required): the third plane of the
 * multi-view exchange */
int r3d_disparity_to_cloud_color_resident(r3d_ctx *ctx, const int16_t *d_disp, int32_t w, int32_t h, const double *Q4x4, int32_t min_valid_x16,
                                          double max_depth, const double *pose4x4, double voxel, double normal_radius, int32_t max_nn,
                                          const uint8_t *d_color, int32_t color_stride, int32_t color_channels, int32_t color_bgr,
                                          int64_t capacity, double *d_out_xyz, double *d_out_normals, double *d_out_colors, int64_t *out_n);
int r3d_icp_dev(r3d_ctx *ctx, const r3d_icp_params *p, const double *d_src, int64_t ns, const double *d_src_normals, const double *d_tgt,
                int64_t nt, const double *d_tgt_normals, const double *init4x4, double *T4x4, r3d_icp_stats *stats);
int r3d_transform_points_dev(r3d_ctx *ctx, const double *d_xyz, int64_t n, const double *T4x4, int32_t rotate_only, double *d_out);
/* n_blocks device arrays of triplets, block b moved by T4x4s[16 b .. 16 b + 15] (rotation only where rotate_only[b] != 0;
 * rotate_only may be NULL), in one launch per 16 blocks: the fuse step of the multi-view exchange (every gathered view's points
 * and normals into view 0's frame before mesh_reconstruction.py:22-37).  Pointer tables and counts are HOST arrays; same
 * arithmetic as r3d_transform_points_dev; asynchronous on the context stream; d_out[b] may equal d_xyz[b]. */
int r3d_transform_blocks_dev(r3d_ctx *ctx, int32_t n_blocks, const double *const *d_xyz, const int64_t *counts, const double *T4x4s,
                             const int32_t *rotate_only, double *const *d_out);


/* ---- RGB-D odometry ("RGB-D odometry") ---------------------------------------------------------------------
 * replaces: o3d.pipelines.odometry.compute_rgbd_odometry(source, target, intrinsic, odo_init,
 *           RGBDOdometryJacobianFromHybridTerm(), OdometryOption())   test/check84.py:239-241 -- the registration of consecutive
 * frames, the one registration of the reference that works on images and not on clouds.  [recalled, Open3D 0.18
 * pipelines/odometry/Odometry.cpp, RGBDOdometryJacobian.cpp, geometry/Image.cpp]: Open3D is absent and the reference recorded no
 * poses, so parity is UNPINNED; tests/rgbd_odometry_ref.py restates the contract with its open choices as named switches.
 * Image pyramids (Gaussian3 + 2x2 mean), a z-buffered warp of the source depth into the target (smallest float32 z' wins, then
 * the smaller source index), a 6x6 Gauss-Newton step per iteration through the registration loop's solver (|det| < 1e-6 =>
 * failure), no convergence test.  All iterations of all levels are enqueued without a host read; the same bits on every run. */
#define R3D_ODOMETRY_HYBRID 0  /* RGBDOdometryJacobianFromHybridTerm: photometric + depth residual, lambda_depth 0.95 */
#define R3D_ODOMETRY_COLOR 1   /* RGBDOdometryJacobianFromColorTerm: the photometric row alone */
typedef struct r3d_odometry_params {   /* 48 bytes */
    double depth_diff_max;             /* 0.03; >= 0 */
    double depth_min, depth_max;       /* 0.0, 4.0 */
    int32_t iterations[4];             /* coarsest level first; 20, 10, 5, 0; each >= 0 */
    int32_t levels;                    /* 1..4; 3 */
    int32_t jacobian;                  /* R3D_ODOMETRY_* */
} r3d_odometry_params;
typedef struct r3d_odometry_stats {    /* 56 bytes */
    int32_t success, failed_level, failed_iteration, reserved;   /* -1, -1 when success; (0, -1): no correspondences at odo_init */
    int64_t correspondences_init, correspondences;               /* at odo_init / at the result, level 0 */
    double r2;                                                   /* sum of r^2 of the last iteration */
    double setup_ms, loop_ms;                                    /* device time: pyramids + normalisation / iterations + information */
} r3d_odometry_stats;
/* source, target: frames of equal size w x h.  init4x4 (NULL: identity) and T4x4 map source camera coordinates to target camera
 * coordinates, row-major.  info6x6 (may be NULL): the information matrix of the level-0 correspondences at the result.
 * trace_T (may be NULL): the pose after every iteration, [sum of iterations][16], rows after a failure zero.  An odometry
 * failure (no correspondences, a singular system) is NOT an error: the call returns 0 with stats->success = 0, T = identity and
 * info = identity.  R3D_E_BADARG: a missing array, w or h < 2^(levels-1), levels outside 1..4, a negative iteration count or
 * depth_diff_max, an unknown jacobian, fx or fy of 0, a stride too small, color_channels other than 1 or 3.
 * r3d_rgbd_odometry: raw HOST images as create_from_color_and_depth(convert_rgb_to_intensity=True) takes them: depth uint16
 * [h][depth_stride], colour uint8 [h][color_stride bytes] with 1 or 3 channels (color_bgr != 0: B, G, R order); intensity =
 * (0.2990f R + 0.5870f G + 0.1140f B) / 255.0f, z = float32(raw) / float32(depth_scale), z > depth_trunc => 0 (cam->flip_yz is
 * not used).  r3d_rgbd_odometry_f32: float32 HOST planes [h][stride floats], intensity in [0, 1], depth in metres (0 or NaN: no
 * measurement).  r3d_rgbd_odometry_f32_dev: the same on DEVICE planes; returns when the result is ready, like r3d_icp_dev. */
int r3d_rgbd_odometry(r3d_ctx *ctx, const r3d_odometry_params *p, const uint16_t *src_depth, const uint8_t *src_color,
                      const uint16_t *tgt_depth, const uint8_t *tgt_color, int32_t w, int32_t h, int32_t depth_stride,
                      int32_t color_stride, int32_t color_channels, int32_t color_bgr, const r3d_depth_camera *cam,
                      const double *init4x4, double *T4x4, double *info6x6, r3d_odometry_stats *stats, double *trace_T);
int r3d_rgbd_odometry_f32(r3d_ctx *ctx, const r3d_odometry_params *p, const float *src_intensity, const float *src_depth,
                          const float *tgt_intensity, const float *tgt_depth, int32_t w, int32_t h, int32_t stride, double fx,
                          double fy, double cx, double cy, const double *init4x4, double *T4x4, double *info6x6,
                          r3d_odometry_stats *stats, double *trace_T);
int r3d_rgbd_odometry_f32_dev(r3d_ctx *ctx, const r3d_odometry_params *p, const float *d_src_intensity, const float *d_src_depth,
                              const float *d_tgt_intensity, const float *d_tgt_depth, int32_t w, int32_t h, int32_t stride,
                              double fx, double fy, double cx, double cy, const double *init4x4, double *T4x4, double *info6x6,
                              r3d_odometry_stats *stats, double *trace_T);
/* the conversion of the raw form alone: out_intensity, out_depth float32 [h][w] on the host */
int r3d_debug_rgbd_convert(r3d_ctx *ctx, const uint16_t *depth, const uint8_t *color, int32_t w, int32_t h, int32_t depth_stride,
                           int32_t color_stride, int32_t color_channels, int32_t color_bgr, const r3d_depth_camera *cam,
                           float *out_intensity, float *out_depth);
/* the preparation alone (host float planes in, as r3d_rgbd_odometry_f32).  Each pyramid output holds the levels one after the
 * other, level l as float32 [h >> l][w >> l], un-normalised; any of them may be NULL.  grad4 (may be NULL): the target gradient
 * records of level grad_level, float32 [h_l][w_l][4] = Sobel dI/dx, dI/dy, dD/dx, dD/dy (not yet multiplied by 0.125, NaN kept).
 * *corr_init: correspondences at init4x4 on level 0; scales2: s_src, s_tgt (0, 0 when there are none). */
int r3d_debug_rgbd_prepare(r3d_ctx *ctx, const r3d_odometry_params *p, const float *src_intensity, const float *src_depth,
                           const float *tgt_intensity, const float *tgt_depth, int32_t w, int32_t h, int32_t stride, double fx,
                           double fy, double cx, double cy, const double *init4x4, float *src_pyr_intensity, float *src_pyr_depth,
                           float *tgt_pyr_intensity, float *tgt_pyr_depth, int32_t grad_level, float *grad4, int64_t *corr_init,
                           double *scales2);
/* prepares (scales from init4x4), then one iteration at `level` from pose4x4: corr (may be NULL) int32 [w_l h_l][4] rows
 * (u_s, v_s, u_t, v_t) in target row-major order, *n_corr of them; sums29: count, sum r^2, the upper triangle of JTJ row by row,
 * JTr; T_after: the pose after the step; *ok = 0 when the step failed (T_after = identity).  R3D_E_BADARG also for a level
 * outside 0..levels-1 and when the normalisation at init4x4 finds no correspondences. */
int r3d_debug_rgbd_iteration(r3d_ctx *ctx, const r3d_odometry_params *p, const float *src_intensity, const float *src_depth,
                             const float *tgt_intensity, const float *tgt_depth, int32_t w, int32_t h, int32_t stride, double fx,
                             double fy, double cx, double cy, const double *init4x4, int32_t level, const double *pose4x4,
                             int32_t *corr, int64_t *n_corr, double *sums29, double *T_after, int32_t *ok);

/* ---- TSDF volume ("TSDF volume") -----------------------------------------------------------------------------
 * replaces: volume = o3d.pipelines.integration.ScalableTSDFVolume(voxel_length, sdf_trunc, color_type); volume.integrate(rgbd,
 *           intrinsic, np.linalg.inv(pose)); volume.extract_point_cloud()   test/check84.py:41-44,295,307 -- the stage every
 * experiment pipeline of the reference ends in.  [recalled, Open3D 0.18 pipelines/integration/ScalableTSDFVolume.cpp,
 * UniformTSDFVolume.cpp]: Open3D is absent and the reference recorded no volume, so parity is UNPINNED; tests/tsdf_ref.py restates
 * the contract.  A sparse volume of 16^3-voxel units behind a device hash table; tsdf and weight float32, colour three float64 per
 * voxel.  The same bits on every run: which pool slot a unit gets is a race, everything a caller can see is ordered by unit index
 * (X, then Y, then Z).  extract_triangle_mesh is r3d_mesh_from_volume below.  Gray32 and unit resolutions other than 16 are not
 * built. */
#define R3D_TSDF_COLOR_NONE 0
#define R3D_TSDF_COLOR_RGB8 1
typedef struct r3d_tsdf r3d_tsdf;
typedef struct r3d_tsdf_params {       /* 32 bytes */
    double voxel_length, sdf_trunc;    /* metres, both > 0 */
    int32_t color_type;                /* R3D_TSDF_COLOR_* */
    int32_t volume_unit_resolution;    /* 16; anything else: R3D_E_UNSUPPORTED */
    int32_t depth_sampling_stride;     /* 4; >= 1: every stride-th pixel of every stride-th row decides which units a frame touches */
    int32_t initial_units;             /* starting capacity of the unit pool, 0 = 1024; pool and table grow when a frame needs more */
} r3d_tsdf_params;
typedef struct r3d_tsdf_info {        /* 48 bytes */
    int64_t units, frames, touched;    /* units in the volume, frames integrated, units the last frame touched */
    int32_t capacity, growths;         /* pool capacity in units, how often it grew */
    double touch_ms, integrate_ms;     /* device time of the last frame: touch + slot assignment / the voxel update */
} r3d_tsdf_info;
/* A volume belongs to the context it was made on and is used through it (any other: R3D_E_BADARG); destroy it before the context. */
int r3d_tsdf_create(r3d_ctx *ctx, const r3d_tsdf_params *p, r3d_tsdf **out);
int r3d_tsdf_destroy(r3d_ctx *ctx, r3d_tsdf *vol);
int r3d_tsdf_reset(r3d_ctx *ctx, r3d_tsdf *vol);   /* no units, no frames; the pool keeps its capacity */
/* One frame.  extrinsic4x4: world -> camera, row-major, last row 0 0 0 1.  The depth image is w x h; the colour image
 * (color_w x color_h, color_stride BYTES per row, color_channels interleaved uint8 in the order given) is read only by an RGB8
 * volume, which refuses (R3D_E_BADARG) a missing one, one of another size and one without exactly 3 channels; a volume without
 * colour accepts NULL.  R3D_E_UNSUPPORTED: a sampled depth pixel lands in a unit whose index leaves +-2^20 (the volume is
 * unchanged).  r3d_tsdf_integrate: raw HOST images, depth uint16 [h][depth_stride], z = float32(raw) / float32(cam->depth_scale),
 * z > cam->depth_trunc => 0 -- the plane r3d_debug_rgbd_convert returns.  r3d_tsdf_integrate_f32: a float32 HOST depth plane in
 * metres [h][depth_stride floats], 0 = no sample.  r3d_tsdf_integrate_f32_dev: the same on DEVICE images; it reads 16 bytes of
 * counters back after the touch pass (how many units are new decides whether the pool grows), enqueues the voxel update on the
 * context stream and returns without waiting for it: the images must stay untouched until the stream has passed. */
int r3d_tsdf_integrate(r3d_ctx *ctx, r3d_tsdf *vol, const uint16_t *depth, const uint8_t *color, int32_t w, int32_t h,
                       int32_t depth_stride, int32_t color_w, int32_t color_h, int32_t color_stride, int32_t color_channels,
                       const r3d_depth_camera *cam, const double *extrinsic4x4);
int r3d_tsdf_integrate_f32(r3d_ctx *ctx, r3d_tsdf *vol, const float *depth, const uint8_t *color, int32_t w, int32_t h,
                           int32_t depth_stride, int32_t color_w, int32_t color_h, int32_t color_stride, int32_t color_channels,
                           double fx, double fy, double cx, double cy, const double *extrinsic4x4);
int r3d_tsdf_integrate_f32_dev(r3d_ctx *ctx, r3d_tsdf *vol, const float *d_depth, const uint8_t *d_color, int32_t w, int32_t h,
                               int32_t depth_stride, int32_t color_w, int32_t color_h, int32_t color_stride,
                               int32_t color_channels, double fx, double fy, double cx, double cy, const double *extrinsic4x4);
int r3d_tsdf_stats(r3d_ctx *ctx, r3d_tsdf *vol, r3d_tsdf_info *out);   /* waits for the last frame when it reports its times */
/* extract_point_cloud(): *out_n = the number of points, always.  cap = 0: the count alone.  cap < count: R3D_E_BADARG and nothing
 * is written.  Otherwise xyz, normals and (RGB8 volumes; else ignored, may be NULL) colors receive count rows of 3 doubles; order:
 * units by (X, Y, Z), voxels by flat index, axes x, y, z.  The _dev form writes DEVICE arrays and returns when they are complete. */
int r3d_tsdf_extract_point_cloud(r3d_ctx *ctx, r3d_tsdf *vol, int64_t cap, double *xyz, double *normals, double *colors,
                                 int64_t *out_n);
int r3d_tsdf_extract_point_cloud_dev(r3d_ctx *ctx, r3d_tsdf *vol, int64_t cap, double *d_xyz, double *d_normals, double *d_colors,
                                     int64_t *out_n);
/* the state, for the tests: *out_n units in (X, Y, Z) order; cap_units = 0: the count alone, cap_units < count: R3D_E_BADARG.
 * idx3 int32 [n][3]; tsdf, weight float32 [n][4096] (voxel (x, y, z) at x*256 + y*16 + z); colour float64 [n][3][4096] (RGB8
 * volumes; else ignored) */
int r3d_debug_tsdf_units(r3d_ctx *ctx, r3d_tsdf *vol, int64_t cap_units, int32_t *idx3, float *tsdf, float *weight, double *colour,
                         int64_t *out_n);
/* replaces: volume.extract_triangle_mesh() (Open3D ScalableTSDFVolume::ExtractTriangleMesh [recalled, 0.18]; parity UNPINNED like
 * the cloud's).  Marching cubes on the device over every cube whose base voxel lies in an existing unit and whose eight corners
 * all lie in existing units with weight != 0 (no 0.98 bound here); DESIGN.md section 4, "Triangle mesh", is the contract,
 * tests/tsdf_mesh_ref.py restates it.  *out_nv / *out_nt = the numbers of vertices and triangles, always.  Both capacities 0: the
 * counts alone.  A capacity below its count: R3D_E_BADARG and nothing is written.  Otherwise vertices and (RGB8 volumes; else
 * ignored, may be NULL) colors receive *out_nv rows of 3 doubles, triangles *out_nt rows of 3 int32 vertex numbers, faces looking
 * from inside (tsdf < 0) outward.  No vertex normals.  Order: a vertex belongs to the lower voxel of its edge: units by (X, Y, Z),
 * voxels by flat index, axes x, y, z; triangles by base voxel in the same order, then in the table's order.  More than 2^31 - 1
 * vertices or triangles: R3D_E_UNSUPPORTED.  The _dev form writes DEVICE arrays and returns when they are complete. */
int r3d_mesh_from_volume(r3d_ctx *ctx, r3d_tsdf *vol, int64_t cap_vertices, int64_t cap_triangles, double *vertices, double *colors,
                         int32_t *triangles, int64_t *out_nv, int64_t *out_nt);
int r3d_mesh_from_volume_dev(r3d_ctx *ctx, r3d_tsdf *vol, int64_t cap_vertices, int64_t cap_triangles, double *d_vertices,
                             double *d_colors, int32_t *d_triangles, int64_t *out_nv, int64_t *out_nt);
/* the inverse of r3d_debug_tsdf_units, for the tests: the volume's content becomes these n units (arrays laid out as that call
 * returns them, keys in any order; colour is read by RGB8 volumes only).  A key that occurs twice or an index outside +-2^20:
 * R3D_E_BADARG and the volume is unchanged.  The frame count stays; the pool grows to n units when it is smaller. */
int r3d_debug_volume_load_units(r3d_ctx *ctx, r3d_tsdf *vol, int64_t n, const int32_t *idx3, const float *tsdf, const float *weight,
                                const double *colour);
/* the marching-cubes triangle table the library was built with, int8 [256][16]; host only: no context, no device */
int r3d_debug_mc_table(int8_t *tri256x16);


/* ---- per-frame stages either side of the matcher in Calib_depth/depth*.py --------------
 * OpenCV is a dependency of the reference that is absent here, and the reference records no output of these calls:
 * parity of this group is UNPINNED (restated from OpenCV 4.x's published algorithms; see oracle/prepost_oracle.py). */

/* replaces: cv2.initUndistortRectifyMap(mtx, dist, R, P, image_size, cv2.CV_16SC2)   depth2.py:125-128 (depth1.py:208-211)
 * camera3x3 row-major; dist: n_dist in {0,4,5,8,12,14} coefficients k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tx ty (tilt must be
 * 0); R3x3 may be NULL (identity); new_camera: 3 x new_camera_cols (3 or 4) row-major, the projection matrix P1/P2 as
 * stored in the calibration file.  Host outputs: map1 int16 [h][w][2] (integer source x, y), map2 uint16 [h][w]
 * (5+5 fraction bits, INTER_TAB_SIZE = 32).  fp64, running sums along each row like the original's scalar loop. */
int r3d_init_undistort_rectify_map(r3d_ctx *ctx, const double *camera3x3, const double *dist, int32_t n_dist, const double *R3x3,
                                   const double *new_camera, int32_t new_camera_cols, int32_t w, int32_t h, int16_t *map1,
                                   uint16_t *map2);

/* replaces: cv2.remap(frame, map_x, map_y, cv2.INTER_LINEAR)   depth2.py:243-244
 * uint8 source with cn = 1, 3 or 4 interleaved channels, fixed-point maps as above, BORDER_CONSTANT(border_value):
 * dst = (sum of 4 taps x 15-bit table weights + 2^14) >> 15.  gray (may be NULL, needs cn >= 3): the BGR2GRAY image of the
 * remapped frame written by the same kernel (depth2.py:247-248 converts the rectified frame right away). */
int r3d_remap_u8(r3d_ctx *ctx, const uint8_t *src, int32_t sw, int32_t sh, int32_t sstride, int32_t cn, const int16_t *map1,
                 const uint16_t *map2, int32_t dw, int32_t dh, int32_t border_value, uint8_t *dst, uint8_t *gray);
int r3d_remap_u8_dev(r3d_ctx *ctx, const uint8_t *d_src, int32_t sw, int32_t sh, int32_t sstride, int32_t cn,
                     const int16_t *d_map1, const uint16_t *d_map2, int32_t dw, int32_t dh, int32_t border_value, uint8_t *d_dst,
                     uint8_t *d_gray);

/* replaces: cv2.cvtColor(img, cv2.COLOR_BGR2GRAY)   depth2.py:247-248:  (B*1868 + G*9617 + R*4899 + 2^13) >> 14 */
int r3d_bgr2gray(r3d_ctx *ctx, const uint8_t *bgr, int32_t w, int32_t h, int32_t stride, int32_t cn, uint8_t *gray);
int r3d_bgr2gray_dev(r3d_ctx *ctx, const uint8_t *d_bgr, int32_t w, int32_t h, int32_t stride, int32_t cn, uint8_t *d_gray);

/* replaces: wls_filter = cv2.ximgproc.createDisparityWLSFilter(matcher_left=stereo_matcher); setLambda(8000);
 * setSigmaColor(1.5)   depth2.py:164-166;   wls_filter.filter(disparity_left, gray_left, None, disparity_right)   :255 */
typedef struct r3d_wls_params {
    double lambda;                 /* setLambda */
    double sigma_color;            /* setSigmaColor */
    double lambda_attenuation;     /* 0.25 */
    double discontinuity_roll_off; /* 0.001 */
    int32_t min_disparity;         /* of the LEFT matcher: ROI = columns [max(0,minD+D), w - max(0,-minD)) */
    int32_t num_disparities;
    int32_t discontinuity_radius;  /* ceil(0.5*blockSize) for an SGBM matcher */
    int32_t lrc_thresh;            /* 24 (1.5 px in x16 units) */
    int32_t num_iter;              /* 3 */
    int32_t solver;                /* R3D_WLS_SOLVER_*: how the smoother's tridiagonal systems are solved */
} r3d_wls_params;
/* CONTRACT of the two solvers (tests/test_prepost_gpu.py asserts it up to 3264x2448, D = 128):
 *   R3D_WLS_SOLVER_SEQUENTIAL  one Thomas sweep per line in the float32 operation order of the CPU original as restated in
 *       oracle/prepost_oracle.py: confidence map and filtered map BIT-EXACT against that restatement.  39 waves on a
 *       1024-SIMD chip: 7.8 ms per 8 MP frame.
 *   R3D_WLS_SOLVER_PARTITIONED (default)  solves the SAME tridiagonal systems block-parallel (31-unknown blocks + Schur
 *       complement over the separators): exact in exact arithmetic, a different float32 rounding order.  TOLERANCE: the
 *       confidence map is bit-exact; the filtered int16 map (x16 fixed point) differs from the sequential solver's by AT MOST
 *       1 LSB (1/16 px) on FEWER THAN 0.1 % of the pixels (a value that rounds half-to-even differently), and not at all
 *       outside the ROI.  0.69 ms per 8 MP frame.  Callers that need the bit-exact map select the sequential solver. */
#define R3D_WLS_SOLVER_PARTITIONED 0
#define R3D_WLS_SOLVER_SEQUENTIAL 1
/* disp_left / disp_right: int16 x16 maps of the left and the right matcher (the right one holds negative values);
 * guide: uint8 left view with guide_cn = 1 or 3 channels.  out: int16 x16, 16*(minD-1) outside the ROI.
 * confidence (may be NULL): float [h][w] map in [0,255] (getConfidenceMap()). */
int r3d_wls_filter(r3d_ctx *ctx, const r3d_wls_params *p, const int16_t *disp_left, const int16_t *disp_right, const uint8_t *guide,
                   int32_t guide_cn, int32_t guide_stride, int32_t w, int32_t h, int16_t *out, float *confidence);
int r3d_wls_filter_dev(r3d_ctx *ctx, const r3d_wls_params *p, const int16_t *d_disp_left, const int16_t *d_disp_right,
                       const uint8_t *d_guide, int32_t guide_cn, int32_t guide_stride, int32_t w, int32_t h, int16_t *d_out,
                       float *d_confidence);

/* replaces: cv2.normalize(filtered_disparity, None, 0, 255, cv2.NORM_MINMAX)   depth2.py:256 (int16 in, int16 out) */
int r3d_normalize_minmax_s16(r3d_ctx *ctx, const int16_t *src, int64_t n, double alpha, double beta, int16_t *dst);
int r3d_normalize_minmax_s16_dev(r3d_ctx *ctx, const int16_t *d_src, int64_t n, double alpha, double beta, int16_t *d_dst);

/* ---- triangle-mesh operations (csrc/trimesh.hip; DESIGN.md section 4, "Triangle-mesh operations") -------------------------------
 * replaces: mesh.filter_smooth_laplacian(5) and the clean-ups of mesh_reconstruction.py:22-37, the NaN scrub of check84.py:315-322.
 * A mesh is nv rows of float64 xyz (optionally normals and colours of the same shape) and nt rows of three int32 vertex numbers.
 * Every entry point refuses (R3D_E_BADARG) a missing required array, a negative count and a triangle index outside [0, nv); no
 * such index is ever used as an address.  R3D_E_UNSUPPORTED: nv above 2^31 - 2 or 6 nt above 2^31 - 1 (offsets are int32).  nv = 0
 * or nt = 0 is valid.  The _dev forms take DEVICE arrays, run on the ctx stream and return once their work is done; their output
 * arrays must not overlap an input array or one another (a kernel would read rows that another thread has replaced): such a call
 * is refused (R3D_E_BADARG) before anything runs.
 *
 * Incidence of vertex v: the corners 3 t + c with triangles[t][c] == v, ascending.  Adjacency: every triangle puts each of its
 * vertices into the sets of the other two (a degenerate (a, a, b) puts a into its own set); a set is listed once, ascending.
 * Both come as CSR: offsets[nv + 1], then the entries.  cap = 0 asks for the number of entries only (*out_n); otherwise offsets
 * and the entries are written when cap >= *out_n and nothing is written when it is not (R3D_E_BADARG). */
int r3d_trimesh_incidence(r3d_ctx *ctx, int64_t nv, int64_t nt, const int32_t *triangles, int64_t cap, int32_t *offsets, int32_t *corners,
                          int64_t *out_n);
int r3d_trimesh_adjacency(r3d_ctx *ctx, int64_t nv, int64_t nt, const int32_t *triangles, int64_t cap, int32_t *offsets, int32_t *neighbours,
                          int64_t *out_n);

#define R3D_SMOOTH_SIMPLE 0    /* out[v] = (prev[v] + sum of prev[nb]) / (deg + 1), added in adjacency order */
#define R3D_SMOOTH_LAPLACIAN 1 /* w = 1 / (|prev[v] - prev[nb]| + 1e-12); out[v] = prev[v] + lambda (sum w prev[nb] / sum w - prev[v]) */
#define R3D_SMOOTH_TAUBIN 2    /* per iteration a Laplacian step with lambda, then one with mu */
#define R3D_SMOOTH_MAX_ITERATIONS (1 << 20) /* every step is a kernel launch: more iterations are R3D_E_UNSUPPORTED */
#define R3D_SCOPE_ALL 0        /* Open3D's FilterScope: which of positions, normals and colours are filtered; the others are copied */
#define R3D_SCOPE_COLOR 1
#define R3D_SCOPE_NORMAL 2
#define R3D_SCOPE_VERTEX 3
/* filter_smooth_simple / _laplacian / _taubin: `iterations` steps from the previous step's arrays, float64, the weights always
 * from the positions, normals not renormalised.  normals / colors may be NULL (then so may their outputs).  A vertex with an empty
 * adjacency set keeps its values (Open3D divides 0 / 0 there).  iterations = 0 copies.  Also refused: iterations < 0, lambda or mu
 * not finite, an unknown kind or scope.  R3D_E_UNSUPPORTED: iterations above R3D_SMOOTH_MAX_ITERATIONS. */
int r3d_trimesh_smooth(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *vertices, const double *normals, const double *colors,
                       const int32_t *triangles, int32_t kind, int32_t iterations, double lambda, double mu, int32_t scope, double *out_vertices,
                       double *out_normals, double *out_colors);
int r3d_trimesh_smooth_dev(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *d_vertices, const double *d_normals, const double *d_colors,
                           const int32_t *d_triangles, int32_t kind, int32_t iterations, double lambda, double mu, int32_t scope,
                           double *d_out_vertices, double *d_out_normals, double *d_out_colors);

#define R3D_NORMALS_RAW 1 /* leave the cross products (triangles) and their sums (vertices) unnormalised */
/* compute_triangle_normals: (v1 - v0) x (v2 - v0), normalised; compute_vertex_normals: the unnormalised cross products added in
 * ascending corner order, then normalised.  A zero vector stays zero.  Either output may be NULL.  Refused: unknown flags. */
int r3d_trimesh_normals(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *vertices, const int32_t *triangles, int32_t flags,
                        double *triangle_normals, double *vertex_normals);
int r3d_trimesh_normals_dev(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *d_vertices, const int32_t *d_triangles, int32_t flags,
                            double *d_triangle_normals, double *d_vertex_normals);

#define R3D_COMPACT_DROP_DEGENERATE 1   /* triangles with two equal indices */
#define R3D_COMPACT_DROP_UNREFERENCED 2 /* vertices no surviving triangle uses */
#define R3D_COMPACT_DROP_NON_FINITE 4   /* vertices with a NaN or an infinity in their position */
/* The clean-ups.  vertex_keep / triangle_keep: one byte per row, 0 = remove, or NULL.  Triangles are decided first: a triangle
 * goes when its mask says so, when DROP_DEGENERATE applies, or when it touches a vertex that its mask or DROP_NON_FINITE removes;
 * "referenced" then means referenced by a surviving triangle.  Survivors keep their order, triangle indices are renumbered,
 * normals and colours (NULL or given) travel with their vertices.  *out_nv and *out_nt are always set; cap_vertices = cap_triangles
 * = 0 asks for them alone; otherwise rows are written when both capacities suffice and nothing is written when one does not
 * (R3D_E_BADARG).  Refused: unknown flags. */
int r3d_trimesh_compact(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *vertices, const double *normals, const double *colors,
                        const int32_t *triangles, const uint8_t *vertex_keep, const uint8_t *triangle_keep, int32_t flags, int64_t cap_vertices,
                        int64_t cap_triangles, double *out_vertices, double *out_normals, double *out_colors, int32_t *out_triangles,
                        int64_t *out_nv, int64_t *out_nt);
int r3d_trimesh_compact_dev(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *d_vertices, const double *d_normals, const double *d_colors,
                            const int32_t *d_triangles, const uint8_t *d_vertex_keep, const uint8_t *d_triangle_keep, int32_t flags,
                            int64_t cap_vertices, int64_t cap_triangles, double *d_out_vertices, double *d_out_normals, double *d_out_colors,
                            int32_t *d_out_triangles, int64_t *out_nv, int64_t *out_nt);


/* ---- mesh topology (csrc/meshtopo.hip; DESIGN.md section 4, "Mesh topology") -----------------------------------------------------------
 * The edge table, connected components and duplicate clean-ups of Open3D's TriangleMesh (get_non_manifold_edges,
 * cluster_connected_triangles, remove_duplicated_vertices, remove_duplicated_triangles).  Parity with Open3D is UNPINNED;
 * tests/meshtopo_ref.py restates the contract.  Sizes, the refusal of an index outside [0, nv), empty meshes and the _dev rules are
 * those of the triangle-mesh operations above.  R3D_E_INTERNAL: a union-find walk passed its cap (never expected; reported, not hung).
 *
 * Edge table: triangle (a, b, c) has the sides (a,b), (b,c), (c,a); a side's edge is (min, max); a degenerate (a, a, b) has a side
 * (a, a) and two on (a, b).  The distinct edges come ascending by (min, max) with their numbers of sides.  cap = 0 asks for the
 * number of edges only (*out_n); otherwise edges int32 [n][2] and counts int32 [n] are written when cap >= *out_n and nothing is
 * written when it is not (R3D_E_BADARG).  stats (optional, always set) = {edges, boundary (count 1), non-manifold (count > 2),
 * degenerate (min == max)}. */
int r3d_meshtopo_edges(r3d_ctx *ctx, int64_t nv, int64_t nt, const int32_t *triangles, int64_t cap, int32_t *edges, int32_t *counts, int64_t *stats,
                       int64_t *out_n);
/* Connected components: two triangles are adjacent when they have a side on the same edge (all triangles on a non-manifold edge
 * are mutually adjacent; a shared vertex alone does not join).  triangle_clusters int32 [nt] numbers the components in ascending
 * order of their lowest triangle; *out_n_clusters is always set.  cap_clusters = 0: labels alone (vertices may be NULL).  Otherwise,
 * when cap_clusters >= *out_n_clusters, cluster_n_triangles int64 [] and cluster_area double [] as well; when it is not, R3D_E_BADARG
 * and nothing is written.  cluster_area[c]: the terms 0.5 * sqrt((n0 n0 + n1 n1) + n2 n2), n = (p1 - p0) x (p2 - p0), float64 without
 * fused multiply-add, of the component's triangles in ascending index, added in consecutive chunks of 256 from the front of each,
 * then the chunk sums from the front. */
int r3d_meshtopo_components(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *vertices, const int32_t *triangles, int64_t cap_clusters,
                            int32_t *triangle_clusters, int64_t *cluster_n_triangles, double *cluster_area, int64_t *out_n_clusters);
int r3d_meshtopo_components_dev(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *d_vertices, const int32_t *d_triangles, int64_t cap_clusters,
                                int32_t *d_triangle_clusters, int64_t *d_cluster_n_triangles, double *d_cluster_area, int64_t *out_n_clusters);

#define R3D_DEDUP_VERTICES 1  /* vertices whose x, y and z compare equal as doubles (-0.0 == +0.0; a row with a NaN equals nothing) */
#define R3D_DEDUP_TRIANGLES 2 /* triangles equal up to rotation ((a,b,c) = (b,c,a) = (c,a,b); (a,c,b) is another) */
/* The welds.  The first occurrence survives, a vertex with its own normal and colour, a triangle in its own rotation; survivors
 * keep their order.  DEDUP_VERTICES renumbers the triangles and drops none; DEDUP_TRIANGLES leaves the vertices alone; with both,
 * vertices go first.  Arrays, capacities and refusals as r3d_trimesh_compact.  Optional outputs (written with the rows):
 * vertex_map int32 [nv], the new number of every input vertex, and triangle_origin int32 [*out_nt], the input triangle each
 * surviving triangle was.  Refused: unknown flags. */
int r3d_meshtopo_dedup(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *vertices, const double *normals, const double *colors, const int32_t *triangles,
                       int32_t flags, int64_t cap_vertices, int64_t cap_triangles, double *out_vertices, double *out_normals, double *out_colors,
                       int32_t *out_triangles, int32_t *vertex_map, int32_t *triangle_origin, int64_t *out_nv, int64_t *out_nt);
int r3d_meshtopo_dedup_dev(r3d_ctx *ctx, int64_t nv, int64_t nt, const double *d_vertices, const double *d_normals, const double *d_colors,
                           const int32_t *d_triangles, int32_t flags, int64_t cap_vertices, int64_t cap_triangles, double *d_out_vertices,
                           double *d_out_normals, double *d_out_colors, int32_t *d_out_triangles, int32_t *d_vertex_map, int32_t *d_triangle_origin,
                           int64_t *out_nv, int64_t *out_nt);
/* the sort under all of the above, for the tests: n host (key, value) pairs in the stable order of the keys, which must be below 2^bits (bits 0..64;
 * eight per pass, at least one pass); values NULL: the index */
int r3d_debug_sort_pairs_u64(r3d_ctx *ctx, const uint64_t *keys, const int32_t *values, int64_t n, int32_t bits, uint64_t *out_keys, int32_t *out_values);

/* ---- Poisson surface reconstruction (mesh_reconstruction.py:22-37, visualizer.py:107-110) ---------------------------------------
 * replaces: o3d.geometry.TriangleMesh.create_from_point_cloud_poisson(pcd, depth).  The screened Poisson formulation on a DENSE
 * 2^depth grid: finite differences, a zero boundary value, densities in samples per cell; float64 throughout, every sum in a fixed
 * order.  Parity with Open3D's octree solver is UNPINNED; DESIGN.md section 4, "Poisson reconstruction", is the contract and
 * tests/poisson_ref.py restates it. */
typedef struct r3d_poisson_params {
    int32_t depth;           /* 2..8 (8): the grid has 2^depth cells and 2^depth + 1 nodes per axis; else R3D_E_UNSUPPORTED */
    int32_t cycles;          /* 10: V-cycles from chi = 0 */
    int32_t pre, post;       /* 2, 2: weighted-Jacobi sweeps before and after the coarse-grid step */
    int32_t coarse_sweeps;   /* 40: sweeps on the coarsest level (at most 5 nodes per axis) */
    int32_t reserved;
    double scale;            /* 1.1: cube side / largest extent of the points */
    double alpha;            /* 4.0: screening weight */
    double omega;            /* 0.8: Jacobi weight */
} r3d_poisson_params;
/* xyz, normals [n][3] float64 (zero-length normals are accepted), colors [n][3] or NULL.  params NULL: the defaults above.
 * *out_nv / *out_nt = the numbers of vertices and triangles, always.  Both capacities 0: the counts alone.  A capacity below its
 * count: R3D_E_BADARG and nothing is written.  Otherwise vertices [*out_nv][3], densities [*out_nv] (samples per cell at the
 * vertex), vertex_colors [*out_nv][3] (only with colors; else ignored, may be NULL) and triangles int32 [*out_nt][3], faces looking
 * from chi < 0 outward (outward for outward normals).  A vertex belongs to the lower node of its edge: nodes by linear index
 * (k G + j) G + i, then axis x, y, z; triangles by base node in the same order, then in the table's order.  Refused with
 * R3D_E_BADARG and nothing written: n <= 0, a missing array, a non-finite coordinate or normal, points that all coincide, a
 * parameter out of range.  The _dev form reads and writes DEVICE arrays and returns when they are complete. */
int r3d_poisson_reconstruct(r3d_ctx *ctx, const double *xyz, const double *normals, const double *colors, int64_t n,
                            const r3d_poisson_params *params, int64_t cap_vertices, int64_t cap_triangles, double *vertices, double *densities,
                            double *vertex_colors, int32_t *triangles, int64_t *out_nv, int64_t *out_nt);
int r3d_poisson_reconstruct_dev(r3d_ctx *ctx, const double *d_xyz, const double *d_normals, const double *d_colors, int64_t n,
                                const r3d_poisson_params *params, int64_t cap_vertices, int64_t cap_triangles, double *d_vertices,
                                double *d_densities, double *d_vertex_colors, int32_t *d_triangles, int64_t *out_nv, int64_t *out_nt);
/* the fields, for the tests (G = 2^depth + 1 nodes per axis, node (i, j, k) at (k G + j) G + i; any output may be NULL):
 * grid4 = {org x, org y, org z, h}; W0, D, b, chi [G^3]; C0 (needs colors), V [3][G^3] (one plane per channel / axis); dens [n];
 * chi after k_cycles V-cycles, 0 <= k_cycles <= params->cycles */
int r3d_debug_poisson_fields(r3d_ctx *ctx, const double *xyz, const double *normals, const double *colors, int64_t n,
                             const r3d_poisson_params *params, int32_t k_cycles, double *grid4, double *W0, double *C0, double *dens, double *V,
                             double *D, double *b, double *chi);
/* the extraction alone, for the tests: marching cubes at iso 0 on a caller's chi, W0 [G^3] and C0 [3][G^3] (or NULL: no colours),
 * with the outputs and the capacity protocol of r3d_poisson_reconstruct */
int r3d_debug_poisson_extract(r3d_ctx *ctx, int32_t depth, const double *org3, double h, const double *chi, const double *W0, const double *C0,
                              int64_t cap_vertices, int64_t cap_triangles, double *vertices, double *densities, double *vertex_colors,
                              int32_t *triangles, int64_t *out_nv, int64_t *out_nt);

/* ---- pose-graph optimisation (csrc/posegraph.hip; test/check84.py:262-273) ---------------------------------------------------------
 * replaces: o3d.pipelines.registration.global_optimization(pose_graph, GlobalOptimizationLevenbergMarquardt(), criteria, option).
 * float64 throughout, every sum in a fixed order.  Parity with Open3D is UNPINNED; DESIGN.md section 4, "Pose-graph optimisation", is
 * the contract and tests/posegraph_ref.py restates it.  A node is a camera-to-world pose, 16 numbers row-major; an edge (s, t) carries
 * T (source camera -> target camera coordinates, 16 numbers row-major), a 6x6 information matrix (36 numbers row-major; the lower
 * triangle of what it contributes is used), an `uncertain` flag (loop closure) and a confidence (the line-process weight). */
typedef struct r3d_posegraph_params {   /* 72 bytes */
    double max_correspondence_distance;     /* 0.03: with the two below, GlobalOptimizationOption */
    double edge_prune_threshold;            /* 0.25 */
    double preference_loop_closure;         /* 1.0 */
    double min_relative_increment;          /* 1e-6: with the three below and the iteration counts, GlobalOptimizationConvergenceCriteria */
    double min_relative_residual_increment; /* 1e-6 */
    double min_right_term;                  /* 1e-6 */
    double min_residual;                    /* 1e-6 */
    int32_t reference_node;                 /* -1: no node is held; 0..n_nodes-1: that node's step is zeroed in every trial */
    int32_t max_iteration;                  /* 100 outer iterations per optimisation */
    int32_t max_iteration_lm;               /* 20 trials per outer iteration */
    int32_t trace_capacity;                 /* 0: rows the trace array can take */
} r3d_posegraph_params;
#define R3D_POSEGRAPH_STOP_RIGHT_TERM 1         /* max|b| < min_right_term */
#define R3D_POSEGRAPH_STOP_INCREMENT 2          /* ||delta|| < min_relative_increment (||x|| + min_relative_increment) */
#define R3D_POSEGRAPH_STOP_RESIDUAL_INCREMENT 3 /* F - F_new < min_relative_residual_increment F */
#define R3D_POSEGRAPH_STOP_RESIDUAL 4           /* F_new < min_residual */
#define R3D_POSEGRAPH_STOP_ITERATIONS 5         /* max_iteration outer iterations */
#define R3D_POSEGRAPH_STOP_NO_EDGES 6           /* nothing to optimise */
typedef struct r3d_posegraph_stats {    /* 80 bytes; the counts are over both optimisations (before and after the pruning) */
    int32_t outer_iterations, trials, rejected_trials, failed_factorizations, edges_pruned;
    int32_t stop_first, stop_second;        /* R3D_POSEGRAPH_STOP_* of the two optimisations */
    int32_t reserved;
    double first_objective, final_objective;
    double linearize_ms, factor_ms, substitute_ms, rest_ms; /* device time by HIP events, summed over the trials */
} r3d_posegraph_stats;
/* global_optimization: optimise, drop the uncertain edges whose confidence is below edge_prune_threshold, optimise the rest.  poses
 * [n_nodes][16] in/out; edge_nodes int32 [n_edges][2] (source, target); edge_uncertain, edge_kept: one byte per edge; edge_confidence
 * [n_edges] in/out (an uncertain edge's initial weight; a certain edge's has to be finite, is not used and not changed); edge_kept out: 0 for a pruned
 * edge.  params NULL: the defaults above.  stats may be NULL.  trace (may be NULL): params->trace_capacity rows of (lambda, F_new, rho,
 * code), one per trial in order, code 1 accepted, 0 rejected, -1 the step was below the increment test (F_new = rho = 0), -2 the
 * factorisation met a pivot <= 0 or not finite (counted as rejected; F_new = rho = 0); trials beyond the capacity are not recorded.
 * Refused with R3D_E_BADARG before anything is written: n_nodes outside 1..1024, n_edges outside 0..2^20, a node id out of range,
 * an edge with source == target, a pose, T, information matrix or confidence that is not finite, reference_node outside
 * -1..n_nodes-1, a negative iteration count.  No edges: the poses are returned unchanged.  The _dev form takes every array but
 * params and stats on the DEVICE (trace too) and returns when they are complete. */
int r3d_posegraph_optimize(r3d_ctx *ctx, const r3d_posegraph_params *params, int64_t n_nodes, double *poses, int64_t n_edges,
                           const int32_t *edge_nodes, const double *edge_T, const double *edge_info, const uint8_t *edge_uncertain,
                           double *edge_confidence, uint8_t *edge_kept, r3d_posegraph_stats *stats, double *trace);
int r3d_posegraph_optimize_dev(r3d_ctx *ctx, const r3d_posegraph_params *params, int64_t n_nodes, double *d_poses, int64_t n_edges,
                               const int32_t *d_edge_nodes, const double *d_edge_T, const double *d_edge_info, const uint8_t *d_edge_uncertain,
                               double *d_edge_confidence, uint8_t *d_edge_kept, r3d_posegraph_stats *stats, double *d_trace);
/* the linearisation alone, for the tests (every edge kept, n_edges >= 1; any output may be NULL): e [n_edges][6], l [n_edges] (the
 * weights), H [6 n_nodes][6 n_nodes] dense (the lower triangle is what is built; the upper one is its mirror image), b [6 n_nodes],
 * F the objective */
int r3d_debug_posegraph_linearize(r3d_ctx *ctx, const r3d_posegraph_params *params, int64_t n_nodes, const double *poses, int64_t n_edges,
                                  const int32_t *edge_nodes, const double *edge_T, const double *edge_info, const uint8_t *edge_uncertain,
                                  const double *edge_confidence, double *e, double *l, double *H, double *b, double *F);
/* the solve alone, for the tests: (A + lambda I) delta = -b for a dense symmetric A of order n <= 6144 (its lower triangle is read).
 * L [n][n] (may be NULL): the Cholesky factor, its strict upper triangle ZERO; delta [n] (may be NULL).  *failed_pivot = -1, or the
 * index of the first pivot that was <= 0 or not finite: then L and delta are all zero (nothing that is not finite is written). */
int r3d_debug_posegraph_solve(r3d_ctx *ctx, int32_t n, const double *A, const double *b, double lambda, double *L, double *delta,
                              int32_t *failed_pivot);

#ifdef __cplusplus
}
#endif
#endif /* R3D_H */
