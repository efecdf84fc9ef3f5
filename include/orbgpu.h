/*
 * orbgpu.h -- C-ABI of the MI355X-native ORB-SLAM3 hot path (liborbgpu.so).
 *
 * This is the drop-in boundary for the one hot path of yutongwangBIT/multi_orbslam3 that this
 * repository re-implements for gfx950: ORBextractor, stereo matching, the Hamming matchers and
 * Optimizer::LocalBundleAdjustment.  The reference has no FFI of its own (its interface is three
 * C++ headers full of cv::Mat / STL / pointer graphs), so every entry point below cites the C++
 * member it replaces; INTEGRATION.md shows the adapter a maintainer adds on the reference side.
 *
 * Conventions: plain pointers + sizes, no C++/torch types, every function returns an int status
 * (ORBG_OK == 0, negative == error, never throws).  Unless a parameter is named d_*, pointers are
 * HOST memory owned by the caller; handles own all device memory, pinned staging and HIP streams.
 * Handles are thread-compatible (one thread at a time per handle), the library is re-entrant
 * across handles.  File:line citations use the path shorthand of SURVEY.md
 * (S/ = src/orb_slam3_ros/orb_slam3/src/, I/ = .../include/, G/ = .../Thirdparty/g2o/g2o/).
 */
#ifndef ORBGPU_H_
#define ORBGPU_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- status codes */
enum {
  ORBG_OK = 0,
  ORBG_EMPTY = -1,         /* empty image: ORBextractor::operator() returns -1, S/ORBextractor.cc:1072-1073 */
  ORBG_BAD_ARG = -2,
  ORBG_CAP_EXCEEDED = -3,  /* caller-provided capacity (or a handle capacity) too small */
  ORBG_HIP_ERROR = -4,
  ORBG_NO_DEVICE = -5,     /* no HIP device / HIP runtime unusable: the product path never falls back to CPU */
  ORBG_INTERNAL = -6
};

/* LBA outcome, lba_result.status (not errors: they mirror the reference's early returns) */
enum {
  LBA_APPLIED = 0,
  LBA_ABORTED_BEFORE_OPT = 1,   /* *pbStopFlag set before optimize(): S/Optimizer.cc:2127-2129 */
  LBA_REJECTED_OUTLIERS = 2     /* >= 50 % of the edges are outliers: S/Optimizer.cc:2257-2261 */
};

#define ORBG_MAX_LEVELS 16
#define ORBG_DESC_BYTES 32
#define ORBG_GRID_COLS 64      /* FRAME_GRID_COLS, I/Frame.h:39 */
#define ORBG_GRID_ROWS 48      /* FRAME_GRID_ROWS, I/Frame.h:38 */
/* Feature indices travel in 16 bits inside the matchers and the stereo matcher (0xFFFF = none): frames / keypoint sets of
 * this many features or more are refused with ORBG_CAP_EXCEEDED (the reference runs with 1000-2000 features per image). */
#define ORBG_MAX_FRAME_FEATURES 65535

/* ---------------------------------------------------------------- ORB extractor */

/* ORBextractor ctor arguments (S/ORBextractor.cc:408-411, values from ORBParameters I/Datatypes.h:43-55)
 * plus the sizes the handle pre-allocates for. */
typedef struct orbx_config {
  int32_t n_features;     /* nfeatures, 1 .. 3500 (the reference's settings use 1000 - 2000); more: ORBG_BAD_ARG */
  float   scale_factor;   /* scaleFactor */
  int32_t n_levels;       /* nlevels (<= ORBG_MAX_LEVELS) */
  int32_t ini_th_fast;    /* iniThFAST   */
  int32_t min_th_fast;    /* minThFAST   */
  int32_t max_width;      /* largest image the handle will be given (<= 4000 x 4000); every pyramid level of an image
                           * must stay larger than the 19-pixel border (else ORBG_BAD_ARG from the extract call) */
  int32_t max_height;
  int32_t n_cams;         /* 1 = mono, 2 = stereo rig (left = cam 0, right = cam 1) */
  int32_t device;         /* HIP device ordinal (1 agent <-> 1 GPU) */
  /* Deployment variants for the two places where the reference's output depends on its build, not on its source
   * (all zero = the defaults the parity tests pin):
   * gauss_taps: outer-to-centre half of the 7-tap Q8 kernel cv::GaussianBlur(7x7, sigma 2) uses on CV_8U
   *   {18,34,49,55} (sum 257, default): OpenCV <= 3.4.1, and the 3.4.2 - 4.4 fixed-point path (each tap rounded on its own);
   *   {18,34,48,56} (sum 256): OpenCV >= 4.5 (getGaussianKernelFixedPoint_ED: rounding error diffused, centre = remainder).
   *   Any taps with 2 (t0+t1+t2) + t3 <= 257 are accepted.
   * octree_oldest_first: DistributeOctTree sorts (size, ExtractorNode*) and splits from the back (S/ORBextractor.cc:679-682):
   *   among equally populated nodes the heap address decides.  0 (default): the most recently created node first
   *   (addresses grow with allocation order); 1: the oldest first (allocators that hand out descending addresses). */
  int32_t gauss_taps[4];
  int32_t octree_oldest_first;
} orbx_config;

/* The cv::KeyPoint fields the reference sets/uses. 24 bytes. */
typedef struct orbx_keypoint {
  float   x, y;       /* pt, level-0 pixels (S/ORBextractor.cc:1131-1133) */
  float   size;       /* (int)(31*mvScaleFactor[l]) (S/ORBextractor.cc:862,871) */
  float   angle;      /* degrees [0,360) (S/ORBextractor.cc:475) */
  float   response;   /* FAST score */
  int32_t octave;     /* pyramid level (S/ORBextractor.cc:870) */
} orbx_keypoint;

typedef struct orbx_handle orbx_handle;

/* ORBextractor::ORBextractor, S/ORBextractor.cc:408-468. */
int orbx_create(const orbx_config* cfg, orbx_handle** out);
int orbx_destroy(orbx_handle* h);

/* Scale tables the reference exposes through getters (I/ORBextractor.h:65-85):
 * mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2 (each n_levels floats) and
 * mnFeaturesPerLevel.  Any output pointer may be NULL. */
int orbx_get_tables(const orbx_handle* h, float* scale, float* inv_scale, float* sigma2,
                    float* inv_sigma2, int32_t* features_per_level);

/* int ORBextractor::operator()(image, mask, keypoints, descriptors, vLappingArea),
 * S/ORBextractor.cc:1068-1150.  img: u8 gray, row stride `stride` bytes.  Keypoints with
 * lap0 <= x <= lap1 are written from the back (S/ORBextractor.cc:1135-1144); *n_mono is the
 * reference's return value (monoIndex).  kps/desc hold `cap` entries; *n is the total count.
 * Returns ORBG_EMPTY for a NULL / zero-sized image. */
int orbx_extract(orbx_handle* h, int cam, const uint8_t* img, int width, int height, int stride,
                 int lap0, int lap1, orbx_keypoint* kps, uint8_t* desc, int cap, int* n, int* n_mono);

/* The stereo Frame ctor's two concurrent ExtractORB calls (S/Frame.cc:92-95,393-400) as ONE
 * batched submission: left+right share every kernel launch.  vLappingArea = {0,0} as there.
 * Output pointers may be NULL (results then stay device-resident for orbx_stereo_match /
 * orbm_frame_from_extractor). */
int orbx_extract_stereo(orbx_handle* h, const uint8_t* img_left, const uint8_t* img_right,
                        int width, int height, int stride,
                        orbx_keypoint* kps_left, uint8_t* desc_left, int cap_left, int* n_left,
                        orbx_keypoint* kps_right, uint8_t* desc_right, int cap_right, int* n_right);

/* Same, images already resident in device memory (d_img_*: device pointers, stride in bytes). */
int orbx_extract_stereo_dev(orbx_handle* h, const uint8_t* d_img_left, const uint8_t* d_img_right,
                            int width, int height, int stride,
                            orbx_keypoint* kps_left, uint8_t* desc_left, int cap_left, int* n_left,
                            orbx_keypoint* kps_right, uint8_t* desc_right, int cap_right, int* n_right);

/* mvImagePyramid[level] (public member read by Frame::ComputeStereoMatches, I/ORBextractor.h:87):
 * dimensions, and a copy of the level (without its 19-px border) into host memory (may be NULL). */
int orbx_get_level(orbx_handle* h, int cam, int level, uint8_t* host_out, int* width, int* height);
/* Same level together with the 19-px REFLECT_101 border copyMakeBorder puts around it (S/ORBextractor.cc:1167-1173):
 * (width+38) x (height+38) bytes, tightly packed.  *width / *height still report the level size without border. */
int orbx_get_level_bordered(orbx_handle* h, int cam, int level, uint8_t* host_out, int* width, int* height);

/* Test/diagnostic view of ComputeKeyPointsOctTree's vToDistributeKeys (S/ORBextractor.cc:776-853)
 * for the last extraction: per level, FAST candidates in the reference's cell-major order,
 * coordinates relative to (minBorderX,minBorderY).  xys = cap x {x,y,score} int32.  cam must be a camera of that extraction
 * (after one image on a two-camera handle: camera 0 only; ORBG_BAD_ARG otherwise, and before the first extraction). */
int orbx_get_candidates(orbx_handle* h, int cam, int level, int32_t* xys, int cap, int* n);

/* Frame::ComputeStereoMatches, S/Frame.cc:785-963, on the device-resident result of the last
 * orbx_extract_stereo*: fills uright[n_left] / depth[n_left] (mvuRight / mvDepth, -1 = none).
 * bf = mbf, b = mb (S/Frame.cc:815-817).  Host outputs may be NULL. */
int orbx_stereo_match(orbx_handle* h, float bf, float b, float* uright, float* depth);

/* ---------------------------------------------------------------- frame view + matchers */

/* What the matchers read from a Frame. */
typedef struct orbm_frame_view {
  int32_t n;                      /* Frame::N */
  const orbx_keypoint* kps;       /* mvKeysUn (== mvKeys when k1 == 0, S/Frame.cc:723-727) */
  const uint8_t* desc;            /* mDescriptors, n x 32 */
  const float* uright;            /* mvuRight, NULL = all -1 */
  const float* depth;             /* mvDepth,  NULL = all -1 */
  float min_x, max_x, min_y, max_y;   /* mnMinX.. (S/Frame.cc:127-144) */
  float fx, fy, cx, cy, bf, b;    /* S/Frame.cc:136-146 */
  int32_t n_levels;
  float   scale_factor;           /* mfScaleFactor; mvScaleFactors rebuilt as S/ORBextractor.cc:413-421 */
} orbm_frame_view;

typedef struct orbm_frame orbm_frame;

int orbm_frame_create(int device, int cap_features, orbm_frame** out);
int orbm_frame_destroy(orbm_frame* f);
/* Upload a host frame view and build the 64x48 feature grid on the device
 * (Frame::AssignFeaturesToGrid / PosInGrid, S/Frame.cc:360-391,699-709). */
int orbm_frame_upload(orbm_frame* f, const orbm_frame_view* view);
/* Same, but features/uright/depth are taken device-to-device from the extractor handle's left
 * camera (no host round trip); view->kps/desc/uright/depth are ignored, view->n must be the
 * left feature count or -1. */
int orbm_frame_from_extractor(orbm_frame* f, orbx_handle* h, const orbm_frame_view* view);
/* Frame::Frame(imLeft, imRight, ...) (S/Frame.cc:71-172) as ONE submission with ONE final synchronisation: both
 * ExtractORB calls (:92-95), ComputeStereoMatches (:117) and AssignFeaturesToGrid (:160).  Images are host u8 gray;
 * `frame` (may be NULL) afterwards views the left features on the device exactly as after
 * orbm_frame_from_extractor.  Host outputs (kps_left, desc_left, uright, depth: cap_left entries) may be NULL. */
int orbx_frame_stereo(orbx_handle* h, orbm_frame* frame, const orbm_frame_view* view, const uint8_t* img_left,
                      const uint8_t* img_right, int width, int height, int stride, float bf, float b,
                      orbx_keypoint* kps_left, uint8_t* desc_left, float* uright, float* depth, int cap_left,
                      int* n_left, int* n_right);
/* Same with the two images already in device memory. */
int orbx_frame_stereo_dev(orbx_handle* h, orbm_frame* frame, const orbm_frame_view* view, const uint8_t* d_img_left,
                          const uint8_t* d_img_right, int width, int height, int stride, float bf, float b,
                          orbx_keypoint* kps_left, uint8_t* desc_left, float* uright, float* depth, int cap_left,
                          int* n_left, int* n_right);
/* The same constructor in two halves: _submit enqueues the whole chain (pyramids .. grid) on the handle's stream and
 * returns, _wait completes it (redoing the frame with the host quad-trees if a device list overflowed) and returns the
 * feature counts.  Between the two calls the handle, `frame` and the images must be left alone; work on OTHER handles /
 * frames (the searches of the previous frame, S/Tracking.cc:2629-2735) may run meanwhile and overlaps on the GPU.
 * One submission per handle at a time; no host copies of the features in this form. */
int orbx_frame_stereo_dev_submit(orbx_handle* h, orbm_frame* frame, const orbm_frame_view* view, const uint8_t* d_img_left,
                                 const uint8_t* d_img_right, int width, int height, int stride, float bf, float b);
int orbx_frame_stereo_dev_wait(orbx_handle* h, int* n_left, int* n_right);
/* The two-halves constructor with HOST images (cv::Mat data, any host memory): Frame::Frame(imLeft, imRight, ...)
 * (S/Frame.cc:71-172) as Tracking::GrabImageStereo (S/Tracking.cc:1014-1083) receives them.  _submit packs the rows into the
 * handle's pinned staging slot, enqueues one copy kernel (host -> HBM over PCIe, ordered before the pyramid on the handle's
 * stream, overlapping the kernels of other handles) and the constructor chain; _wait is orbx_frame_stereo_dev_wait.  The
 * images may be reused as soon as _submit returns with flags == 0.  With ORBX_SUBMIT_ASYNC the packing and the launches are
 * done by the library's ingest thread (one per process, created by the first such call; it inherits that caller's CPU
 * affinity): the call returns at once and the images must stay valid until _wait.  Typical use: the image grabber / camera
 * thread submits frame t+1 (flags 0) while Tracking works on frame t, or Tracking itself submits with ORBX_SUBMIT_ASYNC.
 * One submission per handle at a time (ORBG_BAD_ARG otherwise). */
#define ORBX_SUBMIT_ASYNC 1
/* Host arrays for the features of the two-halves constructor: from now on every _submit of this handle also delivers the LEFT image's
 * mvKeys / mDescriptors / mvuRight / mvDepth -- what the output arguments of orbx_frame_stereo deliver for the synchronous
 * constructor, S/Frame.cc:100-118 -- into these arrays (cap_left entries each; a NULL array is not delivered) by the time _wait
 * returns; ORBG_CAP_EXCEEDED from _wait when the frame has more features.  The arrays belong to the caller and must stay valid while
 * a submission is in flight; all NULL / cap 0 switches the delivery off again.  The handle must be idle. */
int orbx_set_frame_outputs(orbx_handle* h, orbx_keypoint* kps_left, uint8_t* desc_left, float* uright, float* depth, int cap_left);
int orbx_frame_stereo_submit(orbx_handle* h, orbm_frame* frame, const orbm_frame_view* view, const uint8_t* img_left,
                             const uint8_t* img_right, int width, int height, int stride, float bf, float b, int flags);
int orbx_frame_stereo_wait(orbx_handle* h, int* n_left, int* n_right);
/* ---- the monocular Frame constructor (mono agents of BASELINE configs 1 and 5)
 * Frame::Frame(imGray, ..., pCamera, distCoef, ...), S/Frame.cc:260-358: ExtractORB(0, imGray, 0, 1000) (:289 -- the lapping area
 * {0, 1000} covers every image up to 1000 px wide, so ALL keypoints are written from the back: reversed order, monoIndex = 0,
 * S/ORBextractor.cc:1135-1144), UndistortKeyPoints (:301, :721-754), mvuRight = mvDepth = -1 (:303-304), AssignFeaturesToGrid (:344)
 * as ONE submission with ONE final synchronisation, exactly like the stereo constructor above; `frame` views mvKeysUn + mDescriptors
 * with its grid on the device afterwards.
 * dist = mDistCoef {k1, k2, p1, p2, k3} (S/Tracking.cc:71-81); NULL or k1 == 0: mvKeysUn = mvKeys (S/Frame.cc:723-727) and the view's
 * bounds must be the image rectangle.  Otherwise every keypoint goes through cv::undistortPoints(mat, mat, K, mDistCoef, Mat(), mK)
 * (S/Frame.cc:740; K = mK = the view's fx, fy, cx, cy; OpenCV 3.2 cvUndistortPoints: 5 fixed-point iterations in double) on the
 * device, and the view's bounds are the caller's ComputeImageBounds (S/Frame.cc:756-783: orbx_undistort_points of the four corners).
 * Host outputs (cap entries each, any may be NULL): kps = mvKeys, kps_un = mvKeysUn, desc = mDescriptors. */
typedef struct orbx_distortion { float k1, k2, p1, p2, k3; } orbx_distortion;
int orbx_frame_mono(orbx_handle* h, orbm_frame* frame, const orbm_frame_view* view, const orbx_distortion* dist, const uint8_t* img,
                    int width, int height, int stride, orbx_keypoint* kps, orbx_keypoint* kps_un, uint8_t* desc, int cap, int* n);
int orbx_frame_mono_dev(orbx_handle* h, orbm_frame* frame, const orbm_frame_view* view, const orbx_distortion* dist, const uint8_t* d_img,
                        int width, int height, int stride, orbx_keypoint* kps, orbx_keypoint* kps_un, uint8_t* desc, int cap, int* n);
/* The two-halves form (see orbx_frame_stereo_submit): host image / image resident in HBM; _wait collects it (orbx_frame_stereo_dev_wait
 * works too and reports n_right = 0).  orbx_set_frame_outputs' kps_left / desc_left arrays receive mvKeys / mDescriptors,
 * orbx_set_frame_outputs_un's array receives mvKeysUn. */
int orbx_frame_mono_submit(orbx_handle* h, orbm_frame* frame, const orbm_frame_view* view, const orbx_distortion* dist, const uint8_t* img,
                           int width, int height, int stride, int flags);
int orbx_frame_mono_dev_submit(orbx_handle* h, orbm_frame* frame, const orbm_frame_view* view, const orbx_distortion* dist,
                               const uint8_t* d_img, int width, int height, int stride);
int orbx_frame_mono_wait(orbx_handle* h, int* n);
int orbx_set_frame_outputs_un(orbx_handle* h, orbx_keypoint* kps_un /* cap_left of orbx_set_frame_outputs entries, or NULL */);
/* ---- the RGB-D Frame constructor (TUM / Kinect style agents)
 * Tracking::GrabImageRGBD (S/Tracking.cc:1086-1142) + Frame::Frame(imGray, imDepth, ...), S/Frame.cc:174-257, as ONE submission with ONE
 * final synchronisation, like the two constructors above:
 *   cvtColor to gray for a 3- or 4-channel image (S/Tracking.cc:1092-1105; rgb_order = mbRGB; 8-bit fixed point
 *     (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14, a fourth channel is ignored; a 1-channel image is taken as it is),
 *   ExtractORB(0, imGray, 0, 0) (S/Frame.cc:198: lapping area {0, 0}, i.e. the keypoint order of the STEREO constructor's left image),
 *   UndistortKeyPoints (:212; dist and the view's bounds as for orbx_frame_mono),
 *   ComputeStereoFromRGBD (:214, :966-988): d = imDepth.at<float>(v, u) at the DISTORTED keypoint, coordinates truncated to int;
 *     d > 0: mvDepth = d, mvuRight = mvKeysUn.x - bf / d in float32; otherwise both -1 (NaN and d <= 0 fail, +inf passes),
 *   AssignFeaturesToGrid (:256).
 * imDepth.convertTo(CV_32F, mDepthMapFactor) (S/Tracking.cc:1107-1108) is applied to the values that are read: when
 * fabs(depth_factor - 1.0f) > 1e-5 or the depth type is not float32, d = (float)raw * depth_factor (one float32 product, as OpenCV's
 * convertTo computes it for 16-bit unsigned and float input); otherwise the float is taken as it is.  depth_factor is the float
 * Tracking holds (S/Tracking.cc:166-172): 1 when fabs(DepthMapFactor) < 1e-5, else 1.0f / DepthMapFactor.
 * A feature whose truncated coordinates lie outside the image reads no memory and gets -1 (undefined behaviour in the reference; the
 * extractor's own keypoints are always inside).  `frame` afterwards views mvKeysUn, mDescriptors, mvuRight, mvDepth and the grid on the
 * device exactly as after orbx_frame_stereo, so the uRight gates of the searches, the stereo edges of PoseOptimization / local BA,
 * UnprojectStereo and Fuse work on it unchanged.  Limits: pinhole camera, one depth image per frame, features up to the handle's
 * capacity.  struct_size = sizeof(the struct) as the caller was compiled. */
#define ORBX_DEPTH_U16 0   /* CV_16U: raw sensor counts */
#define ORBX_DEPTH_F32 1   /* CV_32F */
typedef struct orbx_rgbd_image {
  uint32_t struct_size;
  int32_t channels;        /* of img: 1 (gray), 3 or 4 (packed 8-bit colour) */
  const uint8_t* img;      /* imRGB: host memory, or device memory for the _dev entry points */
  int32_t stride;          /* bytes per row of img */
  int32_t rgb_order;       /* mbRGB: != 0 the first channel is R, 0 it is B */
  const void* depth;       /* imD: same memory kind as img */
  int32_t depth_type;      /* ORBX_DEPTH_U16 / ORBX_DEPTH_F32 */
  int32_t depth_stride;    /* bytes per row of depth */
  float depth_factor;      /* mDepthMapFactor (already inverted) */
  int32_t reserved;
} orbx_rgbd_image;
/* Arguments as for orbx_frame_mono (ORBG_EMPTY without an image, a distorted camera needs `frame`, bounds rules with and without
 * distortion, one submission per handle); in addition ORBG_BAD_ARG without a depth image, for a depth type or channel count other than
 * the above, strides smaller than a row, and bf <= 0.  A depth image in device memory must be aligned to its element size.
 * Host outputs (cap entries each, any may be NULL): kps = mvKeys, kps_un = mvKeysUn, desc = mDescriptors, uright = mvuRight,
 * depth = mvDepth. */
int orbx_frame_rgbd(orbx_handle* h, orbm_frame* frame, const orbm_frame_view* view, const orbx_distortion* dist, const orbx_rgbd_image* im,
                    int width, int height, float bf, orbx_keypoint* kps, orbx_keypoint* kps_un, uint8_t* desc, float* uright, float* depth,
                    int cap, int* n);
int orbx_frame_rgbd_dev(orbx_handle* h, orbm_frame* frame, const orbm_frame_view* view, const orbx_distortion* dist, const orbx_rgbd_image* im,
                        int width, int height, float bf, orbx_keypoint* kps, orbx_keypoint* kps_un, uint8_t* desc, float* uright, float* depth,
                        int cap, int* n);
/* The two-halves form (see orbx_frame_stereo_submit).  Both host images go through pinned staging slots (the depth image through one of
 * its own, allocated by the handle's first RGB-D frame) and may be reused as soon as _submit returns with flags == 0; with
 * ORBX_SUBMIT_ASYNC they must stay valid until _wait (the descriptor itself is copied).  orbx_set_frame_outputs' arrays receive mvKeys /
 * mDescriptors / mvuRight / mvDepth, orbx_set_frame_outputs_un's array mvKeysUn.  _wait redoes the whole frame, depth lookup included,
 * with the host quad-trees if a device list overflowed. */
int orbx_frame_rgbd_submit(orbx_handle* h, orbm_frame* frame, const orbm_frame_view* view, const orbx_distortion* dist, const orbx_rgbd_image* im,
                           int width, int height, float bf, int flags);
int orbx_frame_rgbd_dev_submit(orbx_handle* h, orbm_frame* frame, const orbm_frame_view* view, const orbx_distortion* dist,
                               const orbx_rgbd_image* im, int width, int height, float bf);
int orbx_frame_rgbd_wait(orbx_handle* h, int* n);
/* Frame::ComputeStereoFromRGBD on n caller-given points (host memory): xy = n x {x, y} of mvKeys, xy_un = the same of mvKeysUn (NULL:
 * xy), depth_img = the raw depth image (depth_type, depth_stride bytes per row, width x height), the conversion rule above; uright /
 * depth receive n floats each.  For callers that hold features already, as orbx_undistort_points is for the undistortion. */
int orbx_depth_at_points(int device, const float* xy, const float* xy_un, int n, const void* depth_img, int depth_type, int depth_stride,
                         int width, int height, float depth_factor, float bf, float* uright, float* depth);
/* cv::undistortPoints(pts, pts, K, mDistCoef, Mat(), K) for n points (xy_in / xy_out: n x {x, y} float32, host memory; in place
 * allowed), on the device: what Frame::ComputeImageBounds (S/Frame.cc:756-783) runs on the four image corners. */
int orbx_undistort_points(int device, const float* xy_in, int n, float fx, float fy, float cx, float cy, const orbx_distortion* dist,
                          float* xy_out);
/* Grid as CSR for tests: cell id = ix*48+iy, items in keypoint-index order (Appendix E-2). */
int orbm_frame_get_grid(orbm_frame* f, int32_t* cell_start /*64*48+1*/, int32_t* cell_items /*n*/);

/* int ORBmatcher::DescriptorDistance(a,b), S/ORBmatcher.cc:2358-2374, as a dense nq x nt matrix
 * (row-major int32) -- the raw Hamming kernel. */
int orbm_hamming_matrix(int device, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* dist);
/* Best / second-best over all t for every q: out4 = nq x {best_dist,best_idx,second_dist,second_idx}. */
int orbm_hamming_best2(int device, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* out4);

/* MapPoint fields read by SearchByProjection(Frame&, vector<MapPoint*>&...) after isInFrustum
 * filled them (SURVEY.md Appendix E-3, S/Frame.cc:529-538).  SoA, m entries. */
typedef struct orbm_mappoints_view {
  int32_t m;
  const uint8_t* track_in_view;   /* mbTrackInView */
  const uint8_t* bad;             /* isBad() */
  const float* proj_x;            /* mTrackProjX */
  const float* proj_y;            /* mTrackProjY */
  const float* proj_xr;           /* mTrackProjXR */
  const float* track_depth;       /* mTrackDepth */
  const int32_t* scale_level;     /* mnTrackScaleLevel */
  const float* view_cos;          /* mTrackViewCos */
  const uint8_t* desc;            /* GetDescriptor(), m x 32 */
  const int32_t* n_obs;           /* Observations() */
} orbm_mappoints_view;

/* World-space map points for the fused isInFrustum + search path (Appendix E-3, second half). */
typedef struct orbm_worldpoints_view {
  int32_t m;
  const float* pos;        /* m x 3  GetWorldPos() */
  const float* normal;     /* m x 3  GetNormal() */
  const float* min_dist;   /* m      mfMinDistance (raw; x0.8 applied as S/MapPoint.cc:617-621) */
  const float* max_dist;   /* m      mfMaxDistance (raw; x1.2 applied as S/MapPoint.cc:623-627) */
  const uint8_t* desc;     /* m x 32 */
  const int32_t* n_obs;    /* m */
  const uint8_t* bad;      /* m */
  const uint8_t* skip;     /* m, 1 = not a candidate (already matched / mnLastFrameSeen, S/Tracking.cc:3088-3109); may be NULL */
} orbm_worldpoints_view;

/* bool Frame::isInFrustum(MapPoint*, 0.5) for m points, S/Frame.cc:466-543 (Nleft == -1 branch):
 * fills the track fields.  Outputs are host arrays of m entries. */
int orbm_is_in_frustum(orbm_frame* f, const float* Tcw /*16, row-major*/, const orbm_worldpoints_view* pts,
                       float viewing_cos_limit, uint8_t* track_in_view, float* proj_x, float* proj_y,
                       float* proj_xr, float* track_depth, int32_t* scale_level, float* view_cos);

/* int ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*>&, th, bFarPoints, thFarPoints),
 * S/ORBmatcher.cc:44-214 (Nleft == -1).  assigned_mp[n] (in/out) is F.mvpMapPoints flattened:
 * -1 = NULL, otherwise an index; indices written by this call are positions in `mps`.
 * assigned_obs[n] (in/out) is Observations() of that map point.  *nmatches = return value. */
int orbm_search_by_projection_mps(orbm_frame* f, const orbm_mappoints_view* mps, float th,
                                  int far_points, float th_far_points, float nnratio,
                                  int32_t* assigned_mp, int32_t* assigned_obs, int* nmatches);

/* Fused Tracking::SearchLocalPoints body (S/Tracking.cc:3111-3153): isInFrustum(.,0.5) for every
 * non-skipped point, then the search above, map points staying resident on the device. */
typedef struct orbm_map orbm_map;
int orbm_map_create(int device, int cap_points, orbm_map** out);
int orbm_map_destroy(orbm_map* m);
int orbm_map_upload(orbm_map* m, const orbm_worldpoints_view* pts);
/* MapPoint::Observations() of the points of the last upload, refreshed without re-uploading the map (host side only: the serial commit
 * reads it, S/ORBmatcher.cc:89-91).  With it a local map stays resident across frames: its static fields (position, normal, distance
 * range, descriptor) are uploaded when Tracking::UpdateLocalPoints / the local BA's write-back changed them, the per-frame exclusions
 * (points the frame already holds, points that became bad) go through `skip`. */
int orbm_map_set_observations(orbm_map* m, const int32_t* n_obs /* m */);
int orbm_search_local_points(orbm_frame* f, orbm_map* m, const float* Tcw, const uint8_t* skip /*m or NULL*/,
                             float th, int far_points, float th_far_points, float nnratio,
                             int32_t* assigned_mp, int32_t* assigned_obs, int* nmatches);
/* Same, and in_frustum[m] (may be NULL) reports for which points isInFrustum() returned true -- the points the loop of
 * Tracking::SearchLocalPoints calls IncreaseVisible() for and counts in nToMatch (S/Tracking.cc:3118-3122). */
int orbm_search_local_points_vis(orbm_frame* f, orbm_map* m, const float* Tcw, const uint8_t* skip /*m or NULL*/,
                                 float th, int far_points, float th_far_points, float nnratio,
                                 int32_t* assigned_mp, int32_t* assigned_obs, int* nmatches, uint8_t* in_frustum /*m or NULL*/);

/* LastFrame fields read by SearchByProjection(Frame &Cur, const Frame &Last, th, bMono)
 * (SURVEY.md Appendix E-4). SoA, n entries (= LastFrame.N). */
typedef struct orbm_lastframe_view {
  int32_t n;
  const uint8_t* mp_valid;    /* LastFrame.mvpMapPoints[i] != NULL */
  const uint8_t* outlier;     /* LastFrame.mvbOutlier[i] */
  const float* world_pos;     /* n x 3, pMP->GetWorldPos() */
  const uint8_t* desc;        /* n x 32, pMP->GetDescriptor() */
  const int32_t* octave;      /* LastFrame.mvKeys[i].octave */
  const float* angle;         /* LastFrame.mvKeysUn[i].angle */
  const int32_t* n_obs;       /* pMP->Observations() */
  float Tcw[16];              /* LastFrame.mTcw, row-major */
} orbm_lastframe_view;

/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono),
 * S/ORBmatcher.cc:1970-2186 (Nleft == -1).  Tcw_cur = CurrentFrame.mTcw.  assigned_* as above
 * (indices are positions i in the last frame). */
int orbm_search_by_projection_frame(orbm_frame* cur, const float* Tcw_cur, const orbm_lastframe_view* last,
                                    float th, int mono, int check_orientation,
                                    int32_t* assigned_mp, int32_t* assigned_obs, int* nmatches);

/* The same search with the last frame's view RESIDENT on the device.  Tracking knows mLastFrame's map points when it has finished
 * tracking that frame (mLastFrame = Frame(mCurrentFrame), S/Tracking.cc:2086-2090) -- a frame time before the next
 * SearchByProjection(Current, Last) reads them: orbm_lastview_upload takes the view then (one packed copy on the library's M stream,
 * asynchronous; the view's arrays may be reused as soon as it returns), orbm_search_by_projection_frame_resident reads it from HBM
 * instead of from pinned host memory over PCIe at the moment the next constructor's images cross it.  Same results as
 * orbm_search_by_projection_frame on the same view. */
typedef struct orbm_lastview orbm_lastview;
int orbm_lastview_create(int device, int cap_features, orbm_lastview** out);
int orbm_lastview_destroy(orbm_lastview* v);
int orbm_lastview_upload(orbm_lastview* v, const orbm_lastframe_view* last);
int orbm_search_by_projection_frame_resident(orbm_frame* cur, const float* Tcw_cur, orbm_lastview* last, float th, int mono,
                                             int check_orientation, int32_t* assigned_mp, int32_t* assigned_obs, int* nmatches);

/* DBoW2::FeatureVector flattened: sorted node ids, CSR feature lists. */
typedef struct orbm_featvec_view {
  int32_t n_nodes;
  const uint32_t* node_id;    /* ascending */
  const uint32_t* start;      /* n_nodes+1 */
  const uint32_t* feat_idx;   /* start[n_nodes] entries */
} orbm_featvec_view;

/* int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame &F, vector<MapPoint*>& vpMapPointMatches),
 * S/ORBmatcher.cc:269-471 (Nleft == -1).  kf_desc: nkf x 32; kf_mp_valid[i] = pMP && !isBad();
 * kf_angle = pKF->mvKeysUn[i].angle.  matches[f->n] out: KF feature index or -1. */
int orbm_search_by_bow(orbm_frame* f, const orbm_featvec_view* fv_frame,
                       const uint8_t* kf_desc, int nkf, const uint8_t* kf_mp_valid, const float* kf_angle,
                       const orbm_featvec_view* fv_kf, float nnratio, int check_orientation,
                       int32_t* matches, int* nmatches);

/* Server-side KeyFrame matchers.  A KeyFrame carries the same undistorted keypoints, descriptors
 * and 64x48 grid as the Frame it was made from (S/KeyFrame.cc:889-940 copies mGrid), so it is an orbm_frame here.
 *
 * int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints,
 *                                    vector<MapPoint*>& vpMatched, int th, float ratioHamming), S/ORBmatcher.cc:473-587
 *   -> camera_project = 1 (projects with pKF->mpCamera->project)
 * and the overload with vpPointsKFs / vpMatchedKF, :589-700 -> camera_project = 0 (float invz projection); the adapter
 * fills vpMatchedKF[idx] = vpPointsKFs[matched[idx]].
 * pts: candidate points resident on the device (pts.skip/bad exclude); already_found[m] (may be NULL) = point is already
 * in vpMatched on entry.  matched[n] in/out: -1 = NULL; entries written are indices into pts. */
int orbm_search_by_projection_sim3(orbm_frame* kf, orbm_map* pts, const float* Scw /*16, row-major Sim3*/,
                                   const uint8_t* already_found, int th, float ratio_hamming, int camera_project,
                                   int32_t* matched, int* nmatches);

/* int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12), S/ORBmatcher.cc:819-959.
 * kf2 = pKF2 with its feature vector fv2 and mp_valid2[i] = (MapPoint present and not bad); the pKF1 side is flattened
 * as for orbm_search_by_bow.  matches12[n1] out: feature index in pKF2 (-> vpMapPoints2[idx]) or -1.
 * Two-camera keyframes (NLeft != -1): the reference leaves out every feature with index >= mvKeysUn.size() on either side
 * (:854-856, :874-876) -- pass mp_valid1 / mp_valid2 = 0 for those. */
/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, const float th,
 * const int ORBdist) -- the relocalisation overload, I/ORBmatcher.h:54, S/ORBmatcher.cc:2188-2310 (Tracking::Relocalization,
 * S/Tracking.cc:3372-3410: th = 10 / ORBdist = 100, then th = 3 / ORBdist = 64).  kf_points: pKF->GetMapPointMatches() uploaded
 * feature by feature with orbm_map_upload (m = pKF->N; bad[i] = 1 where the keyframe has no point or the point isBad());
 * already_found[i] = sAlreadyFound.count(pMP) (NULL: none); kf_angle[i] = pKF->mvKeysUn[i].angle (read when check_orientation).
 * assigned_mp (f's N entries) in: >= 0 where CurrentFrame.mvpMapPoints[idx] != NULL -- here ANY map point blocks a feature
 * (:2246-2247); out: newly matched features hold the index i of the keyframe feature whose point they took. */
int orbm_search_by_projection_reloc(orbm_frame* cur, orbm_map* kf_points, const float* Tcw_cur /*16*/, const uint8_t* already_found /*m or NULL*/,
                                    const float* kf_angle /*m*/, float th, int orb_dist, int check_orientation,
                                    int32_t* assigned_mp, int* nmatches);
struct orbg_camera;
/* orbm_search_by_projection_sim3 with camera_project = 1 and pKF->mpCamera a camera model (a fisheye keyframe): :515 projects through it. */
int orbm_search_by_projection_sim3_cam(orbm_frame* kf, orbm_map* pts, const float* Scw /*16, row-major Sim3*/, const struct orbg_camera* cam,
                                       const uint8_t* already_found, int th, float ratio_hamming, int32_t* matched, int* nmatches);
/* ... the same with CurrentFrame.mpCamera a camera model (a monocular fisheye frame): :2217 projects through it. */
int orbm_search_by_projection_reloc_cam(orbm_frame* cur, orbm_map* kf_points, const float* Tcw_cur /*16*/, const struct orbg_camera* cam,
                                        const uint8_t* already_found /*m or NULL*/, const float* kf_angle /*m*/, float th, int orb_dist,
                                        int check_orientation, int32_t* assigned_mp, int* nmatches);
int orbm_search_by_bow_kf(orbm_frame* kf2, const orbm_featvec_view* fv2, const uint8_t* mp_valid2,
                          const uint8_t* desc1, int n1, const uint8_t* mp_valid1, const float* angle1,
                          const orbm_featvec_view* fv1, float nnratio, int check_orientation,
                          int32_t* matches12, int* nmatches);

/* ---------------------------------------------------------------- Sim3Solver (server place recognition)
 * The link between orbm_search_by_bow_kf and orbm_search_by_projection_sim3 in LoopClosing::DetectCommonRegionsFromBoW
 * (S/LoopClosing.cc:707-718): RANSAC over minimal sets of three matched map points, Horn's closed form per hypothesis, inliers by
 * reprojection in both keyframes.  Every hypothesis of a call is evaluated in ONE kernel launch; the reference's serial rule
 * ("first iteration that converges, else the last one with the largest count") is then replayed over the counts in draw order, so
 * the outcome is the one the serial loop gives for the same draws, including the iteration at which it stops.
 *
 * The flat problem is what the constructor keeps per surviving pair (S/Sim3Solver.cc:38-128): X3Dc1 / X3Dc2 = mvX3Dc1 / mvX3Dc2
 * (n x 3 float, camera frames), max_err1 / max_err2 = mvnMaxError1 / mvnMaxError2 -- vector<size_t> in I/Sim3Solver.h:76-77, i.e.
 * 9.210 * sigma2 TRUNCATED to an integer -- and the intrinsics of pKF1->mpCamera / pKF2->mpCamera (Pinhole::project,
 * S/CameraModels/Pinhole.cpp:41-52; mK1 / mK2 are stored by the reference and never read).  camera_model1/2 must be 0 (pinhole):
 * any other model is refused with ORBG_BAD_ARG.  A point with z <= 0 is not special-cased: the reference does not.
 * struct_size = sizeof(the struct) as the caller was compiled: a struct that can grow says how large the caller believes it is. */
typedef struct orbm_sim3_problem {
  uint32_t struct_size;
  int32_t  n;                    /* N = mvpMapPoints1.size() */
  const float* X3Dc1;            /* n x 3 */
  const float* X3Dc2;            /* n x 3 */
  const uint32_t* max_err1;      /* n */
  const uint32_t* max_err2;      /* n */
  float fx1, fy1, cx1, cy1;      /* pCamera1 */
  float fx2, fy2, cx2, cy2;      /* pCamera2 */
  int32_t camera_model1, camera_model2;
  int32_t fix_scale;             /* mbFixScale */
} orbm_sim3_problem;

/* SetRansacParameters' arguments (S/Sim3Solver.cc:132; defaults 0.99, 6, 300 in I/Sim3Solver.h:46) */
typedef struct orbm_sim3_params {
  double  probability;
  int32_t min_inliers;
  int32_t max_iterations;
} orbm_sim3_params;

/* Outcome of iterate() / find().  T12 / R / t / s / inliers / n_inliers describe mBestT12, mBestRotation, mBestTranslation, mBestScale,
 * mvbBestInliers and mnBestInliers AFTER the call (valid when have_best; they persist between calls as in the reference, and on
 * convergence they are the converged hypothesis).  The reference's outputs follow from the flags: nInliers / vbInliers are
 * n_inliers / inliers when converged and 0 / all false otherwise; the four-argument iterate returns T12 when converged and an empty
 * matrix otherwise, the five-argument one T12 when converged or improved_in_this_call (its local bestSim3, :243,282) and empty otherwise.
 * inliers: caller's buffer of n bytes over the kept pairs (NULL: not wanted); vbInliers[mvnIndices1[i]] = inliers[i].
 * hyp_*: optional per-hypothesis outputs of THIS call in draw order, for checkers (NULL: not read back): inlier counts
 * (iterations), T12 (iterations x 16) and bit-packed masks (iterations x ceil(n / 64) words, bit i & 63 of word i >> 6).  They cover
 * every iteration handed to the launch, also those behind the one that converged. */
typedef struct orbm_sim3_result {
  uint32_t struct_size;
  int32_t  no_more;                /* bNoMore */
  int32_t  converged;              /* bConverge */
  int32_t  n_inliers;              /* mnBestInliers */
  int32_t  iterations_done;        /* mnIterations after the call */
  int32_t  iterations_run;         /* iterations the serial loop would have run in this call */
  int32_t  improved_in_this_call;
  int32_t  best_iteration;         /* 0-based mnIterations index of the hypothesis that became the best in this call, or -1 */
  int32_t  have_best;
  float    T12[16];
  float    R[9];
  float    t[3];
  float    s;
  uint8_t* inliers;
  int32_t* hyp_n_inliers;
  float*   hyp_T12;
  uint64_t* hyp_masks;
} orbm_sim3_result;

typedef struct orbm_sim3 orbm_sim3;

/* Sim3Solver::Sim3Solver after its loop over the matches (S/Sim3Solver.cc:119-127): create + set_problem.  set_problem copies the
 * arrays, resets mnIterations / mnBestInliers and applies SetRansacParameters() at its defaults, as the constructor does. */
int orbm_sim3_create(int device, orbm_sim3** out);
int orbm_sim3_destroy(orbm_sim3* h);
int orbm_sim3_set_stream(orbm_sim3* h, void* hip_stream);
int orbm_sim3_set_problem(orbm_sim3* h, const orbm_sim3_problem* p);
/* void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations), S/Sim3Solver.cc:132-157 (host). */
int orbm_sim3_set_ransac_parameters(orbm_sim3* h, double probability, int min_inliers, int max_iterations);
/* ... the same formula without a handle: *out = mRansacMaxIts for N = n.  Runs without a device. */
int orbm_sim3_ransac_iterations(int n, double probability, int min_inliers, int max_iterations, int* out);
/* The minimal sets of :189-206: draws = the raw DUtils::Random::RandomInt(0, size - 1) results, three per iteration (iteration k
 * draws from lists of n, n - 1 and n - 2 entries; anything else is ORBG_BAD_ARG); idx = the three correspondence indices the
 * swap-with-back removal on mvAllIndices gives.  Host only, runs without a device; the kernel uses the same closed form. */
int orbm_sim3_resolve_draws(int n, const int32_t* draws, int n_iterations, int32_t* idx);
/* cv::Mat Sim3Solver::iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers[, bool& bConverge]),
 * S/Sim3Solver.cc:159-292: up to n_iterations iterations (fewer when mRansacMaxIts is reached) in one launch; draws as above, 3 *
 * n_iterations values, of which the first 3 * iterations_run are the ones the serial loop would have consumed.  N < min_inliers:
 * no_more without a launch (:165-169).  find() (:294-298) is iterate(mRansacMaxIts). */
int orbm_sim3_iterate(orbm_sim3* h, int n_iterations, const int32_t* draws, orbm_sim3_result* result);
/* find() of B fresh solvers -- the candidates DetectCommonRegionsFromBoW tries one after another, of up to four agents -- in ONE
 * launch: problems[b] with SetRansacParameters(params[b]) and draws[b] (3 * mRansacMaxIts(b) values, see
 * orbm_sim3_ransac_iterations).  results[b] as for iterate on a new solver.  All arguments and the device are checked before any
 * result is written.  A problem with min_inliers <= n < 3 cannot draw a minimal set (the reference would index an empty list):
 * ORBG_BAD_ARG, here and in orbm_sim3_iterate. */
int orbm_sim3_solve_batch(int device, const orbm_sim3_problem* problems, int B, const orbm_sim3_params* params,
                          const int32_t* const* draws, orbm_sim3_result* results);

/* ---------------------------------------------------------------- OptimizeSim3 (server place recognition, step 4 of 5)
 * int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
 *                             const bool bFixScale, Eigen::Matrix<double,7,7>& mAcumHessian, const bool bAllPoints),
 * S/Optimizer.cc:4031-4310 -- the overload LoopClosing calls between the two SearchByProjection of DetectCommonRegionsFromBoW
 * (S/LoopClosing.cc:782) and for every keyframe in DetectAndReffineSim3FromLastKF (:555).  The overloads at :3833 and :4312 have no
 * caller and are not provided.  The per-candidate chain is now five exports: orbm_search_by_bow_kf -> orbm_sim3_iterate /
 * orbm_sim3_solve_batch -> orbm_search_by_projection_sim3 (camera_project = 0) -> orbm_sim3_optimize ->
 * orbm_search_by_projection_sim3 (camera_project = 1).
 *
 * The whole refinement -- optimize(5) with Huber, the removal of the pairs with chi2 > th2, optimize(10 or 5) without Huber, the
 * final classification; every Levenberg-Marquardt iteration and trial, with g2o's numeric Jacobians (delta = 1e-9) -- runs in ONE
 * kernel launch, and a batch of problems (the three loop + three merge candidates of up to four agents) in one launch too, one
 * workgroup per problem.  Results do not depend on what else is in the batch, and two runs give the same bits.
 *
 * The flat problem is what the loop :4083-4223 hands to g2o per kept match i (orbgpu::sim3opt_collect in orbgpu_dropin.hpp builds
 * it): X3Dc1 / X3Dc2 = P3D1c / P3D2c, the map points in the two camera frames AS THE FLOATS the reference computes (:4108, :4116);
 * obs1 = pKF1->mvKeysUn[i].pt (:4164-4165), inv_sigma2_1 = pKF1->mvInvLevelSigma2[kpUn1.octave] (:4172); obs2 / inv_sigma2_2 the
 * same for pKF2->mvKeysUn[i2] (:4186-4187, :4210) when pMP2 is observed in pKF2, and otherwise (i2 < 0, kept because bAllPoints)
 * what :4192-4210 produce: obs2 = (x / z, y / z) of P3D2c -- NORMALISED coordinates, compared with a pixel projection -- and
 * inv_sigma2_2 = mvInvLevelSigma2[0], because cv::KeyPoint(Point2f, mnTrackScaleLevel) sets `size` and leaves `octave` 0.  That is
 * the reference's behaviour and is reproduced; such pairs are almost always removed in round 1.
 * fx1 .. cy2: vSim3->pCamera1 / pCamera2 (:4056-4057, Pinhole::project, S/CameraModels/Pinhole.cpp:41-47); camera_model1/2 must be 0
 * (pinhole), anything else is ORBG_BAD_ARG as in orbm_sim3_problem.  A mapped point with z <= 0 is not special-cased, and NaN / inf
 * take the branches the reference's comparisons give them (chi2 > th2 is false for NaN: such a pair stays an inlier). */
typedef struct orbm_sim3opt_problem {
  uint32_t struct_size;
  int32_t  n;                       /* edge pairs = vpEdges12.size() */
  const float* X3Dc1;               /* n x 3, P3D1c (:4108) */
  const float* X3Dc2;               /* n x 3, P3D2c (:4116) */
  const float* obs1;                /* n x 2 (:4165) */
  const float* obs2;                /* n x 2 (:4187 / :4198) */
  const float* inv_sigma2_1;        /* n (:4172) */
  const float* inv_sigma2_2;        /* n (:4210) */
  float fx1, fy1, cx1, cy1;         /* vSim3->pCamera1 */
  float fx2, fy2, cx2, cy2;         /* vSim3->pCamera2 */
  int32_t camera_model1, camera_model2;
  int32_t fix_scale;                /* bFixScale -> vSim3->_fix_scale (:4052) */
  float   th2;                      /* th2; the Huber delta is sqrt(th2) computed in float (:4073) */
  double  q[4], t[3], s;            /* g2oS12 on entry: rotation().coeffs() (x, y, z, w), translation(), scale() */
  int32_t n_correspondences;        /* nCorrespondences (:4160; == n: every counted match gets its pair; the early return is worded on it) */
} orbm_sim3opt_problem;

/* removed[i] over the pairs: 0 kept, 1 NULL-ed at :4244 (round 1), 2 NULL-ed at :4294 (final pass); the caller sets
 * vpMatches1[vnIndexEdge[i]] = NULL where it is not 0.  returned_early: the `return 0` at :4271 (nCorrespondences - nBad < 10) --
 * q / t / s are then the INPUT (the reference does not write g2oS12 there) while `removed` carries the round-1 removals (vpMatches1 is
 * already edited).  mAcumHessian is set to zero by the reference (:4280; the line that would fill it is commented out, :4299): the
 * caller zeroes it unless returned_early.  trace (optional, trace_cap entries of 4 doubles): per LM iteration {round, lambda after
 * the iteration, activeRobustChi2 after it, trials}.  edge_chi2 (optional, 4 x n doubles): chi2 of e12 / e21 as read at :4241 (the
 * LAST trial's errors, no computeError before it) and as read at :4291 (recomputed; 0 for pairs that did not get there). */
typedef struct orbm_sim3opt_result {
  uint32_t struct_size;
  int32_t  n_in;                    /* the return value */
  int32_t  returned_early;
  int32_t  n_bad_round1;            /* nBad (:4249) */
  double   q[4], t[3], s;           /* g2oS12 after the call */
  uint8_t* removed;                 /* n bytes, caller's (NULL: not wanted) */
  int32_t  iters[2];                /* LM iterations run in each round */
  double   chi2[2];                 /* activeRobustChi2 after the last accepted step of each round */
  double*  trace;
  int32_t  trace_cap, trace_len;
  double*  edge_chi2;
} orbm_sim3opt_result;

/* One problem / B problems in one launch.  n == 0: no launch, the outcome g2o gives for an empty graph (optimize() does nothing,
 * 0 - 0 < 10: n_in = 0, returned_early = 1, the input estimate).  All arguments and the device are checked before any result is
 * written: struct_size, NULL arrays with n > 0, a non-finite q / t / s, th2 <= 0 (or NaN), a camera model other than pinhole ->
 * ORBG_BAD_ARG; no device -> ORBG_NO_DEVICE (there is no CPU fallback).  The arguments are checked before the device is looked for.
 * The work runs on the library's M stream of `device` (see "Streams"), with buffers that belong to the calling thread: concurrent
 * calls from several threads are independent. */
int orbm_sim3_optimize(int device, const orbm_sim3opt_problem* p, orbm_sim3opt_result* r);
int orbm_sim3_optimize_batch(int device, const orbm_sim3opt_problem* problems, int B, orbm_sim3opt_result* results);

/* ---------------------------------------------------------------- TwoViewReconstruction (monocular initialisation)
 * bool TwoViewReconstruction::Reconstruct(vKeys1, vKeys2, vMatches12, R21, t21, vP3D, vbTriangulated), S/TwoViewReconstruction.cc:39-127,
 * what Tracking::MonocularInitialization runs through Pinhole::ReconstructWithTwoViews (S/CameraModels/Pinhole.cpp:105): the
 * homography RANSAC and the fundamental-matrix RANSAC (`iterations` hypotheses each, every one scored against every match), the
 * choice between the two models, and ReconstructH / ReconstructF with CheckRT over all 8 / 4 motion hypotheses.  Two kernel launches
 * on one stream, no host round trip between them; the serial rules ("first iteration with the strictly largest score") are replayed
 * on the device over the scores in iteration order, so the outcome is the one the serial loops give for the same draws.
 *
 * keys1 / keys2: the mvKeysUn points of the two frames (n1 x 2 / n2 x 2 float); Normalize (:753-799) runs over ALL of them.
 * matches12: n1 entries, index into keys2 or -1 (any negative value) for "no match"; N = the number of matched keypoints.
 * fx .. cy: mK.  sigma / iterations: the constructor's arguments (1.0 / 200).
 * struct_size = sizeof(the struct) as the caller was compiled. */
#define ORBI_TWO_VIEW_MAX_MATCHES 8192
#define ORBI_TWO_VIEW_MAX_ITERATIONS 4096
typedef struct orbi_two_view_problem {
  uint32_t struct_size;
  int32_t  n1, n2;
  const float* keys1;              /* n1 x 2 */
  const float* keys2;              /* n2 x 2 */
  const int32_t* matches12;        /* n1 */
  float fx, fy, cx, cy;
  float sigma;
  int32_t iterations;
} orbi_two_view_problem;

/* model: 0 = none (SH + SF == 0, :111), 1 = ReconstructH (RH > 0.50), 2 = ReconstructF.  SH / SF: the best scores; best_iteration_H /
 * _F: the 0-based iteration that holds them, -1 when no hypothesis scored above 0 (H21 / F21 are zero then).  R21 / t21 / vP3D /
 * vbTriangulated are written when success (zero otherwise; the reference leaves its outputs untouched on failure).  vP3D (n1 x 3)
 * and vbTriangulated (n1 bytes) are the caller's buffers, indexed by the keypoint index of frame 1 (NULL: not wanted).
 * n_motions: 8 (H), 4 (F), or 0 when no CheckRT ran (model 0, or ReconstructH's d1 / d2 < 1.00001 || d2 / d3 < 1.00001 return, for
 * which h_degenerate is set); motion_nGood / motion_parallax / motion_R / motion_t: per motion hypothesis tried, in the reference's
 * order; best_motion: the one returned, or -1.  n_inliers: N of ReconstructH / F (the inlier count of the chosen model's best mask).
 * T1 / T2: Normalize's matrices of frame 1 / 2.
 * hyp_*: optional per-hypothesis outputs for checkers (NULL: not read back), H hypotheses then F hypotheses: hyp_scores
 * (2 x iterations), hyp_models (2 x iterations x 9: H21i / F21i), hyp_masks (2 x iterations x ceil(N / 64) words; bit i & 63 of
 * word i >> 6 is match i in matches12 order) and hyp_sets (iterations x 8 resolved match indices). */
typedef struct orbi_two_view_result {
  uint32_t struct_size;
  int32_t  success;
  int32_t  model;
  int32_t  best_iteration_H, best_iteration_F;
  int32_t  n_matches;
  int32_t  n_inliers;
  int32_t  n_motions;
  int32_t  best_motion;
  int32_t  h_degenerate;
  float    SH, SF;
  float    H21[9], F21[9];
  float    R21[9], t21[3];
  float    T1[9], T2[9];
  int32_t  motion_nGood[8];
  float    motion_parallax[8];
  float    motion_R[72];
  float    motion_t[24];
  float*   vP3D;
  uint8_t* vbTriangulated;
  float*   hyp_scores;
  float*   hyp_models;
  uint64_t* hyp_masks;
  int32_t* hyp_sets;
} orbi_two_view_result;

/* The minimal sets of :76-96: draws = the raw DUtils::Random::RandomInt(0, size - 1) results, eight per iteration (iteration k draws
 * from lists of n, n - 1, ..., n - 7 entries; anything else is ORBG_BAD_ARG); idx = the eight match indices the swap-with-back
 * removal on vAllIndices gives.  Host only, runs without a device; the kernel uses the same closed form. */
int orbi_two_view_resolve_draws(int n, const int32_t* draws, int iterations, int32_t* idx);
/* Reconstruct().  draws: 8 * iterations raw draws for N matches, as above.  Fewer than 8 matches cannot draw a set (the reference
 * would index an empty list): ORBG_BAD_ARG, as are a struct_size too small, NULL arrays, a match index outside keys2, iterations < 1
 * and a draw out of range.  N > ORBI_TWO_VIEW_MAX_MATCHES or iterations > ORBI_TWO_VIEW_MAX_ITERATIONS: ORBG_CAP_EXCEEDED.  The
 * arguments are checked before the device is looked for; no device: ORBG_NO_DEVICE (there is no CPU fallback).  The work runs on
 * the library's M stream of `device` with buffers that belong to the calling thread. */
int orbi_two_view_reconstruct(int device, const orbi_two_view_problem* p, const int32_t* draws, orbi_two_view_result* r);

/* ---------------------------------------------------------------- CreateNewMapPoints (LocalMapping, once per keyframe)
 * void LocalMapping::CreateNewMapPoints(), S/LocalMapping.cc:520-865: ORBmatcher::SearchForTriangulation (S/ORBmatcher.cc:961-1202)
 * of the current keyframe against each of its 10 (stereo) / 20 (mono) covisible neighbours and the triangulation of every match
 * (:616-863).  In this reference vbMatched2 is declared and never set (:1007,1063), so inside one SearchForTriangulation call every
 * feature of KF1 is matched independently of every other one; the only serial coupling is ACROSS neighbours: a feature idx1 that got
 * a point from neighbour i (AddMapPoint(pMP, idx1), :852) is skipped for neighbours j > i (:1029-1035).  All B neighbours therefore go
 * in ONE kernel launch -- one record per (neighbour, idx1): the match and what the triangulation of it gives -- and the host replays
 * the integer bookkeeping over the records in neighbour order.
 *
 * Scope: pinhole keyframes without a second camera (mpCamera2 == NULL, NLeft == -1, mpCamera a Pinhole).  There is no way to pass
 * any other keyframe: for a rig or a non-pinhole camera the glue must fall back to the reference's body.
 *
 * orbm_newpoints_kf -- one keyframe side.  frame: the resident keyframe (mvKeysUn, mDescriptors, mvuRight, mvDepth; a KeyFrame is an
 * orbm_frame, see the server-side matchers above).  featvec: mFeatVec.  has_mp[n]: GetMapPoint(i) != NULL (:1029, :1060 -- ANY point,
 * bad ones included).  keys_xy: mvKeys[i].pt, n x 2, read by KeyFrame::UnprojectStereo only (S/KeyFrame.cc:947-963); NULL = mvKeys ==
 * mvKeysUn (no distortion, S/Frame.cc:723-727).  Tcw = GetPose() rows 0-2, Twc = GetPoseInverse() rows 0-2, Ow = GetCameraCenter(),
 * AS THE KEYFRAME HOLDS THEM: nothing is re-derived from another (UnprojectStereo reads the stored Twc).  fx .. invfy, mb, mbf: the
 * KeyFrame members.  scale_factors / level_sigma2: mvScaleFactors / mvLevelSigma2, n_levels entries; scale_factor: mfScaleFactor.
 * struct_size = sizeof(the struct) as the caller was compiled. */
#define ORBG_NEWPOINTS_MAX_NEIGHBOURS 64
typedef struct orbm_newpoints_kf {
  uint32_t struct_size;
  orbm_frame* frame;
  orbm_featvec_view featvec;
  const uint8_t* has_mp;
  const float* keys_xy;
  float Tcw[12], Twc[12], Ow[3];
  float fx, fy, cx, cy, invfx, invfy, mb, mbf;
  int32_t n_levels;
  const float* scale_factors;
  const float* level_sigma2;
  float scale_factor;
} orbm_newpoints_kf;

/* only_stereo / coarse: bOnlyStereo / bCoarse of SearchForTriangulation; check_orientation: mbCheckOrientation of the matcher
 * (CreateNewMapPoints constructs ORBmatcher(0.6f, false): 0 there); far_points / th_far_points: mbFarPoints / mThFarPoints (:837). */
typedef struct orbm_newpoints_params {
  uint32_t struct_size;
  int32_t only_stereo, coarse, check_orientation, far_points;
  float th_far_points;
} orbm_newpoints_params;

/* status of a record: accepted, or the `continue` of the reference that ended it.  Codes 1-4: no match (idx2 = -1). */
enum {
  ORBM_NP_ACCEPTED = 0,
  ORBM_NP_HAS_POINT = 1,       /* pMP1 != NULL, S/ORBmatcher.cc:1032 */
  ORBM_NP_NOT_STEREO = 2,      /* bOnlyStereo && !bStereo1, :1039-1041 */
  ORBM_NP_NO_NODE = 3,         /* the feature's vocabulary node is not in KF2's feature vector (or the feature is in no node) */
  ORBM_NP_NO_MATCH = 4,        /* bestIdx2 < 0, :1135 */
  ORBM_NP_W_ZERO = 5,          /* x3D.at<float>(3) == 0, S/LocalMapping.cc:742 */
  ORBM_NP_LOW_PARALLAX = 6,    /* "No stereo and very low parallax", :757-760 */
  ORBM_NP_EMPTY = 7,           /* UnprojectStereo returned an empty matrix (mvDepth <= 0), :764 */
  ORBM_NP_Z1 = 8,              /* :767 */
  ORBM_NP_Z2 = 9,              /* :771 */
  ORBM_NP_REPROJ1 = 10,        /* :786 / :798 */
  ORBM_NP_REPROJ2 = 11,        /* :812 / :823 */
  ORBM_NP_DIST_ZERO = 12,      /* :834 */
  ORBM_NP_FAR = 13,            /* :837 */
  ORBM_NP_SCALE = 14           /* :843 */
};
/* One record per (neighbour b, feature idx1) at [b * n1 + idx1], independent of every other record: what SearchForTriangulation
 * picks for idx1 in neighbour b given has_mp as passed (idx2, -1: none; dist: its Hamming distance) and what :707-844 make of that
 * pair.  x3D: the point when one was formed (status 0 or >= 8); w: x3D.at<float>(3) of the linear triangulation (0 for the
 * UnprojectStereo branches); cos_parallax: cosParallaxRays. */
typedef struct orbm_newpoints_record {
  int32_t idx2, dist, status;
  float x3D[3];
  float w;
  float cos_parallax;
} orbm_newpoints_record;
/* One created point: new MapPoint(x3D, ...), observed at idx1 in the current keyframe and at idx2 in neighbours[neighbour]. */
typedef struct orbm_newpoint {
  int32_t neighbour, idx1, idx2;
  float x3D[3];
} orbm_newpoint;

/* The loop :564-864 over neighbours[0 .. B) (the keyframes that passed the baseline gates :573-590, in vpNeighKFs order): one launch,
 * then the replay in neighbour order.  Per neighbour the replay drops every idx1 claimed by an earlier neighbour (before the rotation
 * vote, as :1029-1035 stand before :1143), applies the vote when check_orientation, and walks the surviving matches in ascending idx1
 * (vMatchedPairs, :1194-1199); an accepted record appends to `out` and claims idx1.
 * out[cap] / *n_out: the created points in the reference's creation order.  The loop's CheckNewKeyFrames() exit (:566) stops
 * between two neighbours: what the reference has created by then is the PREFIX of `out` with neighbour < i, so a caller that polls
 * the flag per neighbour boundary consumes a prefix and discards the rest.  More than cap points: ORBG_CAP_EXCEEDED (*n_out = the
 * count needed).  records (optional, B * n1): the raw records before the replay.  matches (optional, B * n1): vMatches12 of each
 * neighbour after the replay (-1: none).
 * All frames must be on one device (else ORBG_BAD_ARG); B > ORBG_NEWPOINTS_MAX_NEIGHBOURS: ORBG_CAP_EXCEEDED; B == 0 or no common
 * node needs no launch.  Arguments are checked before the device is looked for; no device: ORBG_NO_DEVICE (no CPU fallback).  The
 * work is enqueued on kf1's frame stream, behind what is pending on the neighbours' streams; buffers belong to the calling thread.
 * Arithmetic: csrc/newpoints.hip lists every choice (N-1 ...); the 4 x 4 null vector of the linear triangulation is the smallest
 * eigenvector of A^T A in float64 (cv::SVD::compute is float32 one-sided Jacobi in the reference): points agree with an OpenCV build
 * to float32 rounding, not to the bit.  No atomics: two runs give the same bits. */
int orbm_create_new_points(const orbm_newpoints_kf* kf1, const orbm_newpoints_kf* neighbours, int B, const orbm_newpoints_params* params,
                           orbm_newpoint* out, int cap, int* n_out, orbm_newpoints_record* records, int32_t* matches);
/* int ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse), S/ORBmatcher.cc:961-1202 (the F12
 * argument is unused there): the matcher alone.  pairs[cap x 2] = vMatchedPairs (idx1 ascending), *n = its size (the return value);
 * more than cap pairs: ORBG_CAP_EXCEEDED with *n = the count needed.  far_points / th_far_points are not read. */
int orbm_search_for_triangulation(const orbm_newpoints_kf* kf1, const orbm_newpoints_kf* kf2, const orbm_newpoints_params* params,
                                  int32_t* pairs, int cap, int* n);

/* ---------------------------------------------------------------- Fuse / SearchInNeighbors (LocalMapping, once per keyframe)
 * int ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, float th, bool bRight = false), S/ORBmatcher.cc:1395-1605,
 * as LocalMapping::SearchInNeighbors (S/LocalMapping.cc:868-976) calls it for every target keyframe and once for the current one, and
 * the Sim3 overload int ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint), :1607-1742 (LoopClosing::SearchAndFuse).
 *
 * For one (keyframe k, point i) pair everything up to bestIdx / bestDist (:1451-1566 | :1642-1716) depends on the keyframe's features
 * and pose and on the point's position, normal, distance range and descriptor.  All K x P pairs go in ONE kernel launch, one record
 * per pair at [k * P + i]; the serial part (:1431-1448 and :1569-1590: isBad, IsInKeyFrame, GetMapPoint, Observations, Replace,
 * AddObservation, AddMapPoint) stays with the caller, who replays it over the records in the reference's order
 * (include/orbgpu_localmapping.hpp).  The only input that changes while SearchInNeighbors runs is a point's descriptor (Replace ends in
 * ComputeDistinctiveDescriptors on the survivor): the candidates that passed the level and chi2 gates do not depend on it, so the
 * record carries them -- `cand` holds the first ORBG_FUSE_CAND_CAP = 16 of them in vIndices order, n_cand the exact count -- and the
 * caller rescores over that list (first strict minimum, from bestDist = 256 | INT_MAX); with n_cand > ORBG_FUSE_CAND_CAP it
 * re-evaluates that single pair (K = 1, P = 1) with the new descriptor.
 *
 * Scope: pinhole keyframes, bRight = false.  A keyframe of a rig (NLeft != -1) cannot be passed: the glue falls back.
 *
 * orbm_fuse_kf -- one target keyframe.  frame: the resident keyframe (mvKeysUn, mDescriptors, mvuRight, the grid and the image bounds
 * mnMinX .. mnMaxY).  LocalMapping form: Tcw = GetPose() rows 0-2 (GetRotation / GetTranslation, :1408-1409), Ow = GetCameraCenter(),
 * AS THE KEYFRAME HOLDS THEM; Scw is not read.  Sim3 form: Scw (4 x 4, row-major) is decomposed as :1616-1620, the way
 * orbm_search_by_projection_sim3 does it; Tcw / Ow are not read.  fx .. cy, mbf: the KeyFrame members.  scale_factors /
 * inv_level_sigma2: mvScaleFactors / mvInvLevelSigma2, n_levels entries; log_scale_factor: mfLogScaleFactor.
 * struct_size = sizeof(the struct) as the caller was compiled. */
#define ORBG_FUSE_MAX_KEYFRAMES 512      /* 20 neighbours + 20 x 20 second neighbours + 20 temporal ones, S/LocalMapping.cc:871-917 */
#define ORBG_FUSE_CAND_CAP 16
typedef struct orbm_fuse_kf {
  uint32_t struct_size;
  orbm_frame* frame;
  float Tcw[12], Ow[3];
  float Scw[16];
  float fx, fy, cx, cy, mbf;
  int32_t n_levels;
  const float* scale_factors;
  const float* inv_level_sigma2;
  float log_scale_factor;
} orbm_fuse_kf;

/* th: the search radius factor (3.0 in SearchInNeighbors, I/ORBmatcher.h:85); sim3_form: 0 = :1395 (chi2 gates 7.8 / 5.99, ur,
 * bestDist from 256), 1 = :1607 (the level gate only, bestDist from INT_MAX). */
typedef struct orbm_fuse_params {
  uint32_t struct_size;
  float th;
  int32_t sim3_form;
} orbm_fuse_params;

/* status of a record: it reached the candidate loop with at least one candidate, or the `continue` of the reference that ended it. */
enum {
  ORBM_FUSE_CANDIDATES = 0,    /* best_idx / best_dist are set: the caller compares best_dist with TH_LOW (:1569) | 100 (:1722) */
  ORBM_FUSE_NEG_DEPTH = 1,     /* p3Dc.at<float>(2) < 0.0f, :1455 | :1648 */
  ORBM_FUSE_NOT_IN_IMAGE = 2,  /* !pKF->IsInImage(uv.x, uv.y), :1469 | :1659 */
  ORBM_FUSE_DISTANCE = 3,      /* dist3D outside [minDistance, maxDistance], :1483 | :1669 */
  ORBM_FUSE_NORMAL = 4,        /* PO.dot(Pn) < 0.5 * dist3D, :1492 | :1676 */
  ORBM_FUSE_EMPTY_WINDOW = 5,  /* vIndices.empty(), :1505 | :1688 */
  ORBM_FUSE_NO_CANDIDATE = 6,  /* nothing passed the level / chi2 gates: bestDist keeps its start value, :1569 | :1722 fails */
  ORBM_FUSE_SKIPPED = 7        /* skip[k * P + i] (or bad[i] / skip[i] of the points view): no work was done */
};
/* level: nPredictedLevel (-1 when the pair ended before PredictScale); best_idx = -1 and best_dist = 256 | INT_MAX unless status is
 * ORBM_FUSE_CANDIDATES; n_cand: how many features passed the gates (status 0 <=> n_cand > 0). */
typedef struct orbm_fuse_record {
  int32_t status, best_idx, best_dist, level, n_cand;
} orbm_fuse_record;

/* One launch for kfs[0 .. K) x the m points of `pts` (pos, normal, min_dist, max_dist -- raw, the 0.8 / 1.2 factors are applied as
 * S/MapPoint.cc:617-627 -- and desc are read; bad[i] / skip[i], when given, skip point i for every keyframe; n_obs is not read).
 * skip (K x m, or NULL): skip[k * m + i] marks a pair whose point is bad or already in keyframe k at entry (:1439-1448 | :1638); both
 * conditions only ever become true during a call, so such a pair stays skipped in the replay.  records (K x m) and cand
 * (K x m x ORBG_FUSE_CAND_CAP, unused slots 0xFFFF) are host arrays.
 * K > ORBG_FUSE_MAX_KEYFRAMES, or a frame of ORBG_MAX_FRAME_FEATURES features or more (indices travel in 16 bits): ORBG_CAP_EXCEEDED.  All frames must be on one device (else ORBG_BAD_ARG).  Arguments are checked before
 * the device is looked for; no device: ORBG_NO_DEVICE (no CPU fallback).  K == 0 or m == 0 needs no launch.  The work is enqueued on
 * the calling thread's stream, behind what is pending on the keyframes' streams; buffers belong to the calling thread.  Arithmetic:
 * csrc/fuse.hip lists every choice.  No atomics: two runs give the same bits. */
int orbm_fuse(const orbm_fuse_kf* kfs, int K, const orbm_worldpoints_view* pts, const uint8_t* skip, const orbm_fuse_params* params,
              orbm_fuse_record* records, uint16_t* cand);

/* ---------------------------------------------------------------- ORBmatcher::SearchForInitialization (S/ORBmatcher.cc:702-817)
 *
 * The matcher of Tracking::MonocularInitialization (S/Tracking.cc:2217).  f1 = mInitialFrame, f2 = mCurrentFrame, both monocular
 * (Nleft == -1) and resident: uploaded, views of an extractor, or left by the monocular constructor.  prev_matched is vbPrevMatched
 * (n1 x {x, y}): the query point of feature i1 on entry, overwritten with F2.mvKeysUn[matches12[i1]].pt for the surviving matches
 * (:812-814) -- also when the call answers ORBG_CAP_EXCEEDED for the debug entries, so a caller that repeats the call hands in the
 * original again.  matches12 (n1) is vnMatches12, *n_matches the return value.  n_prev must be n1.
 *
 * The device gathers, per octave-0 feature of F1, the list Frame::GetFeaturesInArea(x, y, window_size, 0, 0) returns, in its order and
 * with the Hamming distances; the host applies :733-814 to the lists (csrc/init_replay.hpp).  Every output equals the reference's.
 *
 * window_size: windowSize (100 at the call site).  nn_ratio: mfNNratio (0.9).  check_orientation: mbCheckOrientation.
 * list_capacity: entries of the candidate buffer, 0 = the default (2^20, or what an earlier call of the thread grew it to).  Lists
 * that do not fit are never cut: the kernel reports the total, the buffer grows to it and the search runs again (n_regrown).  A total
 * above ORBM_INIT_SEARCH_MAX_LIST entries answers ORBG_CAP_EXCEEDED.  The total is an upper bound per query: every octave-0 feature of
 * the cells its window touches.
 *
 * debug (may be NULL): list_start (n1 + 1) receives the lists' CSR offsets, entries the lists as the replay saw them
 * (index2 | dist << 16), when all n_candidates of them fit into entries_cap; otherwise everything else is complete and the call
 * answers ORBG_CAP_EXCEEDED.  n_queries: octave-0 features of F1; n_evictions: :760-764; n_rot_rejected: :801-805.
 *
 * NULL pointers, n_prev != n1, window_size <= 0, list_capacity < 0, a struct_size below the struct's, frames on two devices:
 * ORBG_BAD_ARG, before anything is launched.  No device: ORBG_NO_DEVICE.  A side without features, or without an octave-0 feature:
 * 0 matches, no launch.  Per call: one upload (prev_matched) and two waits for results (the records and the total; the lists), one
 * more per regrowth.  Besides those, a frame built from a wire block is waited for once, since its host keypoints are written by its
 * own stream, and the call leaves its stream drained.  The level-0 view of f2 is built by the first call after its content changed
 * and kept on the frame.  The work is enqueued on the calling thread's stream behind what is pending on the frames' streams; buffers
 * belong to the calling thread.
 *
 * A frame that views an extractor handle (orbm_frame_from_extractor, orbx_frame_mono) reads that handle's feature buffers.  A later
 * extraction on the handle overwrites them without the frame noticing: while such a frame is still wanted as F1, its handle must not
 * extract again.  Extract the following frames on another handle (the constructor test keeps one per frame), or upload F1. */
#define ORBM_INIT_SEARCH_MAX_LIST (1 << 26)
typedef struct orbm_init_search_params {
  uint32_t struct_size; int32_t window_size; float nn_ratio; int32_t check_orientation; int32_t list_capacity;
} orbm_init_search_params;
typedef struct orbm_init_search_debug {   /* optional, for checkers: the candidate lists as the replay saw them */
  int32_t* list_start;  /* n1 + 1 */  uint32_t* entries; int32_t entries_cap;
  int32_t n_queries, n_candidates, n_evictions, n_rot_rejected, n_regrown;
} orbm_init_search_debug;
int orbm_search_for_initialization(orbm_frame* f1, orbm_frame* f2, float* prev_matched /* n1 x {x, y}, in/out */, int n_prev,
                                   const orbm_init_search_params* params, int32_t* matches12 /* n1 */, int* n_matches,
                                   orbm_init_search_debug* debug /* may be NULL */);

/* ---------------------------------------------------------------- bag of words */

/* DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> flattened (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:60-130,
 * m_nodes): node 0 is the root; the children of node i are child_ids[child_start[i] .. child_start[i+1]) in the order of
 * m_nodes[i].children; a node without children is a leaf (= word). */
enum { ORBV_TF_IDF = 0, ORBV_TF = 1, ORBV_IDF = 2, ORBV_BINARY = 3 };           /* WeightingType, BowVector.h:24-30 */
enum { ORBV_NORM_NONE = 0, ORBV_NORM_L1 = 1, ORBV_NORM_L2 = 2 };                /* what mustNormalize() reports (ORBvoc: L1) */
typedef struct orbv_vocab_view {
  int32_t n_nodes;
  int32_t L;                    /* m_L */
  int32_t weighting;            /* ORBV_TF_IDF for ORBvoc.txt */
  int32_t scoring_norm;         /* ORBV_NORM_L1 for ORBvoc.txt (L1_NORM scoring) */
  const int32_t* child_start;   /* n_nodes + 1 */
  const int32_t* child_ids;     /* child_start[n_nodes] node ids */
  const uint8_t* desc;          /* n_nodes x 32, m_nodes[i].descriptor (the root's is unused) */
  const double* weight;         /* n_nodes, m_nodes[i].weight */
  const int32_t* word_id;       /* n_nodes, m_nodes[i].word_id (meaningful for leaves) */
} orbv_vocab_view;
typedef struct orbv_vocab orbv_vocab;
int orbv_vocab_create(int device, const orbv_vocab_view* view, orbv_vocab** out);
int orbv_vocab_destroy(orbv_vocab* v);
/* The vocabulary in the reference's own file format: bool TemplatedVocabulary::loadFromTextFile(const std::string&),
 * Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1427 -- the ORBvoc.txt that System / ClientSystem hand to it -- parsed on the
 * host into an orbv_vocab_view (line 1: `k L scoring weighting`; line i: `parent isLeaf d0..d31 weight`, node ids in file order from 1,
 * children in file order, word ids to the isLeaf > 0 nodes in file order).  m_nodes is protected in the reference
 * (TemplatedVocabulary.h:405-423): this is the way in that needs no edit there.
 * flags: ORBV_TEXT_KEEP_TRAILING_NODE reproduces the extra node the reference's `while(!f.eof()) getline` loop makes of the empty
 * line after the last newline (a child of the root, no children, weight 0; its descriptor is indeterminate in the reference and zero
 * here); default: the tree the file describes.  A malformed file (header out of range, a node line with fewer than 35 fields, a
 * parent that is not an earlier node, node lines after a blank line): ORBG_BAD_ARG.
 * orbv_text_* is the host-only half (no GPU needed); orbv_vocab_from_text = load + orbv_vocab_create + free.
 * scoring (ScoringType, BowVector.h:48-56; ORBvoc.txt: 0 = L1_NORM) selects the BowVector normalisation as mustNormalize() reports it;
 * orbv_score_l1 / orbd_detect_n_best_candidates implement the L1 score only. */
enum { ORBV_TEXT_KEEP_TRAILING_NODE = 1 };
typedef struct orbv_text orbv_text;
int orbv_text_load(const char* path, int flags, orbv_text** out);
/* the parsed tree as a view (pointers valid until orbv_text_free); k / scoring / n_words may be NULL */
int orbv_text_view(const orbv_text* t, orbv_vocab_view* view, int32_t* k, int32_t* scoring, int32_t* n_words);
int orbv_text_free(orbv_text* t);
int orbv_vocab_from_text(int device, const char* path, int flags, orbv_vocab** out);
/* void transform(const TDescriptor& feature, WordId&, WordValue&, NodeId* nid, int levelsup), TemplatedVocabulary.h:1214-1260,
 * for n descriptors (host memory, n x 32): word_id[n], node_id[n] (node at level L - levelsup; 0 = root when that level is
 * <= 0 or -- pinned, the reference leaves it uninitialised -- when a leaf is reached above it), weight[n]. */
int orbv_transform(orbv_vocab* v, const uint8_t* desc, int n, int levelsup, int32_t* word_id, int32_t* node_id, double* weight);
/* the same for the features resident in a device frame (orbm_frame_upload / orbm_frame_from_extractor / orbx_frame_stereo) */
int orbv_transform_frame(orbv_vocab* v, orbm_frame* f, int levelsup, int32_t* word_id, int32_t* node_id, double* weight);
/* void transform(const vector<TDescriptor>&, BowVector&, FeatureVector&, int levelsup), :1127-1199, second half: BowVector
 * (ascending word ids, values weighted / normalised as the vocabulary prescribes) and FeatureVector (orbm_featvec_view layout)
 * from the per-feature outputs above.  Output arrays hold up to n entries (fv_start: n + 1). */
int orbv_bow_assemble(const orbv_vocab* v, const int32_t* word_id, const int32_t* node_id, const double* weight, int n,
                      int32_t* bow_word, double* bow_value, int32_t* n_words,
                      uint32_t* fv_node, uint32_t* fv_start, uint32_t* fv_feat, int32_t* n_fv_nodes);

/* void MapPoint::ComputeDistinctiveDescriptors(), S/MapPoint.cc:448-522, for m map points at once: the descriptors of point p's
 * observations are desc[start[p] .. start[p+1]) (x 32 bytes, in the order the reference pushes them into vDescriptors);
 * best[p] = index inside that list of the descriptor with the least median Hamming distance to the others (first one on
 * ties), or -1 for a point without observations (the reference returns early and keeps the old descriptor). */
int orbm_distinctive_descriptors(int device, const uint8_t* desc, const int32_t* start, int m, int32_t* best);

/* double L1Scoring::score(v1, v2) (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) of one query BowVector against m candidates
 * (the inner loop of KeyFrameDatabase::DetectNBestCandidates, S/KeyFrameDatabase.cc:594-761): candidates as CSR over
 * ascending word ids.  score[m] in [0, 1]. */
int orbv_score_l1(int device, const int32_t* q_word, const double* q_value, int nq, const int32_t* cand_start,
                  const int32_t* cand_word, const double* cand_value, int m, double* score);

/* ---------------------------------------------------------------- place recognition database */

/* What KeyFrameDatabase::DetectNBestCandidates (S/KeyFrameDatabase.cc:594-761) reads, flattened; keyframes are indices
 * 0 .. n_kfs-1 (the caller's KeyFrame* table). */
typedef struct orbd_database_view {
  int32_t n_kfs, n_words;
  const int32_t* inv_start;    /* n_words + 1: CSR over words */
  const int32_t* inv_kf;       /* mvInvertedFile[word] (I/KeyFrameDatabase.h:82): keyframes in insertion order */
  const int32_t* bow_start;    /* n_kfs + 1 */
  const int32_t* bow_word;     /* pKFi->mBowVec, ascending word ids */
  const double*  bow_value;
  const int32_t* covis_start;  /* n_kfs + 1 */
  const int32_t* covis_kf;     /* pKFi->GetBestCovisibilityKeyFrames(10), best first (:682) */
  const int32_t* map_id;       /* n_kfs: pKFi->GetMap() as an id */
  const uint8_t* bad;          /* n_kfs: pKFi->isBad() */
  const uint8_t* map_bad;      /* n_kfs: pKFi->GetMap()->IsBad() */
} orbd_database_view;
typedef struct orbd_database orbd_database;
int orbd_database_create(int device, const orbd_database_view* view, orbd_database** out);   /* uploads the view */
int orbd_database_destroy(orbd_database* d);
/* void KeyFrameDatabase::DetectNBestCandidates(KeyFrame* pKF, vector<KeyFrame*>& vpLoopCand, vector<KeyFrame*>& vpMergeCand,
 *                                              int nNumCandidates), S/KeyFrameDatabase.cc:594-761, for the query keyframe's
 * BowVector (q_word ascending / q_value), its connected keyframes (connected[n_kfs] = spConnectedKF.count, :603,618) and its
 * map.  On the device: the inverted-file walk with the common-word counts (:605-633), the 0.8 * max filter (:638-646), the
 * L1 scores (:652-663) and the covisibility accumulation (:673-701); the ranking (stable sort by accumulated score, :705)
 * and the selection (:713-735) run on the host over the few scored keyframes.  place_score[n_kfs] is
 * pKFi->mPlaceRecognitionScore, in/out: keyframes that share a word without reaching the word threshold keep the score of
 * an earlier query, and the accumulation reads it (the reference does).  Pinned: a bad keyframe is skipped in the selection
 * (the reference's `continue` at :718-719 does not advance its iterator and never terminates).
 * loop_cand / merge_cand: up to n_candidates keyframe indices each. */
int orbd_detect_n_best_candidates(orbd_database* d, const int32_t* q_word, const double* q_value, int nq, const uint8_t* connected,
                                  int32_t query_map_id, int n_candidates, float* place_score, int32_t* loop_cand, int32_t* n_loop,
                                  int32_t* merge_cand, int32_t* n_merge);
/* vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame* F, Map* pMap), S/KeyFrameDatabase.cc:764-876, for the query
 * BowVector of F: the first call of Tracking::Relocalization.  The device phase is the one of orbd_detect_n_best_candidates (walk,
 * minCommonWords = int(max * 0.8f) with the strict >, float L1 scores, covisibility accumulation); what differs is honoured: no
 * connected-keyframe exclusion; no map or bad filter before the very end, so keyframes of other maps are scored and take part in
 * bestAccScore; the selection runs in first-encounter order without a sort and keeps acc > 0.75f * bestAccScore, then filters
 * GetMap() != pMap and de-duplicates; isBad() is not looked at (Relocalization does that itself).  reloc_score[n_kfs] is mRelocScore,
 * in / out like place_score: a neighbour that shares a word without reaching the word threshold contributes what an earlier query
 * left.  cand: n_kfs entries (caller's), *n_cand of them written. */
int orbd_detect_relocalization_candidates(orbd_database* d, const int32_t* q_word, const double* q_value, int nq,
                                          int32_t query_map_id, float* reloc_score, int32_t* cand, int32_t* n_cand);

/* ---------------------------------------------------------------- KeyFrame wire blocks */

/* What a client sends per keyframe feature in orb_slam3_ros/KF (R/msg/KF.msg:29-31): CvKeyPoint {f32 x, f32 y, u8 size, f32 angle,
 * u8 response, i8 octave} (R/msg/CvKeyPoint.msg:1-9, 15 bytes packed) and Descriptor {u8[32]}, as one block [N x 15 | N x 32]
 * with the conversions of Converter::toCvKeyPointMsg / fromCvKeyPointMsg (S/Converter.cc:217-245).  The blocks are what agents
 * exchange (RCCL all-gather on device memory, see multi_orbslam3_amd/harness.py) so that a server GPU can run the KeyFrame
 * matchers on other agents' keyframes. */
int orbk_wire_bytes(int n);                                              /* 47 * n */
int orbk_pack_frame(orbm_frame* f, uint8_t* wire, int wire_on_device);
int orbk_frame_from_wire(orbm_frame* f, const orbm_frame_view* view, const uint8_t* wire, int n, int wire_on_device);
/* host copies of a device-resident frame's features */
int orbm_frame_download(orbm_frame* f, orbx_keypoint* kps, uint8_t* desc);

/* ---------------------------------------------------------------- local bundle adjustment */

/* A GeometricCamera as the optimiser's edges use it (I/CameraModels/GeometricCamera.h:77-92): GetType() and the parameter vector
 * mvParameters = {fx, fy, cx, cy} (Pinhole) / {fx, fy, cx, cy, k1, k2, k3, k4} (KannalaBrandt8), float32 as the reference keeps them. */
#define ORBG_CAM_PINHOLE 0           /* GeometricCamera::CAM_PINHOLE */
#define ORBG_CAM_KANNALA_BRANDT8 1   /* GeometricCamera::CAM_FISHEYE */
typedef struct orbg_camera {
  int32_t model;
  float fx, fy, cx, cy;
  float k[4];                        /* k1..k4 of KannalaBrandt8 (mvParameters[4..7]); ignored for a pinhole */
} orbg_camera;
/* The cameras of a KeyFrame / Frame whose edges go through GeometricCamera::project / projectJac: mpCamera, and -- for the
 * two-fisheye rig (NLeft != -1) -- mpCamera2 with mTrl, the right camera's pose in the left camera's frame
 * (I/KeyFrame.h:635-642, I/Frame.h:277-297).  One rig per problem: every keyframe of a map holds the same camera objects. */
typedef struct orbg_camera_rig {
  orbg_camera left;                  /* mpCamera: EdgeSE3ProjectXYZ / EdgeSE3ProjectXYZOnlyPose (I/OptimizableTypes.h:31-57,89-115) */
  int32_t has_right;                 /* mpCamera2 != NULL */
  orbg_camera right;                 /* mpCamera2: EdgeSE3ProjectXYZToBody / EdgeSE3ProjectXYZOnlyPoseToBody (:59-87,117-144) */
  float Trl[12];                     /* mTrl, 3 x 4 row-major float32 (Converter::toSE3Quat reads exactly these, S/Converter.cc:34-44) */
} orbg_camera_rig;
/* ---- two-camera rig frames in the matcher (Frame::Nleft != -1, S/Frame.cc:1017-1091): the two cameras' features are two orbm_frame
 * objects -- `left` holds mvKeys[0, Nleft) with mGrid, `right` holds mvKeysRight with mGridRight (S/Frame.cc:360-391), neither has
 * uRight; entry Nleft + i of Frame::mvpMapPoints / mDescriptors is feature i of `right`.
 *
 * orbm_is_in_frustum_rig: Frame::isInFrustum for such a frame (S/Frame.cc:545-554): isInFrustumChecks (:1154-1231) through
 * rig->left for the left camera and through rig->right after mTrl for the right one; Tlr = Frame::mTlr (3 x 4 row-major, its
 * translation enters the right camera's centre, :1164).  Outputs, m entries each, per camera: mbTrackInView(R), mTrackProjX(R) /
 * mTrackProjY(R), mTrackDepth(R), mnTrackScaleLevel(R) (-1 where the checks fail, :546-547), mTrackViewCos(R); fields of a point that
 * fails a camera's checks are 0 (the reference leaves the previous frame's values there).
 * rig->has_right == 0: ONE camera behind a model -- a monocular fisheye Frame (Nleft == -1, mpCamera a KannalaBrandt8): the Nleft == -1
 * branch of Frame::isInFrustum (S/Frame.cc:466-543) makes the same checks through mpCamera->project; the left outputs are written, the
 * right ones (and Tlr) may be NULL.  (orbm_is_in_frustum is that branch for a pinhole.) */
int orbm_is_in_frustum_rig(orbm_frame* left, const float* Tcw /*16*/, const orbg_camera_rig* rig, const float* Tlr /*12*/,
                           const orbm_worldpoints_view* pts, float viewing_cos_limit, uint8_t* in_view, float* proj_x, float* proj_y,
                           float* track_depth, int32_t* scale_level, float* view_cos, uint8_t* in_view_r, float* proj_x_r, float* proj_y_r,
                           float* track_depth_r, int32_t* scale_level_r, float* view_cos_r);
/* ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints) on such a frame (S/ORBmatcher.cc:44-214
 * with the right camera's block :145-211).  mps: the left camera's track fields and the per-point fields (bad, track_depth, desc,
 * n_obs; proj_xr is not read); mps_r: track_in_view = mbTrackInViewR, proj_x / proj_y = mTrackProjXR / mTrackProjYR, scale_level =
 * mnTrackScaleLevelR, view_cos = mTrackViewCosR (its other fields are not read).  left_to_right[Nleft] = Frame::mvLeftToRightMatch,
 * right_to_left[Nright] = mvRightToLeftMatch (-1 = none): a match on one side is also written to the stereo partner on the other
 * (:132-136,199-203).  assigned_mp / assigned_obs have Nleft + Nright entries (in/out, as orbm_search_by_projection_mps). */
int orbm_search_by_projection_mps_rig(orbm_frame* left, orbm_frame* right, const orbm_mappoints_view* mps, const orbm_mappoints_view* mps_r,
                                      const int32_t* left_to_right, const int32_t* right_to_left, float th, int far_points,
                                      float th_far_points, float nnratio, int32_t* assigned_mp, int32_t* assigned_obs, int* nmatches);

/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) with CurrentFrame.Nleft != -1
 * (S/ORBmatcher.cc:1970-2186): per map point of the last frame the left camera's search through rig->left (mpCamera->project), then
 * (:2092-2160) the point in the right camera's frame (rig->Trl) projected -- through mpCamera again, as the reference does -- and
 * searched in the right camera's grid; a point whose left window holds no feature is not searched on the right either (:2033).
 * `last`: the last frame's Nleft + Nright entries (octave / angle of mvKeys resp. mvKeysRight).  assigned_*: Nleft + Nright entries.
 * rig->has_right == 0 and right == NULL: a monocular Frame whose camera is a model (Nleft == -1, mpCamera a KannalaBrandt8): the left
 * camera's search alone, through mpCamera->project (orbm_search_by_projection_frame is the same for a pinhole). */
int orbm_search_by_projection_frame_rig(orbm_frame* left, orbm_frame* right, const float* Tcw_cur, const orbg_camera_rig* rig,
                                        const orbm_lastframe_view* last, float th, int mono, int check_orientation, int32_t* assigned_mp,
                                        int32_t* assigned_obs, int* nmatches);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame &F, vector<MapPoint*>&) with F.Nleft != -1 (S/ORBmatcher.cc:269-471, the branch
 * :342-430): `f` holds ALL of the Frame's features -- mvKeys then mvKeysRight, descriptor rows as in mDescriptors, indices as in
 * F.mFeatVec -- and n_left = F.Nleft.  Per keyframe feature the best two of a vocabulary bucket are kept per camera; the left
 * camera's best passes TH_LOW and the ratio test, the right camera's best only TH_LOW, and only when the left one passed TH_LOW
 * (:373-428).  kf_angle[i]: the keyframe keypoint's angle (mvKeysUn / mvKeys / mvKeysRight as :379-382 picks).  Other arguments and
 * `matches` as orbm_search_by_bow. */
int orbm_search_by_bow_rig(orbm_frame* f, int n_left, const orbm_featvec_view* fv_frame, const uint8_t* kf_desc, int nkf,
                           const uint8_t* kf_mp_valid, const float* kf_angle, const orbm_featvec_view* fv_kf, float nnratio,
                           int check_orientation, int32_t* matches, int* nmatches);

/* Frame::ComputeStereoFishEyeMatches (S/Frame.cc:1093-1150): the left-right matcher of the two-fisheye Frame constructor.  The
 * features of the two cameras' lapping areas -- [mono_left, n_left) and [mono_right, n_right): ORBextractor::operator() puts them
 * behind the monocular ones (S/ORBextractor.cc:1136-1160, orbx_extract's lapping arguments) -- are matched brute force (the two
 * nearest right descriptors per left one: cv::BFMatcher::knnMatch, k = 2, NORM_HAMMING), kept under Lowe's ratio 0.7, and
 * triangulated by KannalaBrandt8::TriangulateMatches (parallax, positive depth in both cameras, reprojection error against
 * 5.991 sigma^2 in both; S/CameraModels/KannalaBrandt8.cpp:335-420).  Both cameras must be ORBG_CAM_KANNALA_BRANDT8.
 * Outputs: left_to_right[n_left] = mvLeftToRightMatch, right_to_left[n_right] = mvRightToLeftMatch (-1 = none; of several left features
 * that pick one right feature the last one stays there, as in the reference's loop), depth[n_left] = mvDepth (-1), points3d[3 n_left] =
 * mvStereo3Dpoints (written where a match was accepted), *n_matches = nMatches.
 * The homogeneous solve of Triangulate is cv::SVD::compute in the reference (float32, one-sided Jacobi); here: the smallest
 * eigenvector of A^T A in float64 -- depths and points agree with an OpenCV build to float32 rounding, not to the bit. */
typedef struct orbx_fisheye_stereo_view {
  int32_t n_left, n_right, mono_left, mono_right;    /* Nleft, Nright, monoLeft, monoRight */
  const orbx_keypoint* kps_left;                     /* mvKeys */
  const orbx_keypoint* kps_right;                    /* mvKeysRight */
  const uint8_t* desc_left;                          /* mDescriptors, n_left x 32 */
  const uint8_t* desc_right;                         /* mDescriptorsRight, n_right x 32 */
  const float* level_sigma2;                         /* mvLevelSigma2 */
  int32_t n_levels;
  orbg_camera left, right;                           /* mpCamera, mpCamera2 */
  float Tlr[12];                                     /* mTlr, 3 x 4 row-major: mRlr, mtlr (S/Frame.cc:1073-1074) */
} orbx_fisheye_stereo_view;
int orbx_fisheye_stereo_matches(int device, const orbx_fisheye_stereo_view* view, int32_t* left_to_right, int32_t* right_to_left, float* depth,
                                float* points3d, int* n_matches);

/* `ur` of an observation made by the RIGHT camera of the rig (get<1>(indexes) != -1, S/Optimizer.cc:2086-2120; i >= Nleft,
 * :1121-1150): u, v are then mvKeysRight[rightIndex].pt and the edge is the *ToBody kind.  In a problem whose rig has a right camera
 * any ur <= -1.5 reads as this (mvuRight is -1 throughout on such frames); in every other problem a negative ur is a monocular
 * observation, as it always was. */
#define LBA_UR_RIGHT_CAMERA (-2.0f)

/* One reprojection edge (S/Optimizer.cc:2021-2120): stereo if ur >= 0, the right camera's if ur == LBA_UR_RIGHT_CAMERA, mono
 * otherwise (the reference's mvuRight is -1 there). */
typedef struct lba_edge {
  int32_t pose;        /* index into poses[] */
  int32_t point;       /* index into points[] */
  float   u, v, ur;    /* kpUn.pt.x, kpUn.pt.y, mvuRight (<0 => monocular edge) */
  float   inv_sigma2;  /* mvInvLevelSigma2[kpUn.octave] */
} lba_edge;

/* Everything S/Optimizer.cc:1934-2124 reads.  Poses MUST be ordered
 * free/fixed arbitrarily but listed in ascending vertex id (Optimizer::GetID, I/Optimizer.h:104-112),
 * points likewise; edges in creation order (per point, its observations). */
typedef struct lba_problem {
  int32_t n_poses, n_points, n_edges;
  const float*   poses;        /* n_poses x 16, Tcw row-major float32 (KeyFrame::GetPose) */
  const uint8_t* pose_fixed;   /* n_poses */
  const float*   points;       /* n_points x 3 */
  const lba_edge* edges;
  float fx, fy, cx, cy, bf;
  double lambda_init;          /* 0 = auto (tau*max diag); 100 for inertial maps, S/Optimizer.cc:1924-1925 */
  int32_t its_round1, its_round2;  /* 5 and 10, S/Optimizer.cc:2132,2203 */
  int32_t device;
  /* NULL: mpCamera is the pinhole {fx, fy, cx, cy} above and there is no second camera (every BASELINE configuration).  Otherwise
   * the monocular edges project through rig->left and the right camera's edges through rig->right after mTrl; stereo edges
   * (g2o::EdgeStereoSE3ProjectXYZ carries its own fx, fy, cx, cy, bf, S/Optimizer.cc:2071-2075) keep using the five scalars. */
  const orbg_camera_rig* rig;
} lba_problem;

typedef struct lba_result {
  float*   poses;          /* n_poses x 16 (Converter::toCvMat(SE3Quat)), caller-allocated */
  float*   points;         /* n_points x 3 */
  double*  edge_chi2;      /* n_edges, e->chi2() at S/Optimizer.cc:2219,2249 */
  uint8_t* edge_depth_pos; /* n_edges, e->isDepthPositive() */
  uint8_t* edge_outlier;   /* n_edges, the vToErase predicate (S/Optimizer.cc:2219-2253) */
  int32_t  status;         /* LBA_* */
  int32_t  iters_round1, iters_round2;  /* LM iterations actually run */
  int32_t  n_outliers;
  double   chi2_initial, chi2_final;    /* activeRobustChi2 at first linearisation / after last accepted step */
  double*  trace;          /* optional (may be NULL): per LM iteration {lambda, chi2, trials}; cap trace_cap rows */
  int32_t  trace_cap, trace_len;
} lba_result;

/* void Optimizer::LocalBundleAdjustment(KeyFrame*, bool* pbStopFlag, Map*, int&, int) numerical core,
 * S/Optimizer.cc:1917-2267 + 2321-2396 (state write-back into result).  stop_flag may be NULL;
 * it is polled between LM iterations/trials exactly where g2o polls forceStopFlag
 * (G/core/sparse_optimizer.cpp:376, G/core/optimization_algorithm_levenberg.cpp:149).  A positive value is the
 * reference's `true` (raised by Tracking, S/LocalMapping.cc:381-386).  A NEGATIVE value -k is a deterministic form for
 * tests: the flag reads as raised once k Levenberg-Marquardt trials have been evaluated, whatever the timing (INT32_MIN:
 * k = 0, i.e. raised right after the check that precedes optimize(), S/Optimizer.cc:2127-2129). */
int lba_solve(const lba_problem* p, const volatile int32_t* stop_flag, lba_result* r);
/* The same solve polling the reference's OWN flag: `bool* pbStopFlag` (I/Optimizer.h:42) points at LocalMapping::mbAbortBA,
 * a one-byte bool that LocalMapping::InterruptBA sets from the Tracking thread while the solve runs (S/LocalMapping.cc:381-386,
 * :118 hands &mbAbortBA to the optimiser).  stop_bool is that address, passed through unchanged (any non-zero byte = raised);
 * it is read -- never written -- at exactly the poll points above, so the reference's InterruptBA() needs no change. */
int lba_solve_b(const lba_problem* p, const volatile uint8_t* stop_bool, lba_result* r);

/* Persistent LBA workspace variant: avoids per-call device allocation. */
typedef struct lba_handle lba_handle;
int lba_create(int device, int cap_poses, int cap_points, int cap_edges, lba_handle** out);
int lba_destroy(lba_handle* h);
int lba_solve_h(lba_handle* h, const lba_problem* p, const volatile int32_t* stop_flag, lba_result* r);
int lba_solve_hb(lba_handle* h, const lba_problem* p, const volatile uint8_t* stop_bool, lba_result* r);   /* bool flag, see lba_solve_b */
/* The same solve on a worker thread owned by the handle, as the reference runs it on its LocalMapping thread next to
 * Tracking (S/ClientSystem.cc:105-106).  lba_solve_async returns immediately; lba_wait blocks until the solve is done
* and returns its status (ORBG_OK when nothing was submitted).  problem / stop_flag / result must stay valid until then;
 * one solve in flight per handle (a second lba_solve_async before lba_wait returns ORBG_BAD_ARG). */
int lba_solve_async(lba_handle* h, const lba_problem* problem, const volatile int32_t* stop_flag, lba_result* result);
int lba_solve_async_b(lba_handle* h, const lba_problem* problem, const volatile uint8_t* stop_bool, lba_result* result);
int lba_wait(lba_handle* h, double* solve_ms /* wall time of that solve on the worker, may be NULL */);
/* Measurement hooks (bench.py roofline): with profiling on, one launch per solve of the reduced-camera-system LDL^T
 * (G/solvers/linear_solver_eigen.h:94-124 behind G/core/block_solver.hpp:447) is bracketed by a HIP event pair on the
 * handle's stream; the stats are the summed bracket time, the number of brackets, the unknowns of the last system
 * (6 x free poses) and whether the FP64 matrix-core kernel solved it.  lba_event_overhead: cost of an empty pair. */
int lba_set_profiling(lba_handle* h, int on, int reset);
int lba_get_solver_stats(lba_handle* h, double* sum_ms, int64_t* n_brackets, int32_t* n_unknowns, int32_t* matrix_core);
int lba_event_overhead(lba_handle* h, int reps, float* ms);
/* Health of the handle's solver: how many launches of the eight-workgroup LDL^T (windows of 21 .. 50 free poses) gave up waiting
 * for a participant the dispatcher did not place within 2 s.  Such a launch is NOT taken for a non-positive-definite system (which
 * g2o answers with a rejected LM step, G/core/optimization_algorithm_levenberg.cpp:118-127): the window is solved again on the
 * one-workgroup kernels, which the handle then keeps using, and the event is counted here.  0 on a healthy box. */
int lba_get_watchdog_count(lba_handle* h, int64_t* n_timeouts);

/* ---------------------------------------------------------------- full bundle adjustment (Optimizer::BundleAdjustment) */

/* What the edges of ONE keyframe read (S/Optimizer.cc:202,237-241: e->pCamera = pKF->mpCamera; e->fx .. e->bf = pKF->fx .. pKF->mbf).
 * After a map merge the keyframes of a map belong to different agents: every pose of a ba_problem names its own camera.
 * Monocular edges (EdgeSE3ProjectXYZ) project through `model` (ORBG_CAM_PINHOLE or ORBG_CAM_KANNALA_BRANDT8); stereo edges
 * (g2o::EdgeStereoSE3ProjectXYZ) use the five scalars, as in lba_problem. */
typedef struct ba_camera {
  float fx, fy, cx, cy, bf;
  orbg_camera model;
} ba_camera;

/* Everything S/Optimizer.cc:73-305 reads.  Vertex order follows the rule of lba_problem: poses in ascending vertex id, points
 * likewise; edges in creation order -- per point, its observations in the order the reference walks them, so the edges of a
 * point are consecutive and edge.point never decreases along the list (anything else: ORBG_BAD_ARG).
 * Limits: at most BA_MAX_FREE_POSES free poses (the reduced camera system goes to the widest LDL^T of the library, 8192
 * unknowns); poses, points and edges are counted and addressed in 32 bits everywhere on this path (no 16-bit packed counts).
 * n_edges <= BA_MAX_EDGES: an edge index is an int32 and an edge keeps 27 doubles of Jacobian products on the device (216 B: 17 GB
 * at the cap, addressed in 64 bits); the list of shared-landmark items has 32-bit offsets too, a problem with more than 2^31 - 1 of
 * them is refused once they have been counted (on the device).  A problem beyond the other limits returns ORBG_CAP_EXCEEDED before
 * anything is launched.  An edge with ur == LBA_UR_RIGHT_CAMERA (the mpCamera2 edges of a two-camera keyframe,
 * EdgeSE3ProjectXYZToBody) returns ORBG_BAD_ARG, also before any launch: those edges are not part of this entry point. */
#define BA_MAX_FREE_POSES 1365
#define BA_MAX_EDGES 79000000
typedef struct ba_problem {
  int32_t n_poses, n_points, n_edges, n_cameras;
  const float*   poses;        /* n_poses x 16, Tcw row-major float32 (KeyFrame::GetPose) */
  const uint8_t* pose_fixed;   /* n_poses: pKF->mnId == pMap->GetInitKFid(), or the bUseUniqueId rule of S/Optimizer.cc:110-117 */
  const int32_t* pose_camera;  /* n_poses: index into cameras[] */
  const float*   points;       /* n_points x 3 */
  const lba_edge* edges;
  const ba_camera* cameras;    /* n_cameras */
  int32_t iterations;          /* nIterations: ONE optimize(nIterations), no outlier round */
  int32_t robust;              /* bRobust: Huber kernels on every edge (sqrt 5.99 / sqrt 7.815, S/Optimizer.cc:131-132: not the local BA's 5.991), or none */
  int32_t device;
} ba_problem;

typedef struct ba_result {
  float*   poses;           /* n_poses x 16, caller-allocated */
  float*   points;          /* n_points x 3; a point with point_included == 0 comes back as it went in */
  double*  edge_chi2;       /* n_edges (may be NULL): e->chi2() as S/Optimizer.cc:373,400 reads it */
  uint8_t* edge_depth_pos;  /* n_edges (may be NULL): e->isDepthPositive() */
  uint8_t* point_included;  /* n_points (may be NULL): 0 = the vertex without an edge that S/Optimizer.cc:289-293 removes */
  int32_t  status;          /* LBA_APPLIED, or LBA_ABORTED_BEFORE_OPT when the flag was up before the call did anything */
  int32_t  iters;           /* LM iterations actually run */
  double   chi2_initial, chi2_final;   /* as in lba_result (robust == 0: the plain chi2) */
  double*  trace;           /* optional, as in lba_result: per LM iteration {lambda, chi2, trials} */
  int32_t  trace_cap, trace_len;
} ba_result;

/* void Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, bUseUniqueId, nLoopKF, bRobust), numerical core
 * (S/Optimizer.cc:73-305) and the state read back at :307-446, reached through GlobalBundleAdjustemnt from
 * Tracking::CreateInitialMapMonocular (S/Tracking.cc:2316) and LoopClosing::RunGlobalBundleAdjustment (S/LoopClosing.cc:2627).
 * stop_flag has the poll points and the deterministic negative test form that lba_solve documents; ba_solve_b takes the
 * reference's own flag (&mbStopGBA) unchanged.  Two calls on the same input return the same bits. */
int ba_solve(const ba_problem* p, const volatile int32_t* stop_flag, ba_result* r);
int ba_solve_b(const ba_problem* p, const volatile uint8_t* stop_bool, ba_result* r);
/* Persistent workspace.  The three capacities are accepted for symmetry with lba_create and are not used: the buffers grow on first
 * use and are kept. */
typedef struct ba_handle ba_handle;
int ba_create(int device, int cap_poses, int cap_points, int cap_edges, ba_handle** out);
int ba_destroy(ba_handle* h);
int ba_solve_h(ba_handle* h, const ba_problem* p, const volatile int32_t* stop_flag, ba_result* r);
int ba_solve_hb(ba_handle* h, const ba_problem* p, const volatile uint8_t* stop_bool, ba_result* r);
/* MEASUREMENT ONLY, not part of the stable interface (tools/full_ba_time.py; may change or go with the kernels): device time of the handle's LAST solve by phase, from HIP events around every
 * launch group when `on` was set before that solve -- ms[5] = structure build, linearisation, Schur complement, LDL^T, update and
 * evaluation.  Off by default (the events cost a few microseconds per launch group). */
int ba_set_profiling(ba_handle* h, int on);
int ba_get_phase_ms(ba_handle* h, double* ms /* 5 */);

/* ---------------------------------------------------------------- welding BA (Optimizer::LocalBundleAdjustment of a map merge) */

/* void Optimizer::LocalBundleAdjustment(KeyFrame* pMainKF, vector<KeyFrame*> vpAdjustKF, vector<KeyFrame*> vpFixedKF, bool*),
 * numerical core (S/Optimizer.cc:6305-6983, called by LoopClosing::MergeLocal at S/LoopClosing.cc:1814): a ba_problem solved in two
 * rounds with an outlier level between them.
 *   round 1   optimize(ba.iterations) with Huber kernels on every edge (sqrt 5.99 / sqrt 7.815, S/Optimizer.cc:6459-6460): exactly
 *             ba_solve with robust = 1
 *   levels    only if the flag is down after round 1 (S/Optimizer.cc:6610-6647): an edge whose chi2 -- of round 1's LAST error
 *             evaluation, which may be a rejected trial's -- exceeds chi2_mono (ur < 0) / chi2_stereo, or whose depth in its camera
 *             is not positive at round 1's estimate, goes to level 1; every edge loses its kernel
 *   round 2   optimize(iterations_second) over the level-0 edges alone, no kernels, from round 1's float64 estimate; structure,
 *             lambda's first value and the rejection factor start over.  A point or free keyframe without a level-0 edge keeps
 *             round 1's estimate.  Nothing runs when no edge is left at level 0 or iterations_second <= 0.
 * The levels, the compaction of the edge list and round 2 stay on the device. */
typedef struct ba_weld_problem {
  uint32_t   struct_size;        /* sizeof(ba_weld_problem) */
  ba_problem ba;                 /* ba.iterations: round 1's count (5).  ba.robust is NOT READ: round 1 is always robust, round 2 never */
  int32_t    iterations_second;  /* round 2's count (10) */
  double     chi2_mono, chi2_stereo;   /* 5.991 and 7.815: both the level test and the caller's final check; finite and > 0 */
} ba_weld_problem;

typedef struct ba_weld_result {
  uint32_t  struct_size;         /* sizeof(ba_weld_result) */
  /* Round 1's iters / chi2_initial / chi2_final / trace; poses and points: the final estimate; point_included: round 1's meaning
   * (the point has an edge at all).  edge_chi2 / edge_depth_pos are what the reference's final check reads (S/Optimizer.cc:6665-6705):
   * chi2 of round 2's last evaluation for a level-0 edge, round 1's for a level-1 edge (it was not active in round 2); the depth
   * test of every edge with the final estimate.  Both arrays may be NULL. */
  ba_result ba;
  uint8_t*  edge_level;          /* n_edges, required: 0 or 1; all 0 when no level was assigned (rounds_run == 0, or the flag up after round 1) */
  int32_t   n_level1;
  int32_t   rounds_run;          /* 0: no iteration ran at all; 1: round 1 alone; 2: round 2 was entered */
  int32_t   iters_second;
  double    chi2_initial_second, chi2_final_second;
  double*   trace_second;        /* optional: round 2's rows, as ba_result.trace */
  int32_t   trace_second_cap, trace_second_len;
} ba_weld_result;

/* stop_flag / stop_bool as in the ba_solve family; the count of evaluated trials behind the -k form runs on through both rounds.
 * Up before the call: status LBA_ABORTED_BEFORE_OPT, the input comes back through the float32 conversions, rounds_run = 0 (the
 * reference returns without writing anything back).  Up after round 1: no levels, no round 2.  Refused before a device is selected
 * (ORBG_BAD_ARG): a short struct_size, what ba_solve refuses, thresholds that are not finite and positive, edge_level == NULL with
 * n_edges > 0.  Called with iterations_second = 0 and no flag, `ba` comes back with the bits of ba_solve_h(robust = 1) on the same
 * handle.  Two calls on the same input return the same bits. */
int ba_weld_solve(const ba_weld_problem* p, const volatile int32_t* stop_flag, ba_weld_result* r);
int ba_weld_solve_b(const ba_weld_problem* p, const volatile uint8_t* stop_bool, ba_weld_result* r);
int ba_weld_solve_h(ba_handle* h, const ba_weld_problem* p, const volatile int32_t* stop_flag, ba_weld_result* r);
int ba_weld_solve_hb(ba_handle* h, const ba_weld_problem* p, const volatile uint8_t* stop_bool, ba_weld_result* r);

/* ---------------------------------------------------------------- essential graph (Optimizer::OptimizeEssentialGraph) */

/* The Sim3 pose graph that LoopClosing::CorrectLoop optimises between the fuse and the full BA (S/LoopClosing.cc:1272, body
 * S/Optimizer.cc:2413-2747).  The forms at S/Optimizer.cc:3196 (LoopClosing::MergeLocal, S/LoopClosing.cc:1922) and :3596 set up the
 * same numerical problem -- g2o::VertexSim3Expmap vertices, some fixed, each with its _fix_scale; g2o::EdgeSim3 edges with identity
 * information and no robust kernel; setUserLambdaInit(1e-16); one optimize(20) -- so this one flat problem serves all three
 * ("OptimizeEssentialGraph", says how each maps onto it).
 * A Sim3 is rotation().coeffs() (x, y, z, w), translation(), scale(), all doubles, taken as it is (no renormalisation).
 * FIXING THE GAUGE IS THE CALLER'S JOB, as in the reference: every connected component of the graph needs at least one fixed vertex
 * (the reference fixes the keyframe with mnId == pMap->GetInitKFid()).  Without one the normal equations are singular up to
 * lambda_init and the result is whatever the factorisation makes of that; nothing is checked here. */
#define EG_MAX_FREE_KEYFRAMES 1170       /* 7 x 1170 = 8190 unknowns: the widest LDL^T of the library takes 8192 */
typedef struct eg_vertex {
  double  q[4], t[3], s;   /* the estimate: CorrectedSim3 of the keyframe, or its pose with scale 1 (S/Optimizer.cc:2456-2470) */
  int32_t fixed;           /* VSim3->setFixed(true) */
  int32_t fix_scale;       /* VSim3->_fix_scale: oplusImpl zeroes update[6] */
} eg_vertex;
typedef struct eg_edge {
  int32_t vi, vj;          /* setVertex(0, .), setVertex(1, .): error = log(measurement * Siw * Sjw^-1) */
  double  q[4], t[3], s;   /* setMeasurement(Sji) */
} eg_edge;
typedef struct eg_point {
  float   pos[3];          /* pMP->GetWorldPos() */
  int32_t ref;             /* vertex of mnCorrectedReference / GetReferenceKeyFrame(); < 0: the point keeps its bits (the reference maps
                              a point without a vertex through two default-constructed identities, S/Optimizer.cc:2435-2436) */
} eg_point;
typedef struct eg_problem {
  uint32_t struct_size;    /* sizeof(eg_problem) */
  int32_t  n_vertices;
  const eg_vertex* vertices;
  int32_t  n_edges;
  const eg_edge* edges;    /* in creation order: sums over edges run in this order */
  int32_t  iterations;     /* optimize(20) */
  double   lambda_init;    /* setUserLambdaInit(1e-16); <= 0: g2o's own 1e-5 x the largest diagonal entry */
  int32_t  n_points;       /* may be 0 */
  const eg_point* points;
  int32_t  device;
} eg_problem;
typedef struct eg_result {
  uint32_t struct_size;    /* sizeof(eg_result) */
  double*  estimates;      /* n_vertices x 8 (q, t, s), caller-allocated: VSim3->estimate() after optimize() */
  float*   points;         /* n_points x 3: correctedSwr.map(Srw.map(P)), Srw the vertex's estimate on entry (S/Optimizer.cc:2732-2740) */
  double   err0, errEnd;   /* activeRobustChi2() before and after (doubles here; the reference keeps floats for a message) */
  int32_t  iters;          /* LM iterations actually run */
  double*  trace;          /* optional: per LM iteration {trials, last trial accepted, chi2, lambda} */
  int32_t  trace_cap, trace_len;
  double*  edge_error0;    /* optional, for checkers: n_edges x 7, EdgeSim3::computeError at the estimate on entry */
} eg_result;

/* The numerical core of Optimizer::OptimizeEssentialGraph on the calling thread's work area and stream: numeric Jacobians as g2o
 * takes them for EdgeSim3 (central differences, delta = 1e-9, through oplusImpl), dense normal equations over the free vertices in
 * ascending order, g2o's Levenberg-Marquardt without a stop flag (the reference passes none), then the map points.  Two calls on the
 * same input return the same bits.  ORBG_BAD_ARG (indices out of range, an edge from a vertex to itself, a non-finite value, a scale
 * <= 0, a short struct_size) and ORBG_CAP_EXCEEDED (more than EG_MAX_FREE_KEYFRAMES free vertices) are returned before a device is
 * looked for; a problem without a free vertex, without an edge or with iterations <= 0 launches nothing (the estimates come back as
 * they went in, the points go through them, err0 == errEnd is evaluated on the host); otherwise ORBG_NO_DEVICE where there is none. */
int eg_solve(const eg_problem* p, eg_result* r);
/* MEASUREMENT ONLY, not part of the stable interface (tools/essential_graph_time.py): while `on` is set (process-wide), every
 * eg_solve brackets its launch groups with HIP events; eg_get_phase_ms returns the device time of the calling thread's last solve,
 * ms[4] = linearisation, assembly of the blocks and of the dense system, LDL^T, update and evaluation. */
int eg_set_profiling(int on);
int eg_get_phase_ms(double* ms /* 4 */);

/* ---------------------------------------------------------------- pose-only optimisation */

/* Everything Optimizer::PoseOptimization(Frame*) reads (S/Optimizer.cc:964-1278): one entry per
 * feature that holds a map point. */
typedef struct pose_opt_problem {
  int32_t n;               /* nInitialCorrespondences */
  const float* Xw;         /* n x 3, pMP->GetWorldPos() */
  const float* u;          /* mvKeysUn[i].pt.x */
  const float* v;          /* mvKeysUn[i].pt.y */
  const float* ur;         /* mvuRight[i]; < 0 => monocular edge */
  const float* inv_sigma2; /* mvInvLevelSigma2[octave] */
  float fx, fy, cx, cy, bf;
  float Tcw[16];           /* pFrame->mTcw (row-major), the estimate every round restarts from */
  int32_t device;
  /* NULL: Frame::mpCamera is the pinhole above, mpCamera2 == NULL.  Otherwise as in lba_problem: entries with
   * ur == LBA_UR_RIGHT_CAMERA are features i >= Nleft (u, v = mvKeysRight[i - Nleft].pt, S/Optimizer.cc:1121-1150), the other
   * monocular entries project through rig->left (u, v = mvKeys[i].pt, :1091-1119). */
  const orbg_camera_rig* rig;
} pose_opt_problem;

typedef struct pose_opt_result {
  float    Tcw[16];        /* optimised pose (pFrame->SetPose) */
  uint8_t* outlier;        /* n, pFrame->mvbOutlier for the correspondences (caller-allocated) */
  int32_t  n_inliers;      /* return value: nInitialCorrespondences - nBad (0 if n < 3) */
  int32_t  n_bad;
  int32_t  iters[4];       /* LM iterations run in each of the 4 rounds */
  double   chi2[4];        /* robustified chi2 at the end of each round (active edges) */
} pose_opt_result;

/* int Optimizer::PoseOptimization(Frame *pFrame), S/Optimizer.cc:964-1278: 4 rounds x 10 LM iterations on one SE3
 * vertex with unary reprojection edges (I/OptimizableTypes.h:31-57, G/types/types_six_dof_expmap.h:208-236), outliers
 * re-classified after every round (chi2 > 5.991 / 7.815), Huber kernels dropped for the last round.  The whole solve
 * runs in ONE kernel launch (LM control flow on the device). */
int pose_optimize(const pose_opt_problem* p, pose_opt_result* r);

/* ---------------------------------------------------------------- pose-inertial optimisation (the per-frame optimiser of an inertial agent)
 *
 * Optimizer::PoseInertialOptimizationLastKeyFrame (S/Optimizer.cc:7603-7996) and ...LastFrame (:7998-8424), what
 * Tracking::TrackLocalMap calls instead of PoseOptimization once the IMU is initialised (S/Tracking.cc:2689-2740). */
enum { POSE_INERTIAL_LAST_KEYFRAME = 0, POSE_INERTIAL_LAST_FRAME = 1 };

/* What VertexPose / VertexVelocity / VertexGyroBias / VertexAccBias read of a Frame or KeyFrame (S/G2oTypes.cc:73-119, 648-691):
 * GetImuRotation(), GetImuPosition(), the velocity, mImuBias (bwx.., bax..). */
typedef struct pose_inertial_state {
  float Rwb[9];            /* row-major */
  float twb[3];
  float vwb[3];
  float bg[3];
  float ba[3];
} pose_inertial_state;

/* What EdgeInertial reads of an IMU::Preintegrated (S/G2oTypes.cc:695-800, S/ImuTypes.cc:404-431). */
typedef struct pose_inertial_preint {
  float dT;
  float dR[9], dV[3], dP[3];
  float JRg[9], JVg[9], JVa[9], JPg[9], JPa[9];
  float bg[3], ba[3];      /* Preintegrated::b, the bias the deltas were integrated with */
} pose_inertial_preint;

/* ConstraintPoseImu as it is stored (I/G2oTypes.h:703-746): H after the constructor's conditioning (orbg_condition_prior). */
typedef struct pose_inertial_prior {
  double Rwb[9], twb[3], vwb[3], bg[3], ba[3];
  double H[225];           /* row-major; rows / columns: rotation, translation, velocity, gyro bias, accelerometer bias */
} pose_inertial_prior;

typedef struct pose_inertial_problem {
  uint32_t struct_size;    /* sizeof(pose_inertial_problem) */
  int32_t form;            /* POSE_INERTIAL_LAST_KEYFRAME / POSE_INERTIAL_LAST_FRAME */
  int32_t rec_init;        /* bRecInit */
  int32_t device;
  int32_t n_left;          /* Frame::Nleft; must be -1 (a two-camera Frame is refused with ORBG_BAD_ARG) */
  int32_t n;               /* nInitialCorrespondences: one entry per feature that holds a map point */
  const float* Xw;         /* n x 3, pMP->GetWorldPos() */
  const float* u;          /* mvKeysUn[i].pt.x */
  const float* v;          /* mvKeysUn[i].pt.y */
  const float* ur;         /* mvuRight[i]; < 0 => EdgeMonoOnlyPose, else EdgeStereoOnlyPose */
  const float* inv_sigma2; /* mvInvLevelSigma2[octave] (Pinhole::uncertainty2 is 1) */
  const uint8_t* close;    /* mvpMapPoints[i]->mTrackDepth < 10.f */
  float fx, fy, cx, cy, bf;
  float Tcb[12];           /* mImuCalib.Tcb, rows 0-2 (row-major 3 x 4) */
  pose_inertial_state frame;   /* pFrame */
  pose_inertial_state other;   /* pFrame->mpLastKeyFrame (fixed) / pFrame->mpPrevFrame (optimised with the frame) */
  pose_inertial_preint preint; /* pFrame->mpImuPreintegrated / mpImuPreintegratedFrame */
  double info9[81];        /* EdgeInertial's information (orbg_imu_information) */
  double infoG[9];         /* EdgeGyroRW's */
  double infoA[9];         /* EdgeAccRW's */
  const pose_inertial_prior* prior;   /* LAST_FRAME: pFp->mpcpi (required); LAST_KEYFRAME: ignored */
} pose_inertial_problem;

typedef struct pose_inertial_result {
  uint32_t struct_size;    /* sizeof(pose_inertial_result) */
  int32_t  n_inliers;      /* return value: nInitialCorrespondences - nBad */
  int32_t  n_bad;
  int32_t  rounds_run;     /* 4, or 1 when the graph has fewer than 10 edges */
  int32_t  solve_failed;   /* a factorisation met a pivot that is not positive: that round's iterations ended without an update */
  uint8_t* outlier;        /* n, pFrame->mvbOutlier for the correspondences (caller-allocated) */
  double   Rwb[9], twb[3], vwb[3], bg[3], ba[3];   /* the frame's estimates (SetImuPoseVelocity, mImuBias) */
  double   chi2[4];        /* robustified chi2 of the active edges at the last linearisation of each round: the errors the edges are classified with */
  double   H[225];         /* what the reference passes to the ConstraintPoseImu constructor (before its conditioning) */
} pose_inertial_result;

/* int Optimizer::PoseInertialOptimizationLastKeyFrame(Frame*, bool) / ...LastFrame(Frame*, bool): 4 rounds x 10 Gauss-Newton
 * iterations on the frame's pose, velocity and biases (LAST_FRAME: and the previous frame's, 30 unknowns) with EdgeMonoOnlyPose /
 * EdgeStereoOnlyPose, EdgeInertial, EdgeGyroRW, EdgeAccRW and (LAST_FRAME) EdgePriorPoseImu; outliers re-classified after every
 * round with the error each edge holds (the one before the round's last update for an active edge), recovery below 30 inliers, the
 * Hessian for the next frame's prior (LAST_FRAME: marginalised over the previous frame, Optimizer::Marginalize).  ONE kernel launch
 * and one wait per call.  One deviation: a failed factorisation ends the round's iterations WITHOUT applying an update (the
 * reference applies an undefined one) and sets solve_failed.  Pinhole mpCamera, mpCamera2 == NULL only.  ORBG_BAD_ARG / ORBG_CAP_EXCEEDED
 * (n > 4096) are returned before a device is looked for, ORBG_NO_DEVICE where there is none. */
int pose_inertial_optimize(const pose_inertial_problem* p, pose_inertial_result* r);
/* TEST AID, not part of the stable interface: the kernel's edge arithmetic, compiled for the host, at the estimates handed in.
 * J: 30 x 32 row-major, the stacked Jacobian of the non-visual edges (rows: EdgeInertial 9, EdgeGyroRW 3, EdgeAccRW 3, EdgePriorPoseImu
 * 15; columns: the unknowns, then the error); vis: n x 31, per visual edge the error (3), its chi2, J^T Omega J (21, upper triangle)
 * and -J^T Omega e (6) without robust weights.  No device needed. */
int pose_inertial_host_linearize(const pose_inertial_problem* p, double* J, double* vis);

/* The three C.rowRange().colRange().inv(cv::DECOMP_SVD) reads of an IMU::Preintegrated's covariance C (15 x 15, row-major): rows 0-8 with
 * the symmetrisation and the eigenvalue clamp at 1e-12 of the EdgeInertial constructor (S/G2oTypes.cc:702-714), rows 9-11 and 12-14 as
 * S/Optimizer.cc:7798-7813 reads them.  The inverses are computed in double and rounded to float where the reference reads .at<float>.
 * Host code, no device needed. */
int orbg_imu_information(const float C[225], double info9[81], double infoG[9], double infoA[9]);
/* The ConstraintPoseImu constructor's conditioning of H, in place (I/G2oTypes.h:712-718): eigenvalues below 1e-12 become 0 ((H + H) / 2
 * there is H, not a symmetrisation: the lower triangle is what the eigen solver reads).  pose_inertial_result::H of frame t goes through
 * it into pose_inertial_prior::H of frame t + 1.  Host code, no device needed. */
int orbg_condition_prior(double H[225]);

/* ---------------------------------------------------------------- local inertial BA (the per-keyframe optimiser of an inertial agent)
 *
 * Optimizer::LocalInertialBA (S/Optimizer.cc:4556-5226), what LocalMapping::Run calls instead of LocalBundleAdjustment once the IMU is
 * initialised (S/LocalMapping.cc:213-248).  The caller flattens the graph the reference builds: the window's keyframes (free), the
 * keyframe in front of it (fixed, with its velocity and biases) and the fixed keyframes that observe the local points, all in one list. */
#define INERTIAL_BA_MAX_FREE_KEYFRAMES 32      /* the reference's window holds at most 25 */
#define INERTIAL_BA_MAX_EDGES (1 << 22)

typedef struct inertial_ba_keyframe {
  pose_inertial_state state;   /* VertexPose / VertexVelocity / VertexGyroBias / VertexAccBias of pKFi (velocity and biases unread when !imu) */
  int32_t fixed;               /* setFixed(true): the keyframe in front of the window, the other observers of the local points */
  int32_t imu;                 /* pKFi->bImu: velocity and bias vertices exist (15 unknowns when free, else 6) */
  int32_t link;                /* EdgeInertial + EdgeGyroRW + EdgeAccRW from keyframe `prev` to this one exist (:4791: both bImu, a preintegration) */
  int32_t prev;                /* index of pKFi->mPrevKF in the list (read when link) */
  int32_t last_in_window;      /* i == N - 1: the edge to the fixed keyframe, information * 1e-2 and a Huber kernel (:4826-4837) */
  pose_inertial_preint preint; /* pKFi->mpImuPreintegrated (read when link) */
  double info9[81];            /* orbg_imu_information(pKFi->mpImuPreintegrated->C): EdgeInertial's, EdgeGyroRW's, EdgeAccRW's */
  double infoG[9];
  double infoA[9];
} inertial_ba_keyframe;

typedef struct inertial_ba_problem {
  uint32_t struct_size;        /* sizeof(inertial_ba_problem) */
  int32_t n_keyframes, n_points, n_edges;
  const inertial_ba_keyframe* keyframes;
  const float* points;         /* n_points x 3, pMP->GetWorldPos() */
  const lba_edge* edges;       /* EdgeMono / EdgeStereo in creation order (per point, its observations: `point` never decreases);
                                  pose = index into keyframes[]; inv_sigma2 = mvInvLevelSigma2[octave] (Pinhole::uncertainty2 is 1) */
  const uint8_t* close;        /* n_points, pMP->mTrackDepth < 10.f */
  int32_t rec_init;            /* bRecInit: a Huber kernel on every EdgeInertial */
  int32_t large;               /* bLarge: lambda 1e-2 and 4 iterations instead of 1e0 and 10; never `failed` */
  float fx, fy, cx, cy, bf;    /* the pinhole mpCamera; mpCamera2 == NULL */
  float Tcb[12];               /* mImuCalib.Tcb, rows 0-2 (row-major 3 x 4) */
  int32_t device;
} inertial_ba_problem;

typedef struct inertial_ba_state { double Rwb[9], twb[3], vwb[3], bg[3], ba[3]; } inertial_ba_state;

typedef struct inertial_ba_result {
  uint32_t struct_size;        /* sizeof(inertial_ba_result) */
  inertial_ba_state* states;   /* n_keyframes (caller-allocated), the final estimates; fixed keyframes unchanged */
  float*   points;             /* n_points x 3 (caller-allocated) */
  double*  edge_chi2;          /* n_edges or NULL: e->chi2() after optimize() -- of the LAST evaluation, a rejected trial's if the run ended on one */
  uint8_t* edge_depth_pos;     /* n_edges or NULL: e->isDepthPositive() at the final estimate */
  uint8_t* edge_outlier;       /* n_edges or NULL: the erase predicates of :5097 / :5114 */
  int32_t  n_outliers;
  int32_t  failed;             /* (2 * err < err_end || isnan(err) || isnan(err_end)) && !bLarge on the FLOAT err / err_end (:5128) */
  int32_t  iters;              /* LM iterations run */
  double   chi2_initial;       /* err: activeRobustChi2() in front of optimize() */
  double   chi2_final;         /* err_end: activeRobustChi2() after it (the errors of the last evaluation) */
  double*  trace;              /* optional, trace_cap x 3 as ba_result's: lambda, chi2 and the trials of every iteration */
  int32_t  trace_cap, trace_len;
} inertial_ba_result;

typedef struct inertial_ba_handle inertial_ba_handle;

/* The numerical core of Optimizer::LocalInertialBA: computeActiveErrors(), ONE optimize(bLarge ? 4 : 10) of g2o's Levenberg-Marquardt
 * (user lambda 1e0 / 1e-2) with the map points marginalised, the verdicts.  No abort flag: the reference sets it after optimize().
 * Refused before a device is looked for: ORBG_BAD_ARG (a NULL array, struct_size, an index out of range, an edge list that is not
 * grouped per point, two edges of one keyframe and point, ur == LBA_UR_RIGHT_CAMERA, a link on a fixed keyframe or between keyframes
 * without imu, no free keyframe), ORBG_CAP_EXCEEDED (more than INERTIAL_BA_MAX_FREE_KEYFRAMES free keyframes or INERTIAL_BA_MAX_EDGES
 * edges).  Two solves of the same problem return the same bits. */
int inertial_ba_solve(const inertial_ba_problem* p, inertial_ba_result* r);
/* ... with a handle that keeps the device buffers, the solver object and the stream between calls (one solve at a time per handle). */
int inertial_ba_create(int device, inertial_ba_handle** out);
int inertial_ba_destroy(inertial_ba_handle* h);
int inertial_ba_solve_h(inertial_ba_handle* h, const inertial_ba_problem* p, inertial_ba_result* r);
int inertial_ba_set_stream(inertial_ba_handle* h, void* hip_stream);   /* as lba_set_stream */
int inertial_ba_set_profiling(inertial_ba_handle* h, int on);          /* as ba_set_profiling */
int inertial_ba_get_phase_ms(inertial_ba_handle* h, double* ms /*5: structure, linearise, Schur, LDL^T, update*/);
/* TEST AID, not part of the stable interface: the kernels' edge arithmetic, compiled for the host, at the estimates handed in.
 * vis: n_edges x 31, per visual edge the error (3, third 0 for EdgeMono), its chi2, the point Jacobian (3 x 3) and the pose Jacobian
 * (3 x 6), row-major; inertial: per keyframe with link, in list order, the stacked 15 x 32 Jacobian of EdgeInertial (rows 0-8), EdgeGyroRW
 * (9-11) and EdgeAccRW (12-14) -- columns: keyframe prev's 15, this keyframe's 15, the error in column 30.  No device needed. */
int inertial_ba_host_linearize(const inertial_ba_problem* p, double* vis, double* inertial);

/* ---------------------------------------------------------------- inertial initialisation (what makes the two optimisers above reachable)
 *
 * Optimizer::InertialOptimization, four overloads (S/Optimizer.cc:5344, :5534, :5696, :5858): what LocalMapping::InitializeIMU calls
 * three times per session (S/LocalMapping.cc:1492), LocalMapping::ScaleRefinement every 10 s (:1618) and LoopClosing after a merge
 * (S/LoopClosing.cc:2170).  Every pose is fixed; each keyframe with an mPrevKF adds one EdgeInertialGS (S/G2oTypes.cc:802-927) over the two
 * velocities, ONE gyro bias, ONE accelerometer bias, the gravity direction (VertexGDir, 2 unknowns) and the scale (VertexScale, 1).  The
 * overloads differ only in what is free, the algorithm and the iteration count:
 *   (Map, Rwg, scale, bg, ba, bMono, cov, bFixedVel, bGauss, priorG, priorA): LM, 200 iterations, lambda_init = priorG != 0 ? 1e3 : auto;
 *       free_velocity = free_bias = !bFixedVel, free_gdir = 1, free_scale = bMono, with_priors = 1
 *   (Map, bg, ba, priorG, priorA) and (vector<KeyFrame*>, bg, ba, priorG, priorA): LM, 200, lambda_init = 1e3; free_velocity = free_bias
 *       = 1, free_gdir = free_scale = 0 with Rwg = I and scale = 1, with_priors = 1
 *   (Map, Rwg, scale): Gauss-Newton, 10 iterations; free_gdir = free_scale = 1 only, with_priors = 0 */
#define INERTIAL_INIT_MAX_KEYFRAMES 4096       /* above ba_solve's 1365 and eg_solve's 1170: no map the other solvers accept is refused here */
enum { INERTIAL_INIT_LM = 0, INERTIAL_INIT_GN = 1 };

typedef struct inertial_init_edge {
  int32_t k1, k2;              /* index of pKFi->mPrevKF and of pKFi in keyframes[] */
  pose_inertial_preint preint; /* pKFi->mpImuPreintegrated after SetNewBias(mPrevKF->GetImuBias()) */
  double info9[81];            /* orbg_imu_information(pKFi->mpImuPreintegrated->C): the EdgeInertialGS constructor (S/G2oTypes.cc:809-821)
                                  conditions its information exactly as EdgeInertial's (:702-714) */
} inertial_init_edge;

typedef struct inertial_init_problem {
  uint32_t struct_size;        /* sizeof(inertial_init_problem) */
  int32_t device;
  int32_t algorithm;           /* INERTIAL_INIT_LM / INERTIAL_INIT_GN */
  int32_t iterations;          /* its */
  double lambda_init;          /* setUserLambdaInit; <= 0 = auto (tau * the largest diagonal entry) */
  int32_t free_velocity;       /* !VV->fixed(): the velocity of every keyframe that has an edge */
  int32_t free_bias;           /* !VG->fixed() && !VA->fixed() */
  int32_t free_gdir;           /* !VGDir->fixed() */
  int32_t free_scale;          /* !VS->fixed() */
  int32_t with_priors;         /* EdgePriorAcc / EdgePriorGyro toward 0 exist; they are active only while the biases are free */
  double prior_g, prior_a;     /* infoPriorG, infoPriorA (>= 0) */
  float bg[3], ba[3];          /* vpKFs.front()'s bias: EVERY bias vertex is constructed from it */
  double Rwg[9], scale;        /* VertexGDir's and VertexScale's estimates, row-major */
  int32_t n_keyframes;
  const pose_inertial_state* keyframes;   /* Rwb, twb, vwb; bg and ba are not read */
  int32_t n_edges;
  const inertial_init_edge* edges;        /* in creation order */
} inertial_init_problem;

typedef struct inertial_init_result {
  uint32_t struct_size;        /* sizeof(inertial_init_result) */
  int32_t  iters;              /* iterations run (a Gauss-Newton iteration whose solve failed included) */
  int32_t  n_unknowns;         /* 3 per free velocity in the system + 6 / 2 / 1 for the free biases / direction / scale */
  int32_t  solve_failed;       /* Gauss-Newton met a pivot that is not positive: no update was applied, the run ended */
  double*  vwb;                /* n_keyframes x 3 (caller-allocated); a keyframe without an edge, and every keyframe when the
                                  velocities are fixed, comes back as it went in */
  double   bg[3], ba[3], Rwg[9], scale;
  double   chi2_first;         /* chi2 of the first linearisation */
  double   chi2_final;         /* chi2 of the estimates returned */
  double*  trace;              /* optional, trace_cap x 3 as inertial_ba_result's: lambda, chi2 and the trials of every iteration
                                  (Gauss-Newton: 0, the chi2 the iteration linearised at, 1) */
  int32_t  trace_cap, trace_len;
} inertial_init_result;

/* optimizer.optimize(its) of Optimizer::InertialOptimization: g2o's Levenberg-Marquardt as the bundle adjustments run it (ten trials per
 * iteration, _nBad >= 3, rho == 0) or Gauss-Newton (one update per iteration).  ONE kernel launch and one wait per call: the system
 * (3 x 3 velocity blocks along the mPrevKF forest, a border of up to 9 columns) is eliminated in an order without fill and never formed
 * densely.  One deviation: a pivot that is not positive and finite refuses the solve -- under LM the trial counts as failed, under
 * Gauss-Newton no update is applied, solve_failed is set and the run ends (the reference applies an undefined update there; the same
 * deviation pose_inertial_optimize documents).  Refused before a device is looked for: ORBG_BAD_ARG (a NULL array, struct_size, an
 * index out of range, a keyframe that is k2 of two edges, a cycle, no free unknown, no edge), ORBG_CAP_EXCEEDED (more than
 * INERTIAL_INIT_MAX_KEYFRAMES keyframes).  A keyframe that is k1 of several edges is accepted.  Two solves of the same problem return the
 * same bits. */
int inertial_init_solve(const inertial_init_problem* p, inertial_init_result* r);
/* TEST AID, not part of the stable interface: the kernel's edge arithmetic, compiled for the host, at the estimates handed in.
 * J: n_edges x 9 x 16 row-major, per edge the columns [v1 3 | v2 3 | bg 3 | ba 3 | gdir 2 | s 1 | e 1] of EdgeInertialGS, every vertex taken
 * as free.  No device needed. */
int inertial_init_host_linearize(const inertial_init_problem* p, double* J);

/* ---------------------------------------------------------------- streams, hardware queues, host threads
 * Streams.  Every handle enqueues its work on ONE HIP stream.  By default that stream comes from a per-device pool the library
 * creates with its first handle: four hipStreamNonBlocking streams -- L (local BA handles), E0 / E1 (extractor handles,
 * alternating; a frame built by a constructor is on its extractor's stream until the constructor has been COLLECTED -- from then on its
 * searches run on the frame's own stream, M, and never queue behind constructors of later frames), M (map uploads, PoseOptimization, vocabulary and
 * database handles, host-built frames, the stand-alone utilities).  None of them is the legacy null stream: nothing the library
 * launches joins, or is joined by, the blocking streams of the application (SURVEY.md 8(b) "no hidden global state": the pool is the
 * one piece of per-device state the handles share, and it can be replaced).  *_set_stream hands a handle the CALLER's stream instead
 * (a hipStream_t passed as void*; never the null stream -- NULL means "back to the pool"); the handle must be idle, its old stream
 * is drained first, and the caller's stream is never destroyed by the library.  ORBG_STREAM_POOL=0 in the environment gives every
 * handle a private stream.
 * Hardware queues.  The ROCm runtime multiplexes the streams of a process onto GPU_MAX_HW_QUEUES hardware queues (4 by default); the
 * streams that share a queue are serialised.  The pool's four streams are created together so that they occupy the four default
 * queues.  An application that keeps further streams of its own busy next to the library should start with GPU_MAX_HW_QUEUES =
 * 4 + its own busy streams in the environment (it is read when the runtime initialises; measured here: 4, 5 and 6 are equally good
 * for an agent, 3 costs a third of the frame rate, 8 half of it).
 * Host threads.  A synchronous call blocks its caller by SPINNING on a completion word in pinned memory for up to a bounded time
 * (then it falls back to the runtime's blocking wait); the asynchronous forms own one thread each -- lba_solve_async: one worker per
 * handle, ORBX_SUBMIT_ASYNC: one ingest thread per process -- which spin for a few hundred microseconds between jobs before they
 * sleep.  An agent that uses all three therefore keeps up to three cores busy (tracking thread, local-BA worker, ingest thread);
 * The policy is per ROLE of the waiting thread (orbg_set_wait_policy below): ORBG_ROLE_CALLER (any thread of the application that
 * calls the library: Tracking), ORBG_ROLE_LBA_WORKER, ORBG_ROLE_INGEST.  A role that does not spin waits in the runtime's blocking
 * form / on a condition variable (6-10 us more latency per wait, no busy core).  A host whose CPU quota cannot feed three spinning
 * threads per agent keeps the tracking thread spinning (it is on the frame's critical path) and lets the other two block.
 * ORBG_NO_POLL in the environment sets the start-up policy: "1" / "all" = no role spins; a comma list of caller / lba / ingest =
 * those roles block.
 * Cameras.  The fused Frame constructors (orbx_frame_stereo*) build the grid from the extracted keypoints as they are, i.e. they
 * implement Frame::UndistortKeyPoints for mDistCoef[0] == 0 (rectified stereo: mvKeysUn = mvKeys, S/Frame.cc:723-727).  The
 * reference's image bounds are exactly the image rectangle in that case (S/Frame.cc:775-783) and the undistorted corners otherwise
 * (:753-773): a view whose bounds are not (0, width, 0, height) is refused with ORBG_BAD_ARG.  Distorted cameras (the mono agents
 * with EuRoC intrinsics) use orbx_frame_mono*, which undistorts on the device. */
enum { ORBG_ROLE_CALLER = 0, ORBG_ROLE_LBA_WORKER = 1, ORBG_ROLE_INGEST = 2 };
int orbg_set_wait_policy(int role, int spin);   /* spin != 0: waits of that role spin on completion words; 0: they block.  Process-wide, any time */
int orbg_get_wait_policy(int role);             /* 1 = spins, 0 = blocks, ORBG_BAD_ARG for an unknown role */
int orbx_set_stream(orbx_handle* h, void* hip_stream);
int orbm_frame_set_stream(orbm_frame* f, void* hip_stream);
int orbm_map_set_stream(orbm_map* m, void* hip_stream);
int lba_set_stream(lba_handle* h, void* hip_stream);
int orbv_vocab_set_stream(orbv_vocab* v, void* hip_stream);
int orbd_database_set_stream(orbd_database* d, void* hip_stream);
int pose_opt_set_stream(int device, void* hip_stream);      /* the calling thread's pose_optimize calls on `device` */
int pose_inertial_set_stream(int device, void* hip_stream); /* the calling thread's pose_inertial_optimize calls on `device` */
int inertial_init_set_stream(int device, void* hip_stream); /* the calling thread's inertial_init_solve calls on `device` */

/* ---------------------------------------------------------------- misc */
const char* orbg_version(void);
const char* orbg_strerror(int code);
int orbg_device_count(void);
/* Spins until everything enqueued so far on the library's pooled streams of `device` has completed (handles on caller-supplied
 * streams are the caller's to wait for).  After it, the runtime's own device synchronisation finds nothing outstanding. */
int orbg_quiesce(int device);
/* Device timings (ms, hipEvent on the handle's stream) of the most recent call, for bench.py.
 * ms[0] pyramid, [1] FAST+gather, [2] host quad-trees (wall), [3] orientation+descriptors, [4] stereo match,
 * [5] fast_cells_kernel alone.  orbx_set_profiling: 0 = record nothing, 1 = only [2] and [5] (default),
 * 2 = every stage (more hipEventRecord calls per frame). */
int orbx_set_profiling(orbx_handle* h, int level);
int orbx_get_timings(orbx_handle* h, float* ms /*8*/);
/* Average elapsed time of an EMPTY event pair on the handle's stream: the constant the profiling brackets add to a
 * bracketed kernel's duration (bench.py reports the bracketed time both raw and net of this). */
int orbx_event_overhead(orbx_handle* h, int reps, float* ms);
/* Profiling level 1 brackets fast_cells_kernel with an event pair; with interval k only every k-th extraction is bracketed.
 * The bracket times accumulate in the handle (sum in ms, number of samples) until reset. */
int orbx_set_profile_interval(orbx_handle* h, int interval, int reset);
/* Which kernel of the Frame-constructor chain the level-1 event pair brackets (default: fast_cells_kernel); the
   accumulated times are read with orbx_get_fast_kernel_stats and reset by this call.  For bench.py's roofline line,
   which has to describe whichever kernel dominates the step. */
#define ORBX_PROF_FAST 0
#define ORBX_PROF_OCTREE 1
#define ORBX_PROF_ORIENT_DESC 2
#define ORBX_PROF_PYRAMID 3
int orbx_set_profile_kernel(orbx_handle* h, int which);
/* Host-side timeline of the handle's last Frame constructors (<= 512 kept), oldest first: out[i * 5 + f] in microseconds,
 * f = 0 queue (hand-over to the ingest thread -> it starts; 0 for synchronous submissions), 1 pack (rows copied into the pinned
 * staging slot), 2 enqueue (host time of the launches), 3 wait (time the collecting thread was blocked), 4 latency (hand-over ->
 * constructor complete, as the collecting thread sees it; the synchronous orbx_frame_stereo records pack and latency only).
 * *n = entries written; reset != 0 forgets them.  For bench.py's per-step diagnosis of a shared host. */
int orbx_get_ctor_timeline(orbx_handle* h, float* out, int cap, int* n, int reset);
int orbx_get_fast_kernel_stats(orbx_handle* h, double* sum_ms, int64_t* n);
/* Number of frames this handle ran the device quad-trees on and then redid with the host quad-trees because a device list
 * overflowed (more than 4096 candidates at a level of one camera, or more nodes than a level's list holds).  Such a frame costs a
 * device pass and a host pass; its results are the same.  Frames that go to the host trees at once -- a partial lapping area,
 * ORBG_HOST_OCTREE=1, a per-level target too large for the node list (4 N + 8 > 2048) -- are no redos and do not count.  Read-only;
 * counts from the handle's creation, for synchronous calls and for the two-halves constructors alike. */
int orbx_get_host_redo_count(orbx_handle* h, int64_t* n);

/* ---------------------------------------------------------------- MLPnPsolver (Tracking::Relocalization's RANSAC, prefix orbp_)
 * S/MLPnPsolver.cpp, I/MLPnPsolver.h: RANSAC over minimal sets of six matched map points, MLPnP per hypothesis (null spaces of the
 * bearings, the 12 x 12 -- planar: 9 x 9 -- linear solve, nearest rotation, sign choice, at most five Gauss-Newton iterations), inliers
 * by reprojection.  Every hypothesis of a call is evaluated in ONE kernel launch, all in FP64 up to CheckInliers' float statements; the
 * serial loop of :99-216 is then replayed on the host over the inlier counts in draw order, so the outcome is the one the serial loop
 * gives for the same draws.  Two behaviours of the reference are reproduced as they are:
 *   - Refine() (:288-342) solves on all inliers into a local variable, never stores that pose and then counts the inliers of the
 *     hypothesis that is still in mRi / mti: what iterate returns is the CURRENT hypothesis converted to float, with its inliers, and
 *     exactly when its count exceeds mRansacMinInliers (strictly).  No N-point solve runs on the device.
 *   - the loop condition (:113) is an OR: a call runs max(n_iterations, mRansacMaxIts - mnIterations) iterations unless it returns.
 * The flat problem is what the constructor keeps per surviving match (:54-96): P2D = mvKeysUn[i].pt, sigma2 = mvLevelSigma2[octave],
 * bearing = mpCamera->unproject(pt) divided by its z (NOT normalised to unit length: the reference does not, and the sign test uses it
 * as it is), P3Dw = the map point, kp_index = mvKeyPointIndices with m = mvpMapPointMatches.size(), and the camera of CheckInliers'
 * mpCamera->project(cv::Point3f).  camera.model must be ORBG_CAM_PINHOLE (S/CameraModels/Pinhole.cpp:30-33 in float); any other model
 * is refused with ORBG_BAD_ARG.  Not provided: the covariance path (use_cov, never taken: covs(1)) and a rig's right camera (:70 skips
 * those matches).  struct_size as in orbm_sim3_problem. */
typedef struct orbp_mlpnp_problem {
  uint32_t struct_size;
  int32_t  n;                    /* N = mvP2D.size() */
  const float* P2D;              /* n x 2 */
  const float* sigma2;           /* n */
  const float* bearing;          /* n x 3 */
  const float* P3Dw;             /* n x 3 */
  const int32_t* kp_index;       /* n, each in [0, m) */
  int32_t  m;                    /* mvpMapPointMatches.size() */
  orbg_camera camera;
} orbp_mlpnp_problem;

/* SetRansacParameters' arguments (:218; defaults 0.99, 8, 300, 6, 0.4, 5.991 in I/MLPnPsolver.h; Relocalization uses
 * 0.99, 10, 300, 6, 0.5, 5.991).  min_set must be 6: computePose asserts more than five points and the sign test reads six. */
typedef struct orbp_mlpnp_params {
  double  probability;
  int32_t min_inliers;
  int32_t max_iterations;
  int32_t min_set;
  float   epsilon;
  float   th2;
} orbp_mlpnp_params;

/* Outcome of one iterate().  returned: a non-empty matrix came back -- Tcw (the 4 x 4 float matrix), n_inliers = nInliers and inliers
 * = vbInliers (m bytes through kp_index; caller's buffer, NULL: not wanted) are then set, otherwise zero.  After a return without
 * no_more this is the hypothesis that exceeded min_inliers, which after an earlier call need not be the best one.  best_* / have_best /
 * best_iteration (0-based mnIterations index): mBestTcw, mnBestInliers as they persist between calls.  iterations_run: iterations the
 * serial loop ran in this call; iterations_done: mnIterations after it.
 * hyp_*: optional per-hypothesis outputs of THIS call in draw order, for checkers (NULL: not read back): inlier counts, the planar
 * flag, the pose in double (R: 9 per hypothesis row-major, t: 3) and bit-packed masks (ceil(n / 64) words per hypothesis, bit i & 63
 * of word i >> 6).  They cover every hypothesis of the launch (orbp_mlpnp_iterations_of_call), also those behind the one that returned. */
typedef struct orbp_mlpnp_result {
  uint32_t struct_size;
  int32_t  no_more;                /* bNoMore */
  int32_t  returned;
  int32_t  n_inliers;              /* nInliers */
  int32_t  iterations_done;
  int32_t  iterations_run;
  int32_t  best_iteration;
  int32_t  have_best;
  int32_t  best_inliers;           /* mnBestInliers */
  float    Tcw[16];
  float    best_Tcw[16];           /* mBestTcw */
  uint8_t* inliers;
  int32_t* hyp_n_inliers;
  int32_t* hyp_planar;
  double*  hyp_R;
  double*  hyp_t;
  uint64_t* hyp_masks;
} orbp_mlpnp_result;

typedef struct orbp_mlpnp orbp_mlpnp;

/* The constructor after its loop over the matches: create + set_problem.  set_problem copies the arrays, resets mnIterations /
 * mnBestInliers and applies SetRansacParameters() at its defaults, as the constructor does. */
int orbp_mlpnp_create(int device, orbp_mlpnp** out);
int orbp_mlpnp_destroy(orbp_mlpnp* h);
int orbp_mlpnp_set_stream(orbp_mlpnp* h, void* hip_stream);
int orbp_mlpnp_set_problem(orbp_mlpnp* h, const orbp_mlpnp_problem* p);
/* SetRansacParameters (:218-253, host) with its oddities: int(N * epsilon) truncated, min_inliers raised to it and to min_set, epsilon
 * raised to min_inliers / N in float, pow(epsilon, 3) for a minimal set of six, mvMaxError[i] = sigma2[i] * th2 in float.  It does not
 * reset mnIterations or the best so far. */
int orbp_mlpnp_set_ransac_parameters(orbp_mlpnp* h, double probability, int min_inliers, int max_iterations, int min_set,
                                     float epsilon, float th2);
/* ... the same formula without a handle: *max_its = mRansacMaxIts and *min_inliers_out = mRansacMinInliers for N = n.  No device. */
int orbp_mlpnp_ransac_iterations(int n, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                                 int* max_its, int* min_inliers_out);
/* How many iterations the serial loop can run in the next iterate(n_iterations): max(n_iterations, mRansacMaxIts - mnIterations), or
 * 0 when N < mRansacMinInliers.  The caller supplies six raw draws for each of them. */
int orbp_mlpnp_iterations_of_call(orbp_mlpnp* h, int n_iterations, int* k);
/* The minimal sets of :126-138: draws = the raw DUtils::Random::RandomInt(0, size - 1) results, six per iteration (draw j from a list
 * of n - j entries; anything else is ORBG_BAD_ARG); idx = the six correspondence indices of the swap-with-back removal.  Host only. */
int orbp_mlpnp_resolve_draws(int n, const int32_t* draws, int n_iterations, int32_t* idx);
/* cv::Mat MLPnPsolver::iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers), :99-216: all hypotheses the
 * call can run in one launch, one completion wait.  N < mRansacMinInliers: no_more without a launch (:104-108). */
int orbp_mlpnp_iterate(orbp_mlpnp* h, int n_iterations, const int32_t* draws, orbp_mlpnp_result* result);
/* The first iterate() of B fresh solvers -- the candidate keyframes of one Relocalization (S/Tracking.cc:3400-3425) -- in ONE launch:
 * problems[b] with SetRansacParameters(params[b]) and draws[b] (6 * mRansacMaxIts(b) values).  Because of the OR above every solver is
 * finished or exhausted after that call, so solving them together changes nothing the caller can observe.  All arguments and the
 * device are checked before any result is written. */
int orbp_mlpnp_solve_batch(int device, const orbp_mlpnp_problem* problems, int B, const orbp_mlpnp_params* params,
                           const int32_t* const* draws, orbp_mlpnp_result* results);
/* Stage 5 of computePose alone (:635-647) for the six points given, on the device: rot2rodrigues(R), mlpnp_gn, rodrigues2rot.  For
 * checkers: a rotation with trace 3 gives a NaN pose, as the reference's Jacobian (a division by |omega|^2) does. */
int orbp_mlpnp_gn(int device, const float* P3Dw /*6x3*/, const float* bearing /*6x3*/, const double* R /*9*/, const double* t /*3*/,
                  double* R_out /*9*/, double* t_out /*3*/);

#ifdef __cplusplus
}
#endif
#endif /* ORBGPU_H_ */
