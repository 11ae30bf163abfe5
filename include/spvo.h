/*
 * spvo.h -- C ABI of the MI355X-native SuperPoint stereo-VO front end.
 *
 * This is the drop-in boundary beneath the reference's C++ `FeatureFrontEnd`
 * (reference: src/odml_visual_odometry/include/odml_visual_odometry/
 * feature_detection.hpp:96-178, "hpp" below).  The reference calls TensorRT,
 * OpenCV and Ceres directly from that class; here the class in
 * superpoint-stereo-visual-odometry_amd/host/ keeps the same public API and
 * forwards every heavy call to the entry points below, which run hand-written
 * gfx950 HIP kernels.  Plain pointers and sizes only; no C++, OpenCV, ROS or
 * torch types.  All functions return 0 on success or a negative spvo_status;
 * nothing throws across this boundary (the reference logs ROS_ERROR and
 * returns: neural_network.cpp:53-55,96-100).  A context is NOT thread-safe and
 * is bound to one HIP device (the reference is single-threaded: node.cpp:445-449).
 *
 * "nn.cpp"   = src/odml_visual_odometry/src/feature_detection_neural_network.cpp
 * "base.cpp" = src/odml_visual_odometry/src/feature_detection_base.cpp
 * "cost.hpp" = src/odml_visual_odometry/include/odml_visual_odometry/ceres_cost_function.hpp
 */
#ifndef SPVO_H
#define SPVO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spvo_ctx spvo_ctx;

typedef enum {
  SPVO_OK = 0,
  SPVO_ERR_INVALID = -1,   /* bad argument / shape */
  SPVO_ERR_DEVICE = -2,    /* HIP runtime error, no gfx950 device, ... */
  SPVO_ERR_IO = -3,        /* weight file missing / malformed (nn.cpp:53-55) */
  SPVO_ERR_STATE = -4,     /* call order (no weights loaded, slot empty, ...) */
  SPVO_ERR_CAPACITY = -5   /* caller buffer too small */
} spvo_status;

/* Constructor arguments of SuperPointFeatureFrontEnd that matter below the
 * class (hpp:272-295); defaults are the reference's laptop launch file
 * (launch/visual_odometry_superpoint.launch:3-26). */
typedef struct {
  int device;          /* HIP device ordinal                                  */
  int net_height;      /* input_height, multiple of 8 (hpp:296)     [360]     */
  int net_width;       /* input_width,  multiple of 8               [1176]    */
  int max_batch;       /* images per network call: 1 or 2 (hpp:342-344) [2]   */
  float conf_thresh;   /* heat > conf_thresh, strict (nn.cpp:203)   [0.015]   */
  int dist_thresh;     /* NMS Chebyshev radius (nn.cpp:246-254)     [4]       */
  int border_remove;   /* nn.cpp:239-244                            [4]       */
  int max_keypoints;   /* hpp:368 (static constexpr 1000)           [1000]    */
  int bug_compat_p;    /* 1: keep the reference's no-op principal-point shift
                          (base.cpp:95,111 writes at<float> into a CV_64F P);
                          0: apply the intended cx/cy -= crop offset.   [1]   */
} spvo_config;

void spvo_default_config(spvo_config *cfg);

int spvo_create(const spvo_config *cfg, spvo_ctx **out);
void spvo_destroy(spvo_ctx *ctx);
const char *spvo_last_error(const spvo_ctx *ctx);   /* ctx may be NULL */

/* Replaces loadTrtEngine (nn.cpp:43-137): load a .spvw plan + fp32 weights
 * (written by spvo/weights.py) and repack them on the device. */
int spvo_load_weights(spvo_ctx *ctx, const char *path);

/* ------------------------------------------------------------------ stages
 * One entry point per reference stage so that each can be parity-checked
 * alone.  Unless a name ends in _dev every pointer is HOST memory and the call
 * is synchronous (copies in, runs on the context's stream, copies out).      */

/* Precision of the loaded engine: 0 = FP32, 1 = FP16 (what engine_generation.py:13-56 selects with trtexec --fp16
 * and the engine file name carries, nn.cpp:44-49), 2 = INT8 (an extension: calibrated activation scales travel in
 * the engine file); SPVO_ERR_STATE (negative) before spvo_load_weights.  FP16 and INT8 engines keep fp32 bindings
 * (nn.cpp:117): every entry point takes and returns the same types. */
int spvo_engine_precision(const spvo_ctx *ctx);

/* Opt-in evaluation mode for FP32 engines loaded AFTER the call (environment default: SPVO_FP32_SPLIT=1): every fp32
 * operand of the convolutions is carried as three bf16 pieces (exact: 3 x 8 = 24 significand bits) and every product is
 * the sum of its six leading partial products on the bf16 matrix pipe with fp32 accumulation
 * (csrc/conv_bf16x3.hip.h).  Results agree with the native fp32 engine to fp32 rounding level; the engine file, the
 * bindings and spvo_engine_precision (0) do not change.  Covers convolution + L2-norm graphs (the VGG SuperPoint of
 * nn.cpp:43-137); other graphs fail at spvo_load_weights. */
int spvo_set_fp32_split(spvo_ctx *ctx, int enable);

/* Opt-in mode for INT8 engines loaded AFTER the call (process-wide default: spvo_set_tuning "int8_general", 0; this call
 * overrides it for the context): the loader also accepts the two things the squeeze graph needs and the default refuses --
 *   - a stand-alone 2x2/2 max-pool between two int8 tensors of equal channel count, one level apart, on a map of even height
 *     and width: q_o = clip(rint(f32(max of the four q_i) * m), -127, 127) with m = f32(s_i * (f32(1) / s_o)), one fp32
 *     multiply per value, round-half-even (csrc/conv_i8.hip.h, maxpool2_i8_kernel);
 *   - a convolution whose cin is 16 more than a multiple of 32 (16, 48, ...): its last chunk holds one group of 16 channels
 *     and is padded with zero weights, so the int32 accumulator stays the exact sum over the real cin.
 * The arithmetic of everything else is unchanged: an engine the default mode loads gives the same bits in this mode.  With
 * the mode off both stay refused at spvo_load_weights, with SPVO_ERR_IO.  SPVO_ERR_INVALID for a null context. */
int spvo_set_int8_general(spvo_ctx *ctx, int enable);

/* preprocessImageImpl (base.cpp:68-121) + preprocessImage (nn.cpp:139-161):
 * centre-crop to the network aspect ratio, cv::resize(INTER_LINEAR) 8-bit
 * fixed-point semantics, scale P rows 0-1.  `P` (3x4 row-major, f64) is
 * updated in place.  `resized_u8` (net_height*net_width) may be NULL.
 * Before spvo_load_weights (a context without an engine: the classic front
 * end at a fixed input size, classic.cpp:96-100) only the crop, the resize
 * and P are done -- the same image, no network input plane is written. */
int spvo_preprocess(spvo_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride,
                    double P[12], uint8_t *resized_u8);

/* runNeuralNetwork (nn.cpp:163-176): input [batch,1,H,W] f32 in [0,1];
 * det [batch,65,H/8,W/8] NCHW; desc_nhwc [batch,H/8,W/8,256] (unit L2 norm
 * over the last axis; the reference's NCHW `output_desc` transposed, which is
 * what nn.cpp:339-342 computes on the CPU before sampling). Either output may
 * be NULL. */
int spvo_forward(spvo_ctx *ctx, const float *input, int batch, float *det, float *desc_nhwc);

/* Fetch an intermediate activation of the last spvo_forward as dense NCHW
 * [batch,C,h,w]; tensor ids are the plan's (spvo/weights.py). Test hook. */
int spvo_debug_tensor(spvo_ctx *ctx, int tensor_id, int batch, float *out, size_t out_floats);

/* postprocessDetectionAndDescription, detector half (nn.cpp:266-326):
 * det [65,H/8,W/8] -> heat [H,W]. */
int spvo_heatmap(spvo_ctx *ctx, const float *det, float *heat);

/* processOneHeatmap (nn.cpp:188-262): threshold, rank (confidence desc, then
 * column-major pixel index asc), exact greedy NMS, border filter, cap.
 * xy: [max_keypoints][2] int32 (x, y) in rank order; *n: count. */
int spvo_nms(spvo_ctx *ctx, const float *heat, int32_t *xy, int *n);

/* bilinearInterpolationDesc (nn.cpp:366-431) for n keypoints on one image:
 * desc_nhwc [H/8,W/8,256] -> out [n,256] (re-normalised, nn.cpp:428). */
int spvo_sample_descriptors(spvo_ctx *ctx, const float *desc_nhwc, const int32_t *xy, int n,
                            float *out);

typedef struct {
  int n;            /* keypoints found (<= max_keypoints)                      */
  float *xy;        /* caller buffer [max_keypoints][2]: x, y (integers stored
                       as float, like cv::KeyPoint::pt; nn.cpp:243)            */
  float *desc;      /* caller buffer [max_keypoints][256]                      */
} spvo_features;

/* addStereoImagePair (nn.cpp:449-498), everything but the deque bookkeeping:
 * preprocess both images, run the network, post-process.  P_l/P_r are updated
 * in place (nn.cpp:465-466 clones then mutates).  The device copies of the
 * keypoints/descriptors are kept in feature slots `slot_l`/`slot_r` (0..9: the
 * caller's ring of prevL, prevR, currL, currR of hpp:66-72, plus the slots of up to
 * three pairs submitted ahead) for spvo_match_slots.
 * `resized_l`/`resized_r` (net_height*net_width u8, what nn.cpp:154 pushes to
 * images_dq) may be NULL. */
int spvo_detect(spvo_ctx *ctx, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols,
                size_t stride, double P_l[12], double P_r[12], int slot_l, int slot_r,
                spvo_features *out_l, spvo_features *out_r, uint8_t *resized_l,
                uint8_t *resized_r);

/* Same, with both images already resident in device memory (u8, `stride` bytes
 * per row) and no host copies of descriptors (out_*->desc may be NULL).  The context
 * works on its own NON-BLOCKING streams: the images must be complete in device memory
 * when the call is made (it does not order itself behind work the caller queued on the
 * NULL stream or any other stream), and must stay untouched until the call -- for the
 * asynchronous form, the matching spvo_detect_wait -- has returned. */
int spvo_detect_dev(spvo_ctx *ctx, const void *d_img_l, const void *d_img_r, int rows, int cols,
                    size_t stride, double P_l[12], double P_r[12], int slot_l, int slot_r,
                    spvo_features *out_l, spvo_features *out_r);

/* Asynchronous form of spvo_detect_dev: _submit returns as soon as the whole detector chain (and,
 * with spvo_set_prematch, the two standard matches) is enqueued; _wait blocks until the OLDEST
 * submission has finished and hands out what spvo_detect_dev would have.  At most six submissions
 * may be in flight: the post-processing of one then overlaps with the network of the next.
 * Meanwhile the caller may run spvo_match_slots on precomputed matches and
 * spvo_solve_stereo_odometry for pairs already waited for: the ROS node receives the next image
 * pairs while it is still solving the current one.  The slots named here are rewritten while the
 * submission is in flight and must differ from those of other submissions in flight; the temporal
 * partner of a submission is the left slot of the submission before it.  All other entry points
 * that touch the detector's buffers (spvo_detect, spvo_forward, spvo_nms, ...) return
 * SPVO_ERR_STATE while a submission is in flight. */
int spvo_detect_dev_submit(spvo_ctx *ctx, const void *d_img_l, const void *d_img_r, int rows, int cols,
                           size_t stride, int slot_l, int slot_r);
int spvo_detect_wait(spvo_ctx *ctx, double P_l[12], double P_r[12], spvo_features *out_l,
                     spvo_features *out_r);

/* Trunk pairing (extension; off by default): with `on`, a submission whose network would only queue behind an earlier one is HELD
 * until the next submission arrives, and the network then runs for both stereo pairs in one set of launches (four images per layer:
 * every layer's launch, first loads and last stores are paid once per two pairs; 678 instead of 738 us per pair for the VGG fp32
 * forward pass at 360x1176).  Waiting for a held pair launches it alone, so nothing ever blocks; results do not depend on the
 * grouping.  It pays when the caller hands pairs over at least four ahead (each launch then finds its predecessor still running);
 * with fewer it costs throughput, which is why the caller decides.  At most six submissions may be in flight. */
int spvo_set_trunk_pairing(spvo_ctx *ctx, int on);

/* The asynchronous form for images in HOST memory -- what a ROS node holds (cv_bridge::toCvCopy, node.cpp:163-168).
 * _submit copies the two images into pinned staging buffers of the submission (the caller's buffers are free when it
 * returns), queues the host-to-device copies and the whole detector chain behind them and returns; up to six
 * submissions may be in flight, exactly as with spvo_detect_dev_submit (same slot rules).  `extras`: bit 0 = the resized
 * u8 images (nn.cpp:154, images_dq), bit 1 = the descriptors (descriptors_dq) also travel back, into pinned mirrors of
 * the submission.  _collect completes the OLDEST submission (of either kind) like spvo_detect_wait and hands out what was
 * requested: results are bit-identical to spvo_detect on the same images. */
int spvo_detect_submit(spvo_ctx *ctx, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride,
                       int slot_l, int slot_r, int extras);
int spvo_detect_collect(spvo_ctx *ctx, double P_l[12], double P_r[12], spvo_features *out_l, spvo_features *out_r,
                        uint8_t *resized_l, uint8_t *resized_r);

/* spvo_detect_collect without its host copies: completes the OLDEST submission and hands out POINTERS into the submission's
 * pinned host mirrors -- n[i] keypoints, xy[i] (n[i] x 2 floats), desc[i] (n[i] x 256 floats; NULL unless `extras` bit 1 was
 * set at spvo_detect_submit), resized[i] (net_height x net_width u8; NULL unless bit 0 was set), i = 0 left, 1 right.  The
 * kernels that produce these results write them there; a caller that owns the final containers (descriptors_dq / images_dq,
 * nn.cpp:154, 494-498) copies each of them ONCE, when it suits it.  The pointers stay valid until seven more submissions
 * have been made on this context (each submission owns one of eight sets of mirrors) or the context is destroyed. */
typedef struct {
  int n[2];
  const float *xy[2];
  const float *desc[2];
  const uint8_t *resized[2];
  int token;   /* the submission's set of mirrors (spvo_detect_mirrors_wait) */
} spvo_detect_mirrors;
int spvo_detect_collect_mirrors(spvo_ctx *ctx, double P_l[12], double P_r[12], spvo_detect_mirrors *out);
/* n, xy and resized are complete when spvo_detect_collect_mirrors returns.  The descriptors travel to their mirror BESIDE the
 * submission's matches (a copy kernel on a stream of its own: the matcher reads the device copy): desc[] may be read once this
 * call has returned.  A front end that fills descriptors_dq while the solver runs never waits here. */
int spvo_detect_mirrors_wait(spvo_ctx *ctx, const spvo_detect_mirrors *m);

typedef enum { SPVO_SELECT_NN = 0, SPVO_SELECT_KNN = 1 } spvo_selector;

/* matchDescriptors (base.cpp:434-491) = cv::BFMatcher(NORM_L2) match / knnMatch
 * k=2 + ratio test.  For every query row i: train_idx[i] = matched train row or
 * -1 (this is maps_of_indices, base.cpp:483-491) and distance[i] = L2 distance
 * of the matched pair (valid where train_idx[i] >= 0).  NN + cross_check
 * (base.cpp:27-28) is cv::batchDistance's crosscheck as BFMatcher runs it:
 * every train row votes for its nearest query row and a query row keeps the
 * nearest of its voters -- every mutual nearest-neighbour pair plus the pairs
 * that procedure adds; unmatched rows get -1.  KNN keeps i iff
 * d0 < ratio*d1 (base.cpp:469); with nb < 2 nothing is kept. */
int spvo_match(spvo_ctx *ctx, const float *desc_a, int na, const float *desc_b, int nb,
               int selector, int cross_check, float ratio, int32_t *train_idx, float *distance);

/* ------------------------------------------------------- classic front end: ORB
 * detectKeypoints + describeKeypoints of ClassicFeatureFrontEnd for DetectorType::ORB / DescriptorType::ORB
 * (feature_detection_classic.cpp:12-25, 66-68: cv::ORB::create(2000, 1.2f, 8, 31, 0, 2, FAST_SCORE, 31, 20)) on one 8-bit
 * image in host memory: 8-level pyramid, FAST-9 corners with non-maximum suppression, the best `nfeatures` split over the levels,
 * intensity-centroid direction, 256-bit steered BRIEF on the smoothed level.  OpenCV is not available to this build: the algorithm
 * is the published one as restated by oracle/cpu/orb_cpu.inc (its header lists the open choices and the one deviation, the
 * test-pair table) and the kernels reproduce that restatement bit for bit.  Keypoints come level by level, best response first,
 * in level-0 pixel coordinates; `n` receives their number (<= nfeatures), of which min(n, cap) are written. */
typedef struct {
  float x, y;        /* level-0 coordinates                                  */
  float angle;       /* radians, atan2 of the patch's intensity centroid      */
  float response;    /* FAST score                                            */
  int32_t octave;    /* pyramid level                                         */
} spvo_orb_keypoint;
int spvo_orb_detect(spvo_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, int nfeatures,
                    spvo_orb_keypoint *keypoints, uint8_t *descriptors /* [cap][32] */, int cap, int *n);
/* the tables the descriptor uses: 256 x (x1, y1, x2, y2) test pairs and the 7 smoothing taps (either may be NULL) */
int spvo_orb_tables(float *pattern /* [1024] */, float *taps /* [7] */);

/* detectKeypoints of ClassicFeatureFrontEnd for DetectorType::ShiTomasi (cv::GFTTDetector::create(1000, 0.03, 7.5, 5, false, 0.04),
 * feature_detection_classic.cpp:37-47) on one 8-bit image in host memory: 3x3 Sobel, 5x5 box sums of the gradient products (exact
 * integers), minimum eigenvalue, candidates above quality_level x the image's maximum that are 3x3 local maxima, then greedily, best
 * response first (of equals the later raster position first), every candidate that keeps min_distance from all kept ones, until
 * max_corners are kept (<= 0: no limit).  OpenCV is not available to this build: the algorithm is the published one with OpenCV's
 * tie and border rules as far as they are known, as restated by tests/classic_ref.py (its header lists the choices), and the kernels
 * reproduce that restatement bit for bit.  Only block_size = 5 and min_distance <= 15 are built, images of at least 8 x 8:
 * SPVO_ERR_INVALID otherwise.  Keypoints come in the order they were kept, integer coordinates as float; response = the minimum
 * eigenvalue in OpenCV's scale.  `n` receives their number, of which min(n, cap) are written.  The image stays on the device for
 * a spvo_orb_describe that follows. */
int spvo_gftt_detect(spvo_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, int max_corners, double quality_level,
                     double min_distance, int block_size, float *xy /* [cap][2] */, float *response /* [cap], may be NULL */, int cap,
                     int *n);
/* how the minimum-distance iteration of this context's last spvo_gftt_detect went: candidates still undecided after each of its
 * three grid-wide round launches, and the rounds the one-workgroup finish then took (0: it had nothing to do) */
int spvo_gftt_last_rounds(spvo_ctx *ctx, int *undecided_after_launch /* [3], may be NULL */, int *finish_rounds /* may be NULL */);

/* detectKeypoints for DetectorType::FAST (cv::FastFeatureDetector::create(10, true), feature_detection_classic.cpp:32-36): FAST-9/16
 * at `threshold` on the image itself (3-pixel border), response = the largest threshold at which the pixel is still a corner;
 * with nonmax_suppression a corner stays iff its response is strictly greater than all eight neighbours' (two equal neighbours
 * both go).  Raster order (row, then column), no cap: `n` receives the number found, of which min(n, cap) are written -- at most
 * (rows / 2 + 1) (cols / 2 + 1) with suppression, rows x cols without.  Status and conventions as spvo_gftt_detect. */
int spvo_fast_detect(spvo_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, int threshold, int nonmax_suppression,
                     float *xy /* [cap][2] */, float *response /* [cap], may be NULL */, int cap, int *n);

/* describeKeypoints for DescriptorType::ORB on keypoints the extractor did not detect itself (cv::ORB::create()->compute,
 * feature_detection_classic.cpp:66-68, 110-111), octave 0: keypoints closer than 31 pixels to a border are dropped, order-preserving
 * (`kept` receives the indices into xy that survived, ascending; `n_kept` their number); the others get spvo_orb_detect's direction
 * and 256-bit steered BRIEF on the 7x7-smoothed image -- the same kernels, so a keypoint that spvo_orb_detect reports on level 0
 * gets the same 32 bytes here.  Row i of `desc` / `angle` belongs to keypoint kept[i].  Coordinates must be integers (what both
 * detectors above return): SPVO_ERR_INVALID otherwise.  img = NULL: the image of this context's last spvo_gftt_detect /
 * spvo_fast_detect / spvo_orb_describe, still on the device (no second upload in the detect-then-describe sequence);
 * SPVO_ERR_STATE if none is resident or its shape is not rows x cols. */
int spvo_orb_describe(spvo_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, const float *xy /* [n][2] */, int n,
                      int32_t *kept /* [n] */, float *angle /* [n] rad, may be NULL */, uint8_t *desc /* [n][32] */, int *n_kept);

/* The same extractor on keypoints that carry an octave (cv::ORB::create()->compute on BRISK or AKAZE keypoints: KeyPoint::octave names
 * the pyramid level, scale 1.2^octave) at any coordinates.  OpenCV is not available to this build: the rule is OpenCV's as far as it is
 * known, as restated by tests/orb_octaves_ref.py (its header lists every choice), and the kernels reproduce that restatement bit for
 * bit.  The levels are spvo_orb_detect's (same scales, sizes and resize), built up to the largest octave named; of them only those that
 * hold a kept keypoint are smoothed.  The 31-pixel border rule is applied at LEVEL 0 to the coordinates rounded half to even; the kept
 * keypoints are grouped by octave, ascending, stable within an octave: `kept` receives the indices into xy in output order (ascending
 * only if the list was sorted by octave), `n_kept` their number, row i of `desc` / `angle` belongs to keypoint kept[i].  On its level a
 * keypoint lies at rint((x, y) / scale), clamped into the level; direction (always recomputed) and the 256 tests are spvo_orb_detect's
 * arithmetic on the same tables.  From level 3 on a kept keypoint can lie closer to its level's border than the patch reaches (15
 * pixels for the direction, at most 19 for a test point): the level and the smoothed level are then read at BORDER_REFLECT_101 indices
 * (OpenCV reflects the unsmoothed level into a padded border and smooths that: a documented deviation, like the test-pair table).  A
 * keypoint that spvo_orb_detect reports on any level, fed back with its x, y and octave, gets the same 32 bytes and the same direction;
 * a list at octave 0 with integer coordinates gets spvo_orb_describe's output.
 *   img == NULL   the u8 image left resident by this context's last spvo_gftt_detect / spvo_fast_detect / spvo_brisk_detect /
 *                 spvo_akaze_detect / spvo_*_describe (spvo_brisk_describe's rule); it stays resident
 *   img != NULL   img is uploaded first and stays resident
 * n == 0 is SPVO_OK with n_kept = 0.  Refusals are decided before anything on the device or in the outputs is touched:
 *   SPVO_ERR_INVALID   an octave outside 0..7, a coordinate that is not finite, n < 0, a named octave whose level is smaller than 32
 *                      pixels in either dimension (with that minimum one reflection always suffices)
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight; img == NULL and no image of that shape is resident */
int spvo_orb_describe_octaves(spvo_ctx *ctx, const uint8_t *img /* or NULL */, int rows, int cols, size_t stride,
                              const float *xy /* [n][2] */, const int32_t *octave /* [n] */, int n,
                              int32_t *kept /* [n] */, float *angle /* [n] rad, may be NULL */,
                              uint8_t *desc /* [n][32] */, int *n_kept);

/* describeKeypoints for DescriptorType::BRISK (cv::BRISK::create(30, 3, 1.0f)->compute, feature_detection_classic.cpp:56-65, 110-111) on
 * keypoints at any position and size: per keypoint the scale index from `size`, the border rule of that scale (dropped keypoints leave
 * the list, order-preserving: `kept` receives the surviving indices into xy, ascending, `n_kept` their number), the direction from
 * the 870 long pairs of 60 box-smoothed samples (always recomputed), and the 512 short-pair bits at that rotation.  OpenCV is not
 * available to this build: the algorithm is OpenCV's as far as it is known, as restated by tests/brisk_ref.py (its header lists every
 * choice), and the kernels reproduce that restatement bit for bit on the same tables.  Row i of `angle` / `desc` / `values0` belongs to
 * keypoint kept[i]; coordinates may be fractional; `values0` (test hook) receives the 60 intensities at rotation 0, which tells a wrong
 * descriptor's sampling from its pairs.  img = NULL: the image of this context's last spvo_gftt_detect / spvo_fast_detect /
 * spvo_orb_describe / spvo_brisk_describe, still on the device; SPVO_ERR_STATE if none is resident or its shape is not rows x cols.
 *   SPVO_ERR_INVALID   a size that is not finite and positive, rows * cols * 255 >= 2^31 (the integral image is int32), n < 0
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight
 * One-off cost: the point table (64 scales x 1024 rotations x 60 points x 3 floats = 47 MB) is built once per process on the host
 * and uploaded to a context on its first BRISK call (NOTES.md, "BRISK descriptor extractor": 61 ms and 8 ms measured); the
 * Shi-Tomasi / FAST keypoints of this front end (sizes 5 and 7) read only its 737 KB scale-0 slice.  The extractor's chain also runs
 * behind a detector's list on the device: spvo_classic_detect's BRISK kinds, spvo_brisk_detect_pair, spvo_akaze_brisk_pair,
 * spvo_orb_brisk_pair and spvo_sift_brisk_pair. */
int spvo_brisk_describe(spvo_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, const float *xy /* [n][2] */,
                        const float *size /* [n] */, int n, int32_t *kept /* [n] */, float *angle /* [n] degrees, may be NULL */,
                        uint8_t *desc /* [n][64] */, int32_t *values0 /* [n][60], may be NULL: test hook */, int *n_kept);
/* the tables the extractor uses (no context needed; every pointer may be NULL): the points of one scale, the pairs in descriptor bit
 * order, the 64 scales and their border sizes */
int spvo_brisk_tables(int scale, float *points /* [1024][60][3] x, y, sigma; may be NULL */, int32_t *short_pairs /* [512][2] i, j */,
                      int32_t *long_pairs /* [870][4] i, j, wdx, wdy */, float *scale_list /* [64] */, int32_t *size_list /* [64] */);

/* ------------------------------------------------------- classic front end: SIFT
 * detectKeypoints + describeKeypoints of ClassicFeatureFrontEnd for DetectorType::SIFT / DescriptorType::SIFT (cv::SIFT::create():
 * nfeatures 0, 3 layers per octave, contrast threshold 0.04, edge threshold 10, sigma 1.6) on one 8-bit image in host memory: 2x
 * upsampled base image (first octave -1), Gaussian / difference-of-Gaussians pyramid, 26-neighbour extrema, up to five sub-pixel
 * refinement steps, contrast and edge tests, one keypoint per peak of the 36-bin orientation histogram, 4 x 4 x 8 descriptor scaled
 * by 512 and saturated to 0..255 -- 128 INTEGERS stored as float (the only classic descriptor matched with NORM_L2, base.cpp:18-20:
 * spvo_match_l2).  OpenCV is not available to this build: the algorithm is Lowe 2004 with OpenCV 4.5.4's conventions as far as they
 * are known, as restated by tests/sift_ref.py (its header lists every choice).  The pyramid, the extrema and the refinement reproduce
 * that restatement bit for bit; orientation and descriptor use exp / atan2 and agree with it to rounding level.  Keypoints come in
 * OpenCV's total order (x, y, size, angle, response, octave ascending), records equal in (x, y, size, angle) once (the ordering runs on
 * the host, after one copy of the records; spvo_sift_detect_pair, below, orders on the device, and spvo_sift_brisk_pair runs the detector without its rows in front of the BRISK extractor).  `n` receives their number, of which min(n, cap) rows are written; strided input is accepted.
 *   SPVO_ERR_INVALID   an image smaller than 6 x 6 (the first octave of the doubled image needs an interior inside its 5-pixel border)
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight */
typedef struct {
  float x, y, size;
  float angle;       /* degrees, cv::KeyPoint convention                      */
  float response;    /* |contrast| of the refined extremum                    */
  int32_t octave;    /* OpenCV's packed (octave & 255) | layer << 8 | xi << 16 */
} spvo_sift_keypoint;
int spvo_sift_detect(spvo_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride,
                     spvo_sift_keypoint *kp, float *desc /* [cap][128] */, int cap, int *n);
/* A level of the pyramid of this context's last spvo_sift_detect (test hook): Gaussian layer 0..5, or with `dog` difference layer 0..4,
 * of octave 0.. (octave 0 is the doubled image).  `out` (rows x cols floats) may be NULL to ask for the shape only.  It also serves the
 * Gaussian-only pyramid of the last spvo_sift_describe, below: octave index 0 is then that call's first octave (the doubled image only if
 * the list held an octave -1, else the image at its own size), and dog = 1 is SPVO_ERR_STATE. */
int spvo_sift_debug_level(spvo_ctx *ctx, int octave, int layer, int dog, float *out, int *rows, int *cols);
/* describeKeypoints for DescriptorType::SIFT on keypoints the extractor did not detect itself (cv::SIFT::create()->compute,
 * feature_detection_classic.cpp:71-73, 110-111: SIFT::detectAndCompute with useProvidedKeypoints) -- what ShiTomasi / FAST / ORB / BRISK /
 * AKAZE + SIFT run.  OpenCV is not available to this build: the rule is OpenCV 4.5.4's as far as it is known, as restated by
 * tests/sift_describe_ref.py (its header lists every choice).  Per record the packed `octave` field gives o = its low byte, sign-extended,
 * and layer = its second byte (a detector that leaves octave = 0 gets octave 0, layer 0); the Gaussian pyramid is built for the octaves
 * min(0, min o) .. max o -- from the doubled image only if some o is -1, else from the image at its own size blurred once with
 * sqrt(1.6^2 - 0.5^2) -- with spvo_sift_detect's taps, pass rule and decimation and no difference of Gaussians, bit for bit the
 * restatement's; the descriptor is spvo_sift_detect's (the same device code per sample) at the point (x, y) / 2^o rounded half to even on
 * layer `layer` of octave o, with scale size / 2^o / 2 and orientation 360 - angle (angle = -1, which detectors without an orientation
 * report, is legal).  No keypoint is erased and none is re-ordered: row i of `desc` belongs to record i; a patch without a valid sample
 * gives a row of zeros.  The sums take no float atomics and a fixed order: one image and list always give the same bytes.
 *   img == NULL   the u8 image left resident by this context's last spvo_gftt_detect / spvo_fast_detect / spvo_brisk_detect /
 *                 spvo_akaze_detect / spvo_orb_describe / spvo_brisk_describe / spvo_sift_describe(img) (spvo_brisk_describe's rule;
 *                 spvo_orb_detect and spvo_sift_detect keep images of their own and leave none there)
 *   img != NULL   img is uploaded first and stays resident
 * n == 0 is SPVO_OK.  Runs on the solver's stream; scratch lives in the context and grows on shape change.
 *   SPVO_ERR_INVALID   nothing is written, uploaded or replaced: a record whose x, y, size or angle is not finite or whose size is not
 *                      positive, an unpacked octave < -1, a layer > 5, an octave whose level would be empty (min(rows, cols) >> o < 1)
 *                      or more than 16 octaves, an image spvo_sift_detect refuses
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight; img == NULL and no image of that shape is resident */
int spvo_sift_describe(spvo_ctx *ctx, const uint8_t *img /* or NULL */, int rows, int cols, size_t stride,
                       const spvo_sift_keypoint *kp, int n, float *desc /* [n][128] */);

/* detectKeypoints for DetectorType::BRISK (cv::BRISK::create() -> detect, feature_detection_classic.cpp:9-11: threshold 30, 3 octaves, pattern
 * scale 1) on one 8-bit image in host memory: the six-layer scale space (layer 1 = two-thirds of the image, layer i >= 2 = half of layer
 * i - 2, cv::resize(INTER_AREA)'s arithmetic), the dense AGAST 9-16 score of every layer (the largest b at which the FAST-9/16 segment test
 * still holds: one less than spvo_fast_detect's response) and the 5-8 score of the image for the virtual layer below it, candidates with
 * score >= threshold that pass isMax2D, and per candidate refine3D (the top layer: getScoreMaxBelow and its own 3 x 3 patch): sub-pixel
 * position, continuous scale between the layers, refined score; kept iff that score > threshold (the top layer keeps all).  OpenCV is not
 * available to this build: the algorithm is OpenCV 4.x's as far as it is known, as restated by tests/brisk_detect_ref.py (its header lists
 * every choice -- among them that a score read is a pure function of the layer, where OpenCV's depends on what earlier keypoints left in
 * its cache), and the kernels reproduce that restatement bit for bit in every field.  A record is (x, y, size = 12 * scale, angle = -1,
 * response = refined score, octave = layer 0..5); keypoints come layer by layer, within a layer in raster order of the candidate.  `n`
 * receives their number, of which min(n, cap) are written; strided input is accepted; a layer too small to have an interior contributes
 * nothing.  The image stays on the device for a spvo_brisk_describe(img = NULL) that follows, exactly as after spvo_fast_detect.
 *   SPVO_ERR_INVALID   threshold outside 1 .. 255; octaves != 3 (only the reference's six layers are built); an image smaller than 8 x 8;
 *                      rows * cols * 255 >= 2^31 (so that the spvo_brisk_describe that follows cannot fail on its int32 integral image)
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight; the candidate list overflowed (it holds one entry per interior pixel of every
 *                      layer, so this reports a defect, not an input) */
typedef spvo_sift_keypoint spvo_brisk_keypoint;
int spvo_brisk_detect(spvo_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, int threshold, int octaves,
                      spvo_brisk_keypoint *kp /* [cap] */, int cap, int *n);
/* A layer of the scale space of this context's last spvo_brisk_detect (test hook): what = 0 the layer's image, 1 its AGAST 9-16 score map,
 * 2 (layer 0 only) the 5-8 score map.  `out` (rows x cols bytes) may be NULL to ask for the shape only.  SPVO_ERR_STATE when no result is
 * resident: no call yet, or any other call has since put an image into the context's resident image buffer (spvo_gftt_detect,
 * spvo_fast_detect, spvo_orb_describe / spvo_brisk_describe / spvo_sift_describe with an image, spvo_classic_detect, spvo_brisk_detect_pair,
 * spvo_akaze_detect_pair), the same image
 * included. */
int spvo_brisk_detect_debug_layer(spvo_ctx *ctx, int layer, int what, uint8_t *out, int *rows, int *cols);

/* detectKeypoints for DetectorType::AKAZE (cv::AKAZE::create() -> detect, feature_detection_classic.cpp:26-28: 4 octaves of 4 sublevels,
 * PM_G2 diffusivity, soffset 1.6, derivative factor 1.5, contrast percentile 0.7 over 300 bins, floor min_dthreshold 1e-5) on one 8-bit image
 * in host memory: the nonlinear scale space (level 0 = the image / 255 blurred with sigma 1.6; every further level = the level before --
 * half-sampled with cv::resize(INTER_AREA)'s arithmetic on a new octave -- diffused by its Fast Explicit Diffusion steps under the
 * conductivity of its own sigma 1 blur), the scale-normalised Hessian determinant of every level, the candidates (above the threshold,
 * strict 8-neighbour maxima, inside the descriptor border of their level) and their sub-pixel offsets on the device; the order-dependent
 * suppression between candidates of the same and of neighbouring levels on the host, over the copied list.  Only the detector: the
 * orientation and the MLDB descriptor are spvo_akaze_describe's (OpenCV computes both in compute), so `angle` is 0 as detect leaves it.  OpenCV is not
 * available to this build: the algorithm is OpenCV's as far as it is known, as restated by tests/akaze_ref.py (its header lists every rule
 * and marks what is a decision of this project; it mixes OpenCV generations on purpose: 4.x's sigma_size^4 factor on the determinant, 3.x's
 * reflect-101 blur border and sequential suppression), and the kernels reproduce that restatement bit for bit in every plane and in every field
 * of a record: x, y, size = 2 * 1.5 * esigma, angle = 0, response = Ldet, octave, class_id = level 0 .. 15.  Keypoints come in the order
 * the suppression leaves them.  `n` receives their number, of which min(n, cap) are written; strided input is accepted.  The image stays on
 * the device for a spvo_brisk_describe(img = NULL) that follows, exactly as after spvo_fast_detect and spvo_brisk_detect, and the scale
 * space for a spvo_akaze_describe(img = NULL).
 *   SPVO_ERR_INVALID   a threshold that is not finite and positive; an image smaller than 16 x 16; rows * cols * 255 >= 2^31 (so that the
 *                      spvo_brisk_describe that follows cannot fail on its int32 integral image)
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight; the candidate list overflowed (it is sized from the image, so this reports a
 *                      defect, not an input) */
typedef struct { float x, y, size, angle, response; int32_t octave, class_id; } spvo_akaze_keypoint;
int spvo_akaze_detect(spvo_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, float threshold,
                      spvo_akaze_keypoint *kp /* [cap] */, int cap, int *n);
/* A level of the scale space of this context's last spvo_akaze_detect (test hook): what = 0 Lt, 1 Lsmooth, 2 Lflow (zeros on level 0, which
 * has none), 3 Ldet.  `out` (rows x cols floats) may be NULL to ask for the shape only.  SPVO_ERR_INVALID for a level the image does not
 * have; SPVO_ERR_STATE when no result is resident: no call yet, or any other call has since put an image into the context's resident
 * image buffer, the same image included, or a spvo_sift_detect / spvo_sift_detect_pair has run since (SIFT keeps an image of its own,
 * but the last detector call owns what is resident). */
int spvo_akaze_debug_level(spvo_ctx *ctx, int level, int what, float *out, int *rows, int *cols);
/* The contrast factor k of every octave of the last spvo_akaze_detect, as the kernels left it in device memory.  SPVO_ERR_STATE as above. */
int spvo_akaze_last_contrast(spvo_ctx *ctx, float *k /* [4], per octave */, int *octaves);
/* The detector's tables for a rows x cols image (no context, no device): per level its octave, esigma and sigma_size (up to 16 levels),
 * the number of diffusion steps of each of the levels - 1 transitions and their sizes one transition after the other (`n_tau` receives
 * their number, min(n_tau, tau_cap) are written), the centre and the taps of one side of the Gaussian kernels of sigma 1.6 (g0, 5 floats)
 * and sigma 1 (g1, 3 floats).  Every array may be NULL.  SPVO_ERR_INVALID for an image smaller than 16 x 16. */
int spvo_akaze_tables(int rows, int cols, int *levels, int32_t *octave, float *esigma, int32_t *sigma_size, int32_t *nsteps, float *tau, int tau_cap,
                      int *n_tau, float *g0, float *g1);
/* describeKeypoints for DescriptorType::AKAZE (cv::AKAZE::create() -> compute, feature_detection_classic.cpp:69-70) on AKAZE keypoints: per
 * record the main orientation (Compute_Main_Orientation: 109 Gaussian-weighted samples of the level's scaled first derivatives, their angle
 * by fastAtan32f's polynomial, 42 sliding windows of pi / 3) and the full MLDB descriptor (pattern size 10, 3 channels: the mean of Lt and of
 * the rotated derivatives over the cells of a 2 x 2, a 3 x 3 and a 4 x 4 grid, every pair of cells compared: 486 bits in
 * SPVO_AKAZE_DESC_BYTES = 61 bytes, bits 6 and 7 of the last byte zero), one wave per keypoint in one launch.  The level is the record's
 * class_id, as OpenCV requires.  No keypoint is dropped: `angle` receives n angles in degrees (0 .. 360; the angle that came in is ignored),
 * `desc` n rows, for spvo_match_hamming with desc_bytes = 61.  OpenCV is not available to this build: the definition is
 * tests/akaze_mldb_ref.py (its header lists every rule and marks what is a decision of this project -- chiefly that the grid is rotated by
 * the winning window's normalised direction itself and not by cos / sin of its approximate angle, and that a sample outside the plane
 * reads zero in the orientation and is skipped in the descriptor), which uses no transcendental function, and the kernel reproduces it
 * bit for bit in every angle and every byte.
 *   img == NULL   on the scale space left resident by this context's last spvo_akaze_detect or spvo_akaze_describe(img) of a rows x cols
 *                 image (spvo_akaze_debug_level's rule of validity)
 *   img != NULL   the scale space of img is built first, by spvo_akaze_detect's own chain without its extrema, and stays resident
 * n == 0 is SPVO_OK (with an image, its scale space is still built).
 *   SPVO_ERR_INVALID   nothing is written, uploaded or replaced: a record whose class_id is no level of a rows x cols image, whose octave is
 *                      not that level's, whose x, y or size is not finite or whose size is not positive; an image smaller than 16 x 16
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight (outputs and the resident result stay as they were); img == NULL and no scale
 *                      space of that shape is resident */
#define SPVO_AKAZE_DESC_BYTES 61
int spvo_akaze_describe(spvo_ctx *ctx, const uint8_t *img /* or NULL */, int rows, int cols, size_t stride,
                        const spvo_akaze_keypoint *kp, int n, float *angle /* [n], degrees */, uint8_t *desc /* [n * 61] */);

/* ------------------------------------------------------- classic front end: one submission per stereo pair, features resident
 * detectKeypoints + describeKeypoints of ClassicFeatureFrontEnd for BOTH images of a stereo pair in one call: ORB, or Shi-Tomasi /
 * FAST followed by the ORB extractor or by the BRISK extractor (the five pairs the per-image entry points above cover).  Both images go up through pinned
 * staging, the whole chain of both is enqueued without a host round trip -- for the two non-ORB kinds the keypoints go from the
 * detector to the extractor on the device, the extractor's border rule being an order-preserving compaction there -- and the call
 * waits once for the result, the features (before that, for whatever an earlier call left running on the solver's stream: its staging is reused).  They are left in two BINARY FEATURE SLOTS (0 .. 9; separate from the float slots of spvo_detect*,
 * used as a ring of pairs like those): keypoint records, descriptor rows (32 bytes; 64 for the two BRISK kinds; 61 for
 * spvo_akaze_detect_pair, stored in 64 -- a slot remembers its row width) and the row count stay on the device for spvo_match_hamming_slots.  What the host receives equals, byte for byte, what spvo_orb_detect -- or spvo_gftt_detect /
 * spvo_fast_detect followed by spvo_orb_describe(img = NULL) -- returns for the same image and parameters; for the two non-ORB kinds a
 * record carries the extractor's angle (radians), the DETECTOR's response and octave 0.
 * The two BRISK kinds (SPVO_CLASSIC_GFTT_BRISK, SPVO_CLASSIC_FAST_BRISK): the detector's list stays on the device, the BRISK border rule
 * for keypoints of size 5 (Shi-Tomasi) / 7 (FAST) is an order-preserving compaction there, and the host receives, byte for byte, what
 * spvo_gftt_detect / spvo_fast_detect followed by spvo_brisk_describe(img = NULL, size = 5 / 7) returns with `kept` applied to the
 * detector's xy and response: desc is [cap][64], a record carries the extractor's angle in DEGREES (0 .. 360, spvo_brisk_describe's
 * float), the detector's x, y and response, octave 0.  Their first call in a context uploads the BRISK tables (spvo_brisk_describe).
 *   SPVO_ERR_CAPACITY  an image yields more rows than slot_capacity: out_*->n report the counts, both slots are left unfilled
 *                      (nothing is truncated: a shortened FAST list would not be the reference's)
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight
 * (all ten slots share one allocation size, for 64-byte rows whatever kind comes first: a call with a larger slot_capacity than any
 * before re-allocates and EMPTIES every slot; a change of kind does not)
 *   SPVO_ERR_INVALID   bad or equal slots, slot_capacity outside 1 .. 2^22, sizes / parameters the per-image entry points refuse (for the
 *                      BRISK kinds also rows * cols * 255 >= 2^31: the int32 integral image)
 * With spvo_set_prematch enabled the two standard matches (slot_l -> slot_r, slot_l -> the previous call's slot_l) are enqueued in the
 * same submission behind the features; the call does not wait for them.  A previous left slot of the other row width has no temporal
 * match: it is skipped, not an error (so is a slot of 61-byte rows that spvo_akaze_detect_pair filled). */
/* (kinds 5 and 6, Shi-Tomasi / FAST keypoints with SIFT descriptors, are spvo_classic_sift_pair's, below the SIFT slots: their rows are 128
 * floats, which spvo_classic_features and the binary slots do not hold.  spvo_classic_detect answers SPVO_ERR_INVALID for them.) */
typedef enum { SPVO_CLASSIC_ORB = 0, SPVO_CLASSIC_GFTT_ORB = 1, SPVO_CLASSIC_FAST_ORB = 2, SPVO_CLASSIC_GFTT_BRISK = 3, SPVO_CLASSIC_FAST_BRISK = 4,
               SPVO_CLASSIC_GFTT_SIFT = 5, SPVO_CLASSIC_FAST_SIFT = 6 } spvo_classic_kind;
typedef struct {
  int kind;                               /* spvo_classic_kind */
  int nfeatures;                          /* ORB [2000] */
  int max_corners; double quality_level, min_distance; int block_size;   /* GFTT [1000, 0.03, 7.5, 5] */
  int fast_threshold, fast_nonmax;        /* FAST [10, 1] */
  int slot_capacity;                      /* rows a slot can hold [8192] */
} spvo_classic_opts;
/* the reference's parameters (feature_detection_classic.cpp:12-47) for `kind` */
void spvo_default_classic_opts(spvo_classic_opts *o, int kind);
typedef struct { int n; spvo_orb_keypoint *kp; uint8_t *desc; int cap; } spvo_classic_features;  /* n: out; min(n, cap) rows are written; desc ([cap][32]; [cap][64] for the BRISK kinds), kp may be NULL */
int spvo_classic_detect(spvo_ctx *ctx, const spvo_classic_opts *opts, const uint8_t *img_l, const uint8_t *img_r,
                        int rows, int cols, size_t stride, int slot_l, int slot_r,
                        spvo_classic_features *out_l, spvo_classic_features *out_r);
/* The same for BRISK keypoints with BRISK descriptors (detectKeypoints + describeKeypoints of ClassicFeatureFrontEnd(BRISK, BRISK) for both
 * images of a stereo pair): an entry point of its own, because a BRISK keypoint carries a size and spvo_classic_features' 20-byte records
 * have no room for one.  It fills the same ring of ten BINARY slots with 64-byte rows, so spvo_match_hamming_slots, spvo_classic_slot_rows
 * and spvo_set_prematch serve it as they serve spvo_classic_detect, and the temporal partner is shared with that call: any filled slot of
 * 64-byte rows is one, a 32-byte or a 61-byte one is skipped.  Both images go up through the pinned staging; per image the detector's chain, ONE
 * order-preserving compaction that applies the detector's keep flag and the extractor's border rule at every keypoint's OWN scale index,
 * the extractor and a finishing kernel are enqueued without a host round trip, and the call waits once.  Per image the host receives, byte
 * for byte, what spvo_brisk_detect(img, threshold, octaves) followed by spvo_brisk_describe(img = NULL, the x, y and size of those
 * keypoints) returns: a record is the detector's with `kept` applied -- x, y, size, response and octave = layer unchanged -- and `angle`
 * replaced by the extractor's (degrees, 0 .. 360); desc holds the extractor's rows in the detector's order; out->n is the number that
 * survived the border rule.  The slot's own record array holds (x, y, that angle, response, layer).
 * Afterwards the context's resident image is the RIGHT one: spvo_brisk_describe(img = NULL) works on it, and spvo_brisk_detect_debug_layer
 * answers SPVO_ERR_STATE.  The first BRISK call of a context uploads the tables (spvo_brisk_describe).
 *   SPVO_ERR_INVALID   NULL arguments, cap < 0, bad or equal slots, slot_capacity outside 1 .. 2^22, whatever spvo_brisk_detect refuses
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight; the candidate list overflowed (a defect, not an input: spvo_brisk_detect)
 *   SPVO_ERR_CAPACITY  an image yields more rows than slot_capacity: out_*->n report both counts, both slots are left unfilled, nothing
 *                      is truncated (spvo_classic_detect's rule; so is the re-allocation by a larger slot_capacity than any before) */
typedef struct { int n; spvo_brisk_keypoint *kp; uint8_t *desc /* [cap][64] */; int cap; } spvo_brisk_features;   /* n: out; min(n, cap) rows are written; kp, desc may be NULL */
int spvo_brisk_detect_pair(spvo_ctx *ctx, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride,
                           int threshold, int octaves, int slot_l, int slot_r, int slot_capacity,
                           spvo_brisk_features *out_l, spvo_brisk_features *out_r);
/* The same for AKAZE keypoints with AKAZE descriptors (detectKeypoints + describeKeypoints of ClassicFeatureFrontEnd(AKAZE, AKAZE) for both
 * images of a stereo pair).  It fills the same ring of ten BINARY slots with 61-byte rows: a slot stores such a row in the 16 words the
 * matcher's wide kernel reads, bytes 61 .. 63 zero, which changes no distance, and remembers the width 61.  spvo_match_hamming_slots,
 * spvo_classic_slot_rows and spvo_set_prematch serve it as they serve spvo_classic_detect; the temporal partner is any filled slot of
 * 61-byte rows, a slot of another width (ORB's 32, BRISK's 64) is skipped.  Both images go up through the pinned staging; per image the
 * scale space and the candidates of spvo_akaze_detect, the order-dependent suppression between candidates ON THE DEVICE (one wave walks
 * the candidates in order and scans the list by ballots, one thread per entry runs the second pass, an order-preserving compaction keeps
 * the survivors whose offsets passed), spvo_akaze_describe's kernel on those records with the count read on the device, and a finishing
 * kernel are enqueued without a host round trip, left image first, and the call waits once.  Per image the host receives, byte for byte,
 * what spvo_akaze_detect(img, threshold) followed by spvo_akaze_describe(img = NULL, those keypoints) returns: the records in the
 * detector's order with `angle` replaced by the descriptor's (degrees), the packed 61-byte rows; out->n is the count, of which
 * min(n, cap) rows are written.  The slot's own record array holds (x, y, that angle, response, level).
 * Afterwards the context's resident image and scale space are the RIGHT image's: spvo_akaze_describe(img = NULL),
 * spvo_brisk_describe(img = NULL), spvo_akaze_debug_level and spvo_akaze_last_contrast answer for it.
 * The suppression is quadratic in the candidates in the worst case, as spvo_akaze_detect's host loop is.
 *   SPVO_ERR_INVALID   NULL arguments, cap < 0, bad or equal slots, slot_capacity outside 1 .. 2^22, whatever spvo_akaze_detect refuses
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight (outputs and slots stay as they were); the candidate list overflowed (a
 *                      defect, not an input: spvo_akaze_detect)
 *   SPVO_ERR_CAPACITY  an image yields more rows than slot_capacity: out_*->n report both counts, both slots are left unfilled, nothing
 *                      is truncated (spvo_classic_detect's rule; so is the re-allocation by a larger slot_capacity than any before) */
typedef struct { int n; spvo_akaze_keypoint *kp; uint8_t *desc /* [cap][61] */; int cap; } spvo_akaze_features;   /* n: out; min(n, cap) rows are written; kp, desc may be NULL */
int spvo_akaze_detect_pair(spvo_ctx *ctx, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride,
                           float threshold, int slot_l, int slot_r, int slot_capacity,
                           spvo_akaze_features *out_l, spvo_akaze_features *out_r);
/* The device suppression of spvo_akaze_detect_pair on a caller's candidate list (test hook: images do not reach a slot replaced twice,
 * a removal by the second pass or a candidate whose offsets failed): exactly those kernels, for the level tables of a rows x cols image
 * and no image.  `cand` lists the candidates as the detector would, level by level; `keep` receives the indices of those that stay, in
 * output order, `n_keep` their number (a candidate with ok = 0 suppresses others and is dropped at the end).  A resident scale space is
 * not touched.  SPVO_ERR_INVALID for a level the shape does not have, for levels that are not non-decreasing along the list and for a
 * shape smaller than 16 x 16; SPVO_ERR_STATE beside a spvo_detect*_submit in flight. */
typedef struct { int32_t level, row, col; float response; int32_t ok; } spvo_akaze_candidate;
int spvo_akaze_suppress_debug(spvo_ctx *ctx, int rows, int cols, const spvo_akaze_candidate *cand, int n,
                              int32_t *keep /* [n] */, int *n_keep);
/* The three binary pairs whose detector reports an octave and whose extractor is another algorithm's, pair-resident: BRISK + ORB,
 * AKAZE + ORB (both with the octave-aware ORB extractor of spvo_orb_describe_octaves) and AKAZE + BRISK.  Each follows
 * spvo_brisk_detect_pair / spvo_akaze_detect_pair in protocol -- the pinned staging, the left image's chain then the right's on the
 * solver's stream, one wait, the ring of ten BINARY slots, spvo_match_hamming_slots, spvo_classic_slot_rows, spvo_set_prematch,
 * SPVO_ERR_CAPACITY with both counts and both slots left unfilled, re-allocation by a larger slot_capacity than any before -- and the
 * temporal partner is any filled slot of the same row width: a slot of 32-byte rows that spvo_classic_detect(ORB / GFTT+ORB / FAST+ORB)
 * filled partners with an ORB pair's, a slot spvo_brisk_detect_pair filled with spvo_akaze_brisk_pair's; another width is skipped.
 * Afterwards the resident image (AKAZE: and the scale space) is the RIGHT image's.  Per image the host receives, byte for byte:
 *   spvo_brisk_orb_pair    spvo_brisk_detect(img, threshold, octaves), then spvo_orb_describe_octaves(img = NULL, its x, y, octave):
 *                          the records kp[kept] with `angle` = the extractor's radians, the 32-byte rows in `kept` order, n = n_kept
 *   spvo_akaze_orb_pair    spvo_akaze_detect(img, threshold), then the same
 *   spvo_akaze_brisk_pair  spvo_akaze_detect(img, threshold), then spvo_brisk_describe(img = NULL, its x, y, size): the records kp[kept]
 *                          with `angle` = the extractor's degrees, class_id and octave unchanged, the 64-byte rows
 * The slot's own records hold (x, y, that angle, response, octave).  The ORB pairs replace the host steps of spvo_orb_describe_octaves by
 * a link on the device: one workgroup reads the detector's list where it lies (BRISK: the keep flag applies), applies the border rule at
 * level 0 and groups the survivors by octave, stable, in two walks; levels 1 .. max_octave are built and levels 0 .. max_octave smoothed
 * whether a keypoint names them or not (max_octave: 5 for BRISK, the octave of the shape's last level for AKAZE -- the host does not know
 * the counts); the describe kernel reads the row count on the device.  spvo_akaze_brisk_pair presents the records the suppression kept to
 * spvo_brisk_detect_pair's compaction, describe and finishing launches.
 *   SPVO_ERR_INVALID   what the sibling refuses (spvo_brisk_orb_pair: octaves != 3 too); the ORB pairs: level max_octave of the shape is
 *                      smaller than 32 in a dimension (the text names the level and its size) -- in the place of the per-keypoint
 *                      refusal of spvo_orb_describe_octaves, which the host can no longer evaluate.  Decided before anything is touched.
 *   SPVO_ERR_STATE, SPVO_ERR_CAPACITY  as the siblings */
int spvo_brisk_orb_pair(spvo_ctx *ctx, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride,
                        int threshold, int octaves, int slot_l, int slot_r, int slot_capacity,
                        spvo_brisk_features *out_l, spvo_brisk_features *out_r);   /* desc [cap][32] */
int spvo_akaze_orb_pair(spvo_ctx *ctx, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride,
                        float threshold, int slot_l, int slot_r, int slot_capacity,
                        spvo_akaze_features *out_l, spvo_akaze_features *out_r);   /* desc [cap][32] */
int spvo_akaze_brisk_pair(spvo_ctx *ctx, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride,
                          float threshold, int slot_l, int slot_r, int slot_capacity,
                          spvo_akaze_features *out_l, spvo_akaze_features *out_r);   /* desc [cap][64] */
/* The ORB pairs' device link and describe kernel on a caller's list against the image already resident (test hook: images do not reach
 * octaves that do not ascend along the list, octaves 6 and 7, or keep flags between survivors).  No detector runs, no slot is touched, the
 * image stays resident.  The outputs equal spvo_orb_describe_octaves(img = NULL) on the list without its keep == 0 records (keep = NULL:
 * all take part), with `kept` naming the original indices.  SPVO_ERR_INVALID for max_octave outside 0 .. 7, an octave outside
 * 0 .. max_octave, a coordinate that is not finite, and a level max_octave smaller than 32 in a dimension; SPVO_ERR_STATE without a
 * resident image of that shape or beside a spvo_detect*_submit in flight. */
int spvo_orb_octaves_link_debug(spvo_ctx *ctx, int rows, int cols, const float *xy /* [n][2] */, const int32_t *octave /* [n] */,
                                const uint8_t *keep /* [n] or NULL */, int n, int max_octave,
                                int32_t *kept /* [n] */, float *angle /* [n], may be NULL */, uint8_t *desc /* [n][32] */, int *n_kept);
/* rows a binary feature slot holds; SPVO_ERR_STATE for one that holds nothing (never filled, or left unfilled by SPVO_ERR_CAPACITY) */
int spvo_classic_slot_rows(spvo_ctx *ctx, int slot, int *n);
/* Caller-supplied rows into a binary slot (test hook: images cannot produce the rows the matcher's key layout has to survive --
 * distance 512, exact ties): n rows (0 .. the current slot capacity; slots not allocated yet are allocated at the default 8192) of
 * desc_bytes = 32 or 64 bytes are uploaded, the records are zeroed, the slot is marked filled with that row width, its generation is
 * bumped and stored prematch results are dropped.  SPVO_ERR_INVALID for any other width or count, SPVO_ERR_STATE beside a
 * spvo_detect*_submit in flight. */
int spvo_classic_slot_fill_debug(spvo_ctx *ctx, int slot, const uint8_t *desc /* [n][desc_bytes] */, int n, int desc_bytes /* 32 or 64 */);

/* spvo_match for rows of `dim` floats (1 .. 256; SIFT: 128): the rows are zero-padded to the 256 columns the matcher's kernels are
 * built for while they are uploaded, which changes no distance.  dim = 256 returns exactly what spvo_match returns.  Rows of integers
 * <= 255 (SIFT) have squared distances below 2^24: every distance is exact in float in any summation order, and so are the matches. */
int spvo_match_l2(spvo_ctx *ctx, const float *desc_a, int na, const float *desc_b, int nb, int dim,
                  int selector, int cross_check, float ratio, int32_t *train_idx, float *distance);

/* The same for BINARY descriptors: cv::BFMatcher(NORM_HAMMING), what initMatcher (base.cpp:17-21) builds for the ORB / BRISK /
 * AKAZE descriptors of ClassicFeatureFrontEnd (classic.cpp:66-79) and matchDescriptors (base.cpp:434-500) runs on them.
 * Rows of `desc_bytes` bytes (ORB 32, BRISK 64, AKAZE 61; at most 64), distance = number of differing bits (exact), reported
 * as a float like cv::DMatch::distance; selector / cross_check / ratio and the meaning of train_idx / distance as in
 * spvo_match. */
int spvo_match_hamming(spvo_ctx *ctx, const uint8_t *desc_a, int na, const uint8_t *desc_b, int nb, int desc_bytes,
                       int selector, int cross_check, float ratio, int32_t *train_idx, float *distance);

/* Same on the device-resident descriptors of two feature slots. */
int spvo_match_slots(spvo_ctx *ctx, int slot_a, int slot_b, int selector, int cross_check,
                     float ratio, int32_t *train_idx, float *distance);

/* spvo_match_hamming on the device-resident rows of two BINARY feature slots (spvo_classic_detect): nothing is packed or uploaded,
 * the kernel reads both row counts on the device.  Results equal spvo_match_hamming on the host copies of the two slots, index for
 * index and distance for distance.  Returns the result stored by spvo_classic_detect when spvo_set_prematch is on and this is exactly
 * that match of exactly those slot contents.  Two slots of rows wider than 32 bytes (BRISK's 64, AKAZE's 61 with three zero bytes behind) are matched by the same kernel built for rows
 * of 16 words; slots of different widths (a 61-byte slot against a 64-byte one included): SPVO_ERR_INVALID, the message names both.  SPVO_ERR_STATE for a slot that holds nothing; spvo_match_slots on a binary slot number
 * means the FLOAT slot of that number, as before. */
int spvo_match_hamming_slots(spvo_ctx *ctx, int slot_a, int slot_b, int selector, int cross_check, float ratio,
                             int32_t *train_idx, float *distance);

/* MatcherType::FLANN on BINARY descriptors.  The reference's matchDescriptors converts both descriptor matrices to CV_32F and hands them
 * to cv::FlannBasedMatcher (base.cpp:29-32, 444-451): an L2 search over the descriptor BYTES taken as numbers 0 .. 255 -- not a Hamming
 * search -- through two randomized KD-trees, approximate and not reproducible.  This library computes what those trees approximate: the
 * EXACT L2 nearest neighbours, oracle/matching.py's bf_match on the rows cast to float32, index for index and distance for distance as
 * bits (squared distances <= 64 * 255^2 < 2^24 are exact integers; distance = sqrtf of them).  Parity with cv::FlannBasedMatcher is
 * therefore unpinned.  Arguments, the 1 .. 64-byte limit, empty sides, stream and buffers as spvo_match_hamming; selector / cross_check /
 * ratio as in spvo_match (FLANN itself has no cross-check: the host front end passes 0).  Equals spvo_match_l2 on the float casts. */
int spvo_match_l2_u8(spvo_ctx *ctx, const uint8_t *desc_a, int na, const uint8_t *desc_b, int nb, int desc_bytes,
                     int selector, int cross_check, float ratio, int32_t *train_idx, float *distance);
/* spvo_match_l2_u8 on the device-resident rows of two binary slots, counts read on the device; the rules of spvo_match_hamming_slots
 * (widths, unfilled slots, their messages).  Returns the result a pair call stored when spvo_set_prematch is on, the prematch norm is
 * SPVO_NORM_L2 and this is exactly that match of exactly those slot contents; computes on the spot otherwise. */
int spvo_match_l2_u8_slots(spvo_ctx *ctx, int slot_a, int slot_b, int selector, int cross_check, float ratio,
                           int32_t *train_idx, float *distance);
/* Which matcher the binary pair calls (spvo_classic_detect, spvo_brisk_detect_pair, spvo_akaze_detect_pair and their variants) enqueue
 * behind their features under spvo_set_prematch: SPVO_NORM_HAMMING (the default: spvo_match_hamming_slots is served) or SPVO_NORM_L2
 * (spvo_match_l2_u8_slots is served).  A stored result is served only to a query of the norm that produced it; changing the norm drops
 * the stored results.  SPVO_ERR_INVALID for any other value. */
typedef enum { SPVO_NORM_HAMMING = 0, SPVO_NORM_L2 = 1 } spvo_binary_norm;
int spvo_set_binary_prematch_norm(spvo_ctx *ctx, int norm);

/* ------------------------------------------------------- SIFT: one submission per stereo pair, features resident
 * spvo_sift_detect for BOTH images of a stereo pair in one call.  Both images go up through pinned staging; the chain -- the left image's
 * pyramid, features and ORDERING, then the right image's, the one resident pyramid reused in stream order -- is enqueued on the solver's
 * stream and the call waits once (before that, for whatever an earlier call left running there: its staging is reused).  The ordering
 * and the duplicate removal run on the device (key, rank by counting, order-preserving compaction, gather), so the features stay in two
 * SIFT FEATURE SLOTS (0 .. 9; a third ring, separate from the float and the binary slots): descriptor rows in the L2 matcher's format
 * (256 floats, columns 128.. zero), their squared norms and the row count, for spvo_match_l2_slots.
 *   Byte equality: what the host receives equals, byte for byte in every field and every descriptor, what spvo_sift_detect returns for
 *   the same image.  The records are built on the host, by the function spvo_sift_detect uses, from the {candidate, offsets, angle} the
 *   device hands over per final row.  The `size` the device computes (a double pow) is a sort key only; rows of one candidate get
 *   identical keys on the device as on the host, so ties and duplicates are preserved.
 * All slots are sized by the largest slot_capacity seen (1 .. 32768); growing it empties every slot.
 *   SPVO_ERR_CAPACITY  an image yields more rows than slot_capacity: out_*->n report the counts, both slots are left unfilled, nothing
 *                      is truncated.  (Candidate or raw-row lists that overflow are grown and the pair runs again: a second wait.)
 *   SPVO_ERR_INVALID   bad or equal slots, sizes spvo_sift_detect refuses
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight */
typedef struct { int n; spvo_sift_keypoint *kp; float *desc /* [cap][128] */; int cap; } spvo_sift_features;   /* n: out; min(n, cap) rows are written */
int spvo_sift_detect_pair(spvo_ctx *ctx, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride,
                          int slot_l, int slot_r, int slot_capacity, spvo_sift_features *out_l, spvo_sift_features *out_r);
/* Shi-Tomasi / FAST keypoints with SIFT descriptors (ClassicFeatureFrontEnd(ShiTomasi or FAST, SIFT)) for BOTH images of a stereo pair in
 * one call, into the same ring of ten SIFT slots: opts->kind is SPVO_CLASSIC_GFTT_SIFT or SPVO_CLASSIC_FAST_SIFT, the detector's parameters
 * and slot_capacity (1 .. 32768) are the other fields (spvo_default_classic_opts).  Both images go up through pinned staging.  Per image,
 * left first, on the solver's stream and without a host round trip: the image becomes the context's resident u8 image and goes through the
 * detector's chain (spvo_gftt_detect's / spvo_fast_detect's launches); the SIFT base level ALONE is built from it (one blur at the
 * image's own size: every record of these detectors lies on octave 0, layer 0); spvo_sift_describe's kernel runs on the detector's list
 * where it lies -- a record is {x, y, size 5 (Shi-Tomasi) or 7 (FAST), angle -1, the detector's response, octave 0}, the count is read
 * on the device, a fixed number of waves strides over the records -- and writes rows (256 floats, columns 128.. zero), squared norms,
 * records and the count into the slot and into pinned mirrors.  The call waits once, for the features of both images.
 * spvo_match_l2_slots, spvo_sift_slot_rows and spvo_set_prematch serve the slots as they serve spvo_sift_detect_pair's, with the same
 * temporal partner: any filled SIFT slot is one, whichever of the two calls filled it.
 *   Byte equality: per image the host receives, byte for byte, what spvo_gftt_detect / spvo_fast_detect with the same parameters returns
 *   followed by spvo_sift_describe(img = NULL) on the records above -- the records ClassicFeatureFrontEnd builds from its cv::KeyPoints.
 *   Records come in the detector's order, none is erased; out->n is the count, of which min(n, cap) rows are written.
 *   An image without a keypoint fills its slot with 0 rows: SPVO_OK, and spvo_match_l2_slots treats it as any empty slot.
 * Afterwards the resident u8 image is the RIGHT image: spvo_sift_describe(img = NULL), spvo_orb_describe(NULL) and
 * spvo_brisk_describe(NULL) work on it.  No SIFT pyramid is resident (spvo_sift_debug_level: SPVO_ERR_STATE), and the AKAZE scale
 * space's claim ends, as after spvo_sift_detect_pair.  A slot_capacity larger than any before empties every SIFT slot (the rule above).
 *   SPVO_ERR_CAPACITY  an image yields more rows than slot_capacity: out_*->n report both counts, both slots are left unfilled, nothing
 *                      is truncated
 *   SPVO_ERR_INVALID   nothing is written or touched: NULL arguments, a kind other than 5 / 6, bad or equal slots, slot_capacity outside
 *                      1 .. 32768, cap < 0, whatever spvo_gftt_detect / spvo_fast_detect and spvo_sift_describe refuse of the shape
 *                      or the parameters
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight */
int spvo_classic_sift_pair(spvo_ctx *ctx, const spvo_classic_opts *opts /* kind 5 or 6 */, const uint8_t *img_l, const uint8_t *img_r,
                           int rows, int cols, size_t stride, int slot_l, int slot_r,
                           spvo_sift_features *out_l, spvo_sift_features *out_r);
/* BRISK / AKAZE keypoints with SIFT descriptors (ClassicFeatureFrontEnd(BRISK or AKAZE, SIFT)) for BOTH images of a stereo pair in one
 * call, into the same ring of ten SIFT slots.  Both calls follow spvo_classic_sift_pair in protocol: the pinned staging, the left image's
 * chain then the right's on the solver's stream without a host round trip, one wait; slot rows of 256 floats (columns 128.. zero), squared
 * norms, SiftKey records and the count; spvo_match_l2_slots, spvo_sift_slot_rows and spvo_set_prematch; any filled SIFT slot as temporal
 * partner, whichever call filled it; slot_capacity 1 .. 32768, a larger one than any before emptying every SIFT slot.  Per image:
 *   1. the detector: spvo_brisk_detect's launches up to the refined records with their keep flags / spvo_akaze_detect_pair's launches
 *      through the suppression on the device, which leaves the kept records and their count there;
 *   2. a Gaussian-only SIFT pyramid of the resident u8 image at its own size for octaves 0 .. max_octave -- 5 for BRISK, the octave of the
 *      shape's last level for AKAZE: the host does not know which octaves hold keypoints -- reduced to what is read: every record of these
 *      detectors has layer 0 and an octave derives from layer 3 of the one below, so layers 0 .. 3 of every octave but the last and layer 0
 *      of the last (a layer depends only on the one before: these levels are bit for bit spvo_sift_describe's);
 *   3. spvo_sift_describe's kernel on the detector's records where they lie (byte stride and field offsets; BRISK: the kept records in the
 *      detector's order, by a compaction of indices on the device), the count read on the device, spvo_classic_sift_pair's fixed grid;
 *   4. its sink: the slot, and pinned mirrors of the rows and of the detector's OWN record, unchanged -- 24 bytes for BRISK
 *      (spvo_brisk_keypoint is spvo_sift_keypoint), 28 bytes with class_id for AKAZE.  The extractor changes no angle and erases nothing.
 *   Byte equality: per image the host receives, byte for byte, what spvo_brisk_detect(img, threshold, octaves) / spvo_akaze_detect(img,
 *   threshold) returns followed by spvo_sift_describe(img = NULL) on exactly those records (AKAZE: on {x, y, size, angle, response,
 *   octave} of them; class_id is not passed); row i belongs to record i.  An image without a keypoint fills its slot with 0 rows: SPVO_OK.
 * Afterwards the resident u8 image is the RIGHT image's (spvo_sift_describe(img = NULL), spvo_brisk_describe(NULL) work on it); BRISK:
 * spvo_brisk_detect_debug_layer answers SPVO_ERR_STATE, as after spvo_brisk_detect_pair; AKAZE: the right image's scale space is resident,
 * as after spvo_akaze_orb_pair; no SIFT pyramid is resident (spvo_sift_debug_level: SPVO_ERR_STATE).
 * (ORB + SIFT: spvo_orb_sift_pair, below.)
 *   SPVO_ERR_CAPACITY  an image yields more rows than slot_capacity: out_*->n report both counts, both slots are left unfilled, nothing
 *                      is truncated
 *   SPVO_ERR_INVALID   nothing is written or touched: NULL arguments, cap < 0 or a positive cap with a NULL buffer, bad or equal slots,
 *                      slot_capacity outside 1 .. 32768, whatever spvo_brisk_detect_pair / spvo_akaze_detect_pair and spvo_sift_describe
 *                      refuse of the shape or the parameters, and min(rows, cols) >> max_octave < 1 (the text names the octave; for BRISK
 *                      a dimension below 32) -- in the place of spvo_sift_describe's per-keypoint refusal, which the host can no longer
 *                      evaluate
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight; the detector's candidate list overflowed (it is sized from the image) */
int spvo_brisk_sift_pair(spvo_ctx *ctx, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride,
                         int threshold, int octaves, int slot_l, int slot_r, int slot_capacity,
                         spvo_sift_features *out_l, spvo_sift_features *out_r);
typedef struct { int n; spvo_akaze_keypoint *kp; float *desc /* [cap][128] */; int cap; } spvo_akaze_sift_features;   /* n: out; min(n, cap) rows are written */
int spvo_akaze_sift_pair(spvo_ctx *ctx, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride,
                         float threshold, int slot_l, int slot_r, int slot_capacity,
                         spvo_akaze_sift_features *out_l, spvo_akaze_sift_features *out_r);
/* The ORB detector in front of another algorithm's extractor, pair-resident: ORB + BRISK into the ring of ten BINARY slots (64-byte rows,
 * spvo_brisk_detect_pair's protocol) and ORB + SIFT into the ring of ten SIFT slots (spvo_brisk_sift_pair's protocol).  Per image, left
 * first, on the solver's stream and without a host round trip: the staged image becomes the context's resident u8 image; spvo_orb_detect's
 * launches run with THAT image as level 0 of the pyramid (levels 1 .. 7 and the detector's maps stay its own; ORB's own rows are not kept);
 * one kernel turns the detector's list into 24-byte records {x, y, size = 31 * 1.2^octave (the repeated float product), angle in degrees
 * 0 .. 360, response, octave} -- n = min(the eight levels' counts, nfeatures) -- and the extractor's chain reads them where they lie:
 *   spvo_orb_brisk_pair  the integral image, the border rule at every record's own size as one order-preserving compaction, the rows with
 *                        the count read on the device, the finish launch.  Byte equality: what spvo_orb_detect(img, nfeatures) followed
 *                        by spvo_brisk_describe(its x, y, those sizes) returns -- the records [kept] with `angle` = the extractor's
 *                        degrees, the 64-byte rows.  The slot's own records hold (x, y, that angle, response, octave).
 *   spvo_orb_sift_pair   the reduced Gaussian pyramid for octaves 0 .. max_octave and spvo_sift_describe's kernel on all records;
 *                        max_octave is the highest ORB level of the shape that can hold a keypoint (more than 64 pixels in both
 *                        dimensions at scale 1.2^l), 0 if none can, and every such shape has SIFT's octave max_octave.  Byte equality:
 *                        spvo_orb_detect followed by spvo_sift_describe on exactly those records; none is erased, no angle changes.
 * An image without a keypoint -- a shape without a level that can hold one included -- fills its slot with 0 rows: SPVO_OK.  Afterwards
 * the resident u8 image is the RIGHT image (spvo_brisk_describe(NULL), spvo_sift_describe(NULL), spvo_orb_describe(NULL) work on it).
 * spvo_set_prematch, the temporal partner (any filled slot of the ring and, for the binary ring, of 64-byte rows, whichever call filled
 * it) and the re-allocation by a larger slot_capacity than any before are the siblings'.
 *   SPVO_ERR_INVALID   nothing is written or touched: NULL arguments, bad or equal slots, slot_capacity outside 1 .. 32768,
 *                      nfeatures <= 0, cap < 0 (SIFT: or a positive cap with a NULL buffer), what spvo_brisk_describe (BRISK call) /
 *                      spvo_sift_describe (SIFT call) refuse of the shape
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight (outputs and slots stay as they were)
 *   SPVO_ERR_CAPACITY  a level's corner buffer overflowed (spvo_orb_detect's answer), or an image yields more rows than slot_capacity:
 *                      out_*->n report both counts, both slots are left unfilled, nothing is truncated */
int spvo_orb_brisk_pair(spvo_ctx *ctx, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride,
                        int nfeatures, int slot_l, int slot_r, int slot_capacity,
                        spvo_brisk_features *out_l, spvo_brisk_features *out_r);   /* desc [cap][64] */
int spvo_orb_sift_pair(spvo_ctx *ctx, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride,
                       int nfeatures, int slot_l, int slot_r, int slot_capacity,
                       spvo_sift_features *out_l, spvo_sift_features *out_r);
/* The SIFT detector in front of the BRISK extractor, pair-resident in the ring of ten BINARY slots (64-byte rows, spvo_brisk_detect_pair's
 * protocol: spvo_match_hamming_slots, spvo_match_l2_u8_slots, spvo_classic_slot_rows and spvo_set_prematch work on the slots unchanged, any
 * filled slot of 64-byte rows is the temporal partner, a larger slot_capacity than any before re-allocates).  Per image, left first, on the
 * solver's stream and without a host round trip: the staged image becomes the context's resident u8 image; the SIFT pyramid is built from
 * THAT image; candidates, refinement and the orientation peaks run as in spvo_sift_detect but without the 128-float rows (one keypoint per
 * peak is kept: OpenCV's detector emits them and BRISK describes each); the raw rows are ordered on the device as in
 * spvo_sift_detect_pair; one kernel presents the ordered list as 24-byte records {x, y, size, angle, response, octave}; and the BRISK
 * extractor's chain reads them where they lie: the integral image, the border rule at every record's own scale index as one
 * order-preserving compaction, the rows with the count read on the device, the finish launch.
 *   Byte equality: per image the host receives, byte for byte in every field and row, what spvo_sift_detect(img) followed by
 *   spvo_brisk_describe(img, its x, y, size) returns -- the detector's records [kept] with `angle` replaced by the extractor's degrees, the
 *   64-byte rows in the detector's order.  The slot's own records hold (x, y, that angle, response, octave).
 *   The size: on the device it comes from a double pow, on the host from spvo_sift_detect's own function.  Behind the wait the host
 *   rebuilds every final row's record from the mirrored {candidate, offsets, angle} and compares the sizes bit for bit.  They are expected
 *   to agree always; an image in which one differs gets the host's records uploaded and the extractor's chain once more (a second wait).
 *   spvo_set_tuning("sift_brisk_recheck", 1) forces that second pass for both images (diagnostic).
 * The candidate and raw-row lists grow to what was counted and the pair runs again when they overflow (spvo_sift_detect_pair's rule: a
 * second wait).  An image without a keypoint fills its slot with 0 rows: SPVO_OK.  Afterwards the resident u8 image is the RIGHT image
 * (spvo_brisk_describe(NULL), spvo_sift_describe(NULL) work on it), the right image's SIFT pyramid is resident (spvo_sift_debug_level), the
 * AKAZE scale space's claim has ended and spvo_brisk_detect_debug_layer answers SPVO_ERR_STATE.
 *   SPVO_ERR_INVALID   nothing is written or touched: NULL arguments, bad or equal slots, slot_capacity outside 1 .. 32768, cap < 0, an
 *                      image spvo_sift_detect refuses (under 6 x 6) or spvo_brisk_describe refuses (rows * cols * 255 >= 2^31)
 *   SPVO_ERR_STATE     a spvo_detect*_submit is in flight (outputs and slots stay as they were)
 *   SPVO_ERR_CAPACITY  an image yields more rows than slot_capacity: out_*->n report both counts, both slots are left unfilled, nothing
 *                      is truncated */
int spvo_sift_brisk_pair(spvo_ctx *ctx, const uint8_t *img_l, const uint8_t *img_r, int rows, int cols, size_t stride,
                         int slot_l, int slot_r, int slot_capacity,
                         spvo_brisk_features *out_l, spvo_brisk_features *out_r);   /* desc [cap][64] */
/* spvo_sift_brisk_pair's chain of ONE image up to the records the BRISK extractor's chain reads (test hook): the image becomes the resident
 * u8 image, `rec` receives min(n, cap) records in the detector's order (`angle` is still the detector's), `n` their number.  describe != 0
 * runs the describing form of the orientation kernel in the other's place: the records must not depend on it.
 *   SPVO_ERR_INVALID as spvo_sift_detect; SPVO_ERR_CAPACITY: the lists overflowed (they hold at least 8192 rows); SPVO_ERR_STATE: a
 *   spvo_detect*_submit is in flight */
int spvo_sift_records_debug(spvo_ctx *ctx, const uint8_t *img, int rows, int cols, size_t stride, int describe,
                            spvo_sift_keypoint *rec, int cap, int *n);
/* The link of the ORB / BRISK / AKAZE + SIFT calls above -- compaction by keep flags, the reduced pyramid for octaves 0 .. max_octave, the describe launch on
 * the fixed grid with the count read on the device -- on a caller's list against the u8 image already resident, of shape rows x cols
 * (test hook: lists no image gives).  No detector runs, no slot is touched, the image stays resident.  keep = NULL: all records take
 * part; `kept` names the original indices, and the rows equal spvo_sift_describe(img = NULL) on the kept records.
 *   SPVO_ERR_INVALID   max_octave outside 0 .. 15 or naming an empty level; a record whose unpacked octave is outside 0 .. max_octave or
 *                      whose layer is not 0; a field spvo_sift_describe refuses.  Nothing is written.
 *   SPVO_ERR_STATE     no image of that shape is resident; a spvo_detect*_submit is in flight */
int spvo_sift_link_debug(spvo_ctx *ctx, int rows, int cols, const spvo_sift_keypoint *kp, const uint8_t *keep /* [n] or NULL */,
                         int n, int max_octave, int32_t *kept /* [n] */, float *desc /* [n][128] */, int *n_kept);
/* rows a SIFT slot holds; SPVO_ERR_STATE for one that holds nothing (never filled, or left unfilled by SPVO_ERR_CAPACITY) */
int spvo_sift_slot_rows(spvo_ctx *ctx, int slot, int *n);
/* spvo_match_l2(dim = 128) on the device-resident rows of two SIFT slots: nothing is uploaded, no norm is recomputed.  Results equal
 * spvo_match_l2 on the host copies, index for index and distance for distance (distances are exact integers).  Returns the result stored
 * by spvo_sift_detect_pair when spvo_set_prematch is on and this is exactly that match of exactly those slot contents.  Empty and
 * unfilled slots as in spvo_match_hamming_slots. */
int spvo_match_l2_slots(spvo_ctx *ctx, int slot_a, int slot_b, int selector, int cross_check, float ratio,
                        int32_t *train_idx, float *distance);
/* The ordering stage of spvo_sift_detect_pair alone, on caller-supplied records (test hook): `order` receives the indices of the records
 * that stay, in output order -- OpenCV's total order, of records equal in (x, y, size, angle) the first -- and n_kept their number. */
int spvo_sift_order_debug(spvo_ctx *ctx, const spvo_sift_keypoint *rec, int n, int32_t *order /* [n] */, int *n_kept);

/* Optional latency hiding for the reference's fixed call order (node.cpp:175-198: detect, then
 * match CURR_LEFT->CURR_RIGHT, then CURR_LEFT->PREV_LEFT): when enabled, spvo_detect* enqueues
 * those two matches (slot_l -> slot_r, slot_l -> the previous call's slot_l) with these selector
 * parameters in the same GPU submission, and spvo_match_slots returns the stored result when it
 * is asked for exactly that match (same slots, same slot contents, same parameters).  Results
 * are identical with it on or off.  spvo_classic_detect / spvo_match_hamming_slots do the same on the
 * binary slots, spvo_sift_detect_pair and spvo_classic_sift_pair / spvo_match_l2_slots on the SIFT slots. */
int spvo_set_prematch(spvo_ctx *ctx, int enable, int selector, int cross_check, float ratio);

/* Extension (BASELINE config 5): build the matcher's candidate shortlist with an fp8 (e4m3) distance GEMM instead of
 * the fp32 one.  The GEMM only prunes; the result is EXACT: a first pass re-scores a statistical window canonically, a second
 * pass every column whose rigorous lower bound (from the per-row norms of the fp8 rounding residuals) does not exceed the
 * second canonical distance found -- indices and distances are the brute-force ones on every row (csrc/match.hip.h). */
int spvo_set_match_fp8(spvo_ctx *ctx, int enable);
/* 1 / 0: the fp8 shortlist is on / off in this context (what the host class's setMatchFp8 asked for); negative: error. */
int spvo_get_match_fp8(const spvo_ctx *ctx);
/* Which kernels the most recent L2 match of this context ran (read-only; for tests, which otherwise cannot tell the matcher's three
 * forms apart: their results are identical).  info = {fp8, fused, NCH, jobs}:
 *   fp8    1: fp8 shortlist GEMM + the two-pass re-rank (spvo_set_match_fp8)
 *   fused  1: the distance tile is reduced in LDS and a merge kernel finishes the row (the default up to a matcher capacity of 64
 *             column tiles = 8192 rows); 0: every distance goes to memory and the re-rank kernel reads the row back (fp8, capacities
 *             beyond 8192 rows, tuning "match_fused" = 0)
 *   NCH    re-rank instantiation: 4 = rows of up to 1024 columns held in registers, 0 = chunked with a ring queue (always 0 when fused;
 *             with NN + cross_check the sides are swapped, so the QUERY count decides)
 *   jobs   matches in that launch set (1, or 2 for a detector call's prematch); 0: this context has not matched yet
 * A call that returns without a launch (an empty side, a result served from a prematch) leaves the record as it was. */
int spvo_match_last_form(spvo_ctx *ctx, int info[4]);

/* cv::triangulatePoints + convertPointsFromHomogeneous (base.cpp:211-223):
 * DLT null vector of the 4x4 system in f64, stored f32, then x/w.
 * xy_l, xy_r: [n][2] f32; xyz: [n][3] f32. */
int spvo_triangulate(spvo_ctx *ctx, const double P_l[12], const double P_r[12], const float *xy_l,
                     const float *xy_r, int n, float *xyz);

/* Deterministic P3P-RANSAC standing in for cv::solvePnPRansac(..., true, 500,
 * 2.0, 0.999, inliers, USAC_ACCURATE) (base.cpp:237-239).  K = P_l[:, :3].
 * rvec/tvec: in = motion prior, out = model.  inliers: caller buffer [n].
 * Returns 0 with *ok = 0 when no model with >= 4 inliers was found. */
typedef struct {
  int iterations;          /* [500]   */
  double reproj_error;     /* [2.0]   */
  double confidence;       /* [0.999] (kept for signature parity; the loop is not
                              terminated early so results do not depend on it) */
  uint32_t seed;           /* sample stream seed [0] */
} spvo_ransac_opts;

int spvo_pnp_ransac(spvo_ctx *ctx, const double K[9], const float *xyz, const float *xy, int n,
                    const spvo_ransac_opts *opts, double rvec[3], double tvec[3],
                    int32_t *inliers, int *n_inliers, int *ok);

/* One residual block of the refinement problem (CostFunctor32, cost.hpp:8-58). */
typedef struct {
  float X[3];          /* 3-D point (cv::Vec3f)                 */
  float uv[2];         /* observation (cv::Point2f)             */
  int32_t cam;         /* 0: P_l, 1: P_r                        */
  int32_t inverse;     /* inverse_transformation_ (cost.hpp:35) */
} spvo_obs;

typedef struct {
  int max_iterations;      /* [40] base.cpp:362 */
  double huber_delta;      /* [1.0] base.cpp:286 */
} spvo_refine_opts;

typedef struct {
  int iterations;
  int converged;           /* termination_type == CONVERGENCE (base.cpp:366-367) */
  int usable;
  double initial_cost, final_cost;
} spvo_refine_summary;

/* ceres::Solve on the CostFunctor32 blocks (base.cpp:282-375): Levenberg-
 * Marquardt with Huber loss, quaternion local parameterisation, f64.
 * q: Eigen coefficient order x,y,z,w (base.cpp:302); in = start, out = result. */
int spvo_pnp_refine(spvo_ctx *ctx, const double P_l[12], const double P_r[12],
                    const spvo_obs *obs, int n_obs, const spvo_refine_opts *opts, double q[4],
                    double t[3], spvo_refine_summary *summary);

/* The numeric body of solveStereoOdometry after the correspondence join (base.cpp:209-375) in ONE
 * submission: triangulate -> RANSAC -> gating (base.cpp:241-272; decided on the host when the results are collected) -> residual blocks in the order
 * of base.cpp:291-356 -> LM refinement -> "not converged => keep the RANSAC pose" (base.cpp:366-374).
 * Identical to calling spvo_triangulate, spvo_pnp_ransac and spvo_pnp_refine in sequence with the
 * host-side glue in between, minus the round trips. */
typedef struct {
  int n;                        /* joined correspondences (base.cpp:156-207)            */
  const float *xy_cl, *xy_cr;   /* [n][2] current left / right                          */
  const float *xy_pl, *xy_pr;   /* [n][2] previous left / right                         */
  const float *prev_xyz;        /* [n][3] previous-frame 3-D point of each correspondence,
                                   or NULL before the first solved frame (base.cpp:323)  */
  const int32_t *prev_valid;    /* [n] 1 where prev_xyz[i] exists (base.cpp:326-332)     */
  double P_l[12], P_r[12];
  double rvec_pred[3], tvec_pred[3];   /* motion prior (hpp:156-157)                     */
  int frame_count;              /* hpp:158                                               */
  int refinement_degree;        /* hpp:143                                               */
  spvo_ransac_opts ransac;
  spvo_refine_opts refine;
  /* Round 6 (both optional, zero = as before): */
  const int32_t *prev_index;    /* [n] instead of prev_xyz / prev_valid: index of each correspondence's previous-frame point among the
                                   points the PREVIOUS spvo_solve_submit of this context triangulated (its xyz output, still on the
                                   device), -1 where there is none (base.cpp:323-332).  The host need not have collected them.
                                   They stay reachable when this submission makes the solver's buffers grow (n above the capacity:
                                   max(2048, max_keypoints) at first).  A submission that fails leaves them as they were: the next
                                   prev_index refers to the points of the last submission that succeeded.                      */
  int late_prior;               /* 1: rvec_pred / tvec_pred / frame_count are not known yet (the previous frame's solve is still in
                                   flight) -- they are ignored here and handed to spvo_solve_wait_prior instead.
                                   2: the same, and the chain's LAST kernel is held back: it goes out in one launch with the next
                                   submission's hypotheses (beside which it runs), or alone when this solve is waited for first --
                                   for callers that wait for frame k only after they have submitted frame k + 2 (see below).
                                   Two halves only: spvo_solve_stereo_odometry answers SPVO_ERR_STATE for late_prior != 0.          */
} spvo_solve_input;

typedef struct {
  double q[4], t[3];            /* cam0_prev_T_cam0_curr to invert (base.cpp:377-385); q = x,y,z,w */
  double rvec[3], tvec[3];      /* pose after gating = the new motion prior when `accepted`       */
  int pnp_ok;                   /* solvePnPRansac's return value                                  */
  int accepted;                 /* do_optmz (base.cpp:243-272)                                    */
  int refined;                  /* refinement ran, converged and was kept                         */
  int n_inliers;
  spvo_refine_summary summary;
} spvo_solve_output;

/* One-piece: spvo_solve_submit + spvo_solve_wait of that same solve.  SPVO_ERR_STATE, with nothing queued, while any solve is
 * pending (the wait would complete the oldest one, not this) or for late_prior != 0. */
int spvo_solve_stereo_odometry(spvo_ctx *ctx, const spvo_solve_input *in, spvo_solve_output *out,
                               float *xyz /* [n][3] triangulated points */,
                               int32_t *inliers /* [n] RANSAC inliers, ascending */);

/* The same call in two halves, for a caller with something else to do in between (collecting the next pair's detector
 * output, publishing, bookkeeping).  spvo_solve_submit stages the inputs in pinned memory -- the caller's arrays are free
 * again when it returns -- and enqueues the whole chain on the solver's stream; spvo_solve_wait blocks until the OLDEST
 * pending solve is done and hands out what spvo_solve_stereo_odometry would have.  While a solve is pending the stand-alone
 * solver entry points (spvo_triangulate, spvo_pnp_ransac, spvo_pnp_refine) answer SPVO_ERR_STATE.
 *
 * Up to THREE solves may be pending (round 6).  Nothing the device computes for frame k needs frame k - 1's POSE: the RANSAC's
 * minimal solver is prior-free (as cv::solvePnPRansac's P3P is, base.cpp:237-239), the refinement starts from the RANSAC
 * pose, and the one step that does need the motion prior -- the gate, base.cpp:241-272: three subtractions and a compare --
 * is evaluated by the wait on the host (a submission that carries its prior, late_prior = 0, has it evaluated on the device instead, so
 * that a rejected frame skips its refinement).  What frame k needs of frame k - 1 are its 3-D points (base.cpp:323-332), and
 * `prev_index` refers to them where they lie.  So a caller may submit frame k (late_prior = 1, prev_index) BEFORE it waits
 * for frame k - 1, and hands the prior -- known once k - 1 has been collected -- to spvo_solve_wait_prior.  Results are
 * those of the one-piece call, bit for bit (tests/test_gpu_odometry.py, tests/test_gpu_host.py).  The last kernel of a
 * late_prior = 2 submission's chain (selection, residual blocks, refinement: one workgroup, ~90 us) is held back and goes out in
 * ONE launch with the hypotheses of the next submission, beside which it runs -- or alone, when the solve is waited for
 * first: a caller that waits for frame k only after it has submitted frame k + 2 never waits for the solver's stream, whose
 * work per frame is then max(hypotheses, tail) instead of their sum.  The reference has no counterpart: solveStereoOdometry
 * (base.cpp:125-399) is one blocking call.
 * Buffers: the solver's buffers grow on the first submission that needs more (n correspondences, RANSAC iterations, 4 n residual
 * blocks) -- with a solve pending that submission answers SPVO_ERR_STATE and changes nothing (the pending solves complete as they would
 * have; submit again once they have been waited for).  Growth keeps the last submission's points for the next one's prev_index. */
int spvo_solve_submit(spvo_ctx *ctx, const spvo_solve_input *in);
int spvo_solve_wait(spvo_ctx *ctx, spvo_solve_output *out, float *xyz, int32_t *inliers);
int spvo_solve_wait_prior(spvo_ctx *ctx, const double rvec_pred[3], const double tvec_pred[3], int frame_count,
                          spvo_solve_output *out, float *xyz, int32_t *inliers);
int spvo_solve_pending(spvo_ctx *ctx);   /* solves submitted and not waited for yet (0 .. 3) */

/* ------------------------------------------------------- multi-GPU: pose gather
 * The path shards by stereo stream: one process per GPU, each with its own FeatureFrontEnd
 * state; nothing but the resulting relative poses -- q (x, y, z, w) + t of cam0_curr_T_cam0_prev, base.cpp:377-385,
 * 7 doubles -- is ever exchanged.  The communicator is RCCL over xGMI (ncclAllGather on a stream of its own); librccl
 * is opened when the first communicator is created, not when this library is loaded.  Errors: spvo_last_error(NULL). */
typedef struct spvo_comm spvo_comm;
#define SPVO_COMM_ID_BYTES 128

/* Rank 0 creates the id (ncclGetUniqueId) and hands it to the other ranks out of band (ROS parameter server, a file,
 * MPI, torchrun's store); every rank then calls spvo_comm_create -- collectively, like ncclCommInitRank. */
int spvo_comm_unique_id(unsigned char id[SPVO_COMM_ID_BYTES]);
/* SPVO_OK when librccl can be opened and has the entry points this library uses (dlopen + dlsym: no bootstrap state is created,
 * unlike spvo_comm_unique_id): what every rank checks BEFORE the ranks enter spvo_comm_create together.  A failure INSIDE
 * ncclCommInitRank (a peer that died after this check) is not recoverable collectively: the launcher's job (bench.py: spawn_ranks /
 * torch.distributed.run stop the job when a rank dies). */
int spvo_comm_available(void);
int spvo_comm_create(int device, int rank, int world, const unsigned char id[SPVO_COMM_ID_BYTES], spvo_comm **out);
/* TEST transport, no GPU: ranks exchange through files in `dir` (world-size-2 CPU tests of the N > 1 code path). */
int spvo_comm_create_host(const char *dir, int rank, int world, spvo_comm **out);
int spvo_comm_rank(const spvo_comm *comm);
int spvo_comm_world(const spvo_comm *comm);
void spvo_comm_destroy(spvo_comm *comm);

/* all[r][7] = rank r's pose.  Collective and synchronous (host memory in, host memory out). */
int spvo_pose_allgather(spvo_comm *comm, const double pose[7], double *all /* [world][7] */);
/* Batched form: n poses per rank (the same n on every rank) in ONE collective; all[r][i][7].  56 bytes per frame are
 * pure latency, so a throughput-oriented caller gathers once per batch of frames. */
int spvo_pose_allgather_n(spvo_comm *comm, const double *poses /* [n][7] */, int n, double *all /* [world][n][7] */);

/* ---------------------------------------------------------------- plumbing */
void *spvo_stream(spvo_ctx *ctx);                 /* hipStream_t of the context */
int spvo_synchronize(spvo_ctx *ctx);

/* Per-stage HIP-event timing on the context's stream (bench.py's roofline leg).
 * Stage names: "conv:<op index>", "net", "post", "match", ...; see DESIGN.md. */
int spvo_profile_enable(spvo_ctx *ctx, int on);
int spvo_profile_reset(spvo_ctx *ctx);
/* Restrict the timing to ONE stage (e.g. "conv:1"); NULL or "" = every stage again.  Two event records per step
 * instead of two per kernel: the way to time a kernel inside a throughput measurement without slowing it down. */
int spvo_profile_only(spvo_ctx *ctx, const char *stage);
int spvo_profile_count(spvo_ctx *ctx);
int spvo_profile_get(spvo_ctx *ctx, int i, char *name, size_t name_cap, double *total_ms,
                     long long *calls, double *flops_per_call, double *bytes_per_call);
/* Which kernel family the loaded engine runs a "conv:<op index>" stage on ("conv_wino4_kernel", "conv_wino2_kernel",
 * "conv_mfma_kernel", "conv_f16_kernel", ...), and how many multiply-adds the matrix pipe executes per multiply-add of the
 * direct convolution (Winograd F(4x4,3x3): 0.25, F(2x2,3x3): 4/9, split bf16x3 mode: 6, otherwise 1). */
int spvo_profile_stage_kernel(spvo_ctx *ctx, const char *stage, char *name, size_t name_cap, double *executed_per_algorithmic);
/* Which TILE VARIANT of conv_mfma_kernel / conv_f16_kernel / conv_i8_kernel / conv_s3_kernel the loaded engine runs a "conv:<op index>"
 * stage on -- the launchers' dispatch key: info[0] = kernel size (1 or 3), [1] = input channels per chunk, [2] = wr, [3] = wc (the tile is
 * 4 wr rows x 32 wc columns of pixels), [4] = 1 for a layer with the 2x2 pooling fused -- and the persistent grid of that stage's most
 * recent launch: [5] = tiles, [6] = workgroups (0, 0 before any launch).  A layer that runs no tile variant (a Winograd layer, a
 * single-channel stem, a layer merged into its sibling's launch, an INT8 depthwise + pointwise block in one launch, the fused
 * heads) reports info[0 .. 4] = 0. */
int spvo_profile_stage_variant(spvo_ctx *ctx, const char *stage, int info[7]);
/* What the launches that spvo_profile_stage_variant leaves out last ran.  stage = "conv:<index of a pointwise op>": info[0] = 1 once the
 * INT8 depthwise + pointwise block ran as one launch of dwpw_i8_kernel<G, STEM, POOL, EPI> (0: the op runs layer by layer, or has not run
 * yet -- then all of info is 0), [1] = G (16-channel groups of the depthwise layer: 4 or 8), [2] = STEM (the fp32 stem in the same launch),
 * [3] = POOL, [4] = EPI (1: BatchNorm), [5] = tiles of 64 output channels, and of the most recent launch [6] = tiles of 8 x 32 pixels,
 * [7] = workgroups.  stage = "heads": info[0] = 1 once the fused tail ran, [1] = 1 heads_fused_kernel<false> (FP32 engines), 2
 * heads_fused_kernel<true> (FP16), 3 heads_i8_kernel, [6] = pixel tiles (16 pixels; INT8: 32), [7] = workgroups; [2 .. 5] = 0. */
int spvo_profile_stage_fused(spvo_ctx *ctx, const char *stage, int info[8]);

/* ------------------------------------------------------- diagnostic switches (A/B measurements, parity debugging)
 * Which kernels / streams an engine uses is decided by the library from the plan and the sizes.  The decisions can be overridden
 * for measurements and tests -- through THIS call only: the library reads no environment variable for them, so the environment
 * of the process that hosts it (a ROS node) cannot change kernels by accident.  Process-wide; a value takes effect for contexts
 * created / engines loaded afterwards.  `name` is one of the names INTEGRATION.md lists ("winograd", "wino4", "wino4_item", "wino_narrow",
 * "wino_dynamic", "winograd_min_tiles", "wino4_min_tiles", "merge_siblings", "heads_fused", "heads_on_net", "heads_split",
 * "match_fused", "fp32_split", "prematch", "spin_wait", "trunk_timing", "solve_timing", "nms_first", "upload_side", "conv_variant", "int8_general"); SPVO_ERR_INVALID for any other.
 * spvo_get_tuning returns the value set, or `dflt`; spvo_clear_tuning forgets every value.
 * "wino4_item" selects the item of the F(4x4,3x3) kernel: 3 (the default), 2, 1 or 0, oldest last; all four give the same bits. */
int spvo_set_tuning(const char *name, int value);
int spvo_get_tuning(const char *name, int dflt);
void spvo_clear_tuning(void);

#ifdef __cplusplus
}
#endif
#endif /* SPVO_H */
